// CPU check of gr::dvbt::hip::core<H, P> (gr_dvbt_amd/host/gr/hip_shell.h), the layer between a GNU Radio block shell and the C ABI of libdvbt_hip: it takes its
// four C-ABI functions as constructor arguments, so it runs here over fakes that record what they were given and return scripted side-bands, on the behaving
// stand-in gr::block of oracle/ref_standin/.  No GPU, no library: dvbt_last_error is this file's own.
#include "hip_shell.h"
#include <cstdio>
#include <cstring>

static const char *g_error = "";
extern "C" const char *dvbt_last_error(void) { return g_error; }

struct fake_params { int a, b; };
struct fake_handle { int a, b; };

static struct script {
  int create_rc, produced, n_consumed, n_out_tags;
  std::vector<dvbt_tag> out_tags;                     // what work writes (as many as fit out_cap)
} S;
static struct seen {
  int creates, destroys, works, noutput, ninput, out_cap, n_out_before, n_consumed_before;
  const void *in; void *out;
  std::vector<dvbt_tag> in_tags;
  const dvbt_tag *in_ptr;
} R;

static int f_create(const fake_params *p, fake_handle **out)
{
  R.creates++;
  if (S.create_rc < 0) { g_error = "fake create refused"; return S.create_rc; }
  *out = new fake_handle{p->a, p->b};
  return 0;
}
static int f_forecast(const fake_handle *h, int noutput, int *need) { *need = 2 * noutput + h->a; return 0; }
static int f_work(fake_handle *, int noutput, int ninput, const void *in, void *out, dvbt_sideband *sb)
{
  R.works++; R.noutput = noutput; R.ninput = ninput; R.in = in; R.out = out; R.out_cap = sb->out_cap;
  R.n_out_before = sb->n_out_tags; R.n_consumed_before = sb->n_consumed; R.in_ptr = sb->in_tags;
  R.in_tags.assign(sb->in_tags, sb->in_tags + sb->n_in_tags);
  for (int i = 0; i < S.n_out_tags && i < sb->out_cap; i++) sb->out_tags[i] = S.out_tags[i];
  sb->n_out_tags = S.n_out_tags;                      // the library reports every tag it had, also those that did not fit
  sb->n_consumed = S.n_consumed;
  if (S.produced < 0) g_error = "fake work failed";
  return S.produced;
}
static void f_destroy(fake_handle *h) { R.destroys++; delete h; }

typedef gr::dvbt::hip::core<fake_handle, fake_params> core_t;

struct test_block : gr::block {
  test_block() : gr::block("test", gr::io_signature::make(1, 1, 4), gr::io_signature::make(1, 1, 4)) {}
};

static int errors = 0;
#define CHECK(c) do { if (!(c)) { errors++; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void tag(test_block &b, uint64_t off, const char *key, long v)
{
  gr::tag_t t{off, pmt::string_to_symbol(key), pmt::from_long(v), pmt::pmt_t()};
  b.si_in_tags[0].push_back(t);
}

int main()
{
  const fake_params p = {5, 9};
  int in_buf[8] = {0}, out_buf[8] = {0};

  // a failing create throws with dvbt_last_error's text, and nothing is destroyed
  S.create_rc = -2;
  bool threw = false;
  try { core_t c(p, f_create, f_forecast, f_work, f_destroy); } catch (const std::runtime_error &e) { threw = std::string(e.what()) == "libdvbt_hip: fake create refused"; }
  CHECK(threw && R.creates == 1 && R.destroys == 0);
  S.create_rc = 0;

  {
    core_t c(p, f_create, f_forecast, f_work, f_destroy);
    CHECK(c.handle() && c.handle()->a == 5 && c.handle()->b == 9);                   // the params reach create as given

    // forecast fills every entry of `required`
    gr_vector_int req(3, -1);
    c.forecast(7, req);
    CHECK(req[0] == 19 && req[1] == 19 && req[2] == 19);
    gr_vector_int none;
    c.forecast(7, none);                                                               // a source-like call: nothing to fill, nothing written

    // tags in: known keys translated, unknown dropped, rel_offset = offset - nitems_read, only the window [nitems_read, nitems_read + ninput)
    test_block b;
    b.si_nread[0] = 1000; b.si_nwritten[0] = 50000;
    tag(b, 999, "sync_start", 1);                  // in front of the window
    tag(b, 1000, "sync_start", 11);
    tag(b, 1003, "rx_time", 77);                   // not one of ours
    tag(b, 1003, "superframe_start", 0xaa);
    tag(b, 1009, "symbol_index", 67);
    tag(b, 1010, "symbol_index", 0);               // first item behind the window
    S.produced = 6; S.n_consumed = 10; S.n_out_tags = 2;
    S.out_tags = { {0, DVBT_TAG_SUPERFRAME_START, 1}, {5, DVBT_TAG_SYMBOL_INDEX, 33} };
    int r = c.work(&b, 8, 10, in_buf, out_buf);
    CHECK(r == 6 && R.works == 1 && R.noutput == 8 && R.ninput == 10 && R.in == in_buf && R.out == out_buf);
    CHECK(R.out_cap == 4096 && R.n_out_before == 0 && R.n_consumed_before == 0);
    CHECK(R.in_tags.size() == 3);
    if (R.in_tags.size() == 3) {
      CHECK(R.in_tags[0].rel_offset == 0 && R.in_tags[0].key == DVBT_TAG_SYNC_START && R.in_tags[0].value == 11);
      CHECK(R.in_tags[1].rel_offset == 3 && R.in_tags[1].key == DVBT_TAG_SUPERFRAME_START && R.in_tags[1].value == 0xaa);
      CHECK(R.in_tags[2].rel_offset == 9 && R.in_tags[2].key == DVBT_TAG_SYMBOL_INDEX && R.in_tags[2].value == 67);
    }
    // tags out: at nitems_written + rel_offset, on output 0, with the right symbol; n_consumed reaches consume_each
    CHECK(b.si_out_tags.size() == 2);
    if (b.si_out_tags.size() == 2) {
      CHECK(b.si_out_tags[0].offset == 50000 && pmt::symbol_to_string(b.si_out_tags[0].key) == "superframe_start" && pmt::to_long(b.si_out_tags[0].value) == 1);
      CHECK(b.si_out_tags[1].offset == 50005 && pmt::symbol_to_string(b.si_out_tags[1].key) == "symbol_index" && pmt::to_long(b.si_out_tags[1].value) == 33);
      CHECK(b.si_out_tag_port[0] == 0 && b.si_out_tag_port[1] == 0);
    }
    CHECK(b.si_consumed[0] == 10);

    // a call without input tags hands the library an empty list
    test_block e;
    S.n_out_tags = 0; S.n_consumed = 0; S.produced = 0;
    r = c.work(&e, 1, 1, in_buf, out_buf);
    CHECK(r == 0 && R.in_tags.empty() && R.in_ptr == 0 && e.si_out_tags.empty() && e.si_consumed[0] == 0);

    // work_with: the same marshalling around another call of the library
    struct other { int *calls; int operator()(dvbt_sideband *sb) const { ++*calls; sb->n_consumed = 3; sb->n_out_tags = 1; sb->out_tags[0] = dvbt_tag{2, DVBT_TAG_SYNC_START, 1}; return 4; } };
    int calls = 0;
    other o = { &calls };
    test_block w;
    w.si_nwritten[0] = 7;
    r = c.work_with(&w, 5, o);
    CHECK(r == 4 && calls == 1 && w.si_consumed[0] == 3 && w.si_out_tags.size() == 1 && w.si_out_tags[0].offset == 9 &&
          pmt::symbol_to_string(w.si_out_tags[0].key) == "sync_start");

    // 4096 and 4097 output tags: the vector holds 4096; what did not fit is not read
    S.out_tags.clear();
    for (int i = 0; i < 4097; i++) S.out_tags.push_back(dvbt_tag{i, DVBT_TAG_SYMBOL_INDEX, i % 68});
    for (int n = 4096; n <= 4097; n++) {
      test_block t;
      S.n_out_tags = n; S.produced = 4097; S.n_consumed = 4097;
      r = c.work(&t, 4097, 4097, in_buf, out_buf);
      CHECK(r == 4097 && t.si_out_tags.size() == 4096);
      if (t.si_out_tags.size() == 4096)
        CHECK(t.si_out_tags[4095].offset == 4095 && pmt::to_long(t.si_out_tags[4095].value) == 4095 % 68);
    }

    // a negative return throws with dvbt_last_error's text; nothing is consumed, no tag is attached
    test_block f;
    S.produced = -1; S.n_out_tags = 1; S.n_consumed = 5;
    threw = false;
    try { c.work(&f, 1, 1, in_buf, out_buf); } catch (const std::runtime_error &x) { threw = std::string(x.what()) == "libdvbt_hip: fake work failed"; }
    CHECK(threw && f.si_out_tags.empty() && f.si_consumed[0] == 0);
    CHECK(R.destroys == 0);
  }
  CHECK(R.destroys == 1 && R.creates == 2);                                            // the handle goes with its owner, once

  printf("hip_shell core: %d works, %d errors\n", R.works, errors);
  return errors ? 1 : 0;
}
