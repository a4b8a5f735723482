/*
 * ref_driver.cc -- drives the reference's own blocks, compiled unmodified, without a scheduler.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile target `ref`, tests/test_oracle_ref_blocks.py).
 * A block is made by name through its own make(...); forecast and general_work / work run on
 * caller-supplied buffers, item counts and input tags; the caller gets back the items produced,
 * the items consumed per input and the output tags.  The scheduler's part that remains -- item
 * counters advancing by what was consumed and produced -- is done here, behind each call.
 * The stand-in headers under ref_standin/ supply gr::block (see block.h there).
 *
 * With REF_DRIVER_HIP_SHELLS defined the same driver is compiled with the block sources of gr_dvbt_amd/host/gr in place of the reference's
 * (oracle/_ref/libdvbt_shells_hip.so, tests/test_gpu_gr_shells.py): the block classes are then the HIP shells.  Everything that exists only for them
 * stands under that one switch; without it this file is what it was.
 */
#include <dvbt/bit_inner_deinterleaver.h>
#include <dvbt/bit_inner_interleaver.h>
#include <dvbt/convolutional_deinterleaver.h>
#include <dvbt/convolutional_interleaver.h>
#include <dvbt/demod_reference_signals.h>
#include <dvbt/dvbt_demap.h>
#include <dvbt/dvbt_map.h>
#include <dvbt/energy_descramble.h>
#include <dvbt/energy_dispersal.h>
#include <dvbt/inner_coder.h>
#include <dvbt/reed_solomon_dec.h>
#include <dvbt/reed_solomon_enc.h>
#include <dvbt/reference_signals.h>
#include <dvbt/symbol_inner_interleaver.h>
#include <dvbt/viterbi_decoder.h>

#ifdef REF_DRIVER_HIP_SHELLS
#include <dvbt/ofdm_sym_acquisition.h>
#include <dvbt/fft_hip.h>
#include <dvbt/rx_hip.h>
#include <gnuradio/block_detail.h>
#include <stdexcept>
/* a shell throws std::runtime_error where the library refuses; nothing may throw through extern "C": the message is kept, the call returns `ret` */
static thread_local std::string si_error;
#define SHELL_TRY try {
#define SHELL_CATCH(ret) } catch (const std::exception &e) { si_error = e.what(); return ret; }
#else
#define SHELL_TRY
#define SHELL_CATCH(ret)
#endif

#include <algorithm>
#include <fcntl.h>
#include <unistd.h>

using namespace gr::dvbt;

namespace {
  struct handle {
    gr::block_sptr blk;
  };

  template <class E> E en(int v) { return static_cast<E>(v); }

  /* the blocks print their parameters and progress to stdout: not while a test runs */
  struct quiet {
    int saved;
    quiet() : saved(-1)
    {
      fflush(stdout);
      int nul = open("/dev/null", O_WRONLY);
      if (nul >= 0) { saved = dup(1); dup2(nul, 1); close(nul); }
    }
    ~quiet()
    {
      fflush(stdout);
      if (saved >= 0) { dup2(saved, 1); close(saved); }
    }
  };
}

extern "C" {

/* a: the integer arguments of the block's make(), in its own order; g: its float argument (the mapper's gain), if it has one.
 * returns 0 for an unknown name or a wrong argument count */
void *refblk_make(const char *name, const int *a, int na, float g)
{
  std::string n(name);
  gr::block_sptr b;
  quiet q;
  SHELL_TRY
  if (n == "demod_reference_signals" && na == 11)
    b = demod_reference_signals::make(a[0], a[1], a[2], en<dvbt_constellation_t>(a[3]), en<dvbt_hierarchy_t>(a[4]), en<dvbt_code_rate_t>(a[5]),
                                      en<dvbt_code_rate_t>(a[6]), en<dvbt_guard_interval_t>(a[7]), en<dvbt_transmission_mode_t>(a[8]), a[9], a[10]);
  else if (n == "reference_signals" && na == 11)
    b = reference_signals::make(a[0], a[1], a[2], en<dvbt_constellation_t>(a[3]), en<dvbt_hierarchy_t>(a[4]), en<dvbt_code_rate_t>(a[5]),
                                en<dvbt_code_rate_t>(a[6]), en<dvbt_guard_interval_t>(a[7]), en<dvbt_transmission_mode_t>(a[8]), a[9], a[10]);
  else if (n == "dvbt_demap" && na == 4)
    b = dvbt_demap::make(a[0], en<dvbt_constellation_t>(a[1]), en<dvbt_hierarchy_t>(a[2]), en<dvbt_transmission_mode_t>(a[3]), g);
  else if (n == "dvbt_map" && na == 4)
    b = dvbt_map::make(a[0], en<dvbt_constellation_t>(a[1]), en<dvbt_hierarchy_t>(a[2]), en<dvbt_transmission_mode_t>(a[3]), g);
  else if (n == "symbol_inner_interleaver" && na == 3)
    b = symbol_inner_interleaver::make(a[0], en<dvbt_transmission_mode_t>(a[1]), a[2]);
  else if (n == "bit_inner_deinterleaver" && na == 4)
    b = bit_inner_deinterleaver::make(a[0], en<dvbt_constellation_t>(a[1]), en<dvbt_hierarchy_t>(a[2]), en<dvbt_transmission_mode_t>(a[3]));
  else if (n == "bit_inner_interleaver" && na == 4)
    b = bit_inner_interleaver::make(a[0], en<dvbt_constellation_t>(a[1]), en<dvbt_hierarchy_t>(a[2]), en<dvbt_transmission_mode_t>(a[3]));
  else if (n == "viterbi_decoder" && na == 6)
    b = viterbi_decoder::make(en<dvbt_constellation_t>(a[0]), en<dvbt_hierarchy_t>(a[1]), en<dvbt_code_rate_t>(a[2]), a[3], a[4], a[5]);
  else if (n == "inner_coder" && na == 5)
    b = inner_coder::make(a[0], a[1], en<dvbt_constellation_t>(a[2]), en<dvbt_hierarchy_t>(a[3]), en<dvbt_code_rate_t>(a[4]));
  else if (n == "convolutional_deinterleaver" && na == 3)
    b = convolutional_deinterleaver::make(a[0], a[1], a[2]);
  else if (n == "convolutional_interleaver" && na == 3)
    b = convolutional_interleaver::make(a[0], a[1], a[2]);
  else if (n == "reed_solomon_dec" && na == 8)
    b = reed_solomon_dec::make(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
  else if (n == "reed_solomon_enc" && na == 8)
    b = reed_solomon_enc::make(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
  else if (n == "energy_descramble" && na == 1)
    b = energy_descramble::make(a[0]);
  else if (n == "energy_dispersal" && na == 1)
    b = energy_dispersal::make(a[0]);
#ifdef REF_DRIVER_HIP_SHELLS
  else if (n == "ofdm_sym_acquisition" && na == 4)
    b = ofdm_sym_acquisition::make(a[0], a[1], a[2], a[3], g);
  else if (n == "fft_hip" && na == 3)
    b = fft_hip::make(a[0], a[1] != 0, a[2] != 0);
  else if (n == "rx_hip" && na == 8)
    b = rx_hip::make(en<dvbt_constellation_t>(a[0]), en<dvbt_hierarchy_t>(a[1]), en<dvbt_code_rate_t>(a[2]), en<dvbt_guard_interval_t>(a[3]),
                     en<dvbt_transmission_mode_t>(a[4]), g, a[5], a[6], a[7] != 0);
  else
    si_error = "no block " + n + " with " + std::to_string(na) + " integer arguments";
  if (b)
    b->si_detail = gr::block_detail_sptr(new gr::block_detail(b->input_signature()->max_streams()));
#endif
  SHELL_CATCH(0)
  if (!b)
    return 0;
  handle *h = new handle;
  h->blk = b;
  return h;
}

void refblk_free(void *hv) { delete static_cast<handle *>(hv); }

/* what the block asked of the scheduler in its constructor */
int refblk_output_multiple(void *hv) { return static_cast<handle *>(hv)->blk->output_multiple(); }
double refblk_relative_rate(void *hv) { return static_cast<handle *>(hv)->blk->relative_rate(); }
int refblk_itemsize(void *hv, int output)
{
  gr::block &b = *static_cast<handle *>(hv)->blk;
  return (output ? b.output_signature() : b.input_signature())->sizeof_stream_item(0);
}

/* forecast(noutput) -> req[0..ninputs) */
void refblk_forecast(void *hv, int noutput, int *req, int ninputs)
{
  gr_vector_int r(ninputs, 0);
  static_cast<handle *>(hv)->blk->forecast(noutput, r);
  for (int i = 0; i < ninputs; i++)
    req[i] = r[i];
}

/* a tag on input `input` at absolute item offset `offset` */
void refblk_add_input_tag(void *hv, int input, unsigned long long offset, const char *key, long value)
{
  gr::block &b = *static_cast<handle *>(hv)->blk;
  if ((size_t)input >= b.si_in_tags.size())
    b.si_in_tags.resize(input + 1);
  gr::tag_t t{offset, pmt::string_to_symbol(key), pmt::from_long(value), pmt::pmt_t()};
  std::vector<gr::tag_t> &v = b.si_in_tags[input];
  v.insert(std::upper_bound(v.begin(), v.end(), t, gr::tag_t::offset_compare), t);
}

unsigned long long refblk_nitems_read(void *hv, int input) { return static_cast<handle *>(hv)->blk->nitems_read(input); }
unsigned long long refblk_nitems_written(void *hv, int output) { return static_cast<handle *>(hv)->blk->nitems_written(output); }

/* one general_work call: in[i] exposes ninput_items[i] items from absolute item nitems_read(i) on, out[j] has room for noutput items.
 * returns what the call returned; consumed[i] = what it consumed.  Afterwards the counters stand where a scheduler would have them. */
int refblk_work(void *hv, int noutput, const int *ninput_items, const void *const *in, int nin, void *const *out, int nout, int *consumed)
{
  gr::block &b = *static_cast<handle *>(hv)->blk;
  gr_vector_int ni(ninput_items, ninput_items + nin);
  gr_vector_const_void_star iv(in, in + nin);
  gr_vector_void_star ov(out, out + nout);
  b.si_consumed.assign(std::max<size_t>(nin, b.si_consumed.size()), 0);
  if (b.si_nread.size() < (size_t)nin) b.si_nread.resize(nin, 0);
  if (b.si_nwritten.size() < (size_t)nout) b.si_nwritten.resize(nout, 0);
  int r;
  {
    quiet q;
    SHELL_TRY
    r = b.general_work(noutput, ni, iv, ov);
    SHELL_CATCH(-1000)
  }
  for (int i = 0; i < nin; i++) {
    consumed[i] = b.si_consumed[i];
    b.si_nread[i] += b.si_consumed[i];
  }
  if (r > 0)
    for (int j = 0; j < nout; j++)
      b.si_nwritten[j] += r;
  return r;
}

/* output tags, in the order the block added them */
int refblk_n_output_tags(void *hv) { return (int)static_cast<handle *>(hv)->blk->si_out_tags.size(); }
int refblk_output_tag(void *hv, int i, int *port, unsigned long long *offset, char *key, int keycap, long *value)
{
  gr::block &b = *static_cast<handle *>(hv)->blk;
  if (i < 0 || (size_t)i >= b.si_out_tags.size())
    return -1;
  const gr::tag_t &t = b.si_out_tags[i];
  *port = b.si_out_tag_port[i];
  *offset = t.offset;
  snprintf(key, keycap, "%s", pmt::symbol_to_string(t.key).c_str());
  *value = pmt::to_long(t.value);
  return 0;
}

#ifdef REF_DRIVER_HIP_SHELLS
/* what() of the last exception that refblk_make (returned 0) or refblk_work (returned -1000) caught on this thread */
const char *refblk_last_error(void) { return si_error.c_str(); }
int refblk_tag_propagation_policy(void *hv) { return (int)static_cast<handle *>(hv)->blk->tag_propagation_policy(); }
/* streams the block declared: output = 0 / 1 as in refblk_itemsize, which = 0 the fewest, 1 the most */
int refblk_nstreams(void *hv, int output, int which)
{
  gr::block &b = *static_cast<handle *>(hv)->blk;
  gr::io_signature::sptr s = output ? b.output_signature() : b.input_signature();
  return which ? s->max_streams() : s->min_streams();
}
/* the scheduler's view of input `input`: whether the block upstream has finished, and the items that wait unread */
void refblk_set_input_state(void *hv, int input, int done, int items)
{
  gr::buffer_reader_sptr r = static_cast<handle *>(hv)->blk->detail()->input(input);
  r->si_done = done != 0;
  r->si_items = items;
}
#endif

}
