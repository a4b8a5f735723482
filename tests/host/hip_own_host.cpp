// hip_own_host.cpp -- the owners of gr_dvbt_amd/csrc/hip_own.hpp on the CPU: the few HIP entry points the header uses are counting stubs here (malloc / free plus a set
// of what is live), so every leak, double release and release of something never made shows in the counts printed at the end.  Linked against no HIP library.
#include "hip_own.hpp"
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <memory>
#include <set>
#include <utility>

using namespace hip_own;

static std::set<void *> g_live[4];                 // device memory, page-locked memory, streams, events
static long g_made = 0, g_invalid = 0, g_fail_at = 0, g_calls = 0;   // g_fail_at = k > 0: the k-th creation from now fails

static hipError_t make(int kind, void **out, size_t bytes)
{
  if (g_fail_at && ++g_calls == g_fail_at) { *out = nullptr; return hipErrorOutOfMemory; }
  *out = malloc(bytes ? bytes : 1);
  g_live[kind].insert(*out); g_made++;
  return hipSuccess;
}
static hipError_t unmake(int kind, void *p)
{
  if (!g_live[kind].erase(p)) { g_invalid++; return hipErrorInvalidValue; }   // not live: freed twice, or never made here
  free(p);
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return make(0, p, n); }
hipError_t hipFree(void *p) { return unmake(0, p); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return make(1, p, n); }
hipError_t hipHostFree(void *p) { return unmake(1, p); }
hipError_t hipStreamCreate(hipStream_t *s) { return make(2, (void **)s, 8); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make(2, (void **)s, 8); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return make(2, (void **)s, 8); }
hipError_t hipStreamDestroy(hipStream_t s) { return unmake(2, s); }
hipError_t hipEventCreate(hipEvent_t *e) { return make(3, (void **)e, 8); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(3, (void **)e, 8); }
hipError_t hipEventDestroy(hipEvent_t e) { return unmake(3, e); }
}

static long g_errors = 0;
static size_t live() { return g_live[0].size() + g_live[1].size() + g_live[2].size() + g_live[3].size(); }
#define EXPECT(c) do { if (!(c)) { g_errors++; printf("line %d: %s\n", __LINE__, #c); } } while (0)

// one owner type O, filled by fill(o): scope exit, reset, moves, reallocation
template <class O, class Fill> static void exercise(Fill fill)
{
  const size_t base = live();
  { O a; EXPECT(!a); EXPECT(fill(a) == hipSuccess); EXPECT(a); EXPECT(live() == base + 1); }
  EXPECT(live() == base);                                                     // scope exit
  { O a; a.reset(); EXPECT(!a); fill(a); a.reset(); EXPECT(!a && live() == base); a.reset(); }   // reset: empty, full, empty again
  { O a; fill(a); auto raw = a.get(); O b(std::move(a)); EXPECT(!a && b.get() == raw && live() == base + 1); }   // move construction
  EXPECT(live() == base);
  { O a, b; fill(a); fill(b); auto raw = a.get(); b = std::move(a); EXPECT(!a && b.get() == raw && live() == base + 1); }   // move assignment, full into full
  EXPECT(live() == base);
  { O a, b; fill(a); a = std::move(b); EXPECT(!a && !b && live() == base); }  // ... empty into full
  { O a; fill(a); auto raw = a.get(); O &r = a; a = std::move(r); EXPECT(a.get() == raw && live() == base + 1); }   // ... into itself
  EXPECT(live() == base);
  { O a; fill(a); fill(a); EXPECT(a && live() == base + 1); }                 // a full owner filled again
  EXPECT(live() == base);
  { O a; fill(a); g_fail_at = 1; g_calls = 0; EXPECT(fill(a) != hipSuccess); g_fail_at = 0; EXPECT(!a && live() == base); }   // a failed refill leaves it empty
}

// the streaming entry's device chunks: move-only elements that own memory, in deques
struct Chunk { long label = 0; uint8_t *data = nullptr; DevMem<uint8_t> stolen, own; };
static void deque_pattern()
{
  const size_t base = live();
  {
    std::deque<Chunk> fifo, zombie;
    for (int i = 0; i < 9; i++) {
      Chunk c; c.label = i;
      if (i % 3 == 0) { c.stolen.alloc(64); c.data = c.stolen + 8; } else if (i % 3 == 1) { c.own.alloc(32); c.data = c.own; }
      fifo.push_back(std::move(c));
    }
    EXPECT(live() == base + 6);
    for (int i = 0; i < 5; i++) { zombie.push_back(std::move(fifo.front())); fifo.pop_front(); }
    EXPECT(live() == base + 6);
    fifo.push_front(std::move(zombie.back())); zombie.pop_back();           // a run taken back
    EXPECT(fifo.front().label == 4 && live() == base + 6);
    std::deque<DevMem<uint8_t>> pool;
    while (!zombie.empty()) {
      Chunk c = std::move(zombie.front()); zombie.pop_front();
      if (c.stolen) pool.push_back(std::move(c.stolen));                    // back to the pool; c.own goes with c
    }
    EXPECT(pool.size() == 2 && live() == base + 2 + 3);                     // two in the pool; chunks 4, 6 and 7 still own theirs in fifo
  }
  EXPECT(live() == base);
}

// the create functions: a handle of several owners behind a unique_ptr, abandoned when its k-th creation fails
struct Handle {
  Stream s; Event ev[2]; PinMem<int> host; DevMem<float> a, b[3]; DevMem<uint8_t> c;
  hipError_t build()
  {
    hipError_t e;
    if ((e = s.create(0u, 1)) || (e = ev[0].create()) || (e = ev[1].create(2u)) || (e = host.alloc(4)) || (e = a.alloc(100))) return e;
    for (auto &q : b) if ((e = q.alloc(10))) return e;
    return c.alloc(1000);
  }
};
static int create(Handle **out)
{
  std::unique_ptr<Handle> h(new Handle());
  if (h->build() != hipSuccess) return -1;
  *out = h.release();
  return 0;
}
static void create_pattern()
{
  const size_t base = live();
  const long before = g_made;
  Handle *h = nullptr;
  EXPECT(create(&h) == 0 && h);
  const long n = g_made - before;
  EXPECT(n == 9 && live() == base + 9);
  delete h;
  EXPECT(live() == base);
  for (long k = 1; k <= n; k++) {
    h = nullptr; g_fail_at = k; g_calls = 0;
    EXPECT(create(&h) == -1 && !h);
    g_fail_at = 0;
    EXPECT(live() == base);
  }
}

int main()
{
  exercise<DevMem<float>>([](DevMem<float> &m) { return m.alloc(17); });
  exercise<PinMem<int>>([](PinMem<int> &m) { return m.alloc(5); });
  exercise<Stream>([](Stream &s) { return s.create(); });
  exercise<Stream>([](Stream &s) { return s.create(1u); });
  exercise<Stream>([](Stream &s) { return s.create(1u, -1); });
  exercise<Event>([](Event &e) { return e.create(); });
  exercise<Event>([](Event &e) { return e.create(2u); });
  { DevMem<int> m; m.alloc(4); int *p = m; p[3] = 7; EXPECT(m[3] == 7 && *(m + 3) == 7 && m + 4 > m.get()); }   // the raw pointer's arithmetic, through the conversion
  deque_pattern();
  create_pattern();
  printf("%ld allocations, %zu live, %ld invalid releases, %ld errors\n", g_made, live(), g_invalid, g_errors);
  return 0;
}
