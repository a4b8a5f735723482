// dvbt_rccl.inc -- the exchange step of a sharded stream inside the C ABI (SURVEY 8e; north_star: "C++ host code ... a single RCCL gather of decoded TS
// packets over xGMI").  Included by dvbt_hip.hip.
//
// The data path shards with no collective: every rank decodes its pieces of the one stream (dvbt_rx_stream_* with rank / world).  What remains is ONE exchange
// per step: each rank's run of finished packets travels to the root.  It is a gather of fixed-stride slots -- a 64-byte header {first packet index in the
// stream's TS, byte count, "this rank has nothing more to give", error} in front of the packets, exactly the buffers gr_dvbt_amd/multi.py defines for the Python
// host -- issued as ONE group of ncclSend / ncclRecv on device buffers (what ncclGather is; RCCL moves them over xGMI between the GPUs of a node); the 64-byte
// headers travel to EVERY rank inside the same group, so that every rank knows in the same step whether all streams are drained and whether a rank has failed
// (no second group, no control word).  What the root keeps of a step is its choice: the runs in its device memory (DVBT_GATHER_DEVICE -- north_star's clock ends at "last TS
// byte resident on rank 0"; nothing but the headers is downloaded) or, besides, a page-locked mirror that holds exactly the bytes the headers declare.  The step is asynchronous and double-buffered (dvbt_rx_stream_gather_enqueue / _wait: step k + 1 is issued on the
// communicator's own HIP stream while step k's packets are being consumed), and with dvbt_rx_stream_set_device_output the packets never touch the host on
// their way from a chain's TS buffer to the root.
// librccl is opened with dlopen at the first use: the library has no link-time dependency on it, and a host that never shards never loads it.  A host that
// does not want to link RCCL itself gets the communicator from here as well (dvbt_rccl_unique_id / dvbt_rccl_comm_create: ncclGetUniqueId / ncclCommInitRank).
#include <dlfcn.h>
#include <mutex>
#include <condition_variable>
#include <chrono>

namespace {

struct NcclId { char b[128]; };                                    // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value
struct Rccl {
  void *so = nullptr;
  int (*GetUniqueId)(NcclId *) = nullptr;
  int (*CommInitRank)(void **, int, NcclId, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
constexpr int kNcclUint8 = 1;                                      // ncclDataType_t::ncclUint8
constexpr size_t GATHER_HEADER = 64;                               // multi.py::HEADER_BYTES

Rccl *rccl()
{
  static Rccl R; static bool tried = false;
  if (tried) return R.so ? &R : nullptr;
  tried = true;
  for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { R.so = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (R.so) break; }
  if (!R.so) return nullptr;
#define RSYM(field, sym) R.field = reinterpret_cast<decltype(R.field)>(dlsym(R.so, sym)); if (!R.field) { R.so = nullptr; return nullptr; }
  RSYM(GetUniqueId, "ncclGetUniqueId") RSYM(CommInitRank, "ncclCommInitRank") RSYM(CommDestroy, "ncclCommDestroy") RSYM(GroupStart, "ncclGroupStart")
  RSYM(GroupEnd, "ncclGroupEnd") RSYM(Send, "ncclSend") RSYM(Recv, "ncclRecv") RSYM(GetErrorString, "ncclGetErrorString")
#undef RSYM
  return &R;
}
#define NCCLCHK(x) do { int e_ = (x); if (e_ != 0) return fail(DVBT_ERR_HIP, std::string(#x) + ": " + R->GetErrorString(e_)); } while (0)

// ---- A loopback transport (test hook: dvbt_rccl_comm_create_loopback).  The exchange step's world > 1 logic -- the slot to the root, the headers to every rank, the root's
// download of what the OTHER ranks' headers declare, a failing rank's error-flag slot -- needs more than one rank to run at all, and RCCL refuses two ranks on one device: a test box
// has one.  Here the ranks are THREADS of one process on one device; a send is a posted message (pointer, size, an event recorded behind the sender's stream), a receive waits for its
// message and copies device to device behind that event, a group ends when everything this rank posted has been taken.  Same call pattern as RCCL's (the Rccl table above), nothing of
// its transport: what it proves is the step's own logic, not RCCL.
struct LoopGroup {
  std::mutex m; std::condition_variable cv; int world = 1, refs = 0;
  struct Msg { int src, dst; const void *ptr; size_t n; bool consumed = false; Event ready, taken; };
  std::deque<Msg *> posted;
};
struct LoopEnd { LoopGroup *g; int rank; };
struct LoopOp { bool send; void *buf; size_t n; int peer; LoopEnd *e; hipStream_t st; };
thread_local std::vector<LoopOp> loop_ops; thread_local bool loop_in_group = false;
int loop_group_start() { loop_in_group = true; loop_ops.clear(); return 0; }
int loop_send(const void *buf, size_t n, int, int peer, void *comm, hipStream_t st) { loop_ops.push_back(LoopOp{true, const_cast<void *>(buf), n, peer, (LoopEnd *)comm, st}); return 0; }
int loop_recv(void *buf, size_t n, int, int peer, void *comm, hipStream_t st) { loop_ops.push_back(LoopOp{false, buf, n, peer, (LoopEnd *)comm, st}); return 0; }
int loop_group_end()
{
  loop_in_group = false;
  std::vector<LoopGroup::Msg *> mine;
  int rc = 0;
  // post every send first (a rank's receives may depend on a peer that is waiting for this rank's sends)
  for (LoopOp &o : loop_ops) if (o.send) {
    LoopGroup::Msg *m = new LoopGroup::Msg{o.e->rank, o.peer, o.buf, o.n};
    if (m->ready.create(hipEventDisableTiming) != hipSuccess || m->taken.create(hipEventDisableTiming) != hipSuccess ||
        hipEventRecord(m->ready, o.st) != hipSuccess) rc = 1;
    { std::lock_guard<std::mutex> lk(o.e->g->m); o.e->g->posted.push_back(m); }
    o.e->g->cv.notify_all();
    mine.push_back(m);
  }
  // the receives, in order: the oldest message of the pair (src -> this rank)
  for (LoopOp &o : loop_ops) if (!o.send) {
    LoopGroup *g = o.e->g; LoopGroup::Msg *m = nullptr;
    std::unique_lock<std::mutex> lk(g->m);
    const bool ok = g->cv.wait_for(lk, std::chrono::seconds(60), [&] {
      for (LoopGroup::Msg *q : g->posted) if (!q->consumed && q->src == o.peer && q->dst == o.e->rank) { m = q; return true; }
      return false; });
    if (!ok) { rc = 2; continue; }                                  // (a peer that never posts: the hang RCCL would show, reported instead)
    m->consumed = true;
    lk.unlock();
    if (m->n != o.n) rc = 3;                                        // (a size mismatch: undefined behaviour under RCCL)
    else if (hipStreamWaitEvent(o.st, m->ready, 0) != hipSuccess || hipMemcpyAsync(o.buf, m->ptr, o.n, hipMemcpyDeviceToDevice, o.st) != hipSuccess ||
             hipEventRecord(m->taken, o.st) != hipSuccess) rc = 1;
    { std::lock_guard<std::mutex> lk2(g->m); m->n = (size_t)-1; }   // taken: its `taken` event is recorded
    g->cv.notify_all();
  }
  // everything this rank posted must have been taken before its buffers may be reused: its stream waits behind the takers' copies
  for (size_t i = 0; i < mine.size(); i++) {
    LoopGroup::Msg *m = mine[i];
    LoopOp *op = nullptr; { size_t k = 0; for (LoopOp &o : loop_ops) if (o.send) { if (k == i) op = &o; k++; } }
    LoopGroup *g = op->e->g;
    std::unique_lock<std::mutex> lk(g->m);
    const bool ok = g->cv.wait_for(lk, std::chrono::seconds(60), [&] { return m->n == (size_t)-1; });
    for (auto it = g->posted.begin(); it != g->posted.end(); ++it) if (*it == m) { g->posted.erase(it); break; }
    lk.unlock();
    if (!ok) rc = 2; else if (hipStreamWaitEvent(op->st, m->taken, 0) != hipSuccess) rc = 1;
    if (ok) delete m;   // (a message nobody took stays posted: the test has failed anyway)
  }
  loop_ops.clear();
  return rc;
}
const char *loop_error_string(int e) { return e == 2 ? "loopback: a peer did not post its part of the group within 60 s" : e == 3 ? "loopback: send / receive sizes differ" : "loopback: HIP error"; }
int loop_comm_destroy(void *comm) { LoopEnd *e = (LoopEnd *)comm; bool last; { std::lock_guard<std::mutex> lk(e->g->m); last = --e->g->refs == 0; } if (last) delete e->g; delete e; return 0; }
Rccl *loop_rccl()
{
  static Rccl R;
  R.so = (void *)1; R.GroupStart = loop_group_start; R.GroupEnd = loop_group_end; R.Send = loop_send; R.Recv = loop_recv; R.GetErrorString = loop_error_string; R.CommDestroy = loop_comm_destroy;
  return &R;
}

}  // namespace

struct dvbt_rccl_comm {
  // Members are released in reverse order of declaration: the stream and the events stand in front of the buffers the steps queued on them use, so the buffers go
  // first and the stream last (dvbt_rccl_comm_destroy has drained the stream and destroyed the communicator before that).  last_view / last_dev_view are views.
  void *comm = nullptr; int rank = 0, world = 1, device = 0; Stream st; Event ev[2];
  size_t slot = 0;
  // double-buffered.  Persistent from dvbt_rccl_comm_create on (a step can always exchange its headers): hdr_dev -- this rank's 64-byte header on the device, hdrs --
  // every rank's, and their page-locked mirrors.  Sized by dvbt_rccl_comm_reserve: send -- this rank's slot, recv -- the root's `world` slots (root only), h_send --
  // the staging of a run that comes from the stream's host FIFO, h_recv -- the root's host mirror of the received runs (only when a step asks for it)
  DevMem<uint8_t> hdr_dev[2], hdrs[2]; PinMem<uint8_t> h_hdr[2], h_hdrs[2];
  DevMem<uint8_t> send[2], recv[2]; PinMem<uint8_t> h_send[2], h_recv[2];
  bool busy[2] = {false, false}; int root_of[2] = {0, 0}, flags_of[2] = {0, 0};
  bool staged[2] = {false, false}; int64_t staged_first[2] = {0, 0}, staged_n[2] = {0, 0};   // a run pulled from the host FIFO whose group failed: sent by the next step instead of lost
  long long seq_enq = 0, seq_wait = 0; const uint8_t *last_view = nullptr, *last_dev_view = nullptr;
  bool loopback = false; int debug_fail = 0;                      // test hooks: the loopback transport; the next `debug_fail` steps treat their buffers as not allocated
};
static Rccl *rccl_of(const dvbt_rccl_comm *c) { return c->loopback ? loop_rccl() : rccl(); }

// the root's download: of every rank's slot the header and the bytes its header says are filled -- not the slot (a slot is sized for the most a rank can ever give; at 8 GPUs
// whole slots were 7 x 75 MB per 4.5 ms step = 117 GB/s over a 44 GB/s link, VERDICT r05).  The fill is known on the device only, so a kernel does the copy: it
// reads the count out of the slot's header and writes 16-byte words straight into the page-locked mirror.  grid (x, world).  (Whatever does the copy, the mirror is bound by
// the root's PCIe link, 44 GB/s measured: the TS of three GPUs at the headline rate.  A root that must keep up with eight leaves the runs on the device.)
__global__ __launch_bounds__(256) void gather_download_kernel(const uint8_t *__restrict__ recv, uint8_t *__restrict__ host, size_t slot, int skip_rank)
{
  if ((int)blockIdx.y == skip_rank) return;                                              // (the root's own run has gone through the DMA engine: its size is known to the host)
  const uint8_t *src = recv + (size_t)blockIdx.y * slot; uint8_t *dst = host + (size_t)blockIdx.y * slot;
  long long n = reinterpret_cast<const long long *>(src)[1];
  if (n < 0 || (size_t)n > slot - GATHER_HEADER) n = 0;                                  // (a corrupt header is the waiter's to report: it sees the header)
  const size_t words = (GATHER_HEADER + (size_t)n + 15) / 16;                            // slots are multiples of 64 bytes: the last word stays inside
  const uint4 *s4 = reinterpret_cast<const uint4 *>(src); uint4 *d4 = reinterpret_cast<uint4 *>(dst);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) d4[i] = s4[i];
}

extern "C" int dvbt_rccl_unique_id(void *id128)
{
  if (!id128) return fail(DVBT_ERR_INVALID, "null argument");
  Rccl *R = rccl(); if (!R) return fail(DVBT_ERR_NO_DEVICE, "librccl.so could not be loaded");
  NCCLCHK(R->GetUniqueId((NcclId *)id128));
  return DVBT_OK;
}

static void rccl_free_buffers(dvbt_rccl_comm *c)
{
  for (int b = 0; b < 2; b++) { c->send[b].reset(); c->recv[b].reset(); c->h_send[b].reset(); c->h_recv[b].reset(); }
  c->slot = 0;
}

extern "C" void dvbt_rccl_comm_destroy(dvbt_rccl_comm *c)
{
  if (!c) return;
  Rccl *R = rccl_of(c);
  if (c->st) (void)hipStreamSynchronize(c->st);
  if (R && c->comm) R->CommDestroy(c->comm);
  delete c;
}

static int rccl_comm_finish_create(dvbt_rccl_comm *c);
extern "C" int dvbt_rccl_comm_create(const void *id128, int rank, int world, int device, dvbt_rccl_comm **out)
{
  if (!id128 || !out || world < 1 || rank < 0 || rank >= world) return fail(DVBT_ERR_INVALID, "bad communicator arguments");
  int r = need_device(); if (r) return r;
  Rccl *R = rccl(); if (!R) return fail(DVBT_ERR_NO_DEVICE, "librccl.so could not be loaded");
  HIPCHK(hipSetDevice(device));
  dvbt_rccl_comm *c = new dvbt_rccl_comm(); c->rank = rank; c->world = world; c->device = device;
  NcclId id; memcpy(&id, id128, sizeof id);
  int e = R->CommInitRank(&c->comm, world, id, rank);
  if (e != 0) { delete c; return fail(DVBT_ERR_HIP, std::string("ncclCommInitRank: ") + R->GetErrorString(e)); }
  r = rccl_comm_finish_create(c); if (r) return r;
  *out = c;
  return DVBT_OK;
}
static int rccl_comm_finish_create(dvbt_rccl_comm *c)
{
  const int world = c->world;
  bool ok = c->st.create() == hipSuccess;
  for (int b = 0; b < 2 && ok; b++)
    ok = c->ev[b].create(hipEventDisableTiming) == hipSuccess && c->hdr_dev[b].alloc(GATHER_HEADER) == hipSuccess &&
         c->hdrs[b].alloc(GATHER_HEADER * world) == hipSuccess && c->h_hdr[b].alloc(GATHER_HEADER) == hipSuccess &&
         c->h_hdrs[b].alloc(GATHER_HEADER * world) == hipSuccess;
  if (!ok) { dvbt_rccl_comm_destroy(c); return fail(DVBT_ERR_HIP, "dvbt_rccl_comm_create: stream / event / header buffers"); }
  return DVBT_OK;
}
// test hook: rank `rank` of a loopback group of `world` ranks that are threads of this process on one device.  *group: NULL on the first call (the group is created and returned),
// the returned value on the others.  dvbt_rccl_debug_fail_steps: the communicator's next n steps behave as if their exchange buffers could not be allocated.
extern "C" int dvbt_rccl_comm_create_loopback(void **group, int rank, int world, int device, dvbt_rccl_comm **out)
{
  if (!group || !out || world < 1 || rank < 0 || rank >= world) return fail(DVBT_ERR_INVALID, "bad communicator arguments");
  int r = need_device(); if (r) return r;
  HIPCHK(hipSetDevice(device));
  LoopGroup *g = (LoopGroup *)*group;
  if (!g) { g = new LoopGroup(); g->world = world; *group = g; }
  { std::lock_guard<std::mutex> lk(g->m); g->refs++; }
  dvbt_rccl_comm *c = new dvbt_rccl_comm(); c->rank = rank; c->world = world; c->device = device; c->loopback = true;
  c->comm = new LoopEnd{g, rank};
  r = rccl_comm_finish_create(c); if (r) return r;
  *out = c;
  return DVBT_OK;
}
extern "C" int dvbt_rccl_debug_fail_steps(dvbt_rccl_comm *c, int n) { if (!c) return fail(DVBT_ERR_INVALID, "null argument"); c->debug_fail = n; return DVBT_OK; }

// The exchange buffers for steps of `slot_packets` packets towards `root` (flags: the steps' flags; without DVBT_GATHER_DEVICE the root also gets its page-locked
// mirror).  dvbt_rx_stream_gather_enqueue calls it itself; a host that wants an allocation failure BEFORE any rank has entered a step calls it first, on every
// rank, and treats a failure as the job's.  No step may be in flight when the sizes change.
extern "C" int dvbt_rccl_comm_reserve(dvbt_rccl_comm *c, int root, int slot_packets, int flags)
{
  if (!c || slot_packets < 1 || root < 0 || root >= c->world) return fail(DVBT_ERR_INVALID, "bad reserve arguments");
  HIPCHK(hipSetDevice(c->device));
  const size_t slot = GATHER_HEADER + ((size_t)slot_packets * 188 + 63) / 64 * 64;
  if (slot != c->slot) {
    if (c->busy[0] || c->busy[1]) return fail(DVBT_ERR_STATE, "dvbt_rccl_comm_reserve: slot_packets changed while a step is in flight");
    if (c->staged[0] || c->staged[1]) return fail(DVBT_ERR_STATE, "dvbt_rccl_comm_reserve: a run whose step failed is still staged at the old size");
    rccl_free_buffers(c);
    for (int k = 0; k < 2; k++) { HIPCHK(c->send[k].alloc(slot)); HIPCHK(c->h_send[k].alloc(slot)); }
    c->slot = slot;
  }
  if (c->rank == root) for (int k = 0; k < 2; k++) {               // receive space on the root only
    if (!c->recv[k]) HIPCHK(c->recv[k].alloc(slot * c->world));
    if (!(flags & DVBT_GATHER_DEVICE) && !c->h_recv[k]) HIPCHK(c->h_recv[k].alloc(slot * c->world));
  }
  return DVBT_OK;
}

// ONE exchange step, issued and not waited for.  Every rank (collectively: the same root, slot_packets and flags everywhere) contributes the next contiguous run of
// its finished packets -- possibly none -- in a fixed-stride slot.  With dvbt_rx_stream_set_device_output the run is copied device to device from the stream's ring
// into the slot; otherwise it is pulled from the stream's host FIFO and copied up.  One group: the slot to the root, the 64-byte header to every rank.
// DVBT_GATHER_DEVICE: the runs stay in the root's device memory (north_star's clock ends at "last TS byte resident on rank 0"): nothing is downloaded but the headers.
// Otherwise the root's page-locked mirror receives every rank's header and the bytes that header says are filled (gather_download_kernel).
// Whatever fails on this rank in front of the group -- an allocation, the stream, a copy -- becomes a slot with the error flag in its header (sent from whatever
// device memory of the right size the rank has: the stream's sample buffer, if its own slot could not be allocated): the collective still completes everywhere and
// dvbt_rx_stream_gather_wait returns the failure on EVERY rank, no rank is left waiting in a receive.  (Only a rank with neither its slot nor a sample buffer of
// that size returns before the group: dvbt_rccl_comm_reserve moves that failure in front of the first step.)  A group that fails gives the run back to the stream.
// At most two steps may be in flight.
extern "C" int dvbt_rx_stream_gather_enqueue_ex(dvbt_rx_stream *s, dvbt_rccl_comm *c, int root, int slot_packets, int flags)
{
  if (!s || !c || slot_packets < 1 || root < 0 || root >= c->world || (flags & ~DVBT_GATHER_DEVICE)) return fail(DVBT_ERR_INVALID, "bad gather arguments");
  Rccl *R = rccl_of(c); if (!R) return fail(DVBT_ERR_NO_DEVICE, "librccl.so could not be loaded");
  HIPCHK(hipSetDevice(c->device));
  const size_t slot = GATHER_HEADER + ((size_t)slot_packets * 188 + 63) / 64 * 64;
  const int b = (int)(c->seq_enq & 1);
  if (c->busy[b]) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_gather_enqueue: two steps are in flight already (dvbt_rx_stream_gather_wait first)");
  if (slot != c->slot && (c->busy[0] || c->busy[1])) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_gather_enqueue: slot_packets changed while a step is in flight");
  int64_t first = 0, n = 0, err = 0;
  std::string why;
  if (dvbt_rccl_comm_reserve(c, root, slot_packets, flags) != DVBT_OK) { err = 1; why = g_err; }
  const bool dbg_fail = c->debug_fail > 0;                           // (test hook: as if the buffers were not there)
  if (dbg_fail) { c->debug_fail--; err = 1; why = "dvbt_rccl_debug_fail_steps"; }
  // where this rank's slot is sent from / where the root receives: its own buffers, or -- when they could not be allocated -- the stream's sample buffer (content void: err)
  const bool isroot = c->rank == root;
  uint8_t *fallback = (s->buf[0] && s->cap * sizeof(float2) >= slot) ? (uint8_t *)s->buf[0].get() : nullptr;
  uint8_t *sendp = c->slot == slot && c->send[b] && !dbg_fail ? c->send[b] : fallback;
  uint8_t *recvp = isroot ? (c->slot == slot && c->recv[b] && !dbg_fail ? c->recv[b] : nullptr) : nullptr;
  if (!sendp || (isroot && !recvp && !fallback)) return fail(DVBT_ERR_HIP, "dvbt_rx_stream_gather_enqueue: no exchange buffers (" + why + "): call dvbt_rccl_comm_reserve before the first step");
  // this rank's slot: header + the next run of its packets (the root's own slot needs no transport: it is built where the received ones land)
  uint8_t *mine = !err ? (isroot ? recvp + (size_t)c->rank * slot : sendp) : nullptr;
  DevTake tok;
  if (!err) {
    if (s->dev_out) { if (stream_take_device(s, mine + GATHER_HEADER, slot_packets, c->st, b, &first, &n, &tok) != DVBT_OK) { err = 1; n = 0; why = g_err; } }
    else if (c->staged[b]) { first = c->staged_first[b]; n = c->staged_n[b]; }               // (the run of a step whose group failed)
    else {
      n = dvbt_rx_stream_pull_chunk(s, c->h_send[b] + GATHER_HEADER, (size_t)slot_packets * 188, &first);
      if (n < 0) { err = 1; n = 0; why = g_err; } else { c->staged[b] = true; c->staged_first[b] = first; c->staged_n[b] = n; }
    }
  }
  dvbt_rx_stream_info inf; if (dvbt_rx_stream_status(s, &inf) != DVBT_OK) err = 1;
  const int64_t hdr[8] = {first, n, (!err && inf.finished && inf.ts_bytes_ready == 0) ? 1 : 0, err, c->seq_enq, 0, 0, 0};
  memcpy(c->h_hdr[b], hdr, sizeof hdr);
  // (page-locked sources: the copies are asynchronous; the staging is reused two steps on, behind this step's wait)
  hipError_t he = hipMemcpyAsync(c->hdr_dev[b], c->h_hdr[b], GATHER_HEADER, hipMemcpyHostToDevice, c->st);     // the header every rank receives
  if (he == hipSuccess && mine) {
    he = hipMemcpyAsync(mine, c->h_hdr[b], GATHER_HEADER, hipMemcpyHostToDevice, c->st);                        // ... and the copy in front of the run (multi.py's slot layout)
    if (he == hipSuccess && !s->dev_out && n > 0) he = hipMemcpyAsync(mine + GATHER_HEADER, c->h_send[b] + GATHER_HEADER, (size_t)n, hipMemcpyHostToDevice, c->st);
  }
  // the gather: one group of sends and receives on device buffers
  int e = R->GroupStart();
  if (!e && !isroot) e = R->Send(sendp, slot, kNcclUint8, root, c->comm, c->st);
  if (isroot) for (int r = 0; r < c->world && !e; r++) if (r != c->rank) e = R->Recv(recvp ? recvp + (size_t)r * slot : fallback, slot, kNcclUint8, r, c->comm, c->st);
  for (int r = 0; r < c->world && !e; r++) { e = R->Send(c->hdr_dev[b], GATHER_HEADER, kNcclUint8, r, c->comm, c->st); if (!e) e = R->Recv(c->hdrs[b] + (size_t)r * GATHER_HEADER, GATHER_HEADER, kNcclUint8, r, c->comm, c->st); }
  const int e2 = R->GroupEnd();                                    // (the group is closed whatever happened inside it)
  if (e || e2 || he != hipSuccess) {
    // nothing of this step has left the rank: the run goes back to the stream (device output) or stays staged for the next call (host FIFO)
    if (s->dev_out && !err) stream_untake_device(s, b, tok);
    if (he != hipSuccess) return fail(DVBT_ERR_HIP, std::string("gather: header copy: ") + hipGetErrorString(he));
    return fail(DVBT_ERR_HIP, std::string("RCCL gather: ") + R->GetErrorString(e ? e : e2));
  }
  c->staged[b] = false;
  if (isroot && recvp && !(flags & DVBT_GATHER_DEVICE) && c->h_recv[b]) {
    // the root's own run: its size is known here, the DMA engine takes it (no compute unit involved); the other ranks' fills are known on the device only
    HIPCHK(hipMemcpyAsync(c->h_recv[b] + (size_t)c->rank * slot, recvp + (size_t)c->rank * slot, GATHER_HEADER + (size_t)n, hipMemcpyDeviceToHost, c->st));
    if (c->world > 1) hipLaunchKernelGGL(gather_download_kernel, dim3(16, (unsigned)c->world), dim3(256), 0, c->st, (const uint8_t *)recvp, c->h_recv[b], slot, c->rank);
  }
  HIPCHK(hipMemcpyAsync(c->h_hdrs[b], c->hdrs[b], GATHER_HEADER * c->world, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipEventRecord(c->ev[b], c->st));
  c->busy[b] = true; c->root_of[b] = root; c->flags_of[b] = (isroot && !recvp) ? (flags | 0x100) : flags; c->seq_enq++;   // (0x100: the root had no receive space of its own -- the step's runs landed nowhere: it fails at the wait)
  if (err) g_err = "gather: this rank's slot carries the error flag: " + why;
  return DVBT_OK;
}
extern "C" int dvbt_rx_stream_gather_enqueue(dvbt_rx_stream *s, dvbt_rccl_comm *c, int root, int slot_packets) { return dvbt_rx_stream_gather_enqueue_ex(s, c, root, slot_packets, 0); }

// The OLDEST step in flight: waits for it.  root: chunks[world] describes the runs (from the headers every rank received).  Issued without flags: ts_host
// (cap >= world * slot_packets * 188 bytes) receives them in rank order, or, ts_host NULL, chunks[r].offset counts from dvbt_rccl_step_buffer (the step's page-locked
// mirror).  Issued with DVBT_GATHER_DEVICE: ts_host must be NULL, chunks[r].offset counts from dvbt_rccl_step_device_buffer (device memory).  Returns the runs' bytes.
// Others: ts_host / chunks may be NULL; returns 0.  *all_done (every rank) = 1 once every rank's stream is finished and drained.  A rank that failed in front of
// the step's group fails the step on every rank (DVBT_ERR_STATE).
extern "C" int64_t dvbt_rx_stream_gather_wait(dvbt_rx_stream *s, dvbt_rccl_comm *c, void *ts_host, size_t cap, dvbt_gather_chunk *chunks, int *all_done)
{
  if (!s || !c) return fail(DVBT_ERR_INVALID, "null argument");
  const int b = (int)(c->seq_wait & 1);
  if (!c->busy[b]) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_gather_wait: no step in flight");
  if (c->rank == c->root_of[b]) {                                    // (argument errors leave the step in flight)
    if (!chunks) return fail(DVBT_ERR_INVALID, "root needs chunks");
    if ((c->flags_of[b] & DVBT_GATHER_DEVICE) && ts_host) return fail(DVBT_ERR_INVALID, "gather: the step was issued with DVBT_GATHER_DEVICE: its runs are in device memory (ts_host must be NULL)");
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->ev[b]));
  c->busy[b] = false; c->seq_wait++;
  if (s->dev_out) stream_release_taken(s, b);
  int done = 1, err = 0;
  for (int r = 0; r < c->world; r++) { int64_t h[8]; memcpy(h, c->h_hdrs[b] + (size_t)r * GATHER_HEADER, sizeof h); if (!h[2]) done = 0; if (h[3]) err = 1; }
  if (all_done) *all_done = done;
  if (err || (c->flags_of[b] & 0x100)) return fail(DVBT_ERR_STATE, "gather: a rank failed in front of this step (its slot carries the error flag)");
  int64_t total = 0;
  if (c->rank == c->root_of[b]) {
    const bool on_device = (c->flags_of[b] & DVBT_GATHER_DEVICE) != 0;
    const uint8_t *got = c->h_recv[b];
    for (int r = 0; r < c->world; r++) {
      int64_t h[8]; memcpy(h, c->h_hdrs[b] + (size_t)r * GATHER_HEADER, sizeof h);
      if (h[1] < 0 || (size_t)h[1] > c->slot - GATHER_HEADER) return fail(DVBT_ERR_STATE, "gather: corrupt slot header");
      chunks[r].first_packet = h[0]; chunks[r].nbytes = h[1];
      if (ts_host) {
        if ((size_t)(total + h[1]) > cap) return fail(DVBT_ERR_CAPACITY, "gather: ts_host too small for the step's packets (world * slot_packets * 188 bytes are always enough)");
        memcpy((uint8_t *)ts_host + total, got + (size_t)r * c->slot + GATHER_HEADER, (size_t)h[1]);
        chunks[r].offset = total;
      } else chunks[r].offset = (int64_t)((size_t)r * c->slot + GATHER_HEADER);   // ts_host NULL: where the run sits in the step's own buffer (dvbt_rccl_step_buffer / _device_buffer)
      total += h[1];
    }
    c->last_view = on_device ? nullptr : got; c->last_dev_view = c->recv[b];
  }
  return total;
}

// root, dvbt_rx_stream_gather_wait(ts_host = NULL): the page-locked buffer the last waited step's runs sit in (chunks[r].offset counts from here); valid until the
// second next wait.  A root that writes the packets on (a file, a socket) needs no copy of its own: at the headline rate the TS is 15 GB/s, more than one host
// thread copies
extern "C" const void *dvbt_rccl_step_buffer(const dvbt_rccl_comm *c) { return c ? c->last_view : nullptr; }
// ... and the device buffer they arrived in (every step's runs are there, whatever its flags); valid until the second next wait
extern "C" const void *dvbt_rccl_step_device_buffer(const dvbt_rccl_comm *c) { return c ? c->last_dev_view : nullptr; }

// the step issued and waited for at once (the blocking form: one group, one synchronisation)
extern "C" int64_t dvbt_rx_stream_gather(dvbt_rx_stream *s, dvbt_rccl_comm *c, int root, int slot_packets, void *ts_host, size_t cap, dvbt_gather_chunk *chunks, int *all_done)
{
  if (!s || !c) return fail(DVBT_ERR_INVALID, "bad gather arguments");
  if (c->rank == root && (!ts_host || !chunks)) return fail(DVBT_ERR_INVALID, "root needs ts_host and chunks");
  if (c->rank == root && cap < (size_t)c->world * (size_t)slot_packets * 188) return fail(DVBT_ERR_CAPACITY, "gather: ts_host must hold world * slot_packets * 188 bytes");
  if (c->busy[0] || c->busy[1]) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_gather: steps issued with dvbt_rx_stream_gather_enqueue are still in flight");
  int r = dvbt_rx_stream_gather_enqueue(s, c, root, slot_packets); if (r) return r;
  return dvbt_rx_stream_gather_wait(s, c, ts_host, cap, chunks, all_done);
}
