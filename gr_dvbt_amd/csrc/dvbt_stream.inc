// dvbt_stream.inc -- dvbt_rx_stream_*: the whole chain behind ONE streaming entry (include/dvbt_hip.h).  Included by dvbt_hip.hip.
//
// Samples arrive in calls of any size (a GNU Radio work() call, a file read).  The result is, byte for byte, what one chain over the whole stream
// (dvbt_rx_segment_run on all samples at once, i.e. the reference's flowgraph) delivers -- through every loss of the CP lock.  Two modes:
//
// PIECES (the CP lock holds: the throughput path).  While the stream is inside ONE lock period of the reference's chain -- an EPOCH: from a superframe start
// that demod_reference_signals declared to the next lost lock -- it is cut into pieces of whole superframes with the pre- and post-roll of SURVEY 8e, every
// piece decoded device resident on one of two handles (own HIP stream each: the next piece's samples are copied in while the previous one decodes) and
// trimmed.  This is gr_dvbt_amd/multi.py's plan_cuts / stitch_plan restated in the library:
//   * piece k >= 1 of an epoch owns segment_superframes superframes; it begins STREAM_PRE (+ the epoch's delay mod 68) symbols before its first boundary (CP
//     lock + one whole TPS frame) on the epoch's call grid and ends stream_post() symbols + one acquisition window after its last one; dvbt_rx_set_cut makes its
//     roundings the epoch's;
//   * a piece is launched only when the stream is known to go on far enough for the NEXT piece to find its boundary by itself (STREAM_PRE + 272 symbols behind
//     its begin); at finish() the one piece that has not been launched is decoded to the end of the stream (as a walk window, below);
//   * the descrambler of the whole-stream chain runs in calls of two items (energy_descramble_impl.cc:121-141): the stream keeps the first packet of its next
//     call (`dc`); a piece delivers the calls that start in [its word 11, the next piece's word 11).  Every piece checks on the device that all those calls find
//     their NSYNC (the usual case: its packets are taken in whole groups); otherwise the host follows the descrambler call by call on the piece's sync bitmap.
//
// WALK (no lock period is established: the stream's beginning, and everything from a piece in which the CP lock was lost up to the next established epoch).
// The reference restarts the acquisition after one missed peak (ofdm_sym_acquisition_impl.cc:545-559), demod_reference_signals hunts the superframe start again
// ON COUNTERS THAT WENT ON COUNTING THROUGH THE GAP (demod_reference_signals_impl.cc:115-136; the pilot engine's members live on), the Viterbi decoder is reset
// at the tag (viterbi_decoder_impl.cc:213-229), the byte de-interleaver realigned but not cleared (convolutional_deinterleaver_impl.cc:109-120), the
// descrambler searches again (energy_descramble_impl.cc:121-141).  None of that can be cut into independent pieces: the stream is walked window by window
// (walk_window: the one lock-period walk, which dvbt_rx_segment_run calls for a whole segment, here with the blocks' state carried from window to window), synchronously, on handle 0:
//   * a window = the samples from the search position of the first lock period that is not final yet to the end of what has been pushed; the periods that are
//     final are decoded and appended to the walk's Viterbi stream; the last period that has items is handed to the next window (its end lies in samples to come);
//   * behind every window A8 + A9 run over the words of the Viterbi stream that are final and the host follows the descrambler over them (walk_flush); the
//     stream's tail (11 words of de-interleaver history, the descrambler's four-item look-ahead) stays in the handle, compacted in multiples of 64 words;
//   * an OPEN period (the lock holds to the window's end) that has found its superframe start and holds at least two superframes behind it ESTABLISHES an
//     epoch: the window becomes its head, pieces take over from its first boundary that lies a superframe + a window in front of the samples' end.  The
//     epoch's superframe grid is the one the reference's chain counts on: where the hunt fired on stale counters, `delay` symbols behind a transmitted
//     superframe start, the epoch's pieces deliver from that symbol too (dvbt_rx_cut.start_delay_symbols) -- the reference decodes garbage there until the next
//     loss, and so does the stream, byte for byte on a clean signal;
//   * a piece in which the lock is lost (reported by its asynchronous decode, or a piece whose decode found no superframe start) is decoded again by the walk, which
//     starts at that piece's begin -- with the pilot engine's counters preset to the epoch's (the piece begins inside a lock period whose counters are the
//     transmitted ones), the piece's cut, and the descrambler's call phase -- over all samples pushed since; pieces in flight behind it are dropped.
// What a piece assumes: the CP tracker of a chain that starts STREAM_PRE symbols in front of a boundary has settled on the positions of the chain that has
// been tracking all along by the time the boundary comes (true on every stream of the test suite, noise included; the tracker's next position depends on
// the previous one and the samples only).
//
// SHARDING (SURVEY 8e; rank / world in the parameters): every rank is pushed the same stream and walks its beginning (the plan; rank 0 delivers the head);
// piece k >= 1 of the epoch belongs to rank k % world, which alone copies its samples to the device and decodes it.  What a rank pulls is its pieces' packets
// with their packet index in the stream (dvbt_rx_stream_pull_chunk); the chunks of all ranks, ordered by that index, are the single chain's TS -- the one
// exchange step (an RCCL gather over xGMI in bench.py / gr_dvbt_amd/multi.py / dvbt_rx_stream_gather) is the host's.  A lock lost inside a rank's piece is
// walked to the end of THAT piece's samples (the other ranks own what follows and cannot know): the result is the single chain's whenever the reference's
// chain is back in a lock period on the transmitted superframe grid by the next piece's begin; otherwise status bit 5 is raised (world > 1 only).
// No resampler in front.

namespace {

constexpr int STREAM_PRE = 76;          // gr_dvbt_amd/multi.py::PRE_SYMBOLS
constexpr int STREAM_PIN_SLOTS = 32;    // pinned staging ring of dvbt_rx_stream_push: slots ...
constexpr size_t STREAM_PIN_BYTES = 1u << 20;   // ... of this many bytes (131,072 samples; a 4-symbol call at 8k is 270 KB)
constexpr size_t STREAM_DIRECT_BYTES = 2u << 20; // pushes of at least this much bypass the ring (a 64-symbol call at 8k is 4.3 MB)
constexpr long long WALK_HIST = 64;     // samples kept in front of a walk window's first search position (a tracking window at the left edge of its call reads up to 8 + margin)
constexpr long long WALK_KEEP_WORDS = 2048;   // the walk's Viterbi stream is compacted when the descrambler has left this many RS words behind

struct StreamPiece {
  long long index = 0;                  // 1, 2, ... within the epoch (0: unused)
  int handle = -1;                      // which of the two chains decodes it (its samples sit in buf[handle])
  long long begin = 0, end = 0;         // samples of the stream (end: where its own span ends)
  long long launch_at = 0;              // stream position from which it may be launched as a non-final piece
  long long first_sf = 0, count = 0;    // superframes it owns, counted from the epoch's first superframe start
  long long n = 0;                      // samples decoded
  long long skip = 0;                   // samples at the front of its span that its chain leaves out (a fresh acquisition that drops its lock at once is started a symbol later)
  int phase = 0;                        // dvbt_rx_cut.descr_call_phase it was enqueued with
  dvbt_rx_report rep;
};

// a run of decoded packets waiting to be pulled: in the handle's pinned TS ring (the usual case: the D2H copy is a DMA at full rate) or, when the ring is full
// (a consumer that has fallen far behind), on the heap
struct StreamChunk { long long first_packet; const uint8_t *data; size_t len; bool in_ring; std::vector<uint8_t> heap; };
constexpr size_t STREAM_TS_RING_DEFAULT = 96u << 20;             // ~24 s of the fastest DVB-T transport stream; a chunk is a piece's output (a few MB)

// device output (dvbt_rx_stream_set_device_output): a run of decoded packets in the stream's device ring, waiting for dvbt_rx_stream_gather_enqueue
struct TsBuf { DevMem<uint8_t> mem; size_t cap = 0; };            // a handle's TS buffer away from its handle, with its capacity
// Move-only: `data` is a view -- into the stream's ring (in_ring: nothing owned), into `stolen` (a handle's former TS buffer: back to the pool when released) or of `own`
// (the chunk's overflow allocation: released with the chunk)
struct DevChunk { long long first_packet; uint8_t *data; size_t len, off; bool in_ring; TsBuf stolen; DevMem<uint8_t> own; };

// energy_descramble's state between two calls: the item the next call starts at (always even: a call consumes two) and its offset in packets (d_index / 188)
struct DescrState { long long base = 0; int dp = 0; long long start() const { return base * 8 + dp; } };

}  // namespace

struct dvbt_rx_stream {
  // Members are released in reverse order of declaration: the events stand in front of the chains and of every buffer that copies recorded on them use, so the
  // buffers and the chains (with their HIP streams) go first and the events last.  wb, DevChunk::data, StreamChunk::data and Region::ptr are views.
  dvbt_rx_stream_params prm; Dims d;
  int rank = 0, world = 1;
  static constexpr int MAXH = 4;                               // chains (handle + sample buffer + HIP stream) a stream object can have: dvbt_rx_stream_params.chains
  int nh = 2;                                                  // ... and has: the pieces take them in turn, nh - 1 pieces decode while the next one fills
  Event ev_written[MAXH], ev_copied[MAXH], pin_ev[STREAM_PIN_SLOTS], ev_direct;   // (pin_ev, ev_direct: the host pushes', below)
  std::unique_ptr<dvbt_rx> rx[MAXH];
  DevMem<float2> buf[MAXH]; size_t cap = 0;                    // sample buffers, one per handle
  // host pushes leave through a ring of pinned staging slots: memcpy into a slot, asynchronous H2D on the piece's stream, return.  A push never waits for the
  // device unless the ring has gone round (STREAM_PIN_SLOTS x STREAM_PIN_BYTES of samples are in flight in front of a busy chain: back-pressure).  Allocated at
  // the first host push (a stream fed from device memory never needs it)
  PinMem<uint8_t> pin; bool pin_busy[STREAM_PIN_SLOTS] = {}; int pin_next = 0;
  // ... large pushes (>= STREAM_DIRECT_BYTES) are copied straight out of the caller's buffer (the runtime pins the pages: no staging memcpy, which a single
  // host thread cannot do faster than ~20 GB/s); the call then waits for that copy, as the caller's buffer must be free when it returns
  bool direct_pending = false;
  long long pos = 0;                                           // samples pushed so far
  // borrow_device_pushes: the samples handed to dvbt_rx_stream_push_device are NOT copied: the stream remembers where they are (regions of the stream in the caller's
  // device memory, neighbours merged) and reads them there -- a piece that lies in one region is decoded in place, everything else (a piece across two regions, the
  // walk's windows) is gathered from the regions when it is needed.  The caller keeps a region valid and unchanged until samples_released has passed it
  struct Region { long long pos0; const float2 *ptr; long long n; };
  bool borrow = false; std::deque<Region> regions; long long wb_filled = 0, released = 0;   // (wb_filled: stream position up to which the walk's buffer holds samples)
  long long L = 0, win = 0, post = 0, wsf = 0, ibits = 0, thr = 0, len0 = 0;
  bool finished = false;
  // ---- the epoch (PIECES)
  bool in_pieces = false; long long epoch_id = 0;             // (epoch_id: counts the walks that took over: a plan made before one is void after it)
  long long grid0 = 0, sf_call = 0, count0 = 0;                // call grid origin (stream sample), call of the epoch's superframe start, superframes of its head
  int delay = 0;                                               // dvbt_rx_cut.start_delay_symbols of the epoch's pieces
  long long cp0 = 0;                                           // d_cp_start of the head's acquisition (with grid0 / sf_call: the sample of the epoch's superframe start)
  long long dc = 0; bool dc_valid = false;                     // first packet of the stream descrambler's next call, in RS words from the epoch's superframe start
  long long label0 = 0;                                        // stream packet index of the epoch's RS word 0 (chunk labels)
  bool have_cur = false; StreamPiece cur;                      // the piece of this rank whose samples are arriving (its buffer holds [cur.begin, pos))
  bool have_next = false; StreamPiece next;                    // this rank's piece after that, not begun yet (samples before next.begin are not its business)
  int last_handle = 0;                                         // handle of the piece launched last (the next one takes the other)
  std::vector<StreamPiece> inflight;                           // enqueued, not yet harvested (at most two)
  // ---- the walk
  DevMem<float2> wbuf[2]; size_t wcap = 0;                     // its own sample buffers (allocated when a walk outgrows buf[0]: twice a piece's)
  int wh = 0;                                                  // the handle that walks (0; a sharded stream walks a piece on the piece's own handle: the other one may be busy)
  float2 *wb = nullptr; size_t wb_cap = 0; int wb_which = -1;  // the buffer the walk's samples sit in (buf[0] at the stream's beginning), -1: buf[0], else wbuf[wb_which]
  long long wb_begin = 0;                                      // stream sample of wb[0]
  long long w_hist = 0;                                        // samples in wb in front of the window's first search position
  long long walk_at = 0;                                       // stream position at which the next window runs
  bool w_carry = false; float w_avg = 0.f; bool w_cont = false, w_preset = false; size_t w_acc = 0; int w_delivering = 0;   // walk_window's carried state
  bool w_cut = false; long long w_cut_sym_off = 0; int w_cut_delay = 0; size_t w_pad = 0; long long w_e0 = 0;   // the walk began in a piece of an epoch: its cut, the pad in front of its bytes, its first word in the epoch
  long long w_done = 0;                                        // RS words of the walk's Viterbi stream that are final and decoded
  long long w_pre = -1;                                        // sharded walk from a piece: RS word (of the walk's stream) of 8 packets in front of the first call that go out unchecked
  DescrState w_ds;                                             // the descrambler, in RS items / packets of the walk's Viterbi stream (h->vit of handle 0)
  bool w_emit = true;                                          // this rank delivers the walk's packets
  long long w_label = 0;                                       // label of the walk's next packet (world 1: a running count)
  long long w_clip_lo = -1, w_clip_hi = -1;                    // world > 1, a walk confined to a piece: only packets whose label lies in [lo, hi) go out
  long long w_next_sf = 0;                                     // ... the epoch's superframe the NEXT piece (another rank's) begins with
  std::vector<std::pair<long long, long long>> w_relabel;      // ... (first RS word of a lock period in the walk's stream, label shift of its packets)
  std::deque<StreamChunk> fifo; size_t fifo_off = 0;           // decoded TS of this rank, in order
  PinMem<uint8_t> ts_ring; TsRing ring; size_t ring_bytes = 0;   // pinned ring the chunks live in (ts_ring.hpp: placement and release); allocated at the first emit
  // device output: the decoded TS stays in device memory for the exchange step (dvbt_rccl.inc): chunks that wait (dfifo), chunks an exchange step in flight still
  // reads (dzombie: released when that step has completed), the ring they live in (overflow: own allocations)
  bool dev_out = false; DevMem<uint8_t> dring; size_t dring_bytes = 0; TsRing dalloc; std::deque<DevChunk> dfifo, dzombie; int dzombie_of[2] = {0, 0};
  std::vector<TsBuf> ts_pool;                                  // device output: spare TS buffers (a piece's packets are handed over in the buffer they were decoded into, the handle takes a spare)
  long long packets_out = 0, bytes_pulled = 0;
  long long first_sf_call = -1, first_q0 = -1;                 // dvbt_rx_stream_info: the stream's first superframe start and first packet
  int status = 0;
  // TPS auto-configuration (constellation / hierarchy / code_rate = DVBT_AUTO): the head of the stream is kept on the host until a probe chain has read a
  // BCH-valid TPS word out of it; then the two chains are built for what the stream signals and the head is replayed into them
  bool auto_pending = false; std::vector<float2> head; long long auto_need = 0; int auto_tries = 0;
  int det_constellation = -1, det_hierarchy = -1, det_code_rate = -1;
  std::vector<unsigned long long> bits_host; std::vector<DescrRun> runs_host;
  std::string trace;                                           // dvbt_rx_stream_trace: one line per change of mode / walk window (bounded)
  void log(const char *fmt, ...)
  {
    if (trace.size() > (1u << 16)) return;
    char b[512]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    trace += b; trace += '\n';
  }
};

static long long stream_post(const Dims &d)
{
  const long long ibits = (long long)d.payload * d.m * d.k / d.n;
  return (80ll * 204 * 8 + ibits - 1) / ibits + 3;             // multi.py::post_symbols
}

static void stream_free_chains(dvbt_rx_stream *s)   // a stream_setup that failed half way keeps nothing
{
  for (auto &b : s->wbuf) b.reset();
  for (int i = 0; i < dvbt_rx_stream::MAXH; i++) { s->rx[i].reset(); s->buf[i].reset(); s->ev_written[i].reset(); s->ev_copied[i].reset(); }
}

// everything that depends on the transmission parameters: dimensions, the two chains, the sample buffers; the stream begins as a walk in buf[0]
static int stream_setup(dvbt_rx_stream *s)
{
  const dvbt_rx_stream_params *p = &s->prm;
  Dims d = make_dims(p->rx.constellation, p->rx.hierarchy, p->rx.code_rate, p->rx.guard_interval, p->rx.transmission_mode);
  if (!d.valid) return fail(DVBT_ERR_INVALID, "bad DVB-T parameters");
  s->d = d;
  s->L = d.N + d.cp; s->win = 2 * d.N + d.cp + 16; s->post = stream_post(d);
  s->ibits = (long long)d.payload * d.m * d.k / d.n; s->wsf = 272 * s->ibits / (8 * 204);
  s->thr = (STREAM_PRE + 272) * s->L + s->win;                 // what a piece needs behind its begin to find its boundary and deliver something
  const long long S = s->prm.segment_superframes;
  // the first window must hold the first superframe start (at most ~1.5 superframes into a stream that starts anywhere in a superframe) and leave the head >= 1 superframe
  s->len0 = (272 * (S + 2) + 136 + s->post) * s->L + s->win + 4096;
  const long long piece_len = (STREAM_PRE + 68 + 272 * S + s->post) * s->L + s->win;     // (+ 68: an epoch whose grid is `delay` symbols off a frame boundary begins its pieces that much earlier)
  // a piece waits in its buffer until the next one is known to be viable: that much more of the stream
  s->cap = (size_t)(std::max(s->len0, piece_len) + s->thr + 8 * s->L);
  dvbt_rx_params q = p->rx; q.max_samples = s->cap; q.resample_interp = q.resample_decim = 0; q.launch_graph = 0;   // (every piece has its own cut: nothing to replay)
  for (int i = 0; i < s->nh; i++) {
    dvbt_rx *h = nullptr; int r = dvbt_rx_create(&q, &h); if (r) { stream_free_chains(s); return r; }
    s->rx[i].reset(h);
    if (s->buf[i].alloc(s->cap) != hipSuccess || s->ev_written[i].create(hipEventDisableTiming) != hipSuccess ||
        s->ev_copied[i].create(hipEventDisableTiming) != hipSuccess) { stream_free_chains(s); return fail(DVBT_ERR_HIP, "dvbt_rx_stream: device allocation failed"); }
  }
  // the stream's beginning is a walk: fresh blocks, the samples in buf[0]
  s->in_pieces = false; s->have_cur = s->have_next = false;
  s->wb = s->buf[0]; s->wb_cap = s->cap; s->wb_which = -1; s->wb_begin = 0; s->wb_filled = 0; s->w_hist = 0; s->walk_at = s->len0;
  s->w_carry = false; s->w_avg = 0.f; s->w_cont = false; s->w_preset = false; s->w_acc = 0; s->w_delivering = 0; s->w_cut = false; s->w_pad = 0; s->w_e0 = 0; s->w_done = 0; s->w_ds = DescrState();
  s->w_emit = s->rank == 0; s->w_label = 0; s->w_clip_lo = s->w_clip_hi = -1;
  return DVBT_OK;
}

extern "C" int dvbt_rx_stream_create(const dvbt_rx_stream_params *p, dvbt_rx_stream **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  int r = need_device(); if (r) return r;
  if (p->rx.resample_interp || p->rx.resample_decim) return fail(DVBT_ERR_INVALID, "dvbt_rx_stream takes samples at the OFDM elementary rate (no resampler)");
  if (p->world < 0 || p->rank < 0 || (p->world > 0 && p->rank >= p->world)) return fail(DVBT_ERR_INVALID, "dvbt_rx_stream: rank must lie in [0, world)");
  if (p->ts_ring_bytes < 0) return fail(DVBT_ERR_INVALID, "dvbt_rx_stream: ts_ring_bytes must not be negative");
  if (p->chains != 0 && (p->chains < 2 || p->chains > dvbt_rx_stream::MAXH)) return fail(DVBT_ERR_INVALID, "dvbt_rx_stream: chains must be 0 (two) or lie in [2, 4]");
  const bool au = p->rx.constellation == DVBT_AUTO || p->rx.hierarchy == DVBT_AUTO || p->rx.code_rate == DVBT_AUTO;
  {   // what must be known up front: the front end's dimensions (transmission mode, guard interval); AUTO fields are probed with QPSK 1/2 NH
    Dims d = make_dims(p->rx.constellation == DVBT_AUTO ? 0 : p->rx.constellation, p->rx.hierarchy == DVBT_AUTO ? 0 : p->rx.hierarchy,
                       p->rx.code_rate == DVBT_AUTO ? 0 : p->rx.code_rate, p->rx.guard_interval, p->rx.transmission_mode);
    if (!d.valid) return fail(DVBT_ERR_INVALID, "bad DVB-T parameters");
  }
  std::unique_ptr<dvbt_rx_stream> hold(new dvbt_rx_stream()); dvbt_rx_stream *const s = hold.get();   // released on every early return below
  s->prm = *p;
  s->world = p->world > 0 ? p->world : 1; s->rank = p->world > 0 ? p->rank : 0;
  if (s->prm.segment_superframes <= 0) s->prm.segment_superframes = 16;
  s->ring_bytes = p->ts_ring_bytes > 0 ? (size_t)p->ts_ring_bytes : STREAM_TS_RING_DEFAULT;
  s->borrow = p->borrow_device_pushes != 0;
  s->nh = p->chains ? p->chains : 2;
  if (s->borrow && au) return fail(DVBT_ERR_INVALID, "dvbt_rx_stream: borrow_device_pushes and DVBT_AUTO do not go together (the head of an auto-configured stream is replayed from host memory)");
  if (s->ev_direct.create(hipEventDisableTiming) != hipSuccess) return fail(DVBT_ERR_HIP, "dvbt_rx_stream: event creation failed");
  // the page-locked buffers are taken here, not at the first delivery / the first host push: page-locking 96 + 32 MB takes ~10 ms, which belongs to the set-up and
  // not into the stream's first piece.  A stream that cannot have its TS ring lives on heap chunks; dvbt_rx_stream_set_device_output gives the ring back
  if (s->ts_ring.alloc(s->ring_bytes) != hipSuccess) { (void)hipGetLastError(); s->ring.cap = 0; } else s->ring.cap = s->ring_bytes;
  if (s->pin.alloc(STREAM_PIN_BYTES * STREAM_PIN_SLOTS) != hipSuccess) (void)hipGetLastError();
  else for (int i = 0; i < STREAM_PIN_SLOTS; i++)
    if (s->pin_ev[i].create(hipEventDisableTiming) != hipSuccess) return fail(DVBT_ERR_HIP, "dvbt_rx_stream: event creation failed");
  if (au) {
    // TPS auto-configuration (gr-dvbt's TODO.txt:28 "Autodetect transmission params"): nothing that depends on constellation / hierarchy / code rate is built
    // yet.  The TPS word of a frame is complete 68 symbols after a frame start, a frame start is at most 67 symbols away, the acquisition takes a few: two
    // frames and a margin hold one whole frame for certain
    const Dims d0 = make_dims(0, 0, 0, p->rx.guard_interval, p->rx.transmission_mode);
    s->auto_pending = true; s->auto_need = (long long)(2 * 68 + 24) * (d0.N + d0.cp) + 2 * d0.N + d0.cp + 16;
    *out = hold.release();
    return DVBT_OK;
  }
  r = stream_setup(s); if (r) return r;
  *out = hold.release();
  return DVBT_OK;
}

// ---- borrowed device pushes: the stream's samples [a, b) where the caller left them
static const float2 *stream_region_ptr(const dvbt_rx_stream *s, long long a, long long b)   // one region holds them all: there; else nullptr
{
  for (const auto &r : s->regions) if (a >= r.pos0 && b <= r.pos0 + r.n) return r.ptr + (a - r.pos0);
  return nullptr;
}
static int stream_gather_regions(dvbt_rx_stream *s, long long a, long long b, float2 *dst, hipStream_t st)   // ... copied together to dst, on st
{
  long long covered = 0;
  for (const auto &r : s->regions) {
    const long long lo = std::max(a, r.pos0), hi = std::min(b, r.pos0 + r.n);
    if (hi > lo) { HIPCHK(hipMemcpyAsync(dst + (lo - a), r.ptr + (lo - r.pos0), sizeof(float2) * (size_t)(hi - lo), hipMemcpyDeviceToDevice, st)); covered += hi - lo; }
  }
  if (covered != b - a) return fail(DVBT_ERR_STATE, "dvbt_rx_stream: borrowed samples are no longer on record (internal)");
  return DVBT_OK;
}
// the walk's buffer holds [wb_begin, wb_filled); what has been pushed since is still where the caller left it
static int walk_fill(dvbt_rx_stream *s)
{
  if (!s->borrow || s->wb_filled >= s->pos) return DVBT_OK;
  if (s->wb_filled < s->wb_begin) s->wb_filled = s->wb_begin;
  if ((size_t)(s->pos - s->wb_begin) > s->wb_cap) return fail(DVBT_ERR_CAPACITY, "dvbt_rx_stream: walk buffer too small (internal sizing)");
  int r = stream_gather_regions(s, s->wb_filled, s->pos, s->wb + (s->wb_filled - s->wb_begin), s->rx[s->wh]->own_stream); if (r) return r;
  s->wb_filled = s->pos;
  return DVBT_OK;
}
// regions nothing will read again leave the record (dvbt_rx_stream_info.samples_released: the caller may reuse that memory)
static void stream_release_regions(dvbt_rx_stream *s)
{
  if (!s->borrow) return;
  long long rp = s->pos;
  if (s->in_pieces) {
    for (const StreamPiece &q : s->inflight) rp = std::min(rp, q.begin);
    if (s->have_cur) rp = std::min(rp, s->cur.begin);
    if (s->have_next) rp = std::min(rp, std::min(s->next.begin, s->pos));
  } else rp = std::min(rp, s->wb_begin);                              // (a walk's buffer holds copies, but the pieces that follow it begin inside it and read the regions)
  while (!s->regions.empty() && s->regions.front().pos0 + s->regions.front().n <= rp) s->regions.pop_front();
  s->released = rp;
}

// ---- the plan of an epoch (valid while in_pieces)
static long long stream_first_sf(const dvbt_rx_stream *s, long long k) { return k <= 0 ? 0 : s->count0 + (k - 1) * s->prm.segment_superframes; }
static long long stream_pre(const dvbt_rx_stream *s) { return STREAM_PRE + s->delay % 68; }   // a whole TPS frame must end between the piece's begin and its boundary
static long long stream_begin(const dvbt_rx_stream *s, long long k) { return s->grid0 + (s->sf_call + 272 * stream_first_sf(s, k) - stream_pre(s)) * s->L; }
static long long stream_end(const dvbt_rx_stream *s, long long k) { return s->grid0 + (s->sf_call + 272 * stream_first_sf(s, k + 1) + s->post) * s->L + s->win; }
static void stream_plan_piece(const dvbt_rx_stream *s, long long k, StreamPiece &pc)
{
  pc = StreamPiece();
  pc.index = k; pc.first_sf = stream_first_sf(s, k); pc.count = s->prm.segment_superframes;
  pc.begin = stream_begin(s, k); pc.end = stream_end(s, k); pc.launch_at = stream_begin(s, k + 1) + s->thr;
}
static long long stream_next_owned(const dvbt_rx_stream *s, long long after)   // the next piece of this rank behind piece `after`
{
  long long k = after + 1;
  while (k % s->world != s->rank) k++;
  return k;
}
// first packet of the first descrambler call (phase: that of `dc`) at or behind RS word `lo` of the epoch
static long long stream_call_from(long long dc, long long lo) { return lo + (((dc - lo) % 16) + 16) % 16; }
// sharded streams trim on the 8-packet grid of the transmitted NSYNCs (a rank cannot know what the descrambler did in another rank's piece)
static long long stream_G(const dvbt_rx_stream *s, long long first_sf)
{
  const long long lo = first_sf * s->wsf + 11;
  return lo + (((s->dc - lo) % 8) + 8) % 8;
}

// bytes of a handle's TS tap (device) -> the output FIFO, labelled with the stream packet index of their first packet
// steal (device output, the LAST thing a harvest does with the handle's TS buffer): no copy -- the chunk IS the stretch of the handle's buffer, the handle goes on with a spare
// one (a 62 MB blit per piece, waited for by the host while the other piece's decoder holds the compute units, cost the C++ host 0.5 ms of every 4.5: VERDICT r05 weak 3)
static int stream_emit_bytes(dvbt_rx_stream *s, dvbt_rx *h, const uint8_t *dev, size_t len, long long label, bool steal = false)
{
  if (!len) return DVBT_OK;
  if (s->dev_out && steal && len >= (1u << 20) && dev >= h->ts_out && dev + len <= h->ts_out + h->vit_cap) {
    DevMem<uint8_t> fresh;
    for (size_t i = 0; i < s->ts_pool.size(); i++) if (s->ts_pool[i].cap >= h->vit_cap) { fresh = std::move(s->ts_pool[i].mem); s->ts_pool.erase(s->ts_pool.begin() + i); break; }
    if (!fresh && fresh.alloc(h->vit_cap) != hipSuccess) (void)hipGetLastError();
    if (fresh) {
      DevChunk c; c.first_packet = label; c.len = len; c.off = 0; c.in_ring = false; c.data = const_cast<uint8_t *>(dev); c.stolen.mem = std::move(h->ts_out); c.stolen.cap = h->vit_cap;
      h->ts_out = std::move(fresh);
      s->packets_out += (long long)(len / 188);
      s->dfifo.push_back(std::move(c));
      return DVBT_OK;
    }
  }
  if (s->dev_out) {
    // the packets stay on the device: into the stream's device ring (own allocation when it is full), behind the handle's decode
    if (!s->dring) { if (s->dring.alloc(s->dring_bytes) != hipSuccess) { (void)hipGetLastError(); s->dalloc.cap = 0; } else s->dalloc.cap = s->dring_bytes; }
    DevChunk c; c.first_packet = label; c.len = len; c.off = 0; c.in_ring = false; c.data = nullptr;
    const size_t at = s->dring ? s->dalloc.place(len) : TsRing::NONE;
    if (at != TsRing::NONE) { c.data = s->dring + at; c.in_ring = true; }
    else { HIPCHK(c.own.alloc(len)); c.data = c.own; }
    HIPCHK(hipMemcpyAsync(c.data, dev, len, hipMemcpyDeviceToDevice, h->own_stream));
    HIPCHK(hipStreamSynchronize(h->own_stream));                   // (the handle's TS buffer is reused by its next piece; an exchange step may read the chunk at once)
    s->packets_out += (long long)(len / 188);
    s->dfifo.push_back(std::move(c));
    return DVBT_OK;
  }
  StreamChunk c; c.first_packet = label; c.len = len; c.in_ring = false;
  const size_t at = s->ts_ring ? s->ring.place(c.len) : TsRing::NONE;
  uint8_t *dst;
  if (at != TsRing::NONE) { dst = s->ts_ring + at; c.in_ring = true; }
  else { c.heap.resize(c.len); dst = c.heap.data(); }             // the ring is full (a consumer far behind): this chunk lives on the heap
  c.data = dst;
  // on the handle's own stream (idle by now): a copy on the null stream would wait for the other handle's decode
  HIPCHK(hipMemcpyAsync(dst, dev, c.len, hipMemcpyDeviceToHost, h->own_stream));
  HIPCHK(hipStreamSynchronize(h->own_stream));
  s->packets_out += (long long)(len / 188);
  s->fifo.emplace_back(std::move(c));
  return DVBT_OK;
}

// ---- energy_descramble followed on the host (energy_descramble_impl.cc:121-141, the calls restated in the smallest size the block accepts: 4 items visible,
// 2 consumed): bit w of `bits` (index relative to bit_base) = payload byte 0 of RS word w is 0xB8.  The calls that start in front of `stop_start` and still see
// four items of `nitems` are walked; what they deliver is appended to `runs` (source bytes in the RS output, whole calls of 3008 bytes, neighbours merged)
static void descr_walk(const std::vector<unsigned long long> &bits, long long bit_base, long long nitems, long long stop_start, DescrState &ds,
                       std::vector<DescrRun> &runs, long long &written)
{
  auto nsync = [&](long long pkt) -> bool {
    const long long i = pkt - bit_base;
    if (i < 0 || (size_t)(i >> 6) >= bits.size()) return false;
    return ((bits[(size_t)(i >> 6)] >> (i & 63)) & 1ull) != 0;
  };
  while (ds.base + 4 <= nitems) {
    const long long cs = ds.start();
    if (cs >= stop_start) break;
    if (nsync(cs)) {
      if (!runs.empty() && runs.back().src_byte + runs.back().nbytes == cs * 188) runs.back().nbytes += 3008;
      else runs.push_back(DescrRun{cs * 188, written, 3008});
      written += 3008; ds.base += 2;
    } else {
      int dp = ds.dp;
      while (dp < 16 && !nsync(ds.base * 8 + dp)) dp++;
      if (dp >= 16) { dp = 0; ds.base += 2; }
      ds.dp = dp;
    }
  }
}

// the runs (source bytes relative to h->rs_out) through the PRBS into h->ts_out and out to the FIFO.  running_labels (world 1): the packets are counted as
// they go out (w_label).  Else (a sharded stream): a run's first packet gets the label `source packet + shift`, with the shift of the lock period the packet
// lies in (w_relabel: a junction drops what lay between the loss and the new superframe start, the labels jump), and only labels inside the rank's window
// [w_clip_lo, w_clip_hi) go out, trimmed on whole 8-packet groups
static int stream_emit_runs(dvbt_rx_stream *s, dvbt_rx *h, std::vector<DescrRun> &runs, long long written, bool emit, long long label_shift, bool running_labels)
{
  if (!written || runs.empty()) return DVBT_OK;
  hipStream_t st = h->own_stream;
  if (!emit) { if (running_labels) s->w_label += written / 188; return DVBT_OK; }
  for (size_t a = 0; a < runs.size(); a += DESCR_MAX_RUNS) {
    const size_t nr = std::min<size_t>(DESCR_MAX_RUNS, runs.size() - a);
    std::vector<DescrRun> part(runs.begin() + a, runs.begin() + a + nr);
    const long long d0 = part[0].dst_byte; long long total = 0;
    for (DescrRun &r : part) { r.dst_byte -= d0; total += r.nbytes; }
    const int nri = (int)nr;
    HIPCHK(hipMemcpyAsync(h->descr_runs, part.data(), sizeof(DescrRun) * nr, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->descr_nruns, &nri, sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(&h->st->n_ts_bytes, &total, sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                              // (the sources are stack / vector memory)
    hipLaunchKernelGGL(descramble_runs_kernel, dim3(1024), dim3(256), 0, st, (const uint8_t *)h->rs_out, (const uint8_t *)h->T.prbs,
                       (const RxState *)h->st, (const DescrRun *)h->descr_runs, (const int *)h->descr_nruns, h->ts_out);
    HIPCHK(hipGetLastError());
    if (running_labels) { int r = stream_emit_bytes(s, h, h->ts_out, (size_t)total, s->w_label); if (r) return r; s->w_label += total / 188; }
    else {
      for (const DescrRun &r : part) {
        // a run that crosses a junction is labelled in two parts (cut on the run's own 8-packet grid: the junction's first words are junk either way)
        long long word = r.src_byte / 188, left = r.nbytes / 188, done = 0;
        while (left > 0) {
          long long shift = label_shift, seg = left;
          for (const auto &bp : s->w_relabel) {
            if (word >= bp.first) shift = bp.second;
            else { const long long at = word + ((bp.first - word + 7) / 8) * 8; if (at - word < seg) seg = at - word; }
          }
          long long lab = word + shift, n = seg, skip = 0;
          if (s->w_clip_lo >= 0) {
            if (lab < s->w_clip_lo) skip = ((s->w_clip_lo - lab + 7) / 8) * 8;
            if (lab + n > s->w_clip_hi) n = std::max<long long>(skip, ((s->w_clip_hi - lab) / 8) * 8);
          }
          if (n - skip > 0) { int rr = stream_emit_bytes(s, h, h->ts_out + (size_t)(r.dst_byte + (done + skip) * 188), (size_t)(n - skip) * 188, lab + skip); if (rr) return rr; }
          word += seg; left -= seg; done += seg;
        }
      }
    }
  }
  return DVBT_OK;
}

// A8 + A9 over the RS words [from, to) of handle h's Viterbi stream (from: a multiple of 64, the sync bitmap's granularity), the bitmap of [from, to) to the host
static int stream_rs_range(dvbt_rx_stream *s, dvbt_rx *h, long long from, long long to)
{
  hipStream_t st = h->own_stream;
  const long long n = to - from;
  if (n <= 0) return DVBT_OK;
  HIPCHK(hipMemsetAsync(&h->st->rs_list_n, 0, sizeof(int), st));
  const long long hist = std::min<long long>(11, from);
  hipLaunchKernelGGL(deint_rs_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const uint8_t *)(h->vit + from * 204), (uint8_t *)nullptr, h->rs_out + from * 188,
                     (RxState *)nullptr, n, 0, hist, h->T.rs_tables(), h->prm.rs_oracle_compat, &h->st->rs_fail, &h->st->rs_corr, h->rs_defer, &h->st->rs_list_n, h->rs_defer_cap,
                     h->rs_sync + from / 64);
  hipLaunchKernelGGL(rs_fix_kernel, dim3(512), dim3(64), 0, st, (const RsDefer *)h->rs_defer, (const int *)&h->st->rs_list_n, h->rs_defer_cap, h->rs_out + from * 188,
                     h->T.rs_tables(), h->prm.rs_oracle_compat, &h->st->rs_fail, &h->st->rs_corr, h->rs_sync + from / 64);
  HIPCHK(hipGetLastError());
  (void)s;
  return DVBT_OK;
}
static int stream_fetch_bits(dvbt_rx_stream *s, dvbt_rx *h, long long from_word /* multiple of 64 */, long long to_word)
{
  const size_t nw = (size_t)((to_word - from_word + 63) / 64);
  s->bits_host.assign(nw + 1, 0ull);
  if (nw) {
    HIPCHK(hipMemcpyAsync(s->bits_host.data(), h->rs_sync + from_word / 64, sizeof(unsigned long long) * nw, hipMemcpyDeviceToHost, h->own_stream));
    HIPCHK(hipStreamSynchronize(h->own_stream));
    const long long tail = (to_word - from_word) & 63;             // bits behind `to` belong to words that do not exist (yet)
    if (tail) s->bits_host[nw - 1] &= (1ull << tail) - 1;
  }
  return DVBT_OK;
}

// ---- the walk's tail: behind a window, A8 + A9 over the words of the walk's Viterbi stream that are final, the descrambler over the items that are final
static int walk_flush(dvbt_rx_stream *s, bool eos, long long stop_start /* the head of an epoch: calls from here on belong to its pieces */, bool all_words = false,
                      long long clip8_word = -1 /* sharded head: its share ends at the first transmitted NSYNC at or behind this word (the pieces trim on that grid) */)
{
  dvbt_rx *h = s->rx[s->wh].get();
  hipStream_t st = h->own_stream;
  // final: below the last multiple of 3264 bytes (the next delivering period realigns there, convolutional_deinterleaver_impl.cc:109-120); at the stream's end:
  // the even item count of the whole stream (set_output_multiple(2))
  long long final_words = eos ? (((long long)s->w_acc / 1632) & ~1ll) * 8 : ((long long)s->w_acc / 3264) * 16;
  if (stop_start < (1ll << 60) || all_words) final_words = ((long long)s->w_acc / 204);   // a head's stream goes on in its pieces (a sharded piece's in the next rank's): every word it has is final
  const long long nitems = final_words / 8;
  long long from = std::min(s->w_done, s->w_ds.base * 8); from = (from / 64) * 64; if (from < 0) from = 0;
  if (final_words > from) {
    int r = stream_rs_range(s, h, from, final_words); if (r) return r;
    s->w_done = final_words;
  }
  const long long bit_from = (std::max<long long>(s->w_ds.base * 8, 0) / 64) * 64;
  { int r = stream_fetch_bits(s, h, bit_from, std::max(final_words, bit_from)); if (r) return r; }
  s->runs_host.clear(); long long written = 0;
  if (s->w_pre >= 0 && final_words >= s->w_pre + 8) { s->runs_host.push_back(DescrRun{s->w_pre * 188, 0, 1504}); written = 1504; s->w_pre = -1; }   // (sharded: the second half of a call that began in front of the piece)
  descr_walk(s->bits_host, bit_from, nitems, stop_start, s->w_ds, s->runs_host, written);
  {
    // labels: world 1 counts the packets as they go out (from the RS word of the stream's first packet on); a sharded walk labels with the epoch's packet index
    // (source packet - pad + the piece's first word)
    const bool running = s->world == 1;
    const long long shift = s->label0 + s->w_e0 - (long long)(s->w_pad / 204);
    if (written && s->first_q0 < 0) { s->first_q0 = s->runs_host[0].src_byte / 188 + shift; if (running) s->w_label = s->first_q0; }
    const long long lo0 = s->w_clip_lo, hi0 = s->w_clip_hi;
    if (clip8_word >= 0 && !running) { const long long c = s->w_ds.start(); s->w_clip_lo = 0; s->w_clip_hi = clip8_word + (((c - clip8_word) % 8) + 8) % 8 + shift; }
    int r = stream_emit_runs(s, h, s->runs_host, written, s->w_emit, shift, running);
    s->w_clip_lo = lo0; s->w_clip_hi = hi0;
    if (r) return r;
  }
  // compaction: the descrambler has left these words behind (multiples of 64 words = 4 x 3264 bytes: every alignment of the walk survives)
  if (!eos && !all_words && stop_start >= (1ll << 60) && s->w_ds.base * 8 > WALK_KEEP_WORDS) {   // (a walk that goes on: a head's / a sharded piece's ends here)
    const long long k = ((s->w_ds.base * 8 - 64) / 64) * 64;
    if (k > 0 && (size_t)(k * 204) <= s->w_acc) {
      const size_t keep = s->w_acc - (size_t)k * 204;
      HIPCHK(hipMemcpyAsync(h->ts_out, h->vit + (size_t)k * 204, keep, hipMemcpyDeviceToDevice, st));   // (through a buffer that is idle here: the ranges may overlap)
      HIPCHK(hipMemcpyAsync(h->vit, h->ts_out, keep, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
      s->w_acc = keep; s->w_ds.base -= k / 8; s->w_done = std::max<long long>(0, s->w_done - k);
      s->w_e0 += k - (long long)(s->w_pad / 204); s->w_pad = 0;   // (w_e0 - w_pad / 204 keeps naming the epoch word of buffer word 0)
      for (auto &b : s->w_relabel) b.first -= k;
    }
  }
  return DVBT_OK;
}

static int stream_begin_next(dvbt_rx_stream *s, const float2 *from_mem, long long from_begin, int from_handle, hipStream_t from_stream, long long after_index);

// the walk's samples move to the front of the other walk buffer (what lies in front of `keep_from` is final)
static int walk_rebase(dvbt_rx_stream *s, long long keep_from /* stream sample */)
{
  dvbt_rx *h = s->rx[s->wh].get();
  hipStream_t st = h->own_stream;
  if (!s->wbuf[0]) {
    s->wcap = (size_t)((long long)s->nh * (long long)s->cap + s->thr);
    for (int i = 0; i < 2; i++) if (s->wbuf[i].alloc(s->wcap) != hipSuccess) return fail(DVBT_ERR_HIP, "dvbt_rx_stream: walk buffer allocation failed");
  }
  { int r = walk_fill(s); if (r) return r; }
  const int to = s->wb_which < 0 ? 0 : (s->wb_which ^ 1);
  const long long n = s->pos - keep_from;
  if (n > 0) HIPCHK(hipMemcpyAsync(s->wbuf[to], s->wb + (keep_from - s->wb_begin), sizeof(float2) * (size_t)n, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  s->wb = s->wbuf[to]; s->wb_cap = s->wcap; s->wb_which = to; s->wb_begin = keep_from; s->wb_filled = s->pos;
  return DVBT_OK;
}

// the descrambler's state for a call that starts at RS word `bw` of the walk's stream (bw >= 0)
static DescrState descr_at(long long bw) { DescrState d; d.base = 2 * (bw / 16); d.dp = (int)(bw - d.base * 8); return d; }

// one window of the walk over wb = [wb_begin, pos); last: the stream ends here
static int stream_walk(dvbt_rx_stream *s, bool last)
{
  dvbt_rx *h = s->rx[s->wh].get();
  hipStream_t st = h->own_stream;
  const long long S = s->prm.segment_superframes;
  { int r = walk_fill(s); if (r) return r; }
  const float2 *chain = s->wb + s->w_hist;
  const long long chain_n = s->pos - s->wb_begin - s->w_hist;
  const bool confined = s->w_clip_lo >= 0 && !last;                // sharded: the walk of one piece's samples (the stream goes on in other ranks' pieces)
  const long long winL = (s->win + s->L - 1) / s->L;
  if (chain_n < s->win) {
    if (last || confined) { int r = walk_flush(s, last, 1ll << 62, confined); if (r) return r; if (last) s->finished = true; }
    else s->walk_at = s->wb_begin + s->w_hist + s->win;
    return DVBT_OK;
  }
  WalkIO io;
  io.partial = !last && !confined; io.carry = s->w_carry; io.avg = s->w_avg; io.hist = s->w_hist; io.continuation = s->w_cont; io.tps_preset = s->w_preset; io.acc = s->w_acc; io.delivering = s->w_delivering;
  io.cut = s->w_cut; io.cut_sym_off = s->w_cut_sym_off; io.cut_delay = s->w_cut_delay; io.vit_pad = s->w_pad;
  // an epoch needs a head of at least one superframe and a first piece that stands on its own: two superframes and a window behind the superframe start
  io.establish_calls = 2 * 272 + winL + 1;
  {   // room behind the decoder for everything this window can lay out: what the walk carries, the window's samples as one stream, the realignment gaps between its periods
    const long long vit_bytes = (chain_n / s->L + 2) * s->ibits / 8;
    int r = rx_reserve_vit(h, (size_t)((long long)s->w_acc + (long long)s->w_pad + vit_bytes + vit_bytes / 8 + (4ll << 20))); if (r) return r;
  }
  { int r = walk_window(h, chain, (size_t)chain_n, st, io); if (r) return r; }
  s->status |= io.status_or;
  s->log("walk window: samples [%lld, %lld) hist %lld last %d confined %d: %zu periods final, established %d, acc %zu -> %zu, next_off %zu", s->wb_begin + s->w_hist, s->pos, s->w_hist, (int)last, (int)confined,
         io.per.size(), (int)io.established, s->w_acc, io.acc, io.next_off);
  for (const WalkPeriod &w : io.per) s->log("  period off %zu call0 %d n %d lost %d decoded %d first_out %d vit_off %zu n_vit %lld", w.off, w.call0, w.n_symbols, (int)w.lost, (int)w.decoded, w.first_out, w.vit_off, w.n_vit_bytes);
  s->w_acc = io.acc; s->w_delivering = io.delivering; s->w_cont = io.continuation; s->w_preset = io.tps_preset; s->w_cut = io.cut;
  // the lock was lost inside the stream: a lost period that a period with items follows (in a window that is not the last one the periods kept are exactly those)
  for (size_t i = 0; i < io.per.size(); i++) {
    bool later = io.partial;
    for (size_t j = i + 1; j < io.per.size(); j++) if (io.per[j].n_symbols >= 1) later = true;
    if (io.per[i].lost && later) s->status |= 2;
  }
  if (s->w_clip_lo >= 0) {
    // a sharded walk: where a later lock period's packets sit in the stream (the transmitted superframe grid is the epoch's; a period that starts off that grid
    // -- a superframe start declared on stale counters -- cannot be told to the ranks that own the following pieces: status bit 5)
    for (const WalkPeriod &w : io.per) {
      if (!w.decoded || w.first_out < 0 || w.vit_off == s->w_pad) continue;
      const long long pos_sf = s->wb_begin + s->w_hist + (long long)w.off + (long long)(w.call0 + w.first_out) * s->L + w.cp_start0;
      const long long ref = s->grid0 + s->sf_call * s->L + s->cp0;
      const long long dsym = (pos_sf - ref + s->L / 2) / s->L;
      const long long q = (dsym + 136) / 272;
      if (std::llabs(dsym - 272 * q) > 2) s->status |= 32;
      s->w_relabel.push_back({(long long)w.vit_off / 204, s->label0 + q * s->wsf - (long long)w.vit_off / 204});
    }
    if (confined) {
      // the ranks that own the following pieces decode them as pieces of the epoch: that is the single chain's output only if the reference's chain is back in a
      // lock period that holds to this piece's end, on the transmitted grid, with its superframe start in front of the next piece's first one
      int zl = -1;
      for (size_t i = 0; i < io.per.size(); i++) if (io.per[i].n_symbols >= 1) zl = (int)i;
      bool stable = zl >= 0 && !io.per[(size_t)zl].lost && io.per[(size_t)zl].decoded && io.per[(size_t)zl].first_out >= 0;
      if (stable && io.per[(size_t)zl].vit_off != s->w_pad) {
        const WalkPeriod &w = io.per[(size_t)zl];
        const long long pos_sf = s->wb_begin + s->w_hist + (long long)w.off + (long long)(w.call0 + w.first_out) * s->L + w.cp_start0;
        const long long dsym = (pos_sf - (s->grid0 + s->sf_call * s->L + s->cp0) + s->L / 2) / s->L, q = (dsym + 136) / 272;
        // (strictly in front: where the new superframe start IS the next piece's first one, the descrambler's re-search around the junction -- old-phase calls that
        // reach into the new period's first words, up to 15 packets dropped -- falls into the other rank's piece, which takes its packets in whole groups)
        stable = std::llabs(dsym - 272 * q) <= 2 && q < s->w_next_sf;
      }
      if (!stable) s->status |= 32;
    }
  }
  if (io.established) {
    // ---- an epoch: the window's last period is its head
    const WalkPeriod &w = io.per[(size_t)io.head];
    const long long off_abs = s->wb_begin + s->w_hist + (long long)w.off;
    const long long sf_call = w.call0 + w.first_out;
    long long count0 = (io.head_ncalls - sf_call - winL) / 272 - 1;
    if (count0 < 1) count0 = 1;
    // where the hunt fired relative to the transmitted superframe grid: the pilot engine's counters behind the head's last symbol are the transmitted ones (every
    // frame end with a valid TPS word re-derives them); counted back to the head's first delivered symbol they give its place in the superframe.  (frame_index
    // holds the number of the frame received last, which is what the hunt compares: a symbol in the frame behind frame f sees f)
    int delay = 0;
    {
      TpsState te; HIPCHK(hipMemcpy(&te, h->tps_state, sizeof te, hipMemcpyDeviceToHost));
      if (te.symbol_index_known) {
        const long long p_next = (((te.frame_index - h->d.fi_start) % 4 + 4) % 4) * 68 + (te.symbol_index + 1) % 68;   // place of the symbol behind the last one processed
        delay = (int)((((p_next - (long long)w.n_out_symbols) % 272) + 272) % 272);
      }
    }
    // the head's packets: the descrambler's calls that start in front of word 11 of the epoch's first piece
    const long long a_w = (long long)w.vit_off / 204;               // RS word (of the walk's stream) of the epoch's superframe start
    const long long stop = a_w + count0 * s->wsf + 11;
    { int r = walk_flush(s, false, s->world == 1 ? stop : stop + 16, false, s->world == 1 ? -1 : stop); if (r) return r; }
    s->log("epoch: grid0 %lld sf_call %lld count0 %lld delay %d a_w %lld dc %lld (walk word %lld) label %lld", off_abs, sf_call, count0, delay, a_w, s->w_ds.start() - a_w, s->w_ds.start(), s->w_label);
    if (s->world > 1 && delay) s->status |= 32;                      // a sharded stream trims its pieces on the transmitted NSYNC grid: an epoch that decodes garbage has none
    s->in_pieces = true; s->grid0 = off_abs; s->sf_call = sf_call; s->count0 = count0; s->delay = delay; s->cp0 = w.cp_start0;
    // the descrambler's next call, in words from the epoch's superframe start (it need not have locked: the calls simply go on from where it stands)
    s->dc = s->w_ds.start() - a_w; s->dc_valid = true;
    // labels: world 1 goes on counting; a sharded stream labels with the RS word of the (one) epoch
    s->label0 = s->world == 1 ? s->w_label - s->dc : a_w + s->w_e0 - (long long)(s->w_pad / 204);
    if (s->first_sf_call < 0) s->first_sf_call = sf_call;
    if (s->first_q0 < 0) s->first_q0 = s->label0 + s->dc;            // (nothing has gone out yet: the stream's first packet is the pieces')
    // pieces take over: this rank's first one begins in the walk's buffer
    s->have_cur = false; s->have_next = false;
    s->last_handle = 0;                                              // (the first piece takes another handle than the one whose buffer the walk stands in)
    for (int i = 0; i < s->nh; i++) if (s->wb == s->buf[i]) s->last_handle = i;
    return stream_begin_next(s, s->wb, s->wb_begin, -1, st, 0);
  }
  if (last || confined) {
    int r = walk_flush(s, last, 1ll << 62, confined); if (r) return r;
    if (confined && !s->w_relabel.empty()) {
      // the descrambler has searched its NSYNC again behind the lost lock: its two-item calls now sit on the 16-packet grid it found there.  The ranks that own the
      // pieces behind this one go on with the epoch's phase -- fine for what they deliver (whole 8-packet groups), but the stream's last call and the junction of
      // a later lost lock are rounded on that grid: a phase that differs cannot be told to them (status bit 5)
      const long long epoch_word = s->w_ds.start() + s->w_relabel.back().second - s->label0;
      if (((epoch_word - s->dc) % 16 + 16) % 16 != 0) { s->status |= 32; s->log("  the descrambler's calls behind the lost lock are 8 packets off the epoch's grid"); }
    }
    if (last) s->finished = true;
    return DVBT_OK;
  }
  // ---- the walk goes on: what is final goes out, the rest waits for more samples
  { int r = walk_flush(s, false, 1ll << 62); if (r) return r; }
  const long long next_abs = s->wb_begin + s->w_hist + (long long)io.next_off;
  s->w_carry = io.next_carry; s->w_avg = io.next_avg;
  long long keep_from = std::max(s->wb_begin, next_abs - WALK_HIST);
  const long long step = S * 272 * s->L;                             // new samples in front of the next window
  if ((s->pos - s->wb_begin) + step > (long long)s->wb_cap) {
    // the next window does not fit behind what the buffer holds: what is final leaves, the rest moves to the front of the walk's own (larger) buffers
    const long long big = (long long)s->nh * (long long)s->cap + s->thr;
    if ((s->pos - keep_from) + step > big) {
      // a lock that holds for more than two pieces without ever reaching a superframe start (no decodable TPS): nothing the reference would deliver either;
      // the walk starts afresh two superframes back (status bits 2 and 5)
      s->status |= 4 | 32;
      s->log("walk: a lock period of more than %lld samples without a superframe start does not fit the walk's buffers: everything in front of sample %lld is dropped, the walk starts afresh (status bits 2, 5)",
             big, std::max(keep_from, s->pos - 2 * 272 * s->L));
      keep_from = std::max(keep_from, s->pos - 2 * 272 * s->L);
      int r = walk_rebase(s, keep_from); if (r) return r;
      s->w_carry = false; s->w_avg = 0.f; s->w_hist = 0; s->w_cut = false; s->w_preset = false;
      s->walk_at = s->pos + step;
      return DVBT_OK;
    }
    int r = walk_rebase(s, keep_from); if (r) return r;
  }
  s->w_hist = next_abs - s->wb_begin;
  s->walk_at = std::min(s->pos + step, s->wb_begin + (long long)s->wb_cap);
  if (s->walk_at <= s->pos) s->walk_at = s->pos + 1;
  return DVBT_OK;
}

// A piece starts its chain from a FRESH acquisition STREAM_PRE symbols in front of its boundary, inside a lock period that the chain before it has seen hold (that chain's
// post-roll covers the same symbols).  In noise the reference's peak detector drops a lock every few hundred symbols -- a fresh acquisition may do so within its first
// symbols (or find no peak in its first windows) where the long-running one did not.  Such a loss is not the stream's: the acquisition is started again behind it, on the
// call grid, until its lock holds through the overlap.  mem: the piece's samples; *skip: the samples to leave out (0: the lock holds from the piece's first sample, or
// no start within max_symbols does)
constexpr long long STREAM_PIECE_SKIP_MAX = 6;      // symbols of its pre-roll a piece's chain can give up (STREAM_PRE = a TPS frame + 8)
constexpr long long STREAM_WALK_SKIP_MAX = 40;      // ... and the walk, whose counters are preset (the Viterbi decoder and the byte de-interleaver need 12 symbols of QPSK 1/2 in front of the boundary)
static int stream_probe_skip(dvbt_rx_stream *s, dvbt_rx *h, const float2 *mem, long long n, hipStream_t st, long long *skip, long long max_symbols)
{
  *skip = 0;
  if (s->delay % 68) max_symbols = std::min(max_symbols, STREAM_PIECE_SKIP_MAX);   // (an epoch off the frame grid looks at the frame number in the middle of a frame: walk_preset_tps)
  const long long span = (stream_pre(s) + s->post + 24) * s->L + s->win;
  long long off = 0;
  for (int it = 0; it < 24 && off <= max_symbols * s->L; it++) {
    const long long len = std::min(n - off, span);
    if (len < s->win) break;
    EnqOpt o; o.acq_only = true; o.no_small = true; o.hist = off; o.avail = n - off;
    int r = enqueue(h, mem + off, (size_t)len, st, o); if (r) return r;
    HIPCHK(hipStreamSynchronize(st));
    h->pending = false;
    const RxState &t = *h->st_host;
    if (!(t.status & 3)) { *skip = off; if (off) s->log("  a fresh acquisition at the piece's begin does not hold its lock: started %lld symbols later", off / s->L); return DVBT_OK; }
    const long long behind = (t.status & 1) ? (long long)ACQ_INIT_TRIES * s->L : (long long)(t.call0 + t.n_symbols) * s->L + s->L / 2;
    off = (off + behind + s->L - 1) / s->L * s->L;
  }
  return DVBT_OK;
}
// where a piece's samples are for its chain (borrowed samples: in place when one region holds them, else gathered into the handle's buffer)
static int stream_piece_samples(dvbt_rx_stream *s, const StreamPiece &pc, hipStream_t st, const float2 **iq)
{
  *iq = s->buf[pc.handle];
  if (s->borrow) {
    *iq = stream_region_ptr(s, pc.begin, pc.begin + pc.n);
    if (!*iq) { int r = stream_gather_regions(s, pc.begin, pc.begin + pc.n, s->buf[pc.handle], st); if (r) return r; *iq = s->buf[pc.handle]; }
  }
  return DVBT_OK;
}

// the pilot engine's counters as a chain that has been in the epoch's lock period all along holds them in front of call `c` of the epoch's grid (TpsState of
// the walk's handle; the FIFO is empty: a frame end needs the whole frame anyway).  An acquisition that needs a window more than the chain's does is absorbed
// by the engine itself: it advances its symbol counter by the scattered-pilot phase it sees (reference_signals_impl.cc:1228-1241)
// (late: the window starts behind the piece's begin (stream_probe_skip) and may hold less than one whole TPS frame in front of the piece's boundary.  The engine takes
// its frame number from the TPS word of a COMPLETE frame; the chain that has been there all along will have read it at the end of the frame the window starts in.  The
// counter is preset to that number: it is looked at again only at that frame's end (an epoch on a frame boundary: si_start = 0), and every later frame is complete)
static int walk_preset_tps(dvbt_rx_stream *s, long long call, bool late = false)
{
  dvbt_rx *h = s->rx[s->wh].get();
  // place in the superframe of the symbol BEFORE the window's first one; the epoch's superframe start (sf_call) sits `delay` symbols behind a transmitted one
  const long long p = ((call - 1 - s->sf_call + s->delay) % 272 + 272) % 272;
  TpsState t; memset(&t, 0, sizeof t);
  t.symbol_index = (int)(p % 68); t.symbol_index_known = 1; t.frame_index = (int)((h->d.fi_start + p / 68) % 4); t.prev_mod = t.symbol_index % 4; t.d_init = 0;
  if (late && (p + 1) % 68 != 0) t.frame_index = (int)((h->d.fi_start + 1 + ((p + 1) % 272) / 68) % 4);
  HIPCHK(hipMemcpy(h->tps_state, &t, sizeof t, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(h->tps_prev, 0, sizeof(float2) * h->d.n_tps));
  return DVBT_OK;
}

// the walk continues the epoch inside piece `pc`: the piece's cut, the epoch's counters, the descrambler's next call; the samples are in wb = [pc.begin, ...)
static int walk_from_piece(dvbt_rx_stream *s, const StreamPiece &pc)
{
  dvbt_rx *h0 = s->rx[s->wh].get();
  const long long e0 = pc.first_sf * s->wsf, e0b = e0 * 204;
  s->in_pieces = false;
  s->wb_begin = pc.begin; s->w_hist = pc.skip;
  s->w_carry = false; s->w_avg = 0.f; s->w_cont = false; s->w_preset = true; s->w_acc = 0; s->w_delivering = 0; s->w_done = 0;   // (the counters are preset below)
  s->w_cut = true; s->w_cut_sym_off = 272 * pc.first_sf; s->w_cut_delay = s->delay;
  s->w_pad = (size_t)(e0b % 3264); s->w_e0 = e0; s->w_relabel.clear();
  if (s->w_pad) HIPCHK(hipMemset(h0->vit, 0, s->w_pad));           // (the walk's stream begins a multiple of 3264 bytes into the epoch's: every realignment of A8 is a multiple of 3264 in it)
  { int r = walk_preset_tps(s, (pc.begin + pc.skip - s->grid0) / s->L, pc.skip > 0 && s->delay % 68 == 0); if (r) return r; }
  const long long padw = (long long)(s->w_pad / 204);
  s->w_emit = true;
  if (s->world == 1) {
    // the piece before delivered the calls in front of dc
    s->w_ds = descr_at(s->dc - e0 + padw);
    s->w_label = s->label0 + s->dc; s->w_clip_lo = s->w_clip_hi = -1;
  } else {
    // sharded: the rank's share begins at the piece's first transmitted NSYNC G (8-packet grid); the calls' phase is the epoch's.  The call G lies in may have
    // begun in front of the piece's valid words: its first half is then taken as delivered (the rank in front cannot say)
    const long long G = stream_G(s, pc.first_sf);
    const long long c = stream_call_from(s->dc, G);                 // first call at or behind G: G itself or G + 8
    s->w_ds = descr_at(c - e0 + padw);
    s->w_pre = c > G ? (G - e0 + padw) : -1;
    s->w_clip_lo = s->label0 + G; s->w_clip_hi = s->label0 + stream_G(s, pc.first_sf + pc.count);
    s->w_next_sf = pc.first_sf + pc.count;
  }
  return DVBT_OK;
}

// The CP lock was lost inside piece `pc` (or the piece found no superframe start): the stream leaves the epoch.  World 1: the walk starts at the piece's begin
// over everything pushed since (the pieces in flight behind it are dropped).  Sharded: the piece's own samples are walked, its packets trimmed to its share.
static int stream_enter_walk(dvbt_rx_stream *s, const StreamPiece &pc_in)
{
  StreamPiece pc = pc_in;
  s->status |= 2;
  s->log("piece %lld (first_sf %lld, samples [%lld, +%lld)) leaves the epoch: status %d first_out %d resume %lld; dc %lld pos %lld", pc.index, pc.first_sf, pc.begin, pc.n, pc.rep.status, pc.rep.first_out_symbol,
         (long long)pc.rep.resume_sample, s->dc, s->pos);
  if (s->world == 1) {
    // everything in flight must have stopped touching the buffers; the pieces behind this one are dropped
    for (int i = 0; i < s->nh; i++) { HIPCHK(hipStreamSynchronize(s->rx[i]->own_stream)); s->rx[i]->pending = false; }
    s->wh = 0; s->epoch_id++;
  } else s->wh = pc.handle;                                              // (its decode has finished; the rank's other handle may hold a piece in flight)
  if (s->direct_pending) { HIPCHK(hipEventSynchronize(s->ev_direct)); s->direct_pending = false; }
  hipStream_t st = s->rx[s->wh]->own_stream;
  if (!s->wbuf[0]) {   // the walk's own buffers
    s->wcap = (size_t)((long long)s->nh * (long long)s->cap + s->thr);
    for (int i = 0; i < 2; i++) if (s->wbuf[i].alloc(s->wcap) != hipSuccess) return fail(DVBT_ERR_HIP, "dvbt_rx_stream: walk buffer allocation failed");
  }
  const long long have_k = std::min(s->pos, pc.launch_at) - pc.begin;            // what the piece's own buffer holds
  long long total = have_k;
  if (s->borrow) {
    // (the samples are where the caller left them: the piece's, and -- one stream object -- everything pushed since)
    total = (s->world == 1 ? s->pos : pc.begin + have_k) - pc.begin;
    if ((size_t)total > s->wcap) return fail(DVBT_ERR_CAPACITY, "dvbt_rx_stream: walk buffer too small (internal sizing)");
    int r = stream_gather_regions(s, pc.begin, pc.begin + total, s->wbuf[0], st); if (r) return r;
  } else {
  HIPCHK(hipMemcpyAsync(s->wbuf[0], s->buf[pc.handle], sizeof(float2) * (size_t)have_k, hipMemcpyDeviceToDevice, st));
  }
  if (!s->borrow && s->world == 1 && s->pos > pc.begin + have_k) {
    // the samples behind it are in the buffers of the pieces behind it (launched, or the one being filled; each began in front of its predecessor's end and holds the stream
    // up to its own launch point): the walk's buffer takes from each what the ones before did not hold
    long long at = pc.begin + have_k;                                 // the stream is assembled up to here
    for (long long idx = pc.index + 1; at < s->pos; idx++) {
      const StreamPiece *nx = nullptr;
      for (const StreamPiece &q : s->inflight) if (q.index == idx) nx = &q;
      if (!nx && s->have_cur && s->cur.index == idx) nx = &s->cur;
      if (!nx || nx->begin > at) return fail(DVBT_ERR_STATE, "dvbt_rx_stream: samples behind a piece that lost the lock are not in memory (internal)");
      const long long end = std::min(s->pos, nx->launch_at), n = end - at;
      if (n <= 0) continue;
      if ((size_t)(at - pc.begin + n) > s->wcap) return fail(DVBT_ERR_CAPACITY, "dvbt_rx_stream: walk buffer too small (internal sizing)");
      HIPCHK(hipMemcpyAsync(s->wbuf[0] + (at - pc.begin), s->buf[nx->handle] + (at - nx->begin), sizeof(float2) * (size_t)n, hipMemcpyDeviceToDevice, st));
      total += n; at = end;
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  s->wb = s->wbuf[0]; s->wb_cap = s->wcap; s->wb_which = 0; s->wb_filled = pc.begin + total;
  { int r = walk_from_piece(s, pc); if (r) return r; }
  if (s->world > 1) {
    // sharded: only this piece's samples; the rank's next piece is decoded as planned
    const long long saved_pos = s->pos;
    s->pos = pc.begin + total;
    int r = stream_walk(s, false);
    s->pos = saved_pos;
    s->w_clip_lo = s->w_clip_hi = -1; s->w_pre = -1; s->w_relabel.clear(); s->in_pieces = true; s->wh = 0;
    return r;
  }
  s->inflight.clear(); s->have_cur = false; s->have_next = false;
  return stream_walk(s, false);
}

// a piece has finished on the device: trim and queue its packets
static int stream_harvest(dvbt_rx_stream *s, StreamPiece &pc)
{
  dvbt_rx *h = s->rx[pc.handle].get();
  { int r = dvbt_rx_segment_finish(h, &pc.rep); if (r) return r; }
  if (!s->in_pieces) return DVBT_OK;                                     // (dropped: a walk has taken over in front of it)
  bool lost_inside = (pc.rep.status & 2) && pc.rep.resume_sample && pc.rep.resume_sample < pc.n - pc.skip - 4 * s->L;
  if (lost_inside && pc.skip == 0 && pc.rep.resume_sample < (stream_pre(s) + s->post) * s->L) {
    // the lock is lost in the stretch the chain before this one has seen it hold (stream_probe_skip): the piece's acquisition starts a symbol or two later
    hipStream_t st = h->own_stream;
    const float2 *iq; { int r = stream_piece_samples(s, pc, st, &iq); if (r) return r; }
    long long skip = 0; { int r = stream_probe_skip(s, h, iq, pc.n, st, &skip, STREAM_WALK_SKIP_MAX); if (r) return r; }
    pc.skip = skip;                                                  // (beyond what the piece's own TPS frame search can give up: the walk takes it from there, counters preset)
    if (skip > 0 && skip <= STREAM_PIECE_SKIP_MAX * s->L) {
      dvbt_rx_cut cut = {272 * pc.first_sf, s->delay, pc.phase}; { int r = dvbt_rx_set_cut(h, &cut); if (r) return r; }
      { int r = enqueue(h, iq + skip, (size_t)(pc.n - skip), st); if (r) return r; }
      { int r = dvbt_rx_segment_finish(h, &pc.rep); if (r) return r; }
      lost_inside = (pc.rep.status & 2) && pc.rep.resume_sample && pc.rep.resume_sample < pc.n - pc.skip - 4 * s->L;
    }
  }
  const dvbt_rx_report &rep = pc.rep;
  if (lost_inside || rep.first_out_symbol < 0) return stream_enter_walk(s, pc);
  s->status |= rep.status & ~2;                                           // bit 1 alone: the lock ended with the piece's samples
  const long long e0 = pc.first_sf * s->wsf;                              // the piece's RS word 0 in the epoch
  const long long g = e0 + rep.ts_first_packet;                           // epoch word of the TS tap's first packet
  const long long have = rep.n_ts_bytes / 188;
  if (s->world > 1) {
    // sharded: the piece's share on the transmitted NSYNC grid
    const long long G = stream_G(s, pc.first_sf);
    if (g != G || h->st_host->descr_unclean) s->status |= 64;             // the piece's NSYNC is not where the stream's arithmetic puts it (sync byte hit by noise)
    long long a = G, b = stream_G(s, pc.first_sf + pc.count);
    if (a < g || b - g > have) { s->status |= 32; if (b - g > have) b = g + have; if (a < g) a = g; }
    if (b <= a) return DVBT_OK;
    return stream_emit_bytes(s, h, h->ts_out + (size_t)(a - g) * 188, (size_t)(b - a) * 188, s->label0 + a, true);
  }
  // world 1: the descrambler's calls that start in [dc, first call at or behind the next piece's word 11)
  const long long next_lo = (pc.first_sf + pc.count) * s->wsf + 11;
  const int phase_now = (int)(((s->dc - e0) % 16 + 16) % 16) + 1;
  if (!h->st_host->descr_unclean && pc.phase == phase_now && s->dc >= g && ((s->dc - g) % 8) == 0) {
    const long long a = s->dc, b = stream_call_from(s->dc, next_lo);
    if (b - g <= have) {
      int r = stream_emit_bytes(s, h, h->ts_out + (size_t)(a - g) * 188, (size_t)(b - a) * 188, s->label0 + a, true); if (r) return r;
      s->dc = b;
      return DVBT_OK;
    }
  }
  // the stream's descrambler searches again inside this piece (a sync byte the RS decoder could not restore, a phase another piece left behind): followed call
  // by call on the piece's sync bitmap.  Items are counted on the epoch's grid: the piece's words are shifted by e0 mod 16
  s->status |= 64;
  s->log("piece %lld: descrambler followed on the host (unclean %d, phase %d / %d, dc %lld, g %lld, have %lld)", pc.index, h->st_host->descr_unclean, pc.phase, phase_now, s->dc, g, have);
  const long long nw = rep.n_rs_bytes / 188;
  { int r = stream_fetch_bits(s, h, 0, nw); if (r) return r; }
  const long long sh = ((e0 % 16) + 16) % 16;
  DescrState ds = descr_at(s->dc - e0 + sh);
  s->runs_host.clear(); long long written = 0;
  descr_walk(s->bits_host, sh, (nw + sh) / 8, next_lo - e0 + sh, ds, s->runs_host, written);
  for (DescrRun &r : s->runs_host) r.src_byte -= sh * 188;
  const long long dc_new = ds.start() - sh + e0;
  s->w_label = s->label0 + s->dc;
  { int r = stream_emit_runs(s, h, s->runs_host, written, true, 0, true); if (r) return r; }
  s->label0 += written / 188 - (dc_new - s->dc);                          // the labels go on counting the packets that went out
  s->dc = dc_new;
  return DVBT_OK;
}

static int stream_harvest_handle(dvbt_rx_stream *s, int handle)
{
  for (size_t i = 0; i < s->inflight.size(); i++)
    if (s->inflight[i].handle == handle) { StreamPiece q = s->inflight[i]; s->inflight.erase(s->inflight.begin() + i); return stream_harvest(s, q); }
  return DVBT_OK;
}

// this rank's next piece becomes the one being filled; what the stream has already delivered of it sits in `from_mem` (the buffer of the piece before, or the
// walk's), whose first sample is stream sample from_begin
static int stream_begin_next(dvbt_rx_stream *s, const float2 *from_mem, long long from_begin, int from_handle, hipStream_t from_stream, long long after_index)
{
  StreamPiece nx; stream_plan_piece(s, stream_next_owned(s, after_index), nx);
  nx.handle = (s->last_handle + 1) % s->nh;
  s->have_cur = false; s->have_next = true; s->next = nx;
  if (nx.begin > s->pos) return DVBT_OK;                                  // its samples have not arrived yet
  // its handle may still hold the piece before the previous one: those packets go out first
  { const long long ep = s->epoch_id; int r = stream_harvest_handle(s, nx.handle); if (r) return r;
    if (!s->in_pieces || ep != s->epoch_id) return DVBT_OK; }             // (that harvest found a lost lock: the walk has taken over, this plan is void)
  const long long ov = s->pos - nx.begin;
  if (ov > 0 && !s->borrow) {                                            // (borrowed samples stay where they are until the piece is launched)
    if (!from_mem || nx.begin < from_begin || nx.handle == from_handle) return fail(DVBT_ERR_STATE, "dvbt_rx_stream: piece plan out of range (internal)");
    if ((size_t)ov > s->cap) return fail(DVBT_ERR_CAPACITY, "dvbt_rx_stream: piece exceeds its buffer (internal sizing)");
    hipStream_t sn = s->rx[nx.handle]->own_stream;
    const int ei = from_handle < 0 ? nx.handle : from_handle;
    // [nx.begin, pos) -> the other buffer, behind everything written into this one and in front of what that handle does next
    HIPCHK(hipEventRecord(s->ev_written[ei], from_stream));
    HIPCHK(hipStreamWaitEvent(sn, s->ev_written[ei], 0));
    HIPCHK(hipMemcpyAsync(s->buf[nx.handle], from_mem + (nx.begin - from_begin), sizeof(float2) * (size_t)ov, hipMemcpyDeviceToDevice, sn));
    HIPCHK(hipEventRecord(s->ev_copied[ei], sn));
    HIPCHK(hipStreamWaitEvent(from_stream, s->ev_copied[ei], 0));        // that buffer is overwritten (two pieces on) only after the copy has read it
  }
  s->cur = nx; s->have_cur = true; s->have_next = false;
  return DVBT_OK;
}

// decode the piece being filled as a piece of the plan (samples [begin, end))
static int stream_launch(dvbt_rx_stream *s)
{
  StreamPiece pc = s->cur;
  const int hi = pc.handle;
  dvbt_rx *h = s->rx[hi].get();
  hipStream_t st = h->own_stream;
  pc.n = std::min(pc.end, s->pos) - pc.begin;
  const long long e0 = pc.first_sf * s->wsf;
  pc.phase = s->world == 1 && s->dc_valid ? (int)(((s->dc - e0) % 16 + 16) % 16) + 1 : 0;
  dvbt_rx_cut cut = {272 * pc.first_sf, s->delay, pc.phase}; { int r = dvbt_rx_set_cut(h, &cut); if (r) return r; }
  const float2 *iq; { int r = stream_piece_samples(s, pc, st, &iq); if (r) return r; }   // (borrowed samples: decoded in place when one region holds the piece)
  { int r = enqueue(h, iq, (size_t)pc.n, st); if (r) return r; }
  s->last_handle = hi;
  s->inflight.push_back(pc);
  return DVBT_OK;
}

// the end of the stream inside an epoch: the piece being filled runs to the stream's end -- as a walk window that continues the epoch (its cut, the epoch's
// counters, the descrambler's next call), through every loss of the lock and with the stream-end roundings
static int stream_finish_in_pieces(dvbt_rx_stream *s)
{
  // everything before must be out first (order)
  while (!s->inflight.empty() && s->in_pieces) { StreamPiece q = s->inflight.front(); s->inflight.erase(s->inflight.begin()); int r = stream_harvest(s, q); if (r) return r; }
  if (!s->in_pieces) return stream_walk(s, true);                         // a harvest found a lost lock: the walk that took over runs to the end
  if (!s->have_cur) { s->finished = true; return DVBT_OK; }
  const bool is_final = s->pos >= s->cur.begin + s->thr;                  // (sharded streams: else the piece before it, another rank's, covers these samples)
  if (!is_final) { s->finished = true; return DVBT_OK; }
  StreamPiece pc = s->cur;
  for (int i = 0; i < s->nh; i++) HIPCHK(hipStreamSynchronize(s->rx[i]->own_stream));
  if (s->direct_pending) { HIPCHK(hipEventSynchronize(s->ev_direct)); s->direct_pending = false; }
  s->wb = s->buf[pc.handle]; s->wb_cap = s->cap; s->wb_which = -1; s->wh = 0; s->wb_filled = s->borrow ? pc.begin : s->pos;
  s->wb_begin = pc.begin;
  { int r = walk_fill(s); if (r) return r; }                               // (borrowed samples: gathered into the piece's buffer)
  { int r = stream_probe_skip(s, s->rx[0].get(), s->wb, s->pos - pc.begin, s->rx[0]->own_stream, &pc.skip, STREAM_WALK_SKIP_MAX); if (r) return r; }
  { int r = walk_from_piece(s, pc); if (r) return r; }
  if (s->world > 1) s->w_clip_hi = 1ll << 61;                             // the stream's last piece: everything behind its first packet is this rank's
  s->have_cur = false;
  return stream_walk(s, true);
}

static int stream_append(dvbt_rx_stream *s, const float2 *src, size_t n, bool device, hipStream_t user)
{
  while (n) {
    float2 *dst; hipStream_t st; size_t take;
    if (!s->in_pieces) {
      // the walk: the samples gather in its buffer until the next window is due (walk_at never lies beyond the buffer)
      st = s->rx[s->wh]->own_stream;
      const long long room = std::min(s->walk_at, s->wb_begin + (long long)s->wb_cap) - s->pos;
      if (room <= 0) { int r = stream_walk(s, false); if (r) return r; continue; }
      take = (size_t)std::min<long long>((long long)n, room);
      dst = s->wb + (s->pos - s->wb_begin);
    } else if (!s->have_cur) {
      // between two of this rank's pieces: the samples in front of the next one are another rank's
      if (!s->have_next) return fail(DVBT_ERR_STATE, "dvbt_rx_stream: no piece planned (internal)");
      const long long skip = std::min<long long>((long long)n, s->next.begin - s->pos);
      if (skip > 0) { s->pos += skip; src += skip; n -= (size_t)skip; }
      if (s->pos >= s->next.begin) {
        { const long long ep = s->epoch_id; int r = stream_harvest_handle(s, s->next.handle); if (r) return r;
          if (!s->in_pieces || ep != s->epoch_id) continue; }
        s->cur = s->next; s->have_cur = true; s->have_next = false;
      }
      continue;
    } else {
      StreamPiece &f = s->cur;
      const long long room = f.launch_at - s->pos;
      take = (size_t)std::min<long long>((long long)n, std::max<long long>(room, 0));
      st = s->rx[f.handle]->own_stream;
      if ((size_t)(s->pos - f.begin) + take > s->cap) return fail(DVBT_ERR_CAPACITY, "dvbt_rx_stream: piece exceeds its buffer (internal sizing)");
      dst = s->buf[f.handle] + (s->pos - f.begin);
    }
    if (take) {
      if (device && s->borrow) {
        // nothing moves: the stream remembers where the samples are (a neighbour in the stream AND in memory extends the last region)
        if (!s->regions.empty() && s->regions.back().pos0 + s->regions.back().n == s->pos && s->regions.back().ptr + s->regions.back().n == src) s->regions.back().n += (long long)take;
        else s->regions.push_back(dvbt_rx_stream::Region{s->pos, src, (long long)take});
      } else if (device) {
        if (user && user != st) { const int ei = s->in_pieces ? s->cur.handle : 0; HIPCHK(hipEventRecord(s->ev_written[ei], user)); HIPCHK(hipStreamWaitEvent(st, s->ev_written[ei], 0)); }   // the caller's samples are ready when its stream says so
        HIPCHK(hipMemcpyAsync(dst, src, sizeof(float2) * take, hipMemcpyDeviceToDevice, st));
      } else {
        // through the pinned ring: the samples have left the caller's buffer when memcpy returns; the H2D copy is queued on the piece's stream (behind the
        // decode that may still read this buffer's previous contents: that ordering is the stream's, the host does not wait for it)
        constexpr size_t slot_samples = STREAM_PIN_BYTES / sizeof(float2);
        if (take * sizeof(float2) >= STREAM_DIRECT_BYTES) {
          if (s->direct_pending) HIPCHK(hipEventSynchronize(s->ev_direct));                // (a push that spans two pieces: the first part's copy, on the other chain's stream)
          HIPCHK(hipMemcpyAsync(dst, src, sizeof(float2) * take, hipMemcpyHostToDevice, st));
          HIPCHK(hipEventRecord(s->ev_direct, st)); s->direct_pending = true;
        } else {
          if (!s->pin) {   // (it could not be had at create: once more, now that it is needed)
            if (s->pin.alloc(STREAM_PIN_BYTES * STREAM_PIN_SLOTS) != hipSuccess) return fail(DVBT_ERR_HIP, "dvbt_rx_stream: pinned staging allocation failed");
            for (int i = 0; i < STREAM_PIN_SLOTS; i++)
              if (s->pin_ev[i].create(hipEventDisableTiming) != hipSuccess) return fail(DVBT_ERR_HIP, "dvbt_rx_stream: event creation failed");
          }
          for (size_t done = 0; done < take;) {
            const size_t n1 = std::min(take - done, slot_samples);
            const int k = s->pin_next; s->pin_next = (k + 1) % STREAM_PIN_SLOTS;
            if (s->pin_busy[k]) HIPCHK(hipEventSynchronize(s->pin_ev[k]));                 // the ring has gone round: wait for that slot's copy
            uint8_t *slot = s->pin + (size_t)k * STREAM_PIN_BYTES;
            memcpy(slot, src + done, n1 * sizeof(float2));
            HIPCHK(hipMemcpyAsync(dst + done, slot, n1 * sizeof(float2), hipMemcpyHostToDevice, st));
            HIPCHK(hipEventRecord(s->pin_ev[k], st)); s->pin_busy[k] = true;
            done += n1;
          }
        }
      }
      s->pos += (long long)take; src += take; n -= take;
    }
    if (!s->in_pieces) { if (s->pos >= std::min(s->walk_at, s->wb_begin + (long long)s->wb_cap)) { int r = stream_walk(s, false); if (r) return r; } continue; }
    if (s->have_cur && s->pos >= s->cur.launch_at) {
      const StreamPiece done = s->cur;
      int r = stream_launch(s); if (r) return r;
      r = stream_begin_next(s, s->buf[done.handle], done.begin, done.handle, s->rx[done.handle]->own_stream, done.index); if (r) return r;
    }
  }
  return DVBT_OK;
}

// TPS auto-configuration: a probe chain (QPSK 1/2 non-hierarchical for the fields that are AUTO: the front end -- acquisition, FFT, pilots, the TPS carriers'
// DBPSK, the BCH check -- does not depend on them) over the head of the stream kept on the host; a BCH-valid TPS word (reference_signals_impl.cc:385-425,
// layout :883-916) names constellation, hierarchy and the HP code rate.  Then the chains are built and the head is replayed into them.
// Returns 1 = configured, 0 = no valid TPS word in this much of the stream, < 0 = error
static int stream_autodetect(dvbt_rx_stream *s)
{
  dvbt_rx_params q = s->prm.rx;
  if (q.constellation == DVBT_AUTO) q.constellation = DVBT_QPSK;
  if (q.hierarchy == DVBT_AUTO) q.hierarchy = DVBT_NH;
  if (q.code_rate == DVBT_AUTO) q.code_rate = DVBT_C1_2;
  q.max_samples = s->head.size(); q.resample_interp = q.resample_decim = 0; q.soft_decision = 0; q.descramble = 0; q.launch_graph = 0;
  dvbt_rx *probe = nullptr;
  int r = dvbt_rx_create(&q, &probe); if (r) return r;
  dvbt_rx_report rep;
  r = dvbt_rx_segment_run(probe, s->head.data(), s->head.size(), &rep);
  dvbt_rx_destroy(probe);
  if (r) return r;
  s->auto_tries++;
  if (!rep.tps_valid) return 0;
  if (rep.tps_constellation > 2 || rep.tps_hierarchy > 3 || rep.tps_code_rate_hp > 4) return 0;      // reserved encodings: not a word this chain can follow
  const dvbt_rx_params before = s->prm.rx;
  if (s->prm.rx.constellation == DVBT_AUTO) s->prm.rx.constellation = rep.tps_constellation;
  if (s->prm.rx.hierarchy == DVBT_AUTO) s->prm.rx.hierarchy = rep.tps_hierarchy;
  if (s->prm.rx.code_rate == DVBT_AUTO) s->prm.rx.code_rate = rep.tps_code_rate_hp;
  r = stream_setup(s);
  if (r) {
    // the stream signals something the chains cannot be built for (hierarchical QPSK, no memory): the stream has failed -- nothing half-built is kept, no
    // later push probes again (ADVICE r04)
    s->prm.rx = before; s->auto_pending = false; s->finished = true; s->status |= 4; s->head.clear(); s->head.shrink_to_fit();
    return r;
  }
  s->det_constellation = s->prm.rx.constellation; s->det_hierarchy = s->prm.rx.hierarchy; s->det_code_rate = s->prm.rx.code_rate;
  s->auto_pending = false;
  std::vector<float2> head; head.swap(s->head);
  r = stream_append(s, head.data(), head.size(), false, nullptr); if (r) return r;
  if (s->direct_pending) { HIPCHK(hipEventSynchronize(s->ev_direct)); s->direct_pending = false; }   // (the replayed head leaves `head` before it is freed)
  for (int i = 0; i < STREAM_PIN_SLOTS; i++) if (s->pin_busy[i]) { HIPCHK(hipEventSynchronize(s->pin_ev[i])); s->pin_busy[i] = false; }
  return 1;
}
// samples that arrive while the parameters are still unknown
static int stream_auto_take(dvbt_rx_stream *s, const float2 *src, size_t n, bool device, hipStream_t user)
{
  const size_t at = s->head.size();
  s->head.resize(at + n);
  if (device) { if (user) HIPCHK(hipStreamSynchronize(user)); HIPCHK(hipMemcpy(s->head.data() + at, src, sizeof(float2) * n, hipMemcpyDeviceToHost)); }
  else memcpy(s->head.data() + at, src, sizeof(float2) * n);
  if ((long long)s->head.size() < s->auto_need) return DVBT_OK;
  const int r = stream_autodetect(s); if (r < 0) return r;
  if (r == 0) {
    // no TPS word yet (a stream that begins with silence, a lock lost inside the head): look again with twice as much, up to ~4 superframes; then give up
    if (s->auto_tries >= 4) { s->status |= 4; s->finished = true; s->auto_pending = false; s->head.clear(); s->head.shrink_to_fit(); return fail(DVBT_ERR_STATE, "dvbt_rx_stream: no valid TPS word found, parameters cannot be detected"); }
    s->auto_need *= 2;
  }
  return DVBT_OK;
}

extern "C" int dvbt_rx_stream_push(dvbt_rx_stream *s, const void *iq_host, size_t nsamples)
{
  if (!s || (!iq_host && nsamples)) return fail(DVBT_ERR_INVALID, "null argument");
  if (s->finished) return fail(DVBT_ERR_STATE, "dvbt_rx_stream: push after finish");
  HIPCHK(hipSetDevice(s->prm.rx.device));
  if (s->auto_pending) return stream_auto_take(s, (const float2 *)iq_host, nsamples, false, nullptr);
  if (s->borrow) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_push: the stream borrows its samples from device memory (borrow_device_pushes): dvbt_rx_stream_push_device only");
  // the samples have left the caller's buffer when this returns (they sit in the pinned ring or on the device); small pushes wait for nothing,
  // a large one for its own copy
  int r = stream_append(s, (const float2 *)iq_host, nsamples, false, nullptr);
  if (s->direct_pending) { HIPCHK(hipEventSynchronize(s->ev_direct)); s->direct_pending = false; }
  return r;
}

extern "C" int dvbt_rx_stream_push_device(dvbt_rx_stream *s, const void *iq_device, size_t nsamples, void *stream)
{
  if (!s || (!iq_device && nsamples)) return fail(DVBT_ERR_INVALID, "null argument");
  if (s->finished) return fail(DVBT_ERR_STATE, "dvbt_rx_stream: push after finish");
  HIPCHK(hipSetDevice(s->prm.rx.device));
  if (s->auto_pending) return stream_auto_take(s, (const float2 *)iq_device, nsamples, true, (hipStream_t)stream);
  if (s->borrow && stream) HIPCHK(hipStreamSynchronize((hipStream_t)stream));   // (borrowed samples are read later, on the chains' streams: they must be there)
  const int r = stream_append(s, (const float2 *)iq_device, nsamples, true, (hipStream_t)stream);
  stream_release_regions(s);
  return r;
}

extern "C" int dvbt_rx_stream_finish(dvbt_rx_stream *s)
{
  if (!s) return fail(DVBT_ERR_INVALID, "null handle");
  if (s->finished) return DVBT_OK;
  HIPCHK(hipSetDevice(s->prm.rx.device));
  if (s->auto_pending) {   // the stream ended before the parameters were known: one attempt on what there is
    int r = (long long)s->head.size() >= 2 * 8192 + 2048 + 16 ? stream_autodetect(s) : 0;
    if (r < 0) return r;
    if (r == 0) { s->status |= 4; s->finished = true; s->auto_pending = false; s->head.clear(); return DVBT_OK; }
  }
  if (s->in_pieces) { int r = stream_finish_in_pieces(s); if (r) return r; }
  else { int r = stream_walk(s, true); if (r) return r; }
  s->finished = true;
  return DVBT_OK;
}

// pieces whose decode has finished on the device, oldest first (never waits for the device unless the stream is finished)
static int stream_collect(dvbt_rx_stream *s)
{
  if (s->auto_pending) return DVBT_OK;                             // nothing decoded before the parameters are known
  while (!s->inflight.empty() && s->in_pieces) {
    StreamPiece &q = s->inflight.front();
    if (!s->finished && hipStreamQuery(s->rx[q.handle]->own_stream) != hipSuccess) break;
    StreamPiece c = q; s->inflight.erase(s->inflight.begin());
    int r = stream_harvest(s, c); if (r) return r;
  }
  return DVBT_OK;
}

static void stream_pop(dvbt_rx_stream *s)
{
  const StreamChunk &c = s->fifo.front();
  if (c.in_ring) {   // the ring's tail moves to the next chunk that lives in it (chunks leave in the order they came)
    size_t next = TsRing::NONE;
    for (size_t i = 1; i < s->fifo.size(); i++) if (s->fifo[i].in_ring) { next = (size_t)(s->fifo[i].data - s->ts_ring); break; }
    s->ring.release(next);
  }
  s->fifo.pop_front(); s->fifo_off = 0;
}

extern "C" int dvbt_rx_stream_set_device_output(dvbt_rx_stream *s, size_t ring_bytes)
{
  if (!s) return fail(DVBT_ERR_INVALID, "null handle");
  if (s->pos || s->packets_out) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_set_device_output: before the first push");
  s->dev_out = true; s->dring_bytes = ring_bytes ? ring_bytes : (64u << 20);
  s->ts_ring.reset(); s->ring.cap = 0;  // (nothing is delivered through the host ring any more)
  return DVBT_OK;
}

// device output: up to max_packets of the oldest waiting chunk (never across two chunks) -> dst (device), copied on `st`; the chunk's memory is released when the
// exchange step that reads it has completed (stream_release_taken(buffer))
struct DevTake { size_t take = 0; bool moved = false; };          // what stream_take_device did (stream_untake_device undoes it)
static int stream_take_device(dvbt_rx_stream *s, uint8_t *dst, int max_packets, hipStream_t st, int buffer, int64_t *first_packet, int64_t *nbytes, DevTake *tok = nullptr)
{
  *first_packet = 0; *nbytes = 0;
  int r = stream_collect(s); if (r) return r;
  if (s->dfifo.empty()) return DVBT_OK;
  DevChunk &c = s->dfifo.front();
  const size_t take = std::min((size_t)max_packets * 188, c.len - c.off);
  *first_packet = c.first_packet + (int64_t)(c.off / 188); *nbytes = (int64_t)take;
  HIPCHK(hipMemcpyAsync(dst, c.data + c.off, take, hipMemcpyDeviceToDevice, st));
  c.off += take; s->bytes_pulled += (long long)take;
  if (tok) { tok->take = take; tok->moved = false; }
  if (c.off == c.len) { s->dzombie.push_back(std::move(c)); s->dzombie_of[buffer]++; s->dfifo.pop_front(); if (tok) tok->moved = true; }
  return DVBT_OK;
}
// the exchange step that was to carry the run did not take place: the run is the stream's oldest waiting one again
static void stream_untake_device(dvbt_rx_stream *s, int buffer, const DevTake &tok)
{
  if (!tok.take) return;
  if (tok.moved && !s->dzombie.empty() && s->dzombie_of[buffer] > 0) { s->dfifo.push_front(std::move(s->dzombie.back())); s->dzombie.pop_back(); s->dzombie_of[buffer]--; }
  if (s->dfifo.empty()) return;
  DevChunk &c = s->dfifo.front();
  c.off -= std::min(c.off, tok.take); s->bytes_pulled -= (long long)tok.take;
}
static void stream_release_taken(dvbt_rx_stream *s, int buffer)
{
  for (; s->dzombie_of[buffer] > 0 && !s->dzombie.empty(); s->dzombie_of[buffer]--) {
    DevChunk c = std::move(s->dzombie.front()); s->dzombie.pop_front();
    if (c.stolen.mem) { s->ts_pool.push_back(std::move(c.stolen)); continue; }
    if (!c.in_ring) continue;                                        // (its own allocation goes with c)
    size_t next = TsRing::NONE;                                      // the ring's tail moves to the next chunk that lives in it (chunks leave in the order they came)
    for (const DevChunk &z : s->dzombie) if (z.in_ring) { next = (size_t)(z.data - s->dring); break; }
    if (next == TsRing::NONE) for (const DevChunk &z : s->dfifo) if (z.in_ring) { next = (size_t)(z.data - s->dring); break; }
    s->dalloc.release(next);
  }
  s->dzombie_of[buffer] = 0;
}

extern "C" int64_t dvbt_rx_stream_pull(dvbt_rx_stream *s, void *ts_host, size_t cap)
{
  if (!s || (!ts_host && cap)) return fail(DVBT_ERR_INVALID, "null argument");
  if (s->dev_out) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_pull: the stream's output lives on the device (dvbt_rx_stream_set_device_output): dvbt_rx_stream_gather_* delivers it");
  int r = stream_collect(s); if (r) return r;
  size_t done = 0;
  while (done < cap && !s->fifo.empty()) {
    const StreamChunk &v = s->fifo.front();
    const size_t take = std::min(cap - done, v.len - s->fifo_off);
    memcpy((uint8_t *)ts_host + done, v.data + s->fifo_off, take);
    done += take; s->fifo_off += take;
    if (s->fifo_off == v.len) stream_pop(s);
  }
  s->bytes_pulled += (long long)done;
  return (int64_t)done;
}

extern "C" int64_t dvbt_rx_stream_pull_chunk(dvbt_rx_stream *s, void *ts_host, size_t cap, int64_t *first_packet)
{
  if (!s || (!ts_host && cap) || !first_packet) return fail(DVBT_ERR_INVALID, "null argument");
  if (s->dev_out) return fail(DVBT_ERR_STATE, "dvbt_rx_stream_pull_chunk: the stream's output lives on the device (dvbt_rx_stream_set_device_output): dvbt_rx_stream_gather_* delivers it");
  int r = stream_collect(s); if (r) return r;
  if (s->fifo.empty()) return 0;
  StreamChunk &c = s->fifo.front();
  const size_t left = c.len - s->fifo_off;
  size_t take = std::min(cap, left);
  take -= take % 188;                                                    // whole packets: the index stays a packet index
  if (take == 0) return left ? fail(DVBT_ERR_CAPACITY, "dvbt_rx_stream_pull_chunk: room for less than one packet") : 0;
  *first_packet = c.first_packet + (int64_t)(s->fifo_off / 188);
  memcpy(ts_host, c.data + s->fifo_off, take);
  s->fifo_off += take;
  if (s->fifo_off == c.len) stream_pop(s);
  s->bytes_pulled += (long long)take;
  return (int64_t)take;
}

// the Viterbi stage's proof + repair passes (dvbt_rx_params.viterbi_verify) summed over every launch of the stream's two chains so far: chunks, chunks decoded again, chunks the
// sequential pass took (not_proven: -1, the streaming entry runs no final check unless rx.viterbi_verify asks for it -- and then the count is a launch's, not a sum).  Blocking.
extern "C" int dvbt_rx_stream_viterbi_proof(const dvbt_rx_stream *s, dvbt_viterbi_proof *out)
{
  if (!s || !out) return fail(DVBT_ERR_INVALID, "null argument");
  out->chunks = out->decoded_again = out->sequential = 0; out->not_proven = -1;
  for (int i = 0; i < s->nh; i++) {
    const dvbt_rx *h = s->rx[i].get();
    if (!h || !h->vproof.ctl) continue;
    int acc[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(acc, h->vproof.ctl + V3_CTL_ACC, sizeof acc, hipMemcpyDeviceToHost));
    out->chunks += acc[0]; out->decoded_again += acc[1]; out->sequential += acc[2];
  }
  return DVBT_OK;
}

extern "C" int dvbt_rx_stream_status(const dvbt_rx_stream *s, dvbt_rx_stream_info *info)
{
  if (!s || !info) return fail(DVBT_ERR_INVALID, "null argument");
  memset(info, 0, sizeof *info);
  info->status = s->status; info->samples_pushed = s->pos; info->ts_bytes_decoded = s->packets_out * 188; info->ts_bytes_pulled = s->bytes_pulled;
  size_t q = 0; for (auto &v : s->fifo) q += v.len; info->ts_bytes_ready = (int64_t)(q - s->fifo_off);
  for (auto &v : s->dfifo) info->ts_bytes_ready += (int64_t)(v.len - v.off);
  info->pieces_in_flight = (int32_t)s->inflight.size(); info->finished = s->finished ? 1 : 0;
  info->first_superframe_call = s->first_sf_call; info->first_ts_packet = s->first_q0;
  info->constellation = s->auto_pending ? -1 : s->prm.rx.constellation; info->hierarchy = s->auto_pending ? -1 : s->prm.rx.hierarchy;
  info->code_rate = s->auto_pending ? -1 : s->prm.rx.code_rate; info->auto_configured = s->det_constellation >= 0 ? 1 : 0;
  if (s->auto_pending) info->samples_pushed = (int64_t)s->head.size();
  info->in_walk = s->in_pieces ? 0 : 1;
  info->samples_released = s->borrow ? s->released : s->pos;
  return DVBT_OK;
}

// test hook (dvbt_hip.h): descr_walk on host bytes, window by window
extern "C" int64_t dvbt_debug_descr_follow(const uint8_t *rs, size_t nitems, const int64_t *windows, int nwindows, int64_t *runs_out, size_t cap_runs)
{
  if (!rs || !windows || nwindows < 1 || (!runs_out && cap_runs)) return fail(DVBT_ERR_INVALID, "null argument");
  const size_t npk = nitems * 8;
  std::vector<unsigned long long> bits((npk + 63) / 64, 0ull);
  for (size_t w = 0; w < npk; w++) if (rs[w * 188] == 0xB8) bits[w >> 6] |= 1ull << (w & 63);
  DescrState ds; std::vector<DescrRun> runs; long long written = 0, seen = 0;
  for (int k = 0; k < nwindows; k++) {
    if (windows[k] < seen || (size_t)windows[k] > nitems) return fail(DVBT_ERR_INVALID, "windows must ascend and stay inside the items");
    seen = windows[k];
    descr_walk(bits, 0, seen, 1ll << 62, ds, runs, written);
  }
  if (runs.size() > cap_runs) return fail(DVBT_ERR_CAPACITY, "more runs than the caller has room for");
  for (size_t i = 0; i < runs.size(); i++) { runs_out[2 * i] = runs[i].src_byte / 188; runs_out[2 * i + 1] = runs[i].nbytes / 188; }
  return (int64_t)runs.size();
}

extern "C" int64_t dvbt_rx_stream_trace(const dvbt_rx_stream *s, char *dst, size_t cap)
{
  if (!s || (!dst && cap)) return fail(DVBT_ERR_INVALID, "null argument");
  const size_t n = std::min(cap ? cap - 1 : 0, s->trace.size());
  if (cap) { memcpy(dst, s->trace.data(), n); dst[n] = 0; }
  return (int64_t)s->trace.size();
}

extern "C" void dvbt_rx_stream_destroy(dvbt_rx_stream *s)
{
  if (!s) return;
  for (int i = 0; i < dvbt_rx_stream::MAXH; i++) if (s->rx[i] && s->rx[i]->own_stream) (void)hipStreamSynchronize(s->rx[i]->own_stream);
  delete s;
}
