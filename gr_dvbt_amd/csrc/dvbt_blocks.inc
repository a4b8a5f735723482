// dvbt_blocks.inc -- per-block C ABI entry points (one create/forecast/work/destroy per
// reference block).  Every block has one `run` routine that enqueues its kernels on device buffers
// and a stream; dvbt_<blk>_work() stages the caller's HOST buffers through device memory around it
// (H2D, run, D2H, synchronise: the gr::block contract), dvbt_<blk>_work_device() hands the caller's
// DEVICE buffers and stream straight to it, so that adjacent HIP blocks of a flowgraph pass items
// without crossing PCIe.  State the reference block keeps in members lives in the handle.
// Included at the end of dvbt_hip.hip.

namespace {

struct PinBuf {           // growable pinned host staging (mem owns, p views: as DevBuf)
  PinMem<uint8_t> mem; void *p = nullptr; size_t cap = 0;
  int reserve(size_t n) { if (n <= cap) return DVBT_OK; p = nullptr; cap = 0; HIPCHK(mem.alloc(n + 64)); p = mem; cap = n; return DVBT_OK; }
};
// The host-pointer entries (dvbt_<blk>_work) move their items through PINNED staging buffers of the handle: memcpy + asynchronous H2D in, asynchronous D2H +
// memcpy out behind the call's one synchronisation.  A copy straight from / to the caller's pageable buffer makes the runtime pin and unpin those pages on
// every call (GNU Radio's buffers move through a circular mapping: never the same address twice in a row): 8-20 GB/s effective against ~50 for pinned memory,
// and the copies of the ten blocks' threads serialise inside the runtime.
struct BlockCtx {
  Stream s; DevBuf din, dout, aux; PinBuf pin_in, pin_out;   // (s first: released after the buffers its copies use)
  struct Pending { void *host; size_t off, bytes; };
  std::vector<Pending> pending; size_t pin_in_used = 0, pin_out_used = 0;
  int init() { int r = need_device(); if (r) return r; HIPCHK(s.create()); return DVBT_OK; }
  // a caller's buffer that is page-locked already (dvbt_host_register, or hipHostMalloc'd by the host) needs no staging: the DMA engines read / write it directly
  static bool is_pinned(const void *host)
  {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, host) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
  }
  int put(DevBuf &b, const void *host, size_t bytes, size_t offset = 0)
  {
    int r = b.reserve(offset + bytes); if (r) return r;
    if (!bytes) return DVBT_OK;
    if (is_pinned(host)) { HIPCHK(hipMemcpyAsync((char *)b.p + offset, host, bytes, hipMemcpyHostToDevice, s)); return DVBT_OK; }
    if (pin_in_used + bytes > pin_in.cap) {                        // full: what is staged already must have left first, then the buffer starts over
      if (pin_in_used) HIPCHK(hipStreamSynchronize(s));
      pin_in_used = 0;
      if (bytes > pin_in.cap) { r = pin_in.reserve(std::max(bytes, 2 * pin_in.cap)); if (r) return r; }   // grow only when the call itself does not fit (ADVICE r04)
    }
    char *st = (char *)pin_in.p + pin_in_used;
    memcpy(st, host, bytes);
    HIPCHK(hipMemcpyAsync((char *)b.p + offset, st, bytes, hipMemcpyHostToDevice, s));
    pin_in_used += (bytes + 63) & ~(size_t)63;
    return DVBT_OK;
  }
  int get(void *host, const void *dev, size_t bytes)
  {
    if (!bytes) return DVBT_OK;
    if (is_pinned(host)) { HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s)); return DVBT_OK; }   // complete at the call's sync()
    if (pin_out_used + bytes > pin_out.cap) {
      int r = sync(); if (r) return r;                             // deliver what is pending, then grow
      r = pin_out.reserve(std::max(bytes, 2 * pin_out.cap)); if (r) return r;
    }
    HIPCHK(hipMemcpyAsync((char *)pin_out.p + pin_out_used, dev, bytes, hipMemcpyDeviceToHost, s));
    pending.push_back(Pending{host, pin_out_used, bytes});
    pin_out_used += (bytes + 63) & ~(size_t)63;
    return DVBT_OK;
  }
  int sync()
  {
    HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipGetLastError());
    for (const Pending &q : pending) memcpy(q.host, (const char *)pin_out.p + q.off, q.bytes);
    pending.clear(); pin_in_used = 0; pin_out_used = 0;
    return DVBT_OK;
  }
  // history + new input made contiguous in din for a _work_device call: device-to-device on the caller's stream
  int put_dev(DevBuf &b, const void *dev, size_t bytes, size_t offset, hipStream_t st)
  { int r = b.reserve_keep(offset + bytes, offset, st); if (r) return r; if (bytes) HIPCHK(hipMemcpyAsync((char *)b.p + offset, dev, bytes, hipMemcpyDeviceToDevice, st)); return DVBT_OK; }
};
// NULL = the device's default stream: blocks chained without an explicit stream are ordered on it
inline hipStream_t pick(void *stream, const BlockCtx &) { return (hipStream_t)stream; }

inline const dvbt_tag *find_tag(const dvbt_sideband *sb, int key, int64_t lo, int64_t hi)
{
  if (!sb || !sb->in_tags) return nullptr;
  const dvbt_tag *best = nullptr;
  for (int i = 0; i < sb->n_in_tags; i++) {
    const dvbt_tag &t = sb->in_tags[i];
    if (t.key == key && t.rel_offset >= lo && t.rel_offset < hi && (!best || t.rel_offset < best->rel_offset)) best = &t;
  }
  return best;
}
inline void add_tag(dvbt_sideband *sb, int64_t off, int key, int value)
{
  if (!sb) return;
  if (sb->out_tags && sb->n_out_tags < sb->out_cap) { sb->out_tags[sb->n_out_tags].rel_offset = off; sb->out_tags[sb->n_out_tags].key = key; sb->out_tags[sb->n_out_tags].value = value; }
  sb->n_out_tags++;
}
inline void sb_begin(dvbt_sideband *sb) { if (sb) { sb->n_out_tags = 0; sb->n_consumed = 0; } }

}  // namespace

#define WCHK(x) do { int r_ = (x); if (r_) return r_; } while (0)
// the handle lives in `hold` until the create function hands it out (*out = hold.release()): every early return releases what has been built
#define BLK_CREATE_PROLOGUE(T) if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument"); std::unique_ptr<T> hold(new T()); T *const h = hold.get(); WCHK(h->c.init())

// ============================================================================ A2 fft
struct dvbt_fft { dvbt_fft_params p; BlockCtx c; Tables T; };
extern "C" int dvbt_fft_create(const dvbt_fft_params *p, dvbt_fft **out)
{
  BLK_CREATE_PROLOGUE(dvbt_fft);
  h->p = *p;
  int N = p->fft_size;
  // forward: the RX flowgraphs' fft_vxx(forward, shift=True); forward = 0: the TX flowgraphs' fft_vxx(reverse, shift=True) (k_fft.hpp)
  if (!p->shift || N < 64 || N > 8192 || (N & (N - 1))) return fail(DVBT_ERR_INVALID, "only shifted, power-of-two sizes 64..8192 (the configuration of the RX and TX flowgraphs)");
  WCHK(h->T.fft.build(N));
  WCHK(set_lds(p->forward ? (const void *)fft_items_kernel : (const void *)ifft_items_kernel, h->T.fft.lds()));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_fft_forecast(const dvbt_fft *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
static void fft_run(dvbt_fft *h, int n, const void *din, void *dout, hipStream_t s)
{
  const FftPlan &f = h->T.fft;
  if (h->p.forward) hipLaunchKernelGGL(fft_items_kernel, dim3(n), dim3(FFT_THREADS), f.lds(), s, (const float2 *)din, f.N, n, (const float2 *)f.tw, (float2 *)dout);
  else hipLaunchKernelGGL(ifft_items_kernel, dim3(n), dim3(FFT_THREADS), f.lds(), s, (const float2 *)din, f.N, n, (const float2 *)f.tw, (float2 *)dout);
}
extern "C" int dvbt_fft_work(dvbt_fft *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  size_t N = h->p.fft_size, bytes = (size_t)n * N * 8;
  WCHK(h->c.put(h->c.din, in, bytes)); WCHK(h->c.dout.reserve(bytes));
  fft_run(h, n, h->c.din.p, h->c.dout.p, h->c.s);
  WCHK(h->c.get(out, h->c.dout.p, bytes)); WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_fft_work_device(dvbt_fft *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  fft_run(h, n, in, out, pick(stream, h->c));
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" void dvbt_fft_destroy(dvbt_fft *h) { delete h; }

// ============================================================================ A4 dvbt_demap
struct dvbt_demap { dvbt_demap_params p; BlockCtx c; Tables T; };
extern "C" int dvbt_demap_create(const dvbt_demap_params *p, dvbt_demap **out)
{
  BLK_CREATE_PROLOGUE(dvbt_demap);
  h->p = *p;
  h->T.d = make_dims(p->constellation, p->hierarchy, 0, 0, p->transmission_mode);
  if (!h->T.d.valid || p->nsize <= 0 || p->nsize > 49152) return fail(DVBT_ERR_INVALID, "bad demap parameters");
  WCHK(h->T.build_inner(p->gain));
  WCHK(set_lds((const void *)inner_kernel<1>, inner_lds_bytes((size_t)p->nsize)));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_demap_forecast(const dvbt_demap *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
static void demap_run(dvbt_demap *h, int n, const void *din, void *dout, hipStream_t s)
{
  const size_t P = h->p.nsize;
  InnerParams ip = h->T.inner_params((int)P);
  hipLaunchKernelGGL(inner_kernel<1>, dim3(n), dim3(INNER_THREADS), inner_lds_bytes(P), s, (const float2 *)din, (const uint8_t *)nullptr, ip,
                     (const RxState *)nullptr, n, (const int *)nullptr, (const float2 *)h->T.points, (const unsigned char *)h->T.label_tab,
                     (const uint16_t *)nullptr, (const uint16_t *)nullptr, (uint8_t *)nullptr, (uint8_t *)nullptr, (uint8_t *)dout);
}
extern "C" int dvbt_demap_work(dvbt_demap *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  size_t P = h->p.nsize;
  WCHK(h->c.put(h->c.din, in, (size_t)n * P * 8)); WCHK(h->c.dout.reserve((size_t)n * P));
  demap_run(h, n, h->c.din.p, h->c.dout.p, h->c.s);
  WCHK(h->c.get(out, h->c.dout.p, (size_t)n * P)); WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_demap_work_device(dvbt_demap *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  demap_run(h, n, in, out, pick(stream, h->c));
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" void dvbt_demap_destroy(dvbt_demap *h) { delete h; }

// ============================================================================ A5 symbol_inner_interleaver
struct dvbt_symbol_inner_interleaver { dvbt_symbol_inner_interleaver_params p; BlockCtx c; Tables T; int symbol_index = 0; std::vector<int> idx; unsigned ring = 0; };
extern "C" int dvbt_symbol_inner_interleaver_create(const dvbt_symbol_inner_interleaver_params *p, dvbt_symbol_inner_interleaver **out)
{
  BLK_CREATE_PROLOGUE(dvbt_symbol_inner_interleaver);
  h->p = *p;
  h->T.d = make_dims(1, 0, 0, 0, p->transmission_mode);
  if (!h->T.d.valid || p->nsize != h->T.d.payload) return fail(DVBT_ERR_INVALID, "nsize must equal the payload length of the transmission mode (reference assert, symbol_inner_interleaver_impl.cc:125)");
  WCHK(h->T.build_inner(1.0f));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_symbol_inner_interleaver_forecast(const dvbt_symbol_inner_interleaver *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
// the items' symbol indices (tags on RX, a counter on TX) into h->idx; the table travels to the device ahead of the kernel
static int sym_indices(dvbt_symbol_inner_interleaver *h, int n, dvbt_sideband *sb)
{
  h->idx.assign(n, 0);
  for (int k = 0; k < n; k++) {
    if (h->p.direction) { h->idx[k] = h->symbol_index ^ 1; h->symbol_index = (h->symbol_index + 1) % 68; }   // TX parity rule is the mirror of RX (:182-209)
    else {
      const dvbt_tag *t = find_tag(sb, DVBT_TAG_SYMBOL_INDEX, k, k + 1);
      if (!t) return fail(DVBT_ERR_STATE, "de-interleave needs one SYMBOL_INDEX tag per item (symbol_inner_interleaver_impl.cc:199)");
      h->idx[k] = t->value;
    }
  }
  return DVBT_OK;
}
static int sym_run(dvbt_symbol_inner_interleaver *h, int n, const void *din, void *dout, hipStream_t s)
{
  const size_t P = h->p.nsize;
  // the index table of every call in flight needs its own device slot: a ring of 64 tables
  const size_t slot = (size_t)(h->ring++ & 63) * 4096 * 4;
  if (n > 4096) return fail(DVBT_ERR_CAPACITY, "at most 4096 items per call");
  WCHK(h->c.aux.reserve(64 * 4096 * 4));
  HIPCHK(hipMemcpyAsync((char *)h->c.aux.p + slot, h->idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  InnerParams ip; memset(&ip, 0, sizeof ip); ip.payload = (int)P; ip.m = 4;
  hipLaunchKernelGGL(inner_kernel<2>, dim3(n), dim3(INNER_THREADS), inner_lds_bytes(P), s, (const float2 *)nullptr, (const uint8_t *)din, ip,
                     (const RxState *)nullptr, n, (const int *)((char *)h->c.aux.p + slot), (const float2 *)nullptr, (const unsigned char *)nullptr,
                     (const uint16_t *)h->T.H, (const uint16_t *)h->T.Hinv, (uint8_t *)nullptr, (uint8_t *)nullptr, (uint8_t *)dout);
  return DVBT_OK;
}
extern "C" int dvbt_symbol_inner_interleaver_work(dvbt_symbol_inner_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  size_t P = h->p.nsize;
  WCHK(sym_indices(h, n, sb));
  WCHK(h->c.put(h->c.din, in, (size_t)n * P)); WCHK(h->c.dout.reserve((size_t)n * P));
  WCHK(sym_run(h, n, h->c.din.p, h->c.dout.p, h->c.s));
  WCHK(h->c.get(out, h->c.dout.p, (size_t)n * P)); WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_symbol_inner_interleaver_work_device(dvbt_symbol_inner_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  WCHK(sym_indices(h, n, sb));
  WCHK(sym_run(h, n, in, out, pick(stream, h->c)));
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" void dvbt_symbol_inner_interleaver_destroy(dvbt_symbol_inner_interleaver *h) { delete h; }

// ============================================================================ A6 bit_inner_deinterleaver
struct dvbt_bit_inner_deinterleaver { dvbt_bit_inner_deinterleaver_params p; BlockCtx c; Dims d; };
extern "C" int dvbt_bit_inner_deinterleaver_create(const dvbt_bit_inner_deinterleaver_params *p, dvbt_bit_inner_deinterleaver **out)
{
  BLK_CREATE_PROLOGUE(dvbt_bit_inner_deinterleaver);
  h->p = *p;
  h->d = make_dims(p->constellation, p->hierarchy, 0, 0, p->transmission_mode);
  if (!h->d.valid || p->nsize <= 0 || p->nsize % 126 || p->nsize > 49152) return fail(DVBT_ERR_INVALID, "nsize must be a positive multiple of 126");
  if (p->hierarchy != DVBT_NH && h->d.m == 2) return fail(DVBT_ERR_INVALID, "hierarchical QPSK does not exist (the reference's constructor divides by d_v - 2 = 0)");
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_bit_inner_deinterleaver_forecast(const dvbt_bit_inner_deinterleaver *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
static void bit_run(dvbt_bit_inner_deinterleaver *h, int n, const void *din, void *dout, hipStream_t s, void *dout_lp = nullptr)
{
  const size_t P = h->p.nsize;
  InnerParams ip; memset(&ip, 0, sizeof ip); ip.payload = (int)P; ip.m = h->d.m; ip.hier = h->p.hierarchy != DVBT_NH ? 1 : 0;
  hipLaunchKernelGGL(inner_kernel<4>, dim3(n), dim3(INNER_THREADS), inner_lds_bytes(P), s, (const float2 *)nullptr, (const uint8_t *)din, ip,
                     (const RxState *)nullptr, n, (const int *)nullptr, (const float2 *)nullptr, (const unsigned char *)nullptr,
                     (const uint16_t *)nullptr, (const uint16_t *)nullptr, (uint8_t *)nullptr, (uint8_t *)nullptr, (uint8_t *)dout, (uint8_t *)dout_lp);
}
// hierarchical modes: both output streams (io_signature (1, 2) of the reference block)
extern "C" int dvbt_bit_inner_deinterleaver_work_hier(dvbt_bit_inner_deinterleaver *h, int nout, int nin, const void *in, void *out_hp, void *out_lp, dvbt_sideband *sb)
{
  if (!h || !in || !out_hp || !out_lp) return fail(DVBT_ERR_INVALID, "null argument");
  if (h->p.hierarchy == DVBT_NH) return fail(DVBT_ERR_STATE, "a non-hierarchical bit_inner_deinterleaver has one output");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  size_t P = h->p.nsize;
  WCHK(h->c.put(h->c.din, in, (size_t)n * P)); WCHK(h->c.dout.reserve((size_t)n * P)); WCHK(h->c.aux.reserve((size_t)n * P));
  bit_run(h, n, h->c.din.p, h->c.dout.p, h->c.s, h->c.aux.p);
  WCHK(h->c.get(out_hp, h->c.dout.p, (size_t)n * P)); WCHK(h->c.get(out_lp, h->c.aux.p, (size_t)n * P)); WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_bit_inner_deinterleaver_work_hier_device(dvbt_bit_inner_deinterleaver *h, int nout, int nin, const void *in, void *out_hp, void *out_lp, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out_hp || !out_lp) return fail(DVBT_ERR_INVALID, "null argument");
  if (h->p.hierarchy == DVBT_NH) return fail(DVBT_ERR_STATE, "a non-hierarchical bit_inner_deinterleaver has one output");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  bit_run(h, n, in, out_hp, pick(stream, h->c), out_lp);
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_bit_inner_deinterleaver_work(dvbt_bit_inner_deinterleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  size_t P = h->p.nsize;
  WCHK(h->c.put(h->c.din, in, (size_t)n * P)); WCHK(h->c.dout.reserve((size_t)n * P));
  bit_run(h, n, h->c.din.p, h->c.dout.p, h->c.s);
  WCHK(h->c.get(out, h->c.dout.p, (size_t)n * P)); WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_bit_inner_deinterleaver_work_device(dvbt_bit_inner_deinterleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  bit_run(h, n, in, out, pick(stream, h->c));
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" void dvbt_bit_inner_deinterleaver_destroy(dvbt_bit_inner_deinterleaver *h) { delete h; }

// ============================================================================ A7 viterbi_decoder
// Streaming: the chunk decoders only need the input bytes back to (first wanted byte - warm-up), so the block keeps the tail of what it has consumed and the
// running step count since the last reset.  The reference runs ONE decoder over the stream (viterbi_decoder_impl.cc:192-324); so does this block, by construction:
// every call's launch proves its chunks against their predecessors and decodes the unproven ones again (k_viterbi3.hpp), and the decoder's state is carried from
// call to call -- the last chunk's decoder leaves it at the last top of a block of windows in front of the call's end (grid0: at most 23 bytes back), the next call's
// chunk 0 starts there with that state instead of a warm-up's and writes only the bytes the call owes.
struct dvbt_viterbi_decoder {
  dvbt_viterbi_decoder_params p; BlockCtx c; Dims d; VitParams vp;
  size_t hist = 0; long long in_total = 0, steps = 0; int d_init = 0;      // hist: bytes of consumed input kept at the front of din
  static constexpr size_t kTail = 8192;
  bool walk = false;                                                       // dvbt_viterbi_decoder_set_walk
  int chunk_next = 11 * V3_BLK, verify = VIT_REPAIR, verify_next = VIT_REPAIR;   // test hooks: dvbt_viterbi_decoder_set_chunk_bytes, _set_verify (both adopted at the next reset)
  VitProof proof; DevMem<int> carry; int cur = 0; bool have_carry = false; long long grid0 = 0;   // carry: 2 x 32 words (ping-pong), [cur] = the state at byte grid0
};
extern "C" int dvbt_viterbi_decoder_create(const dvbt_viterbi_decoder_params *p, dvbt_viterbi_decoder **out)
{
  BLK_CREATE_PROLOGUE(dvbt_viterbi_decoder);
  h->p = *p;
  h->d = make_dims(p->constellation, p->hierarchy, p->code_rate, 0, 0);
  if (!h->d.valid || p->bsize <= 0 || (2 * h->d.k * p->bsize) % 16 || (p->bsize * h->d.n) % h->d.m || (p->bsize * h->d.k) % 8)
    return fail(DVBT_ERR_INVALID, "bsize must make bsize*n/m and bsize*k/8 integral and 2*k*bsize a multiple of 16");
  h->vp = make_vit_params(h->d, p->bsize, 11 * V3_BLK);          // chunks of 264 bytes: a whole number of blocks of windows (the proof's condition)
  if (h->carry.alloc(2 * V3_SLOT) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMalloc (viterbi_decoder carry)");
  WCHK(h->proof.reserve(256));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_viterbi_decoder_forecast(const dvbt_viterbi_decoder *h, int n, int *req)
{ if (!h || !req) return DVBT_ERR_INVALID; *req = n * 8 * h->d.n / (h->d.k * h->d.m); return DVBT_OK; }   // viterbi_decoder_impl.cc:181-189
// one call, host or device buffers (dev): history (the input tail the chunk decoders' warm-up needs) + the new input are made
// contiguous in din; the decoded bytes land in `out` (device) or go through dout (host)
static int viterbi_call(dvbt_viterbi_decoder *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int d_nout = h->vp.d_nbits / 16, d_nsym = h->vp.d_nsymbols;
  int nblocks = nout / d_nout;                                   // :198
  if (nblocks * d_nsym > nin) nblocks = nin / d_nsym;
  if (nblocks <= 0) return 0;
  const dvbt_tag *t = find_tag(sb, DVBT_TAG_SUPERFRAME_START, 0, (int64_t)nblocks * d_nsym);
  if (t) {                                                       // :213-229
    h->d_init = 0; h->steps = 0; h->in_total = 0; h->hist = 0; h->have_carry = false; h->grid0 = 0;
    h->vp.chunk_bytes = h->chunk_next; h->verify = h->verify_next;   // (the test hooks: the chunk grid and the passes change where no state is carried)
    if (t->rel_offset > 0) { if (sb) sb->n_consumed = (int)t->rel_offset; return 0; }
    HIPCHK(hipMemsetAsync(h->proof.ctl + V3_CTL_ACC, 0, 3 * sizeof(int), s));
  }
  const size_t nbytes = (size_t)nblocks * d_nsym, hist = h->hist;
  WCHK(h->c.din.reserve_keep(dvbt_viterbi_decoder::kTail + nbytes + 64, hist, s));
  if (dev) WCHK(h->c.put_dev(h->c.din, in, nbytes, hist, s)); else { HIPCHK(hipMemcpyAsync((char *)h->c.din.p + hist, in, nbytes, hipMemcpyHostToDevice, s)); }
  const long long in_base = h->in_total - (long long)hist;
  long long out_lo = h->steps / 8 - h->d.ntb; if (out_lo < 0) out_lo = 0;
  h->steps += (long long)nblocks * (h->vp.d_nbits / 2);
  h->in_total += (long long)nbytes;
  long long out_hi = h->steps / 8 - h->d.ntb; if (out_hi < 0) out_hi = 0;
  const long long produced = out_hi - out_lo;
  if (produced > 0) {
    uint8_t *o = (uint8_t *)out;
    if (!dev) { WCHK(h->c.dout.reserve((size_t)produced)); o = (uint8_t *)h->c.dout.p; }
    const int B = h->vp.chunk_bytes;
    const long long g0 = h->have_carry ? h->grid0 : 0, chunks = (out_hi - g0 + B - 1) / B;
    if (chunks + 2 > h->proof.cap) { HIPCHK(hipStreamSynchronize(s)); int acc[8]; HIPCHK(hipMemcpy(acc, h->proof.ctl + V3_CTL_ACC, sizeof acc, hipMemcpyDeviceToHost));      // (the sums and the shortcut's counters: words 8..15)
                                     WCHK(h->proof.reserve(2 * chunks + 2)); HIPCHK(hipMemcpy(h->proof.ctl + V3_CTL_ACC, acc, sizeof acc, hipMemcpyHostToDevice)); }
    V3Aux ax = h->proof.aux();
    ax.grid0 = g0; ax.carry_in = h->have_carry ? h->carry + h->cur * V3_SLOT : nullptr;
    const long long b0_last = g0 + (chunks - 1) * B;
    ax.carry_rel = (int)((out_hi - b0_last) / V3_BLK) * V3_BLK; ax.carry_out = h->carry + (h->cur ^ 1) * V3_SLOT;
    launch_viterbi(s, (const uint8_t *)h->c.din.p, o, (const RxState *)nullptr, h->steps, h->vp, in_base, out_lo, produced, &ax, h->verify, h->walk);
    h->cur ^= 1; h->have_carry = true; h->grid0 = b0_last + ax.carry_rel;
    if (!dev) WCHK(h->c.get(out, h->c.dout.p, (size_t)produced));
  }
  // keep the tail for the next call's warm-up: through aux (source and destination may overlap)
  {
    const size_t total = hist + nbytes, keep = total < dvbt_viterbi_decoder::kTail ? total : dvbt_viterbi_decoder::kTail;
    if (total > keep) {
      WCHK(h->c.aux.reserve(dvbt_viterbi_decoder::kTail));
      HIPCHK(hipMemcpyAsync(h->c.aux.p, (const char *)h->c.din.p + total - keep, keep, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(h->c.din.p, h->c.aux.p, keep, hipMemcpyDeviceToDevice, s));
    }
    h->hist = keep;
  }
  if (!dev) WCHK(h->c.sync());
  if (h->d_init == 0) { add_tag(sb, 0, DVBT_TAG_SUPERFRAME_START, 1); h->d_init = 1; }     // :298-312
  if (sb) sb->n_consumed = (int)nbytes;
  return (int)produced;
}
extern "C" int dvbt_viterbi_decoder_work(dvbt_viterbi_decoder *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return viterbi_call(h, nout, nin, in, out, sb, false, h->c.s);
}
// The counts are fixed by the call's sizes and tags, so nothing is read back: the call only enqueues.
extern "C" int dvbt_viterbi_decoder_work_device(dvbt_viterbi_decoder *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return viterbi_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
// The chunk decoders' warm-up (dvbt_rx_params.viterbi_warm_windows for the single block; make()'s arguments have no room for it): 0 = the default of 72 windows, else a multiple of 24
// in [48, 576] -- the block keeps kTail = 8192 bytes of consumed input, which covers 576 + ntraceback windows in the hungriest mode (QPSK 1/2: 8 bytes per window).  Takes effect
// with the next call.  It moves speed only (fewer or more chunks to decode again): the bytes are the streaming decoder's at any warm-up.
extern "C" int dvbt_viterbi_decoder_set_warm_windows(dvbt_viterbi_decoder *h, int windows)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  if (windows == 0) windows = V3_WARM;
  if (windows < 2 * V3_BLK || windows > 576 || windows % V3_BLK != 0) return fail(DVBT_ERR_INVALID, "warm-up must be 0 (default) or a multiple of 24 in [48, 576]");
  h->vp.warm = windows;
  return DVBT_OK;
}
extern "C" int dvbt_viterbi_decoder_proof(dvbt_viterbi_decoder *h, dvbt_viterbi_proof *out)
{
  if (!h || !out) return fail(DVBT_ERR_INVALID, "null argument");
  int acc[3] = {0, 0, 0};
  HIPCHK(hipMemcpy(acc, h->proof.ctl + V3_CTL_ACC, sizeof acc, hipMemcpyDeviceToHost));      // (blocking: behind everything the block's stream holds)
  out->chunks = acc[0]; out->decoded_again = acc[1]; out->sequential = acc[2]; out->not_proven = -1;
  if (h->verify >= VIT_REPAIR_COUNT) {                           // the final check ran behind the last launch (dvbt_viterbi_decoder_set_verify)
    int un = -1;
    HIPCHK(hipMemcpy(&un, h->proof.ctl + V3_CTL_UNPROVEN, sizeof un, hipMemcpyDeviceToHost));
    out->not_proven = un;
  }
  return DVBT_OK;
}
// Test hooks.  The chunk size of the block's launches: 0 = the default of 264 bytes, else a multiple of 24 (a block of windows) in [24, 264].  Adopted by the next call that carries a
// superframe-start tag (a stream reset): the chunk grid never changes under a carried state.  proof.reserve grows with the chunk count and kTail covers the warm-up at any chunk size.
extern "C" int dvbt_viterbi_decoder_set_chunk_bytes(dvbt_viterbi_decoder *h, int bytes)
{
  if (bytes == 0) bytes = 11 * V3_BLK;
  if (bytes < V3_BLK || bytes > 11 * V3_BLK || bytes % V3_BLK != 0) return fail(DVBT_ERR_INVALID, "chunk size must be 0 (default) or a multiple of 24 in [24, 264]");
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  h->chunk_next = bytes;
  return DVBT_OK;
}
// dvbt_rx_params.viterbi_verify for the block's launches (-1 .. 4; the default is 0, proof + repair without the final check).  Adopted by the next call that
// carries a superframe-start tag, like the chunk size: the plain decoders (-1) carry no state and the proof alone (2) carries an unrepaired one, so a stream keeps its mode
extern "C" int dvbt_viterbi_decoder_set_verify(dvbt_viterbi_decoder *h, int mode)
{
  if (mode < VIT_PLAIN || mode > VIT_FORCE_CONFLICT) return fail(DVBT_ERR_INVALID, "verify mode must be in [-1, 4]");
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  h->verify_next = mode;
  return DVBT_OK;
}
// the 16 header words of the last launch's control block (k_viterbi3.hpp, V3_CTL_*); blocking, like _proof
extern "C" int dvbt_viterbi_decoder_last_ctl(dvbt_viterbi_decoder *h, int out[16])
{
  if (!h || !out) return fail(DVBT_ERR_INVALID, "null argument");
  HIPCHK(hipMemcpy(out, h->proof.ctl, V3_CTL_HDR * sizeof(int), hipMemcpyDeviceToHost));
  return DVBT_OK;
}
// the traceback's shortcut (k_viterbi3.hpp): always != 0 = every chain of the following calls walks all its hops; the counters of shortcut / walked iterations since the block was created
extern "C" int dvbt_viterbi_decoder_set_walk(dvbt_viterbi_decoder *h, int always)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  h->walk = always != 0;
  return DVBT_OK;
}
extern "C" int dvbt_viterbi_decoder_shortcut(dvbt_viterbi_decoder *h, long long out[2])
{
  if (!h || !out) return fail(DVBT_ERR_INVALID, "null argument");
  HIPCHK(hipMemcpy(out, h->proof.ctl + V3_CTL_SHORT, 2 * sizeof(long long), hipMemcpyDeviceToHost));      // (blocking: behind everything the block's stream holds)
  return DVBT_OK;
}
extern "C" void dvbt_viterbi_decoder_destroy(dvbt_viterbi_decoder *h) { delete h; }

// ============================================================================ A8 convolutional_deinterleaver
struct dvbt_convolutional_deinterleaver { dvbt_convolutional_deinterleaver_params p; BlockCtx c; size_t hist = 0; long long pos = 0; };   // hist: input bytes kept at the front of din
extern "C" int dvbt_convolutional_deinterleaver_create(const dvbt_convolutional_deinterleaver_params *p, dvbt_convolutional_deinterleaver **out)
{
  BLK_CREATE_PROLOGUE(dvbt_convolutional_deinterleaver);
  h->p = *p;
  if (p->I != 12 || p->M != 17 || p->blocks != 136) return fail(DVBT_ERR_INVALID, "only the DVB-T outer interleaver I=12, M=17, blocks=136 (every RX flowgraph; assert at convolutional_deinterleaver_impl.cc:68)");
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_convolutional_deinterleaver_forecast(const dvbt_convolutional_deinterleaver *h, int n, int *req)
{ if (!h || !req) return DVBT_ERR_INVALID; *req = n * h->p.I * h->p.blocks; return DVBT_OK; }
static int convdeint_call(dvbt_convolutional_deinterleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int item = h->p.I * h->p.blocks;
  int n = nout & ~1;                                             // set_output_multiple(2)
  if ((long long)n * item > nin) n = (nin / item) & ~1;
  if (n <= 0) return 0;
  const dvbt_tag *t = find_tag(sb, DVBT_TAG_SUPERFRAME_START, 0, (int64_t)n * item);
  if (t && t->rel_offset > 0) { if (sb) sb->n_consumed = (int)t->rel_offset; return 0; }   // :109-120 (FIFOs are not cleared: B-16)
  const size_t nbytes = (size_t)n * item, hist = h->hist, keep_max = 2244;
  WCHK(h->c.din.reserve_keep(keep_max + nbytes + 64, hist, s));
  if (dev) WCHK(h->c.put_dev(h->c.din, in, nbytes, hist, s)); else { HIPCHK(hipMemcpyAsync((char *)h->c.din.p + hist, in, nbytes, hipMemcpyHostToDevice, s)); }
  uint8_t *o = (uint8_t *)out;
  if (!dev) { WCHK(h->c.dout.reserve(nbytes)); o = (uint8_t *)h->c.dout.p; }
  hipLaunchKernelGGL(conv_deint_kernel, dim3(512), dim3(256), 0, s, (const uint8_t *)h->c.din.p, (long long)hist, h->pos, (long long)nbytes, o);
  if (!dev) WCHK(h->c.get(out, h->c.dout.p, nbytes));
  h->pos += (long long)nbytes;
  {
    const size_t total = hist + nbytes, keep = total < keep_max ? total : keep_max;
    if (total > keep) {
      WCHK(h->c.aux.reserve(keep_max));
      HIPCHK(hipMemcpyAsync(h->c.aux.p, (const char *)h->c.din.p + total - keep, keep, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(h->c.din.p, h->c.aux.p, keep, hipMemcpyDeviceToDevice, s));
    }
    h->hist = keep;
  }
  if (!dev) WCHK(h->c.sync());
  if (sb) sb->n_consumed = (int)nbytes;
  return n;
}
extern "C" int dvbt_convolutional_deinterleaver_work(dvbt_convolutional_deinterleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return convdeint_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_convolutional_deinterleaver_work_device(dvbt_convolutional_deinterleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return convdeint_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_convolutional_deinterleaver_destroy(dvbt_convolutional_deinterleaver *h) { delete h; }

// ============================================================================ A9 reed_solomon_dec
struct dvbt_reed_solomon_dec { dvbt_reed_solomon_dec_params p; BlockCtx c; Tables T; DevMem<int> cnt; };
extern "C" int dvbt_reed_solomon_dec_create(const dvbt_reed_solomon_dec_params *p, dvbt_reed_solomon_dec **out)
{
  BLK_CREATE_PROLOGUE(dvbt_reed_solomon_dec);
  h->p = *p;
  if (p->p != 2 || p->m != 8 || p->gfpoly != 0x11d || p->n != 255 || p->k != 239 || p->t != 8 || p->s != 51 || p->blocks <= 0)
    return fail(DVBT_ERR_INVALID, "only RS(255,239,t=8) over GF(2^8)/0x11d shortened by 51 (the DVB-T outer code)");
  WCHK(h->T.build_rs());
  if (h->cnt.alloc(2) != hipSuccess || hipMemset(h->cnt, 0, 8) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMalloc");
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_reed_solomon_dec_forecast(const dvbt_reed_solomon_dec *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
static void rs_run(dvbt_reed_solomon_dec *h, long long words, const void *din, void *dout, hipStream_t s)
{
  hipLaunchKernelGGL(deint_rs_kernel, dim3((unsigned)((words + 63) / 64)), dim3(64), 0, s, (const uint8_t *)din, (uint8_t *)nullptr,
                     (uint8_t *)dout, (RxState *)nullptr, words, 1, 0ll, h->T.rs_tables(), h->p.oracle_compat, h->cnt, h->cnt + 1);   // cnt: failures / corrections, cumulative
}
extern "C" int dvbt_reed_solomon_dec_work(dvbt_reed_solomon_dec *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  long long words = (long long)n * h->p.blocks;
  WCHK(h->c.put(h->c.din, in, (size_t)words * 204)); WCHK(h->c.dout.reserve((size_t)words * 188));
  rs_run(h, words, h->c.din.p, h->c.dout.p, h->c.s);
  WCHK(h->c.get(out, h->c.dout.p, (size_t)words * 188)); WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_reed_solomon_dec_work_device(dvbt_reed_solomon_dec *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  sb_begin(sb);
  int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  rs_run(h, (long long)n * h->p.blocks, in, out, pick(stream, h->c));
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" void dvbt_reed_solomon_dec_destroy(dvbt_reed_solomon_dec *h) { delete h; }

// ============================================================================ next row: energy_descramble
struct dvbt_energy_descramble { dvbt_energy_descramble_params p; BlockCtx c; Tables T; int d_index = 0; DevMem<RxState> dstate; unsigned ring = 0; };
extern "C" int dvbt_energy_descramble_create(const dvbt_energy_descramble_params *p, dvbt_energy_descramble **out)
{
  BLK_CREATE_PROLOGUE(dvbt_energy_descramble);
  h->p = *p;
  WCHK(h->T.build_rs());
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_energy_descramble_forecast(const dvbt_energy_descramble *, int n, int *req) { if (req) *req = 4 * (n / 1504); return DVBT_OK; }   // :101-105
static int descramble_call(dvbt_energy_descramble *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  nout -= nout % (4 * 1504);                                     // set_output_multiple(4*8*188), :90
  if (nout <= 0 || nin < nout / 1504) return 0;
  // NSYNC search over the first two items (:121-123): the 16 sync positions of the window
  uint8_t probe[16];
  if (dev) {   // 16 single bytes 188 apart: one strided copy + one synchronisation (the search decides how much is consumed)
    HIPCHK(hipMemcpy2DAsync(probe, 1, in, 188, 1, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  } else for (int i = 0; i < 16; i++) probe[i] = ((const uint8_t *)in)[i * 188];
  while (h->d_index < 2 * 1504 && probe[h->d_index / 188] != 0xB8) h->d_index += 188;
  if (h->d_index >= 2 * 1504) { h->d_index = 0; if (sb) sb->n_consumed = 2; return 0; }
  const int to_consume = nout / 1504 - 2;
  const size_t nbytes = (size_t)to_consume * 1504;
  const uint8_t *src = (const uint8_t *)in + h->d_index;
  if (!dev) { WCHK(h->c.put(h->c.din, src, nbytes)); WCHK(h->c.dout.reserve(nbytes)); }
  if (!h->dstate) {
    HIPCHK(h->dstate.alloc(64));
  }
  RxState st; memset(&st, 0, sizeof st); st.n_ts_bytes = (long long)nbytes;
  RxState *slot = h->dstate + (h->ring++ & 63);                   // a slot per call in flight
  HIPCHK(hipMemcpyAsync(slot, &st, sizeof st, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(descramble_apply_kernel, dim3(256), dim3(256), 0, s, dev ? src : (const uint8_t *)h->c.din.p, (const uint8_t *)h->T.prbs,
                     (const RxState *)slot, dev ? (uint8_t *)out : (uint8_t *)h->c.dout.p);
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, nbytes)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = to_consume;
  return (int)nbytes;
}
extern "C" int dvbt_energy_descramble_work(dvbt_energy_descramble *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return descramble_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_energy_descramble_work_device(dvbt_energy_descramble *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return descramble_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_energy_descramble_destroy(dvbt_energy_descramble *h) { delete h; }

// ============================================================================ next row 2: rational_resampler_ccc + multiply_const
struct dvbt_resampler { dvbt_resampler_params p; BlockCtx c; ResamplerDesign D; long long M = 0, Nc = 0; size_t hist = 0; };
extern "C" int dvbt_resampler_create(const dvbt_resampler_params *p, dvbt_resampler **out)
{
  BLK_CREATE_PROLOGUE(dvbt_resampler);
  h->p = *p;
  WCHK(h->D.build(p->interpolation, p->decimation));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_resampler_forecast(const dvbt_resampler *h, int n, int *req)
{ // rational_resampler_base::forecast: max(1, noutput * decimation / interpolation + history() - 1)
  if (!h) return DVBT_ERR_INVALID;
  long long r = (long long)n * h->D.rd / h->D.ri + h->D.nt - 1;
  if (req) *req = (int)(r < 1 ? 1 : r);
  return DVBT_OK;
}
extern "C" int dvbt_resampler_get_taps(const dvbt_resampler *h, float *taps, int cap, int *interpolation, int *decimation)
{
  if (!h) return DVBT_ERR_INVALID;
  if (interpolation) *interpolation = h->D.ri; if (decimation) *decimation = h->D.rd;
  if (taps) for (int i = 0; i < cap && i < (int)h->D.taps.size(); i++) taps[i] = h->D.taps[i];
  return (int)h->D.taps.size();
}
static int resampler_call(dvbt_resampler *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  if (nout <= 0 || nin <= 0) return 0;
  const int ri = h->D.ri, rd = h->D.rd, nt = h->D.nt;
  // general_work: outputs while (i < noutput && count < ninput); output M reads up to input floor(M rd / ri)
  const long long M_end = ((h->Nc + nin) * ri + rd - 1) / rd;      // first output whose newest input is not in this window
  long long cnt = M_end - h->M; if (cnt > nout) cnt = nout; if (cnt < 0) cnt = 0;
  long long consumed = ((h->M + cnt) * rd) / ri - h->Nc; if (consumed > nin) consumed = nin; if (consumed < 0) consumed = 0;
  const size_t tl = h->hist;                                      // samples of history at the front of din
  WCHK(h->c.din.reserve_keep((tl + (size_t)nin) * 8 + 64, tl * 8, s));
  if (dev) WCHK(h->c.put_dev(h->c.din, in, (size_t)nin * 8, tl * 8, s)); else HIPCHK(hipMemcpyAsync((char *)h->c.din.p + tl * 8, in, (size_t)nin * 8, hipMemcpyHostToDevice, s));
  if (cnt) {
    float2 *o = (float2 *)out;
    if (!dev) { WCHK(h->c.dout.reserve((size_t)cnt * 8)); o = (float2 *)h->c.dout.p; }
    hipLaunchKernelGGL(resample_scale_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (const float2 *)h->c.din.p, h->Nc - (long long)tl,
                       (long long)(tl + nin), h->M, cnt, ri, rd, nt, (const float *)h->D.br, h->p.scale == 0.f ? 1.0f : h->p.scale, o);
    if (!dev) WCHK(h->c.get(out, h->c.dout.p, (size_t)cnt * 8));
  }
  // history for the next call: the nt-1 samples before the new consumption point
  {
    const size_t total = tl + (size_t)consumed, keep = total < (size_t)(nt - 1) ? total : (size_t)(nt - 1);
    if (total > keep) {
      WCHK(h->c.aux.reserve((size_t)nt * 8));
      HIPCHK(hipMemcpyAsync(h->c.aux.p, (const char *)h->c.din.p + (total - keep) * 8, keep * 8, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(h->c.din.p, h->c.aux.p, keep * 8, hipMemcpyDeviceToDevice, s));
    }
    h->hist = keep;
  }
  if (!dev) WCHK(h->c.sync());
  h->M += cnt; h->Nc += consumed;
  if (sb) sb->n_consumed = (int)consumed;
  return (int)cnt;
}
extern "C" int dvbt_resampler_work(dvbt_resampler *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return resampler_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_resampler_work_device(dvbt_resampler *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return resampler_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_resampler_destroy(dvbt_resampler *h) { delete h; }

// ============================================================================ A3 demod_reference_signals
struct dvbt_demod_reference_signals {
  dvbt_demod_reference_signals_params p; BlockCtx c; Tables T; FrontParams fp;
  DevBuf eq, tpsval, info, maj, symidx, flags, syncf; DevMem<TpsState> ts; DevMem<float2> prev_tps; bool have_prev = false, locked = false;
  std::vector<int> h_flags, h_symidx; std::vector<unsigned char> h_sync;
};
extern "C" int dvbt_demod_reference_signals_create(const dvbt_demod_reference_signals_params *p, dvbt_demod_reference_signals **out)
{
  BLK_CREATE_PROLOGUE(dvbt_demod_reference_signals);
  h->p = *p;
  h->T.d = make_dims(p->constellation, p->hierarchy, p->code_rate_hp, p->guard_interval, p->transmission_mode);
  const Dims &d = h->T.d;
  if (!d.valid || p->itemsize != 8 || p->ninput != d.N || p->noutput != d.payload) return fail(DVBT_ERR_INVALID, "itemsize must be 8 (gr_complex), ninput the FFT length, noutput the payload length");
  WCHK(h->T.build_front());
  h->fp = make_front_params(d, 30.0f);
  if (h->ts.alloc(1) != hipSuccess || h->prev_tps.alloc(d.n_tps) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMalloc");
  if (hipMemset(h->ts, 0, sizeof(TpsState)) != hipSuccess || hipMemset(h->prev_tps, 0, sizeof(float2) * d.n_tps) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMemset");
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_demod_reference_signals_forecast(const dvbt_demod_reference_signals *, int n, int *req) { if (req) *req = n + 1; return DVBT_OK; }   // needs the next item too (:88-94)
static int demod_call(dvbt_demod_reference_signals *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const Dims &d = h->T.d;
  int n = nout < nin - 1 ? nout : nin - 1; if (n <= 0) return 0;
  const size_t N = d.N, P = d.payload;
  const float2 *din = (const float2 *)in;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)(n + 1) * N * 8)); din = (const float2 *)h->c.din.p; }
  WCHK(h->tpsval.reserve((size_t)(n + 1) * d.n_tps * 8)); WCHK(h->info.reserve((size_t)(n + 1) * sizeof(SymInfo)));
  WCHK(h->maj.reserve((size_t)(n + 1) * 4)); WCHK(h->symidx.reserve((size_t)(n + 1) * 4)); WCHK(h->flags.reserve((size_t)(n + 1) * 4));
  h->h_sync.assign(n + 1, 0);
  bool resync = false;
  if (sb && sb->in_tags) for (int i = 0; i < sb->n_in_tags; i++) if (sb->in_tags[i].key == DVBT_TAG_SYNC_START && sb->in_tags[i].rel_offset >= 0 && sb->in_tags[i].rel_offset < n) { h->h_sync[sb->in_tags[i].rel_offset] = 1; resync = true; }
  WCHK(h->syncf.reserve((size_t)n + 1));
  HIPCHK(hipMemcpyAsync(h->syncf.p, h->h_sync.data(), (size_t)n + 1, hipMemcpyHostToDevice, s));
  // device buffers in, superframe already found and no sync_start in this window: every item will be produced, so the equalised
  // carriers are written straight into the caller's output; otherwise into scratch, and the produced items are gathered afterwards
  const bool direct = dev && h->locked && !resync;
  float2 *eqbuf = (float2 *)out;
  if (!direct) { WCHK(h->eq.reserve((size_t)n * P * 8)); eqbuf = (float2 *)h->eq.p; }
  FrontParams fp = h->fp; fp.ncalls = n + 1;
  hipLaunchKernelGGL(demod_kernel, dim3(n), dim3(256), 0, s, din, fp, (const RxState *)nullptr, n + 1, h->T.demod_tables(), eqbuf, (float2 *)h->tpsval.p, (SymInfo *)h->info.p);
  hipLaunchKernelGGL(tps_vote_kernel, dim3((n + 63) / 64), dim3(256), 0, s, (const float2 *)h->tpsval.p, d.n_tps, (const RxState *)nullptr, n + 1,
                     (const float2 *)h->prev_tps, (int *)h->maj.p);
  hipLaunchKernelGGL(tps_fsm_kernel, dim3(1), dim3(256), 0, s, fp, (RxState *)nullptr, n + 1, (const SymInfo *)h->info.p, (const int *)h->maj.p, h->ts,
                     (int *)h->symidx.p, (int *)h->flags.p, (const unsigned char *)h->syncf.p, (const int *)nullptr);
  HIPCHK(hipMemcpyAsync(h->prev_tps, (const float2 *)h->tpsval.p + (size_t)(n - 1) * d.n_tps, sizeof(float2) * d.n_tps, hipMemcpyDeviceToDevice, s));
  h->h_flags.resize(n); h->h_symidx.resize(n);
  // which items were produced and their symbol indices become stream tags: two small read-backs and ONE synchronisation per call
  HIPCHK(hipMemcpyAsync(h->h_flags.data(), h->flags.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h->h_symidx.data(), h->symidx.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int produced = 0, run_i = -1, run_p = 0;                       // produced items leave in runs of consecutive ones (normally one run: the whole call)
  auto flush = [&](int end_i) -> int {
    if (run_i < 0 || direct) { run_i = -1; return DVBT_OK; }
    const size_t bytes = (size_t)(end_i - run_i) * P * 8;
    char *dst = (char *)out + (size_t)run_p * P * 8; const char *src = (const char *)h->eq.p + (size_t)run_i * P * 8;
    run_i = -1;
    if (dev) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); return DVBT_OK; }
    return h->c.get(dst, src, bytes);                            // through the handle's pinned staging, delivered by c.sync() below
  };
  for (int i = 0; i < n; i++) {
    if (!h->h_flags[i]) { WCHK(flush(i)); continue; }            // still hunting the superframe start: item dropped (:131-135)
    if (run_i < 0) { run_i = i; run_p = produced; }
    if (h->h_flags[i] == 2) add_tag(sb, produced, DVBT_TAG_SUPERFRAME_START, 0xaa);
    add_tag(sb, produced, DVBT_TAG_SYMBOL_INDEX, h->h_symidx[i]);
    produced++;
  }
  WCHK(flush(n));
  h->locked = n > 0 && h->h_flags[n - 1] != 0;
  if (!dev) WCHK(h->c.sync());
  if (sb) sb->n_consumed = n;
  return produced;
}
extern "C" int dvbt_demod_reference_signals_work(dvbt_demod_reference_signals *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return demod_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_demod_reference_signals_work_device(dvbt_demod_reference_signals *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return demod_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_demod_reference_signals_destroy(dvbt_demod_reference_signals *h) { delete h; }

// ============================================================================ A1 ofdm_sym_acquisition
struct dvbt_ofdm_sym_acquisition {
  dvbt_ofdm_sym_acquisition_params p; BlockCtx c; FrontParams fp; DevBuf g_init, l_init, g_trk, l_trk, meta, outb, centre, drift, drift_flags;
  DevMem<RxState> st; PinMem<RxState> st_host; DevMem<AcqState> as; PinMem<AcqState> as_host; bool acquired = false;
};
extern "C" int dvbt_ofdm_sym_acquisition_create(const dvbt_ofdm_sym_acquisition_params *p, dvbt_ofdm_sym_acquisition **out)
{
  BLK_CREATE_PROLOGUE(dvbt_ofdm_sym_acquisition);
  h->p = *p;
  int N = p->fft_length, cp = p->cp_length;
  if (p->blocks != 1 || N < 64 || N > 8192 || (N & (N - 1)) || cp <= 0 || cp > N) return fail(DVBT_ERR_INVALID, "blocks must be 1, fft_length a power of two <= 8192");
  Dims d; d.N = N; d.cp = cp;
  h->fp = make_front_params(d, p->snr);
  h->fp.N = N; h->fp.cp = cp;
  if (h->st.alloc(1) != hipSuccess || h->as.alloc(1) != hipSuccess || h->st_host.alloc(1) != hipSuccess || h->as_host.alloc(1) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMalloc");
  if (hipMemset(h->st, 0, sizeof(RxState)) != hipSuccess || hipMemset(h->as, 0, sizeof(AcqState)) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMemset");
  WCHK(set_lds((const void *)derot_fft_kernel, fft_lds_bytes(N)));
  *out = hold.release(); return DVBT_OK;
}
// the tracking window may look 8 (+margin) samples past 2N+cp: ask for 16 more than the reference (:474-481)
extern "C" int dvbt_ofdm_sym_acquisition_forecast(const dvbt_ofdm_sym_acquisition *h, int n, int *req)
{ if (!h || !req) return DVBT_ERR_INVALID; *req = (n - 1) * (h->fp.N + h->fp.cp) + 2 * h->fp.N + h->fp.cp + 16; return DVBT_OK; }
static int acq_call(dvbt_ofdm_sym_acquisition *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int N = h->fp.N, cp = h->fp.cp;
  if (nin < 2 * N + cp + 16 || nout <= 0) return 0;
  int C = (nin - (2 * N + cp + 16)) / (N + cp) + 1; if (C > nout) C = nout;
  FrontParams fp = h->fp; fp.ncalls = C; fp.avail = nin;          // (a tracking window that creeps beyond what the call was given reads zeros)
  const float2 *iq = (const float2 *)in;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)nin * 8)); iq = (const float2 *)h->c.din.p; }
  WCHK(h->g_init.reserve(sizeof(float2) * ACQ_INIT_TRIES * N)); WCHK(h->l_init.reserve(sizeof(float) * ACQ_INIT_TRIES * N));
  WCHK(h->g_trk.reserve(sizeof(float2) * (size_t)C * 2 * ACQ_R)); WCHK(h->l_trk.reserve(sizeof(float) * (size_t)C * 2 * ACQ_R));
  WCHK(h->meta.reserve(sizeof(SymMeta) * (size_t)C));
  float2 *items = (float2 *)out;                                 // device buffers: the derotated, CP-stripped items go straight to the caller's output
  if (!dev) { WCHK(h->outb.reserve((size_t)C * N * 8)); items = (float2 *)h->outb.p; }
  const bool was_acquired = h->acquired;                         // host copy of the lock state after the previous call
  int tries = C < ACQ_INIT_TRIES ? C : ACQ_INIT_TRIES;
  if (!was_acquired)
    hipLaunchKernelGGL(acq_metric_kernel, dim3((N + 255) / 256, tries), dim3(256), 0, s, iq, fp, (const RxState *)h->st, 0, (float2 *)h->g_init.p, (float *)h->l_init.p, 0);
  hipLaunchKernelGGL(acq_init_fsm_kernel, dim3(1), dim3(256), (size_t)N * 5, s, fp, h->st, (const float2 *)h->g_init.p, (const float *)h->l_init.p, (const AcqState *)h->as, 0, ACQ_INIT_TRIES);
  // one work() call's window is short: every call's lags are centred on the carried CP position; a call that needs others computes them itself
  WCHK(h->centre.reserve(sizeof(int) * ((size_t)C + 4)));
  hipLaunchKernelGGL(acq_centre_kernel, dim3(1), dim3(1024), 0, s, fp, (const RxState *)h->st, (const int *)h->centre.p + C + 1, 0, (int *)h->centre.p);
  hipLaunchKernelGGL(acq_track_metric_kernel, dim3((C + ACQ_TM_CALLS - 1) / ACQ_TM_CALLS), dim3(256), 0, s, iq, fp, (const RxState *)h->st, (const int *)h->centre.p, (float2 *)h->g_trk.p, (float *)h->l_trk.p);
  hipLaunchKernelGGL(acq_track_kernel, dim3(1), dim3(64), 0, s, fp, h->st, (const float2 *)h->g_trk.p, (const float *)h->l_trk.p, (SymMeta *)h->meta.p, (const int *)nullptr, h->as,
                     (const int *)h->centre.p, iq);
  // the wander of the reference's float phase accumulator inside every item (k_drift.hpp): the tracker above carries the accumulator's own value from call to call
  WCHK(h->drift.reserve(sizeof(float) * (size_t)C * (N / 32))); WCHK(h->drift_flags.reserve(16));
  hipLaunchKernelGGL(drift_table_entry_kernel, dim3(C), dim3(N / 32 < 256 ? N / 32 : 256), 0, s, fp, (const RxState *)h->st, (const SymMeta *)h->meta.p, (float *)h->drift.p, (int *)h->drift_flags.p);
  hipLaunchKernelGGL(derot_fft_kernel, dim3(C), dim3(FFT_THREADS), fft_lds_bytes(N), s, iq, fp, (const RxState *)h->st, (const SymMeta *)h->meta.p,
                     (const float2 *)nullptr, items, (float2 *)nullptr, (const float *)h->drift.p, (const int *)h->drift_flags.p);
  // how many items came out and how much was consumed depends on the data: one small read-back and ONE synchronisation per call
  HIPCHK(hipMemcpyAsync(h->st_host, h->st, sizeof(RxState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h->as_host, h->as, sizeof(AcqState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const RxState &st = *h->st_host;
  int produced = st.n_symbols;
  // (every host call ends in c.sync(), also one that produced nothing: it is what returns the pinned staging of the input -- a block that is fed dead air
  // call after call staged every call's samples behind the previous ones and doubled the pinned buffer without bound: ADVICE r04)
  if (!dev) { if (produced > 0) WCHK(h->c.get(out, h->outb.p, (size_t)produced * N * 8)); WCHK(h->c.sync()); }
  // consumption (:564-567): N+cp per call; calls spent on failed initial searches consume too;
  // the call that loses lock consumes (N+cp)/2 (:548-558)
  long long consumed;
  if (st.status & 1) consumed = (long long)tries * (N + cp);
  else {
    consumed = (long long)(st.call0 + produced) * (N + cp);
    if (h->as_host->lost) consumed += (N + cp) / 2;
  }
  h->acquired = h->as_host->acquired != 0;
  if (!was_acquired) add_tag(sb, 0, DVBT_TAG_SYNC_START, 1);                                // :507
  if (sb) sb->n_consumed = (int)consumed;
  return produced;
}
extern "C" int dvbt_ofdm_sym_acquisition_work(dvbt_ofdm_sym_acquisition *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return acq_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_ofdm_sym_acquisition_work_device(dvbt_ofdm_sym_acquisition *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return acq_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_ofdm_sym_acquisition_destroy(dvbt_ofdm_sym_acquisition *h) { delete h; }
