// dvbt_txblocks.inc -- per-block C ABI entry points of the transmit chain (apps/dvbt_tx_demo*.grc, the per-block apps energy_dispersal.grc ..
// dvbt_tx.grc): energy_dispersal, reed_solomon_enc, convolutional_interleaver, inner_coder, bit_inner_interleaver, dvbt_map, reference_signals.
// The same pattern as dvbt_blocks.inc: one `run` routine per block enqueues its kernel (k_txblocks.hpp) on device buffers and a stream;
// dvbt_<blk>_work stages host buffers around it, dvbt_<blk>_work_device only enqueues.  Tables are the modulator's (dvbt_tx.inc helpers).
// State the reference keeps in members lives in the handle; what a kernel reads of it lives on the device, ping-pong, so that a refused
// call changes nothing and the device entries never wait.  Included from dvbt_hip.hip after dvbt_blocks.inc and dvbt_tx.inc.

namespace {
inline bool misaligned(const void *p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }
}

// ============================================================================ T1 energy_dispersal
struct dvbt_energy_dispersal { dvbt_energy_dispersal_params p; BlockCtx c; DevMem<uint8_t> prbs; PinBuf probe; };
extern "C" int dvbt_energy_dispersal_create(const dvbt_energy_dispersal_params *p, dvbt_energy_dispersal **out)
{
  BLK_CREATE_PROLOGUE(dvbt_energy_dispersal);
  h->p = *p;
  if (p->nblocks <= 0 || p->nblocks > 4096) return fail(DVBT_ERR_INVALID, "nblocks must be in [1, 4096]");
  WCHK(upload(energy_prbs(), h->prbs));
  WCHK(h->probe.reserve(188));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_energy_dispersal_forecast(const dvbt_energy_dispersal *h, int n, int *req)
{ if (!h || !req) return DVBT_ERR_INVALID; *req = 8 * 189 * h->p.nblocks * n; return DVBT_OK; }     // :86-91
static int dispersal_call(dvbt_energy_dispersal *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  if (nout <= 0 || nin <= 0) return 0;
  if (dev && misaligned(out, 16)) return fail(DVBT_ERR_INVALID, "energy_dispersal: the output must be 16-byte aligned");
  const int win = nin < 188 ? nin : 188;
  const uint8_t *w = (const uint8_t *)in;
  if (dev) {                                                      // the SYNC search decides what is consumed: read the window back (:117-121)
    HIPCHK(hipMemcpyAsync(h->probe.p, in, (size_t)win, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    w = (const uint8_t *)h->probe.p;
  }
  int index = 0;
  while (index < win && w[index] != 0x47) index++;
  if (index == 188) { if (sb) sb->n_consumed = 188; return 0; }  // :136-140
  if (index == win) return 0;                                     // fewer than 188 bytes visible and no sync among them: wait for more
  const long long item = 1504LL * h->p.nblocks;
  long long n = (nin - index) / item; if (n > nout) n = nout;
  if (n <= 0) { if (sb) sb->n_consumed = index; return 0; }      // the sync found, not one item behind it yet: the bytes in front of it go
  const size_t nbytes = (size_t)(n * item);
  const uint8_t *src = (const uint8_t *)in + index;
  uint8_t *o = (uint8_t *)out;
  if (!dev) { WCHK(h->c.put(h->c.din, src, nbytes)); WCHK(h->c.dout.reserve(nbytes)); src = (const uint8_t *)h->c.din.p; o = (uint8_t *)h->c.dout.p; }
  const long long nvec = (long long)nbytes / 16;
  hipLaunchKernelGGL(txb_dispersal_kernel, dim3((unsigned)((nvec + TXB_THREADS - 1) / TXB_THREADS)), dim3(TXB_THREADS), 0, s, src, nvec,
                     (const uint8_t *)h->prbs, (uint4 *)o);
  HIPCHK(hipGetLastError());
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, nbytes)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = (int)(index + nbytes);
  return (int)n;
}
extern "C" int dvbt_energy_dispersal_work(dvbt_energy_dispersal *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return dispersal_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_energy_dispersal_work_device(dvbt_energy_dispersal *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return dispersal_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_energy_dispersal_destroy(dvbt_energy_dispersal *h) { delete h; }

// ============================================================================ T2 reed_solomon_enc
struct dvbt_reed_solomon_enc { dvbt_reed_solomon_enc_params p; BlockCtx c; DevMem<uint8_t> enc; };
extern "C" int dvbt_reed_solomon_enc_create(const dvbt_reed_solomon_enc_params *p, dvbt_reed_solomon_enc **out)
{
  BLK_CREATE_PROLOGUE(dvbt_reed_solomon_enc);
  h->p = *p;
  if (p->p != 2 || p->m != 8 || p->gfpoly != 0x11d || p->n != 255 || p->k != 239 || p->t != 8 || p->s != 51 || p->blocks <= 0 || p->blocks > 4096)
    return fail(DVBT_ERR_INVALID, "only RS(255,239,t=8) over GF(2^8)/0x11d shortened by 51 (the DVB-T outer code), blocks in [1, 4096]");
  WCHK(upload(rs_encoder_rows(), h->enc));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_reed_solomon_enc_forecast(const dvbt_reed_solomon_enc *, int n, int *req) { if (req) *req = n; return DVBT_OK; }   // :58-62
static int rs_enc_call(dvbt_reed_solomon_enc *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  if (dev && (misaligned(in, 4) || misaligned(out, 4))) return fail(DVBT_ERR_INVALID, "reed_solomon_enc: input and output must be 4-byte aligned");
  const long long npk = (long long)n * h->p.blocks;
  const void *src = in; void *o = out;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)npk * 188)); WCHK(h->c.dout.reserve((size_t)npk * 204)); src = h->c.din.p; o = h->c.dout.p; }
  hipLaunchKernelGGL(txb_rs_enc_kernel, dim3((unsigned)((npk + TX_OUTER_PK - 1) / TX_OUTER_PK)), dim3(TX_OUTER_PK), 0, s, (const uint8_t *)src, npk,
                     (const uint4 *)h->enc.get(), (uint8_t *)o);
  HIPCHK(hipGetLastError());
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, (size_t)npk * 204)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_reed_solomon_enc_work(dvbt_reed_solomon_enc *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return rs_enc_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_reed_solomon_enc_work_device(dvbt_reed_solomon_enc *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return rs_enc_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_reed_solomon_enc_destroy(dvbt_reed_solomon_enc *h) { delete h; }

// ============================================================================ T3 convolutional_interleaver
// hist[2]: the last (I-1) M I input bytes of the stream (ping-pong: the call reads hist[cur], its kernel writes hist[cur ^ 1])
struct dvbt_convolutional_interleaver { dvbt_convolutional_interleaver_params p; BlockCtx c; DevMem<uint8_t> hist[2]; int cur = 0, H = 0; };
extern "C" int dvbt_convolutional_interleaver_create(const dvbt_convolutional_interleaver_params *p, dvbt_convolutional_interleaver **out)
{
  BLK_CREATE_PROLOGUE(dvbt_convolutional_interleaver);
  h->p = *p;
  if (p->blocks <= 0 || p->I <= 0 || p->M < 0 || (long long)p->I * p->blocks > (1 << 20) || (long long)(p->I - 1) * p->M * p->I > (1 << 26) || (p->I * p->blocks) % 4)
    return fail(DVBT_ERR_INVALID, "convolutional_interleaver: blocks, I >= 1, M >= 0, I * blocks a multiple of 4 (at most 2^20), (I - 1) M I at most 2^26");
  h->H = (p->I - 1) * p->M * p->I;
  for (int i = 0; i < 2; i++) {
    if (h->hist[i].alloc((size_t)h->H + 64) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMalloc (convolutional_interleaver history)");
    if (hipMemset(h->hist[i], 0, (size_t)h->H + 64) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMemset (convolutional_interleaver history)");
  }
  *out = hold.release(); return DVBT_OK;
}
// sync_interpolator(I * blocks): noutput bytes need noutput / (I * blocks) items
extern "C" int dvbt_convolutional_interleaver_forecast(const dvbt_convolutional_interleaver *h, int n, int *req)
{ if (!h || !req) return DVBT_ERR_INVALID; *req = n / (h->p.I * h->p.blocks); return DVBT_OK; }
static int convint_call(dvbt_convolutional_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int item = h->p.I * h->p.blocks;
  if (nout % item) return fail(DVBT_ERR_INVALID, "convolutional_interleaver: noutput_items must be a multiple of I * blocks (a sync_interpolator)");
  int n = nout / item; if (n > nin) n = nin;
  if (n <= 0) return 0;
  if (dev && misaligned(out, 4)) return fail(DVBT_ERR_INVALID, "convolutional_interleaver: the output must be 4-byte aligned");
  const long long nbytes = (long long)n * item;
  const void *src = in; void *o = out;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)nbytes)); WCHK(h->c.dout.reserve((size_t)nbytes)); src = h->c.din.p; o = h->c.dout.p; }
  const long long lanes = nbytes / 4 + h->H;
  hipLaunchKernelGGL(txb_conv_int_kernel, dim3((unsigned)((lanes + TXB_THREADS - 1) / TXB_THREADS)), dim3(TXB_THREADS), 0, s, (const uint8_t *)src, nbytes,
                     h->p.I, h->p.I * h->p.M, (const uint8_t *)h->hist[h->cur], h->H, h->hist[h->cur ^ 1], (uint32_t *)o);
  HIPCHK(hipGetLastError());
  h->cur ^= 1;
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, (size_t)nbytes)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = n;
  return (int)nbytes;
}
extern "C" int dvbt_convolutional_interleaver_work(dvbt_convolutional_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return convint_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_convolutional_interleaver_work_device(dvbt_convolutional_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return convint_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_convolutional_interleaver_destroy(dvbt_convolutional_interleaver *h) { delete h; }

// ============================================================================ T4 inner_coder
// prev[2]: the last input byte of the stream, whose low 6 bits are the encoder's register (ping-pong, as hist above)
struct dvbt_inner_coder { dvbt_inner_coder_params p; BlockCtx c; Dims d; TxbCoderParams cp; DevMem<uint8_t> prev; int cur = 0; };
extern "C" int dvbt_inner_coder_create(const dvbt_inner_coder_params *p, dvbt_inner_coder **out)
{
  BLK_CREATE_PROLOGUE(dvbt_inner_coder);
  h->p = *p;
  h->d = make_dims(p->constellation, p->hierarchy, p->code_rate, 0, 0);
  if (!h->d.valid) return fail(DVBT_ERR_INVALID, "bad inner_coder parameters");
  if (p->noutput <= 0 || p->noutput % 1512 || p->noutput > (1 << 20)) return fail(DVBT_ERR_INVALID, "noutput must be a positive multiple of 1512 (reference assert, inner_coder_impl.cc:165)");
  if (p->ninput != 1) return fail(DVBT_ERR_INVALID, "ninput must be 1: the reference's input items are bytes whatever ninput says (inner_coder_impl.cc:138), its consume_each divides by ninput");
  const Dims &d = h->d;
  memset(&h->cp, 0, sizeof h->cp);
  h->cp.m = d.m; h->cp.k = d.k; h->cp.n = d.n;
  for (int j = 0, o = 0; j < d.k; j++) {                          // :56-121: x then y of every info bit, kept where the puncture vector says 1
    if (d.punct[2 * j]) h->cp.cmap[o++] = (uint8_t)(j << 1);
    if (d.punct[2 * j + 1]) h->cp.cmap[o++] = (uint8_t)((j << 1) | 1);
  }
  if (h->prev.alloc(64) != hipSuccess || hipMemset(h->prev, 0, 64) != hipSuccess) return fail(DVBT_ERR_HIP, "hipMalloc (inner_coder state)");
  *out = hold.release(); return DVBT_OK;
}
static long long coder_input(const dvbt_inner_coder *h, long long n)                    // :208-216, :262
{ return n * h->p.noutput * h->d.k * h->d.m / ((long long)h->p.ninput * 8 * h->d.n); }
extern "C" int dvbt_inner_coder_forecast(const dvbt_inner_coder *h, int n, int *req)
{ if (!h || !req) return DVBT_ERR_INVALID; *req = (int)coder_input(h, n); return DVBT_OK; }
static int coder_call(dvbt_inner_coder *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  if (nout % 4) return fail(DVBT_ERR_INVALID, "inner_coder: noutput_items must be a multiple of 4 (set_output_multiple(4), inner_coder_impl.cc:172)");
  int n = nout;
  while (n > 0 && coder_input(h, n) > nin) n -= 4;
  if (n <= 0) return 0;
  if (dev && misaligned(out, 4)) return fail(DVBT_ERR_INVALID, "inner_coder: the output must be 4-byte aligned");
  const long long nbytes = coder_input(h, n), nsym = (long long)n * h->p.noutput;
  const void *src = in; void *o = out;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)nbytes)); WCHK(h->c.dout.reserve((size_t)nsym)); src = h->c.din.p; o = h->c.dout.p; }
  const long long lanes = nsym / 4;
  hipLaunchKernelGGL(txb_inner_coder_kernel, dim3((unsigned)((lanes + TXB_THREADS - 1) / TXB_THREADS)), dim3(TXB_THREADS), 0, s, (const uint8_t *)src, nbytes,
                     nsym, h->cp, (const uint8_t *)(h->prev + 32 * h->cur), h->prev + 32 * (h->cur ^ 1), (uint32_t *)o);
  HIPCHK(hipGetLastError());
  h->cur ^= 1;
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, (size_t)nsym)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = (int)nbytes;
  return n;
}
extern "C" int dvbt_inner_coder_work(dvbt_inner_coder *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return coder_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_inner_coder_work_device(dvbt_inner_coder *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return coder_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_inner_coder_destroy(dvbt_inner_coder *h) { delete h; }

// ============================================================================ T5 bit_inner_interleaver
struct dvbt_bit_inner_interleaver { dvbt_bit_inner_interleaver_params p; BlockCtx c; TxbBitParams bp; };
extern "C" int dvbt_bit_inner_interleaver_create(const dvbt_bit_inner_interleaver_params *p, dvbt_bit_inner_interleaver **out)
{
  BLK_CREATE_PROLOGUE(dvbt_bit_inner_interleaver);
  h->p = *p;
  const Dims d = make_dims(p->constellation, p->hierarchy, 0, 0, p->transmission_mode);
  if (!d.valid || p->nsize <= 0 || p->nsize % 252 || p->nsize > 49392) return fail(DVBT_ERR_INVALID, "nsize must be a positive multiple of 252 (126-word blocks, 4-byte items)");
  if (p->hierarchy != DVBT_NH)
    return fail(DVBT_ERR_INVALID, "only hierarchy NH: the reference's hierarchical branch writes outside its bit matrix (bit_inner_interleaver_impl.cc:161-167)");
  memset(&h->bp, 0, sizeof h->bp);
  h->bp.m = d.m;
  for (int kk = 0; kk < d.m; kk++) h->bp.kinv[(kk / (d.m / 2)) + 2 * (kk % (d.m / 2))] = (uint8_t)kk;    // :97-98: bit kk goes to row perm(kk)
  static const uint8_t hoff[6] = {0, 63, 105, 42, 21, 84};                                              // :37-57 H(e, w)
  memcpy(h->bp.hoff, hoff, 6);
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_bit_inner_interleaver_forecast(const dvbt_bit_inner_interleaver *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
static int bitint_call(dvbt_bit_inner_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  if (dev && misaligned(out, 4)) return fail(DVBT_ERR_INVALID, "bit_inner_interleaver: the output must be 4-byte aligned");
  const long long nbytes = (long long)n * h->p.nsize;
  const void *src = in; void *o = out;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)nbytes)); WCHK(h->c.dout.reserve((size_t)nbytes)); src = h->c.din.p; o = h->c.dout.p; }
  const long long lanes = nbytes / 4;
  hipLaunchKernelGGL(txb_bit_int_kernel, dim3((unsigned)((lanes + TXB_THREADS - 1) / TXB_THREADS)), dim3(TXB_THREADS), 0, s, (const uint8_t *)src, nbytes, h->bp,
                     (uint32_t *)o);
  HIPCHK(hipGetLastError());
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, (size_t)nbytes)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_bit_inner_interleaver_work(dvbt_bit_inner_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return bitint_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_bit_inner_interleaver_work_device(dvbt_bit_inner_interleaver *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return bitint_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_bit_inner_interleaver_destroy(dvbt_bit_inner_interleaver *h) { delete h; }

// ============================================================================ T6 dvbt_map
struct dvbt_map { dvbt_map_params p; BlockCtx c; Tables T; };
extern "C" int dvbt_map_create(const dvbt_map_params *p, dvbt_map **out)
{
  BLK_CREATE_PROLOGUE(dvbt_map);
  h->p = *p;
  h->T.d = make_dims(p->constellation, p->hierarchy, 0, 0, p->transmission_mode);
  if (!h->T.d.valid || p->nsize <= 0 || p->nsize % 2 || p->nsize > (1 << 20) || !std::isfinite(p->gain))
    return fail(DVBT_ERR_INVALID, "bad dvbt_map parameters (nsize a positive even number, gain finite)");
  WCHK(h->T.build_inner(p->gain));                             // make_constellation_points with gain * norm and the hierarchy's alpha (:56-139)
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_map_forecast(const dvbt_map *, int n, int *req) { if (req) *req = n; return DVBT_OK; }
static int map_call(dvbt_map *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  if (dev && misaligned(out, 16)) return fail(DVBT_ERR_INVALID, "dvbt_map: the output must be 16-byte aligned");
  const long long nl = (long long)n * h->p.nsize;
  const void *src = in; void *o = out;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)nl)); WCHK(h->c.dout.reserve((size_t)nl * 8)); src = h->c.din.p; o = h->c.dout.p; }
  const long long pairs = nl / 2;
  hipLaunchKernelGGL(txb_map_kernel, dim3((unsigned)((pairs + TXB_THREADS - 1) / TXB_THREADS)), dim3(TXB_THREADS), 0, s, (const uint8_t *)src, pairs,
                     (const float2 *)h->T.points, (float4 *)o);
  HIPCHK(hipGetLastError());
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, (size_t)nl * 8)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_map_work(dvbt_map *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return map_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_map_work_device(dvbt_map *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return map_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_map_destroy(dvbt_map *h) { delete h; }

// ============================================================================ T7 reference_signals
// symbols: the items emitted so far (symbol_index = symbols mod 68, frame_index = (symbols / 68) mod 4: update_output :1175-1183)
struct dvbt_reference_signals { dvbt_reference_signals_params p; BlockCtx c; Dims d; TxbRefParams rp; TxTables tt; long long symbols = 0;
                                DevMem<uint16_t> pay, pil, tps; DevMem<float> pref, tps_base, tps_sign; };
extern "C" int dvbt_reference_signals_create(const dvbt_reference_signals_params *p, dvbt_reference_signals **out)
{
  BLK_CREATE_PROLOGUE(dvbt_reference_signals);
  h->p = *p;
  h->d = make_dims(p->constellation, p->hierarchy, p->code_rate_hp, p->guard_interval, p->transmission_mode);
  const Dims &d = h->d;
  if (!d.valid || p->code_rate_lp < 0 || p->code_rate_lp > 4) return fail(DVBT_ERR_INVALID, "bad DVB-T parameters");
  if (p->itemsize != 8 || p->ninput != d.payload || p->noutput != d.N)
    return fail(DVBT_ERR_INVALID, "itemsize must be 8 (gr_complex), ninput the payload and noutput the FFT length of the transmission mode");
  if (p->include_cell_id < 0 || p->include_cell_id > 1 || p->cell_id < 0 || p->cell_id > 0xffff) return fail(DVBT_ERR_INVALID, "bad cell id parameters");
  TxClasses cl;
  WCHK(tx_carrier_classes(d, cl));
  const std::vector<float> pref = pilot_ref_table(d);
  TxTps tp;
  tx_tps_tables(d, p->code_rate_lp, p->include_cell_id, p->cell_id, pref, tp);
  WCHK(upload(cl.pay, h->pay)); WCHK(upload(cl.pil, h->pil)); WCHK(upload(pref, h->pref));
  WCHK(upload(tp.car, h->tps)); WCHK(upload(tp.base, h->tps_base)); WCHK(upload(tp.sign, h->tps_sign));
  memset(&h->rp, 0, sizeof h->rp);
  h->rp.payload = d.payload; h->rp.zl = d.zl; h->rp.K = d.K; h->rp.n_tps = (int)tp.car.size();
  for (int c = 0; c < TX_NCLASS; c++) h->rp.npil[c] = cl.npil[c];
  memset(&h->tt, 0, sizeof h->tt);
  h->tt.pay = h->pay; h->tt.pil = h->pil; h->tt.pref = h->pref; h->tt.tps = h->tps; h->tt.tps_base = h->tps_base; h->tt.tps_sign = h->tps_sign;
  WCHK(set_lds(d.N == 8192 ? (const void *)txb_refsig_kernel<8192> : (const void *)txb_refsig_kernel<2048>, txb_refsig_lds_bytes(d.N)));
  *out = hold.release(); return DVBT_OK;
}
extern "C" int dvbt_reference_signals_forecast(const dvbt_reference_signals *, int n, int *req) { if (req) *req = n; return DVBT_OK; }   // :1280-1284
static int refsig_call(dvbt_reference_signals *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, bool dev, hipStream_t s)
{
  sb_begin(sb);
  const int n = nout < nin ? nout : nin; if (n <= 0) return 0;
  if (dev && (misaligned(in, 8) || misaligned(out, 16))) return fail(DVBT_ERR_INVALID, "reference_signals: input 8-byte and output 16-byte aligned");
  const size_t P = h->d.payload, N = h->d.N;
  const void *src = in; void *o = out;
  if (!dev) { WCHK(h->c.put(h->c.din, in, (size_t)n * P * 8)); WCHK(h->c.dout.reserve((size_t)n * N * 8)); src = h->c.din.p; o = h->c.dout.p; }
  TxbRefParams rp = h->rp;
  rp.S0 = h->symbols; rp.nsym = n;
  const size_t lds = txb_refsig_lds_bytes((int)N);
  if (N == 8192) hipLaunchKernelGGL(txb_refsig_kernel<8192>, dim3(n), dim3(FFT_THREADS), lds, s, (const float2 *)src, rp, h->tt, (float4 *)o);
  else hipLaunchKernelGGL(txb_refsig_kernel<2048>, dim3(n), dim3(FFT_THREADS), lds, s, (const float2 *)src, rp, h->tt, (float4 *)o);
  HIPCHK(hipGetLastError());
  h->symbols += n;
  if (!dev) { WCHK(h->c.get(out, h->c.dout.p, (size_t)n * N * 8)); WCHK(h->c.sync()); }
  if (sb) sb->n_consumed = n;
  return n;
}
extern "C" int dvbt_reference_signals_work(dvbt_reference_signals *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return refsig_call(h, nout, nin, in, out, sb, false, h->c.s);
}
extern "C" int dvbt_reference_signals_work_device(dvbt_reference_signals *h, int nout, int nin, const void *in, void *out, dvbt_sideband *sb, void *stream)
{
  if (!h || !in || !out) return fail(DVBT_ERR_INVALID, "null argument");
  return refsig_call(h, nout, nin, in, out, sb, true, pick(stream, h->c));
}
extern "C" void dvbt_reference_signals_destroy(dvbt_reference_signals *h) { delete h; }
