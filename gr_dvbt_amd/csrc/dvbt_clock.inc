// dvbt_clock.inc -- dvbt_clock_*: a sample-clock offset of some ppm between a modulator and a receiver (windowed-sinc resampling), as one streaming handle
// (DESIGN.md 4i) over k_clock.hpp.  Included from dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of input samples it has seen, the number of the next output (both exact integers: the count a call emits
// is host arithmetic on them, clock_E of k_clock_math.hpp, so nothing waits for the device) and -- on the device -- the last CLK_HIST input samples, in two
// buffers written alternately (a call reads one and writes the other).

struct dvbt_clock {
  dvbt_clock_params p;                // taps already resolved (0 -> 16)
  ClockArgs a;
  DevMem<float2> hist[2]; int cur = 0;
  long long pos = 0;                  // input samples since first_in
  unsigned long long m_next = 0;      // the next output: max(E(first_in + pos), first_out)
  DevBuf din, dout;                   // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

namespace {

inline int clock_check_params(const dvbt_clock_params *p)
{
  if (!std::isfinite(p->ppm) || fabs(p->ppm) > CLK_MAX_PPM) return fail(DVBT_ERR_INVALID, "ppm must be finite and within +-1000");
  if (!(p->start >= 0.0) || !(p->start < 2147483648.0)) return fail(DVBT_ERR_INVALID, "start must be in [0, 2^31)");
  if (p->taps != 0 && p->taps != 16 && p->taps != 32 && p->taps != 64) return fail(DVBT_ERR_INVALID, "taps must be 16, 32 or 64 (0: 16)");
  if (p->first_out < 0 || p->first_out > CLK_MAX_INDEX) return fail(DVBT_ERR_INVALID, "first_out must be in [0, 2^48]");
  if (p->first_in < 0 || p->first_in > CLK_MAX_INDEX) return fail(DVBT_ERR_INVALID, "first_in must be in [0, 2^48]");
  return DVBT_OK;
}

inline int clock_taps(const dvbt_clock_params *p) { return p->taps ? p->taps : 16; }

// the next output once n_in_total inputs have been pushed
inline unsigned long long clock_next(const ClockStep &c, int taps, long long first_out, long long first_in, long long n_in_total)
{
  return std::max(clock_E(c, taps / 2, (unsigned long long)(first_in + n_in_total)), (unsigned long long)first_out);
}

// back to first_in / first_out: zero history in the buffer the next call reads
inline int clock_rewind(dvbt_clock *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->hist[h->cur], 0, sizeof(float2) * CLK_HIST, h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  h->m_next = clock_next(h->a.c, h->p.taps, h->p.first_out, h->p.first_in, 0);
  return DVBT_OK;
}

// what a call of n_in samples emits (count) and every check of its arguments; out_cap is compared last
inline int clock_check_call(const dvbt_clock *h, const void *in, size_t n_in, const void *out, size_t out_cap, unsigned long long *m_after, size_t *count)
{
  if (n_in > (size_t)1 << 31) return fail(DVBT_ERR_INVALID, "n_in must be <= 2^31 per call (a longer stream continues over calls)");
  if ((long long)n_in > CLK_MAX_TOTAL - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^56 input samples");
  *m_after = clock_next(h->a.c, h->p.taps, h->p.first_out, h->p.first_in, h->pos + (long long)n_in);
  *count = (size_t)(*m_after - h->m_next);
  if (n_in == 0) return DVBT_OK;
  if (!in || (*count && !out)) return fail(DVBT_ERR_INVALID, "null buffer");
  if (misaligned8(in, out)) return fail(DVBT_ERR_INVALID, "the sample buffers must be 8-byte aligned");
  if (*count && samples_overlap(in, n_in, out, *count)) return fail(DVBT_ERR_INVALID, "the input and output ranges overlap");
  if (out_cap < *count) return fail(DVBT_ERR_CAPACITY, "out_cap is below what the call emits (dvbt_clock_outputs_for)");
  return DVBT_OK;
}

// the call's launch on stream st; the caller has checked the buffers.  0 < n_in <= 2^31, count = m_after - m_next outputs.
inline int clock_enqueue(dvbt_clock *h, const float2 *in, long long n_in, float2 *out, unsigned long long m_after, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const int nxt = h->cur ^ 1;
  const long long n0 = (long long)h->p.first_in + h->pos, nout = (long long)(m_after - h->m_next);    // nout < 2^31 (1 + 2e-3): one launch
  const unsigned cblocks = (unsigned)((nout + CLK_THREADS - 1) / CLK_THREADS);
  const dim3 grid(cblocks + 1), block(CLK_THREADS);
  const float2 *const hist = h->hist[h->cur]; float2 *const hist_next = h->hist[nxt];
  switch (h->p.taps) {
    case 16: hipLaunchKernelGGL(clock_kernel<16>, grid, block, 0, st, in, out, hist, hist_next, n0, n_in, h->m_next, nout, cblocks, h->a); break;
    case 32: hipLaunchKernelGGL(clock_kernel<32>, grid, block, 0, st, in, out, hist, hist_next, n0, n_in, h->m_next, nout, cblocks, h->a); break;
    default: hipLaunchKernelGGL(clock_kernel<64>, grid, block, 0, st, in, out, hist, hist_next, n0, n_in, h->m_next, nout, cblocks, h->a); break;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->cur = nxt; h->pos += n_in; h->m_next = m_after;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_clock_outputs(const dvbt_clock_params *p, int64_t n_in_total, int64_t *n_out_total)
{
  if (!p || !n_out_total) return fail(DVBT_ERR_INVALID, "null argument");
  int r = clock_check_params(p); if (r) return r;
  if (n_in_total < 0 || n_in_total > CLK_MAX_TOTAL) return fail(DVBT_ERR_INVALID, "n_in_total must be in [0, 2^56]");
  const ClockStep c = clock_step(p->ppm, p->start);
  const int taps = clock_taps(p);
  *n_out_total = (int64_t)(clock_next(c, taps, p->first_out, p->first_in, n_in_total) - clock_next(c, taps, p->first_out, p->first_in, 0));
  return DVBT_OK;
}

extern "C" int dvbt_clock_create(const dvbt_clock_params *p, dvbt_clock **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = clock_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_clock> hold(new dvbt_clock()); dvbt_clock *const h = hold.get();   // released on every early return below
  h->p = *p; h->p.taps = clock_taps(p);
  ClockArgs &a = h->a;
  memset(&a, 0, sizeof a);
  a.c = clock_step(p->ppm, p->start);
  const int H = h->p.taps / 2;
  for (int i = 0; i < h->p.taps; i++) {
    const int k = i - (H - 1);
    const double th = M_PI * (double)k / (double)(H + 1), sgn = (k & 1) ? 0.46 : -0.46;      // sin(pi (k - phi)) = -(-1)^k sin(pi phi)
    a.wc[i] = (float)(sgn * cos(th)); a.ws[i] = (float)(sgn * sin(th));
  }
  HIPCHK(h->ord.create());
  for (int i = 0; i < 2; i++) { HIPCHK(h->hist[i].alloc(CLK_HIST)); HIPCHK(hipMemsetAsync(h->hist[i], 0, sizeof(float2) * CLK_HIST, h->ord.s)); }
  if ((r = clock_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_clock_outputs_for(const dvbt_clock *h, size_t n_in, size_t *n_out)
{
  if (!h || !n_out) return fail(DVBT_ERR_INVALID, "null argument");
  if ((long long)n_in < 0 || (long long)n_in > CLK_MAX_TOTAL - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^56 input samples");
  *n_out = (size_t)(clock_next(h->a.c, h->p.taps, h->p.first_out, h->p.first_in, h->pos + (long long)n_in) - h->m_next);
  return DVBT_OK;
}

extern "C" int dvbt_clock_run_device(dvbt_clock *h, const void *iq_device, size_t n_in, void *out_device, size_t out_cap, size_t *n_out, void *stream)
{
  if (!h || !n_out) return fail(DVBT_ERR_INVALID, "null argument");
  unsigned long long m_after; size_t count;
  int r = clock_check_call(h, iq_device, n_in, out_device, out_cap, &m_after, &count); if (r) return r;
  *n_out = count;
  if (n_in == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return clock_enqueue(h, (const float2 *)iq_device, (long long)n_in, (float2 *)out_device, m_after, (hipStream_t)stream);
}

extern "C" int dvbt_clock_run(dvbt_clock *h, const void *iq_host, size_t n_in, void *out_host, size_t out_cap, size_t *n_out)
{
  if (!h || !n_out) return fail(DVBT_ERR_INVALID, "null argument");
  unsigned long long m_after; size_t count;
  int r = clock_check_call(h, iq_host, n_in, out_host, out_cap, &m_after, &count); if (r) return r;
  *n_out = count;
  if (n_in == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->dout, iq_host, n_in * sizeof(float2), out_host, count * sizeof(float2), [&](const void *in, void *out) {
    return clock_enqueue(h, (const float2 *)in, (long long)n_in, (float2 *)out, m_after, h->ord.s); });
}

extern "C" int dvbt_clock_reset(dvbt_clock *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return clock_rewind(h);
}

extern "C" void dvbt_clock_destroy(dvbt_clock *h) { delete h; }
