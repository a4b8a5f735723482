// dvbt_channel.inc -- dvbt_channel_*: static echoes, a carrier offset and seeded AWGN between a modulator and a receiver, as one streaming handle
// (DESIGN.md 4i) over k_channel.hpp.  Included from dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of samples it has seen (the absolute index of the next one = first_sample + pos: the noise and the phase
// are functions of it) and -- on the device -- the last CH_MAX_DELAY input samples, in two buffers written alternately (a call reads one and writes the other).

struct dvbt_channel {
  dvbt_channel_params p;
  ChannelArgs a;
  DevMem<float2> hist[2]; int cur = 0;
  long long pos = 0;                  // samples since first_sample
  DevMem<double> partial, result;     // dvbt_channel_power
  DevBuf din, dout;                   // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

namespace {

// inc = round(cfo / fft_length 2^64) mod 2^64: the quotient is one double division, the scaling is exact, the rounding is to nearest even
inline uint64_t channel_phase_inc(double cfo, int fft_length)
{
  if (cfo == 0.0) return 0;
  const double two64 = 18446744073709551616.0;
  const double m = fmod(nearbyint(ldexp(cfo / (double)fft_length, 64)), two64);      // exact, |m| < 2^64
  return m < 0 ? (uint64_t)0 - (uint64_t)(-m) : (uint64_t)m;
}

inline int channel_check_params(const dvbt_channel_params *p)
{
  if (p->n_paths < 0 || p->n_paths > DVBT_CHANNEL_MAX_PATHS) return fail(DVBT_ERR_INVALID, "n_paths must be in [0, DVBT_CHANNEL_MAX_PATHS]");
  for (int i = 0; i < p->n_paths; i++) {
    if (p->delay[i] < 1 || p->delay[i] > DVBT_CHANNEL_MAX_DELAY) return fail(DVBT_ERR_INVALID, "a path's delay must be in [1, DVBT_CHANNEL_MAX_DELAY]");
    if (!std::isfinite(p->amp_re[i]) || !std::isfinite(p->amp_im[i])) return fail(DVBT_ERR_INVALID, "a path's amplitude must be finite");
  }
  if (!std::isfinite(p->cfo)) return fail(DVBT_ERR_INVALID, "cfo must be finite");
  if (p->cfo != 0.0 && p->fft_length <= 0) return fail(DVBT_ERR_INVALID, "fft_length must be > 0 where cfo != 0");
  if (!(p->noise_sigma >= 0.f) || !std::isfinite(p->noise_sigma)) return fail(DVBT_ERR_INVALID, "noise_sigma must be a finite number >= 0");
  if (p->first_sample < 0) return fail(DVBT_ERR_INVALID, "first_sample must be >= 0");
  return DVBT_OK;
}

// back to first_sample: zero history in the buffer the next call reads
inline int channel_rewind(dvbt_channel *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->hist[h->cur], 0, sizeof(float2) * CH_MAX_DELAY, h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  return DVBT_OK;
}

// the call's launch on stream st; the caller has checked the buffers.  0 < n <= 2^31.
inline int channel_enqueue(dvbt_channel *h, const float2 *in, long long n, float2 *out, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const int nxt = h->cur ^ 1;
  const long long n0 = (long long)h->p.first_sample + h->pos;
  const long long p_first = n0 >> 1, npairs = ((n0 + n - 1) >> 1) + 1 - p_first;     // <= 2^30 + 1: one launch
  const unsigned cblocks = (unsigned)((npairs + CH_THREADS - 1) / CH_THREADS);
  hipLaunchKernelGGL(channel_kernel, dim3(cblocks + CH_HIST_BLOCKS), dim3(CH_THREADS), 0, st, in, out, (const float2 *)h->hist[h->cur], h->hist[nxt].get(), n0, n,
                     p_first, npairs, cblocks, h->a);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->cur = nxt; h->pos += n;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_channel_create(const dvbt_channel_params *p, dvbt_channel **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = channel_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_channel> hold(new dvbt_channel()); dvbt_channel *const h = hold.get();   // released on every early return below
  h->p = *p;
  ChannelArgs &a = h->a;
  memset(&a, 0, sizeof a);
  a.n_paths = p->n_paths;
  for (int i = 0; i < p->n_paths; i++) { a.delay[i] = p->delay[i]; a.are[i] = p->amp_re[i]; a.aim[i] = p->amp_im[i]; }
  a.inc = channel_phase_inc(p->cfo, p->fft_length); a.has_cfo = p->cfo != 0.0;
  a.sigma = p->noise_sigma; a.key0 = (uint32_t)p->seed; a.key1 = (uint32_t)(p->seed >> 32);
  HIPCHK(h->ord.create());
  for (int i = 0; i < 2; i++) { HIPCHK(h->hist[i].alloc(CH_MAX_DELAY)); HIPCHK(hipMemsetAsync(h->hist[i], 0, sizeof(float2) * CH_MAX_DELAY, h->ord.s)); }
  HIPCHK(h->partial.alloc(CH_POW_BLOCKS)); HIPCHK(h->result.alloc(1));
  if ((r = channel_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_channel_run_device(dvbt_channel *h, const void *iq_device, size_t n, void *out_device, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = check_samples(iq_device, n, out_device); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return channel_enqueue(h, (const float2 *)iq_device, (long long)n, (float2 *)out_device, (hipStream_t)stream);
}

extern "C" int dvbt_channel_run(dvbt_channel *h, const void *iq_host, size_t n, void *out_host)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = check_samples(iq_host, n, out_host); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->dout, iq_host, n * sizeof(float2), out_host, n * sizeof(float2), [&](const void *in, void *out) {
    return channel_enqueue(h, (const float2 *)in, (long long)n, (float2 *)out, h->ord.s); });
}

extern "C" int dvbt_channel_power(dvbt_channel *h, const void *iq_device, size_t n, void *stream, double *mean_power)
{
  if (!h || !mean_power) return fail(DVBT_ERR_INVALID, "null argument");
  if (!iq_device || n == 0) return fail(DVBT_ERR_INVALID, "the mean power needs at least one sample");
  if (n > (size_t)1 << 40) return fail(DVBT_ERR_INVALID, "n must be <= 2^40");
  if ((uintptr_t)iq_device & 7) return fail(DVBT_ERR_INVALID, "the sample buffer must be 8-byte aligned");
  HIPCHK(hipSetDevice(h->p.device));
  const hipStream_t st = (hipStream_t)stream;
  HIPCHK(h->ord.join(st));                        // the partial sums are the handle's: behind its last call
  hipLaunchKernelGGL(channel_power_kernel, dim3(CH_POW_BLOCKS), dim3(CH_THREADS), 0, st, (const float2 *)iq_device, (long long)n, h->partial.get());
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(channel_power_final_kernel, dim3(1), dim3(CH_THREADS), 0, st, (const double *)h->partial, (long long)n, h->result.get());
  HIPCHK(hipGetLastError());
  double v = 0.0;
  HIPCHK(hipMemcpyAsync(&v, h->result, sizeof v, hipMemcpyDeviceToHost, st));
  HIPCHK(h->ord.mark(st));
  HIPCHK(hipStreamSynchronize(st));
  *mean_power = v;
  return DVBT_OK;
}

extern "C" int dvbt_channel_reset(dvbt_channel *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return channel_rewind(h);
}

extern "C" void dvbt_channel_destroy(dvbt_channel *h) { delete h; }
