// dvbt_cfr.inc -- dvbt_cfr_*: crest-factor reduction of a DVB-T baseband stream by iterative clipping and filtering, symbol by symbol, as one streaming
// handle (DESIGN.md 4i) over k_cfr.hpp.  Included from dvbt_hip.hip.
//
// A symbol's output depends on (the struct, its index in the stream, its samples) alone, so all a handle carries from call to call on the host is the number
// of symbols it has seen; the five accumulators live on the device and only dvbt_cfr_read and dvbt_cfr_reset touch them from the host.

struct dvbt_cfr {
  dvbt_cfr_params p;
  Dims d;
  FftPlan fft;
  DevMem<unsigned char> free_bins;    // [4][N]: CfrArgs::free_bins
  DevMem<unsigned long long> acc;     // [CFR_ACC_WORDS]
  long long pos = 0;                  // symbols since first_symbol
  DevBuf dio;                         // staging of the host entry: the kernel runs in place on it
  CallOrder ord;                      // last: see CallOrder
};

namespace {

constexpr int CFR_MAX_ITERATIONS = 8;

inline int cfr_check_params(const dvbt_cfr_params *p)
{
  if (p->transmission_mode < 0 || p->transmission_mode > 1) return fail(DVBT_ERR_INVALID, "transmission_mode must be DVBT_T2k or DVBT_T8k");
  if (p->guard_interval < 0 || p->guard_interval > 3) return fail(DVBT_ERR_INVALID, "guard_interval must be DVBT_G1_32 .. DVBT_G1_4");
  if (!(p->threshold > 0.f) || !std::isfinite(p->threshold)) return fail(DVBT_ERR_INVALID, "threshold must be a finite number > 0");
  if (p->iterations < 0 || p->iterations > CFR_MAX_ITERATIONS) return fail(DVBT_ERR_INVALID, "iterations must be in [0, 8]");
  if (p->oversampling != 1 && p->oversampling != 2 && p->oversampling != 4) return fail(DVBT_ERR_INVALID, "oversampling must be 1, 2 or 4");
  if (p->keep & ~(DVBT_CFR_KEEP_PILOTS | DVBT_CFR_KEEP_TPS)) return fail(DVBT_ERR_INVALID, "keep has bits that mean nothing");
  if (p->first_symbol < 0) return fail(DVBT_ERR_INVALID, "first_symbol must be >= 0");
  if (p->device < 0) return fail(DVBT_ERR_INVALID, "no such device");
  return DVBT_OK;
}

// where the filter lets the clipping error through: [phase][bin]
inline std::vector<unsigned char> cfr_free_bins(const Dims &d, int keep)
{
  const int N = d.N, half = d.Kmax / 2;
  std::vector<unsigned char> carrier(d.K, 1), v((size_t)4 * N, 0);
  if (keep & DVBT_CFR_KEEP_PILOTS) for (int c : cpilot_table(d)) carrier[c] = 0;
  if (keep & DVBT_CFR_KEEP_TPS) for (int c : tps_table(d)) carrier[c] = 0;
  for (int ph = 0; ph < 4; ph++)
    for (int k = 0; k < N; k++) {
      const int kap = k < N / 2 ? k : k - N;
      if (kap < -half || kap > half) continue;
      const int c = kap + half;
      const bool scattered = (keep & DVBT_CFR_KEEP_PILOTS) && c % 12 == 3 * ph;
      v[(size_t)ph * N + k] = carrier[c] && !scattered;
    }
  return v;
}

inline int cfr_check_call(const dvbt_cfr *h, const void *in, size_t n, const void *out)
{
  int r = check_samples(in, n, out, true); if (r) return r;   // in place is fine: a symbol's output is written after its input is read
  if (n % (size_t)(h->d.cp + h->d.N)) return fail(DVBT_ERR_INVALID, "nsamples must be a whole number of symbols (guard + useful part)");
  return DVBT_OK;
}

// the call's launch on stream st; the caller has checked the buffers.  n > 0, a multiple of the symbol length.
inline int cfr_enqueue(dvbt_cfr *h, const float2 *in, size_t n, float2 *out, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const int nsym = (int)(n / (size_t)(h->d.cp + h->d.N));
  CfrArgs a;
  a.G = h->d.cp; a.iterations = h->p.iterations; a.os = h->p.oversampling; a.phase0 = (int)(((long long)h->p.first_symbol + h->pos) & 3);
  a.A = h->p.threshold; a.A2 = h->p.threshold * h->p.threshold;
  a.free_bins = h->free_bins; a.acc = h->acc;
  const size_t lds = h->fft.lds() + CFR_LDS_EXTRA;
  if (h->d.N == 8192) hipLaunchKernelGGL(cfr_kernel<8192>, dim3((unsigned)nsym), dim3(FFT_THREADS), lds, st, in, out, nsym, (const float2 *)h->fft.tw, a);
  else hipLaunchKernelGGL(cfr_kernel<2048>, dim3((unsigned)nsym), dim3(FFT_THREADS), lds, st, in, out, nsym, (const float2 *)h->fft.tw, a);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->pos += nsym;
  return DVBT_OK;
}

// the accumulators and the symbol counter back to the state after create
inline int cfr_rewind(dvbt_cfr *h)
{
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemsetAsync(h->acc, 0, CFR_ACC_WORDS * sizeof(unsigned long long), h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_cfr_create(const dvbt_cfr_params *p, dvbt_cfr **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = cfr_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_cfr> hold(new dvbt_cfr()); dvbt_cfr *const h = hold.get();   // released on every early return below
  h->p = *p;
  h->d = make_dims(DVBT_QAM64, DVBT_NH, DVBT_C1_2, p->guard_interval, p->transmission_mode);   // (N, the guard and the carrier tables: the same for every constellation and rate)
  HIPCHK(h->ord.create());
  if ((r = h->fft.build(h->d.N)) || (r = upload(cfr_free_bins(h->d, p->keep), h->free_bins))) return r;
  if ((r = h->d.N == 8192 ? set_lds((const void *)cfr_kernel<8192>, h->fft.lds() + CFR_LDS_EXTRA) : set_lds((const void *)cfr_kernel<2048>, h->fft.lds() + CFR_LDS_EXTRA))) return r;
  HIPCHK(h->acc.alloc(CFR_ACC_WORDS));
  if ((r = cfr_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_cfr_run_device(dvbt_cfr *h, const void *iq_device, size_t n, void *out_device, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = cfr_check_call(h, iq_device, n, out_device); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return cfr_enqueue(h, (const float2 *)iq_device, n, (float2 *)out_device, (hipStream_t)stream);
}

extern "C" int dvbt_cfr_run(dvbt_cfr *h, const void *iq_host, size_t n, void *out_host)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = cfr_check_call(h, iq_host, n, out_host); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->dio, h->dio, iq_host, n * sizeof(float2), out_host, n * sizeof(float2), [&](const void *in, void *out) {
    return cfr_enqueue(h, (const float2 *)in, n, (float2 *)out, h->ord.s); });
}

extern "C" int dvbt_cfr_read(dvbt_cfr *h, dvbt_cfr_result *res)
{
  if (!h || !res) return fail(DVBT_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->p.device));
  unsigned long long acc[CFR_ACC_WORDS];
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemcpyAsync(acc, h->acc, sizeof acc, hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipStreamSynchronize(h->ord.s));
  memset(res, 0, sizeof *res);
  res->symbols = (long long)acc[CFR_ACC_SYMBOLS]; res->symbols_clipped = (long long)acc[CFR_ACC_CLIPPED];
  res->symbols_nonfinite = (long long)acc[CFR_ACC_NONFINITE]; res->samples_over = (long long)acc[CFR_ACC_OVER];
  const uint32_t bits = (uint32_t)acc[CFR_ACC_PEAK];
  memcpy(&res->peak_power_in, &bits, sizeof bits);
  return DVBT_OK;
}

extern "C" int dvbt_cfr_reset(dvbt_cfr *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return cfr_rewind(h);
}

extern "C" void dvbt_cfr_destroy(dvbt_cfr *h) { delete h; }
