// dvbt_tuner.inc -- dvbt_tuner_*: a recording from an SDR (complex64, int16, int8 or uint8 I/Q at the capture's rate, the channel off-centre) to complex64
// baseband at the OFDM elementary rate: convert, mix, resample by L/M, as one streaming handle (DESIGN.md 4h4, 4i) over k_tuner.hpp.  Included from
// dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of input samples it has seen (the count a call emits is host arithmetic on it, tuner_total, so nothing
// waits for the device) and -- on the device -- the last TUN_HIST converted and mixed samples, in two buffers written alternately (a call reads one and
// writes the other).  A value of z is a function of the raw sample and its absolute index alone, so keeping z instead of the raw bytes changes no bit.

struct dvbt_tuner {
  dvbt_tuner_params p;
  TunerArgs a;
  std::vector<float> taps;            // the prototype in use (the caller's, or the designed one)
  DevMem<float> br;                   // its branches as [k][b]
  DevMem<float2> hist[2]; int cur = 0;
  long long pos = 0;                  // input samples since first_in
  size_t lds = 0; int ncu = 256;
  DevBuf din, dout;                   // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

namespace {

// the reduced ratio of a struct whose ratio is in range
inline int tuner_ratio(const dvbt_tuner_params *p, int *L, int *M)
{
  if (p->interpolation < 1 || p->decimation < 1) return fail(DVBT_ERR_INVALID, "interpolation and decimation must be >= 1");
  int a = p->interpolation, b = p->decimation;
  while (b) { const int t = a % b; a = b; b = t; }
  *L = p->interpolation / a; *M = p->decimation / a;
  if (*L > TUN_MAX_L || *M > TUN_MAX_M) return fail(DVBT_ERR_INVALID, "the reduced ratio must have interpolation <= 128 and decimation <= 1024");
  if (*M > TUN_MAX_RATIO * *L) return fail(DVBT_ERR_INVALID, "decimation / interpolation must be <= 8");
  return DVBT_OK;
}

inline int tuner_check_params(const dvbt_tuner_params *p, int *L, int *M)
{
  if (p->format < DVBT_IQ_CF32 || p->format > DVBT_IQ_CU8) return fail(DVBT_ERR_INVALID, "format must be DVBT_IQ_CF32, _CS16, _CS8 or _CU8");
  int r = tuner_ratio(p, L, M); if (r) return r;
  if (p->swap_iq != 0 && p->swap_iq != 1) return fail(DVBT_ERR_INVALID, "swap_iq must be 0 or 1");
  if (!std::isfinite(p->shift) || fabs(p->shift) > 0.5) return fail(DVBT_ERR_INVALID, "shift must be finite and within +-0.5 cycles per input sample");
  if (!std::isfinite(p->scale) || p->scale == 0.0f) return fail(DVBT_ERR_INVALID, "scale must be finite and not 0");
  if (!(p->atten_db >= 40.0) || !(p->atten_db <= 90.0)) return fail(DVBT_ERR_INVALID, "atten_db must lie in [40, 90]");
  if (!(p->pass_edge > 0.0) || !(p->pass_edge < p->stop_edge) || !(p->stop_edge <= 1.0)) return fail(DVBT_ERR_INVALID, "0 < pass_edge < stop_edge <= 1 is required");
  if (p->first_in < 0 || p->first_in > TUN_MAX_INDEX) return fail(DVBT_ERR_INVALID, "first_in must be in [0, 2^48]");
  return DVBT_OK;
}

inline int tuner_check_ntaps(int L, int ntaps)
{
  if (ntaps < 1) return fail(DVBT_ERR_INVALID, "ntaps must be >= 1");
  const long long nt = ((long long)ntaps + L - 1) / L;
  if (nt > TUN_MAX_NT || (long long)L * nt > TUN_MAX_BRANCH_FLOATS) return fail(DVBT_ERR_INVALID, "the prototype is too long: taps per branch <= 320 and interpolation * taps per branch <= 8192");
  return DVBT_OK;
}

// Io by its power series (the series of resampler_taps)
inline double tuner_izero(double x)
{
  double sum = 1, u = 1; const double halfx = x / 2.0; int n = 1;
  do { double t = halfx / (double)n; n += 1; t *= t; u *= t; sum += u; } while (u >= 1e-21 * sum);
  return sum;
}

// the design rule of the header, in double; the struct has passed tuner_check_params
inline int tuner_design(const dvbt_tuner_params *p, int L, int M, std::vector<float> &taps)
{
  const double A = p->atten_db, pass = p->pass_edge;
  double stop = p->stop_edge;
  if (L > M) stop = std::min(stop, (double)M / (double)L - pass);                  // the images of the capture
  if (!(stop > pass)) return fail(DVBT_ERR_INVALID, "no room between the pass band and the capture's first image: lower pass_edge");
  const double fp = pass / M, fs = stop / M, fc = (fp + fs) / 2.0;
  const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0);
  const double want = ceil((A - 7.95) / (2.285 * 2.0 * M_PI * (fs - fp))) + 1.0;
  if (!(want < 1e6)) return fail(DVBT_ERR_INVALID, "the prototype is too long: widen the transition band");
  int ntaps = (int)want;
  if ((ntaps & 1) == 0) ntaps++;
  int r = tuner_check_ntaps(L, ntaps); if (r) return r;
  std::vector<double> h(ntaps);
  const double c = (ntaps - 1) / 2.0, ib = 1.0 / tuner_izero(beta);
  double sum = 0;
  for (int i = 0; i < ntaps; i++) {
    const double d = (double)i - c, t = d / c, x = 2.0 * fc * d;
    const double sinc = d == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
    h[i] = 2.0 * fc * sinc * tuner_izero(beta * sqrt(std::max(0.0, 1.0 - t * t))) * ib;
    sum += h[i];
  }
  taps.resize(ntaps);
  for (int i = 0; i < ntaps; i++) taps[i] = (float)(h[i] * ((double)L / sum));
  return DVBT_OK;
}

// outputs in front of input N of the stream (absolute): ceil(N L / M).  N <= 2^49, L <= 128.
inline unsigned long long tuner_total(int L, int M, long long N) { return ((unsigned long long)N * (unsigned)L + (unsigned)M - 1) / (unsigned)M; }

// back to first_in: zero history in the buffer the next call reads
inline int tuner_rewind(dvbt_tuner *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->hist[h->cur], 0, sizeof(float2) * TUN_HIST, h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  return DVBT_OK;
}

// what a call of n_in samples emits (count) and every check of its arguments; out_cap is compared last
inline int tuner_check_call(const dvbt_tuner *h, const void *in, size_t n_in, const void *out, size_t out_cap, size_t *count)
{
  if (n_in > (size_t)1 << 31) return fail(DVBT_ERR_INVALID, "n_in must be <= 2^31 per call (a longer stream continues over calls)");
  if ((long long)n_in > TUN_MAX_INDEX - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^48 input samples");
  const long long n0 = (long long)h->p.first_in + h->pos;
  *count = (size_t)(tuner_total(h->a.L, h->a.M, n0 + (long long)n_in) - tuner_total(h->a.L, h->a.M, n0));
  if (n_in == 0) return DVBT_OK;
  if (!in || (*count && !out)) return fail(DVBT_ERR_INVALID, "null buffer");
  const size_t bps = (size_t)tun_bytes(h->p.format);
  if (((uintptr_t)in & (bps - 1)) != 0) return fail(DVBT_ERR_INVALID, "the input must be aligned to one raw sample");
  if (misaligned8(out)) return fail(DVBT_ERR_INVALID, "the output must be 8-byte aligned");
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
  if (*count && a < b + *count * sizeof(float2) && b < a + n_in * bps) return fail(DVBT_ERR_INVALID, "the input and output ranges overlap");
  if (out_cap < *count) return fail(DVBT_ERR_CAPACITY, "out_cap is below what the call emits (dvbt_tuner_outputs_for)");
  return DVBT_OK;
}

template <int FMT>
inline void tuner_launch(const dvbt_tuner *h, dim3 grid, hipStream_t st, const void *in, float2 *out, const float2 *hist, float2 *hist_next, long long n0,
                         long long n_in, unsigned long long m0, long long nout, unsigned cblocks, int tpw)
{
  if (h->a.inc) hipLaunchKernelGGL((tuner_kernel<FMT, true>), grid, dim3(TUN_THREADS), h->lds, st, in, out, hist, hist_next, (const float *)h->br, n0, n_in, m0, nout, cblocks, tpw, h->a);
  else hipLaunchKernelGGL((tuner_kernel<FMT, false>), grid, dim3(TUN_THREADS), h->lds, st, in, out, hist, hist_next, (const float *)h->br, n0, n_in, m0, nout, cblocks, tpw, h->a);
}

template <int FMT> inline int tuner_set_lds(const dvbt_tuner *h)
{
  int r = h->a.inc ? set_lds((const void *)tuner_kernel<FMT, true>, h->lds) : set_lds((const void *)tuner_kernel<FMT, false>, h->lds);
  return r;
}

// the call's launch on stream st; the caller has checked the buffers.  0 < n_in <= 2^31, count outputs.
inline int tuner_enqueue(dvbt_tuner *h, const void *in, long long n_in, float2 *out, long long nout, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const int nxt = h->cur ^ 1;
  const long long n0 = (long long)h->p.first_in + h->pos;
  const unsigned long long m0 = tuner_total(h->a.L, h->a.M, n0);
  const long long ntiles = (nout + TUN_THREADS - 1) / TUN_THREADS;
  // tiles per workgroup: the table is loaded once per workgroup, so a long call gives each a run of tiles, but never fewer than ~16 workgroups per CU
  int tpw = (int)std::min<long long>(8, std::max<long long>(1, ntiles / (16ll * h->ncu)));
  while ((ntiles + tpw - 1) / tpw > 0x7ffffff0ll) tpw *= 2;                                            // (nout up to 2^38: the grid stays below 2^31)
  const unsigned cblocks = (unsigned)((ntiles + tpw - 1) / tpw);
  const dim3 grid(cblocks + 1);
  const float2 *const hist = h->hist[h->cur]; float2 *const hist_next = h->hist[nxt];
  switch (h->p.format) {
    case DVBT_IQ_CF32: tuner_launch<TUN_CF32>(h, grid, st, in, out, hist, hist_next, n0, n_in, m0, nout, cblocks, tpw); break;
    case DVBT_IQ_CS16: tuner_launch<TUN_CS16>(h, grid, st, in, out, hist, hist_next, n0, n_in, m0, nout, cblocks, tpw); break;
    case DVBT_IQ_CS8:  tuner_launch<TUN_CS8>(h, grid, st, in, out, hist, hist_next, n0, n_in, m0, nout, cblocks, tpw); break;
    default:           tuner_launch<TUN_CU8>(h, grid, st, in, out, hist, hist_next, n0, n_in, m0, nout, cblocks, tpw); break;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->cur = nxt; h->pos += n_in;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_tuner_design(const dvbt_tuner_params *p, float *taps, int cap, int *ntaps)
{
  if (!p || !ntaps) return fail(DVBT_ERR_INVALID, "null argument");
  int L, M;
  int r = tuner_check_params(p, &L, &M); if (r) return r;
  std::vector<float> t;
  if ((r = tuner_design(p, L, M, t))) return r;
  if (taps && cap < (int)t.size()) return fail(DVBT_ERR_CAPACITY, "cap is below the tap count");
  *ntaps = (int)t.size();
  if (taps) memcpy(taps, t.data(), t.size() * sizeof(float));
  return DVBT_OK;
}

extern "C" int dvbt_tuner_outputs(const dvbt_tuner_params *p, int ntaps, int64_t n_in_total, int64_t *n_out_total)
{
  if (!p || !n_out_total) return fail(DVBT_ERR_INVALID, "null argument");
  int L, M;
  int r = tuner_check_params(p, &L, &M); if (r) return r;
  if (ntaps == 0) { std::vector<float> t; if ((r = tuner_design(p, L, M, t))) return r; }
  else if ((r = tuner_check_ntaps(L, ntaps))) return r;
  if (n_in_total < 0 || n_in_total > TUN_MAX_INDEX) return fail(DVBT_ERR_INVALID, "n_in_total must be in [0, 2^48]");
  *n_out_total = (int64_t)(tuner_total(L, M, p->first_in + n_in_total) - tuner_total(L, M, p->first_in));
  return DVBT_OK;
}

extern "C" int dvbt_tuner_create(const dvbt_tuner_params *p, const float *taps, int ntaps, dvbt_tuner **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int L, M;
  int r = tuner_check_params(p, &L, &M); if (r) return r;
  std::vector<float> t;
  if (taps) {
    if ((r = tuner_check_ntaps(L, ntaps))) return r;
    for (int i = 0; i < ntaps; i++) if (!std::isfinite(taps[i])) return fail(DVBT_ERR_INVALID, "the taps must be finite");
    t.assign(taps, taps + ntaps);
  } else if ((r = tuner_design(p, L, M, t))) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_tuner> hold(new dvbt_tuner()); dvbt_tuner *const h = hold.get();   // released on every early return below
  h->p = *p; h->taps = t;
  TunerArgs &a = h->a;
  memset(&a, 0, sizeof a);
  a.L = L; a.M = M; a.swap = p->swap_iq; a.scale = p->scale;
  const double inc = nearbyint(ldexp(p->shift, 64));                                      // |shift| <= 0.5: at most 2^63 either way; ties to even
  a.inc = inc >= 0.0 ? (unsigned long long)inc : 0ull - (unsigned long long)-inc;
  std::vector<float> b = resampler_branches(t, L, a.nt), bt(b.size());
  for (int i = 0; i < L; i++) for (int k = 0; k < a.nt; k++) bt[(size_t)k * L + i] = b[(size_t)i * a.nt + k];
  h->lds = tun_lds_bytes(L, M, a.nt);
  (void)hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, p->device);
  switch (p->format) {
    case DVBT_IQ_CF32: r = tuner_set_lds<TUN_CF32>(h); break;
    case DVBT_IQ_CS16: r = tuner_set_lds<TUN_CS16>(h); break;
    case DVBT_IQ_CS8:  r = tuner_set_lds<TUN_CS8>(h); break;
    default:           r = tuner_set_lds<TUN_CU8>(h); break;
  }
  if (r) return r;
  HIPCHK(h->br.alloc(bt.size()));
  HIPCHK(hipMemcpy(h->br, bt.data(), bt.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(h->ord.create());
  for (int i = 0; i < 2; i++) { HIPCHK(h->hist[i].alloc(TUN_HIST)); HIPCHK(hipMemsetAsync(h->hist[i], 0, sizeof(float2) * TUN_HIST, h->ord.s)); }
  if ((r = tuner_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_tuner_get_taps(const dvbt_tuner *h, float *taps, int cap, int *ntaps)
{
  if (!h || !ntaps) return fail(DVBT_ERR_INVALID, "null argument");
  if (taps && cap < (int)h->taps.size()) return fail(DVBT_ERR_CAPACITY, "cap is below the tap count");
  *ntaps = (int)h->taps.size();
  if (taps) memcpy(taps, h->taps.data(), h->taps.size() * sizeof(float));
  return DVBT_OK;
}

extern "C" int dvbt_tuner_info(const dvbt_tuner *h, dvbt_tuner_desc *d)
{
  if (!h || !d) return fail(DVBT_ERR_INVALID, "null argument");
  d->interpolation = h->a.L; d->decimation = h->a.M; d->ntaps = (int)h->taps.size(); d->nt = h->a.nt;
  d->delay_num = (int64_t)h->taps.size() - 1; d->delay_den = 2 * (int64_t)h->a.M;
  d->phase_inc = h->a.inc;
  return DVBT_OK;
}

extern "C" int dvbt_tuner_outputs_for(const dvbt_tuner *h, size_t n_in, size_t *n_out)
{
  if (!h || !n_out) return fail(DVBT_ERR_INVALID, "null argument");
  if ((long long)n_in < 0 || (long long)n_in > TUN_MAX_INDEX - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^48 input samples");
  const long long n0 = (long long)h->p.first_in + h->pos;
  *n_out = (size_t)(tuner_total(h->a.L, h->a.M, n0 + (long long)n_in) - tuner_total(h->a.L, h->a.M, n0));
  return DVBT_OK;
}

extern "C" int dvbt_tuner_run_device(dvbt_tuner *h, const void *raw_device, size_t n_in, void *out_device, size_t out_cap, size_t *n_out, void *stream)
{
  if (!h || !n_out) return fail(DVBT_ERR_INVALID, "null argument");
  size_t count;
  int r = tuner_check_call(h, raw_device, n_in, out_device, out_cap, &count); if (r) return r;
  *n_out = count;
  if (n_in == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return tuner_enqueue(h, raw_device, (long long)n_in, (float2 *)out_device, (long long)count, (hipStream_t)stream);
}

extern "C" int dvbt_tuner_run(dvbt_tuner *h, const void *raw_host, size_t n_in, void *out_host, size_t out_cap, size_t *n_out)
{
  if (!h || !n_out) return fail(DVBT_ERR_INVALID, "null argument");
  size_t count;
  int r = tuner_check_call(h, raw_host, n_in, out_host, out_cap, &count); if (r) return r;
  *n_out = count;
  if (n_in == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->dout, raw_host, n_in * (size_t)tun_bytes(h->p.format), out_host, count * sizeof(float2), [&](const void *in, void *out) {
    return tuner_enqueue(h, in, (long long)n_in, (float2 *)out, (long long)count, h->ord.s); });
}

extern "C" int dvbt_tuner_reset(dvbt_tuner *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return tuner_rewind(h);
}

extern "C" void dvbt_tuner_destroy(dvbt_tuner *h) { delete h; }
