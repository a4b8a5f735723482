// dvbt_spectrum.inc -- dvbt_spectrum_*: a spectrum analyser for complex64 baseband -- Welch's averaged periodogram, the power sum, the peak and a histogram
// of |x|^2 -- as one streaming handle (DESIGN.md 4i) over k_spectrum.hpp.  It consumes a stream and changes nothing.  Included from dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of samples it has seen (the number of complete segments is host arithmetic on it, so nothing waits for
// the device) and, on the device, the up to N - 1 samples behind the last complete segment's start, in two buffers written alternately (as dvbt_clock), the
// open group's state, likewise in two buffers, and the accumulators.  dvbt_spectrum_read synchronises and copies on the handle's own stream, and changes nothing.

struct dvbt_spectrum {
  dvbt_spectrum_params p;             // hop already resolved (0 -> N/2)
  DevMem<float> win; FftPlan fft;
  DevMem<float2> hist[2]; int cur = 0;
  DevMem<double> open[2]; int ocur = 0;            // the open group: its power sum, then N floats (the open slab)
  DevMem<double> res;                              // N doubles (PSD sums), 1 (power sum), SPEC_HIST_BINS uint64, 1 word (the peak's bits)
  long long pos = 0;                  // samples since create / reset
  double sum_w2 = 0.0;
  DevBuf slabs;                       // the closed groups of one launch: floats [groups][N], then a double per group
  DevBuf din;                         // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

namespace {

constexpr long long SPEC_MAX_TOTAL = 1ll << 56;
constexpr int SPEC_MAX_GROUPS = 2048;              // groups per launch: bounds the slab buffer (64 MB at N = 8192)

inline size_t spec_res_doubles(int N) { return (size_t)N + 1 + SPEC_HIST_BINS + 1; }
inline size_t spec_open_doubles(int N) { return 1 + (size_t)(N + 1) / 2; }

inline int spectrum_hop(const dvbt_spectrum_params *p) { return p->hop ? p->hop : p->fft_size / 2; }

inline int spectrum_check_params(const dvbt_spectrum_params *p)
{
  const int N = p->fft_size;
  if (N < 64 || N > 8192 || (N & (N - 1))) return fail(DVBT_ERR_INVALID, "fft_size must be a power of two in 64..8192");
  if (p->hop != 0 && (p->hop < N / 8 || p->hop > N)) return fail(DVBT_ERR_INVALID, "hop must be in [fft_size / 8, fft_size] (0: fft_size / 2)");
  if (p->window < 0 || p->window > 2) return fail(DVBT_ERR_INVALID, "window must be 0 (rectangular), 1 (Hann) or 2 (Blackman-Harris)");
  if (p->device < 0) return fail(DVBT_ERR_INVALID, "no such device");
  return DVBT_OK;
}

// the periodic window (argument n / N) in double, rounded to float
inline std::vector<float> spectrum_window(int N, int window)
{
  std::vector<float> w(N);
  for (int n = 0; n < N; n++) {
    const double t = 2.0 * M_PI * (double)n / (double)N;
    const double v = window == 0 ? 1.0 : window == 1 ? 0.5 - 0.5 * cos(t) : 0.35875 - 0.48829 * cos(t) + 0.14128 * cos(2.0 * t) - 0.01168 * cos(3.0 * t);
    w[n] = (float)v;
  }
  return w;
}

// complete segments once `pos` samples have been pushed
inline long long spectrum_segments(long long pos, int N, int hop) { return pos >= N ? (pos - N) / hop + 1 : 0; }

inline int spectrum_check_call(const dvbt_spectrum *h, const void *in, size_t n)
{
  if (n == 0) return DVBT_OK;
  if (!in) return fail(DVBT_ERR_INVALID, "null buffer");
  if (n > (size_t)1 << 31) return fail(DVBT_ERR_INVALID, "n must be <= 2^31 per call (a longer stream continues over calls)");
  if ((long long)n > SPEC_MAX_TOTAL - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^56 samples");
  if (misaligned8(in)) return fail(DVBT_ERR_INVALID, "the sample buffer must be 8-byte aligned");
  return DVBT_OK;
}

template <int NB>
inline void spectrum_launch(dvbt_spectrum *h, const float2 *in, const SpecArgs &a, long long g_first, int groups, const double *open_in, double *open_out,
                            hipStream_t st)
{
  const int N = a.N;
  float *const slabs = (float *)h->slabs.p;
  double *const psums = (double *)((char *)h->slabs.p + (size_t)SPEC_MAX_GROUPS * N * sizeof(float));
  double *const res = h->res;
  hipLaunchKernelGGL(spectrum_kernel<NB>, dim3((unsigned)groups), dim3(FFT_THREADS), spec_lds(N), st, in, (const float2 *)h->hist[h->cur],
                     (const float *)h->win, (const float2 *)h->fft.tw, a, g_first, open_in, open_out, slabs, psums,
                     (unsigned long long *)(res + N + 1), (unsigned *)(res + N + 1 + SPEC_HIST_BINS));
}

// the call's launches on stream st; the caller has checked the buffer.  0 < n <= 2^31.
inline int spectrum_enqueue(dvbt_spectrum *h, const float2 *in, long long n, hipStream_t st)
{
  const int N = h->p.fft_size, hop = h->p.hop;
  SpecArgs a;
  a.N = N; a.hop = hop; a.pos0 = h->pos;
  a.s0 = spectrum_segments(h->pos, N, hop); a.s1 = spectrum_segments(h->pos + n, N, hop);
  a.hbase = a.s0 * hop;
  const long long first = a.s1 * hop, cnt = h->pos + n - first;            // what the next call needs: 0 <= cnt < N
  if (a.s1 > a.s0) { int r = h->slabs.reserve((size_t)SPEC_MAX_GROUPS * (N * sizeof(float) + sizeof(double))); if (r) return r; }
  HIPCHK(h->ord.join(st));
  const int nxt = h->cur ^ 1, onxt = h->ocur ^ 1;
  const bool to_open = a.s1 > a.s0 && (a.s1 % SPEC_GROUP) != 0;
  if (a.s1 > a.s0) {
    const long long g0 = a.s0 / SPEC_GROUP, g1 = (a.s1 - 1) / SPEC_GROUP;  // the call's groups: g0 .. g1
    double *const res = h->res;
    for (long long g = g0; g <= g1; g += SPEC_MAX_GROUPS) {
      const int groups = (int)std::min<long long>(SPEC_MAX_GROUPS, g1 - g + 1);
      const double *const oin = h->open[h->ocur]; double *const oout = h->open[onxt];
      switch (N / FFT_THREADS) {
        case 0: case 1: spectrum_launch<1>(h, in, a, g, groups, oin, oout, st); break;
        case 2: spectrum_launch<2>(h, in, a, g, groups, oin, oout, st); break;
        case 4: spectrum_launch<4>(h, in, a, g, groups, oin, oout, st); break;
        case 8: spectrum_launch<8>(h, in, a, g, groups, oin, oout, st); break;
        default: spectrum_launch<16>(h, in, a, g, groups, oin, oout, st); break;
      }
      HIPCHK(hipGetLastError());
      const int closed = groups - ((g + groups - 1 == g1 && to_open) ? 1 : 0);
      if (closed > 0) {
        hipLaunchKernelGGL(spectrum_fold_kernel, dim3((unsigned)(N / 256 + 1)), dim3(256), 0, st, (const float *)h->slabs.p,
                           (const double *)((char *)h->slabs.p + (size_t)SPEC_MAX_GROUPS * N * sizeof(float)), N, closed, res, res + N);
        HIPCHK(hipGetLastError());
      }
    }
  }
  if (cnt > 0) {
    hipLaunchKernelGGL(spectrum_carry_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, in, (const float2 *)h->hist[h->cur], a.pos0, a.hbase,
                       first, (int)cnt, (float2 *)h->hist[nxt]);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(h->ord.mark(st));
  if (cnt > 0) h->cur = nxt;
  if (to_open) h->ocur = onxt;
  h->pos += n;
  return DVBT_OK;
}

// back to the state after create: the accumulators zeroed (the history and the open group are not read before they are written again)
inline int spectrum_rewind(dvbt_spectrum *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->res, 0, sizeof(double) * spec_res_doubles(h->p.fft_size), h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_spectrum_create(const dvbt_spectrum_params *p, dvbt_spectrum **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = spectrum_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_spectrum> hold(new dvbt_spectrum()); dvbt_spectrum *const h = hold.get();   // released on every early return below
  h->p = *p; h->p.hop = spectrum_hop(p);
  const int N = p->fft_size;
  const std::vector<float> w = spectrum_window(N, p->window);
  for (int n = 0; n < N; n++) h->sum_w2 += (double)w[n] * (double)w[n];
  if ((r = upload(w, h->win)) || (r = h->fft.build(N))) return r;
  const void *fn = N <= FFT_THREADS ? (const void *)spectrum_kernel<1> : N == 2 * FFT_THREADS ? (const void *)spectrum_kernel<2>
                 : N == 4 * FFT_THREADS ? (const void *)spectrum_kernel<4> : N == 8 * FFT_THREADS ? (const void *)spectrum_kernel<8>
                 : (const void *)spectrum_kernel<16>;
  if ((r = set_lds(fn, spec_lds(N)))) return r;
  HIPCHK(h->ord.create());
  for (int i = 0; i < 2; i++) {
    HIPCHK(h->hist[i].alloc(N)); HIPCHK(hipMemsetAsync(h->hist[i], 0, sizeof(float2) * N, h->ord.s));
    HIPCHK(h->open[i].alloc(spec_open_doubles(N))); HIPCHK(hipMemsetAsync(h->open[i], 0, sizeof(double) * spec_open_doubles(N), h->ord.s));
  }
  HIPCHK(h->res.alloc(spec_res_doubles(N)));
  if ((r = spectrum_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_spectrum_push_device(dvbt_spectrum *h, const void *iq_device, size_t n, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = spectrum_check_call(h, iq_device, n); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return spectrum_enqueue(h, (const float2 *)iq_device, (long long)n, (hipStream_t)stream);
}

extern "C" int dvbt_spectrum_push(dvbt_spectrum *h, const void *iq_host, size_t n)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = spectrum_check_call(h, iq_host, n); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->din, iq_host, n * sizeof(float2), nullptr, 0, [&](const void *in, void *) {
    return spectrum_enqueue(h, (const float2 *)in, (long long)n, h->ord.s); });
}

extern "C" int dvbt_spectrum_read(dvbt_spectrum *h, dvbt_spectrum_result *res, double *psd, unsigned long long *hist)
{
  if (!h || !res) return fail(DVBT_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->p.device));
  const int N = h->p.fft_size, hop = h->p.hop;
  const long long S = spectrum_segments(h->pos, N, hop);
  const bool open = (S % SPEC_GROUP) != 0;
  std::vector<double> r(spec_res_doubles(N)), o(spec_open_doubles(N));
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemcpyAsync(r.data(), h->res, sizeof(double) * r.size(), hipMemcpyDeviceToHost, h->ord.s));
  if (open) HIPCHK(hipMemcpyAsync(o.data(), h->open[h->ocur], sizeof(double) * o.size(), hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipStreamSynchronize(h->ord.s));
  const float *const oa = (const float *)(o.data() + 1);
  const unsigned long long *const h64 = (const unsigned long long *)(r.data() + N + 1);
  unsigned pk; memcpy(&pk, r.data() + N + 1 + SPEC_HIST_BINS, sizeof pk);
  memset(res, 0, sizeof *res);
  res->segments = S; res->samples_pushed = h->pos; res->samples_counted = S * hop;
  for (int b = SPEC_HIST_BINS - 8; b < SPEC_HIST_BINS; b++) res->nonfinite += (long long)h64[b];
  res->sum_power = open ? r[N] + o[0] : r[N];
  memcpy(&res->peak_power, &pk, sizeof pk);
  if (psd) {
    const double norm = (double)S * (double)N * h->sum_w2;
    for (int b = 0; b < N; b++) psd[b] = S ? (open ? r[b] + (double)oa[b] : r[b]) / norm : 0.0;
  }
  if (hist) memcpy(hist, h64, sizeof(unsigned long long) * SPEC_HIST_BINS);
  return DVBT_OK;
}

extern "C" int dvbt_spectrum_reset(dvbt_spectrum *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return spectrum_rewind(h);
}

extern "C" void dvbt_spectrum_destroy(dvbt_spectrum *h) { delete h; }
