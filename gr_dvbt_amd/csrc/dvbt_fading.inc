// dvbt_fading.inc -- dvbt_fading_*: time-varying multipath with a Doppler spectrum between a modulator and a receiver, as one streaming handle
// (DESIGN.md 4i) over k_fading.hpp.  Included from dvbt_hip.hip.
//
// What a handle keeps from call to call, as dvbt_channel does: the number of samples it has seen (the gains are functions of first_sample + pos) and -- on
// the device -- the last CH_MAX_DELAY input samples in two buffers written alternately.  The sinusoid table is computed on the host in double, by operations
// whose bits do not depend on the machine (tests/fadingref.py::table is the same arithmetic), and written to the device once at create.

struct dvbt_fading {
  dvbt_fading_params p;
  int M = 0;
  DevMem<float2> hist[2]; int cur = 0;
  long long pos = 0;                  // samples since first_sample
  DevMem<FadePath> paths; DevMem<FadeSin> tab;
  DevBuf din, dout;                   // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

namespace {

constexpr uint32_t FADING_TAG = 0x46414445u;      // "FADE": counter word 3 of the table's Philox blocks; the noise generator's is 0

// cos(2 pi alpha) for alpha in [0, 1] from IEEE double + - * / alone, in the order of tests/fadingref.py::cos_turns line by line (the file is built with
// -ffp-contract=off): the nearest quarter turn comes off, the rest (|x| <= pi / 4) goes through the Taylor series of cos and sin, 12 terms behind the first
inline double fading_cos_turns(double alpha)
{
  const int q = (int)floor(alpha * 4.0 + 0.5);
  const double x = (alpha - (double)q * 0.25) * 6.283185307179586;
  const double z = x * x;
  double c = 1.0, s = x, ct = 1.0, st = x;
  for (int k = 1; k < 13; k++) {
    ct = -ct * z / (double)((2 * k - 1) * (2 * k));
    c = c + ct;
    st = -st * z / (double)((2 * k) * (2 * k + 1));
    s = s + st;
  }
  switch (q & 3) { case 0: return c; case 1: return -s; case 2: return -c; default: return s; }
}

inline int fading_sinusoids(const dvbt_fading_params *p) { return p->n_sinusoids ? p->n_sinusoids : 16; }

inline int fading_check_params(const dvbt_fading_params *p)
{
  if (p->n_paths < 1 || p->n_paths > DVBT_FADING_MAX_PATHS) return fail(DVBT_ERR_INVALID, "n_paths must be in [1, DVBT_FADING_MAX_PATHS]");
  for (int i = 0; i < p->n_paths; i++) {
    if (p->delay[i] < 0 || p->delay[i] > DVBT_FADING_MAX_DELAY) return fail(DVBT_ERR_INVALID, "a path's delay must be in [0, DVBT_FADING_MAX_DELAY]");
    if (!std::isfinite(p->los_re[i]) || !std::isfinite(p->los_im[i])) return fail(DVBT_ERR_INVALID, "a path's fixed part must be finite");
    if (!(p->sigma[i] >= 0.f) || !std::isfinite(p->sigma[i])) return fail(DVBT_ERR_INVALID, "a path's sigma must be a finite number >= 0");
  }
  if (!(p->doppler >= 0.0) || !(p->doppler <= 0.000244140625)) return fail(DVBT_ERR_INVALID, "doppler must be in [0, 2^-12] cycles per sample");
  if (p->n_sinusoids < 0 || p->n_sinusoids > DVBT_FADING_MAX_SINUSOIDS) return fail(DVBT_ERR_INVALID, "n_sinusoids must be 0 or in [1, DVBT_FADING_MAX_SINUSOIDS]");
  if (p->first_sample < 0) return fail(DVBT_ERR_INVALID, "first_sample must be >= 0");
  return DVBT_OK;
}

// the table of a checked struct: n_paths x M words each
inline void fading_fill_table(const dvbt_fading_params *p, uint64_t *inc, uint64_t *phase)
{
  const int M = fading_sinusoids(p);
  for (int i = 0; i < p->n_paths; i++)
    for (int m = 0; m < M; m++) {
      uint32_t w[4];
      philox4x32_10((uint32_t)m, (uint32_t)i, 0u, FADING_TAG, (uint32_t)p->seed, (uint32_t)(p->seed >> 32), w);
      const double u = ((double)w[0] + 0.5) * 2.3283064365386963e-10;               // 2^-32
      const double alpha = ((double)m + u) / (double)M;
      const double f = p->doppler * fading_cos_turns(alpha);
      const double r = nearbyint(ldexp(f, 64));                                      // |f 2^64| <= 2^52: exact scaling, ties to even
      inc[i * M + m] = r < 0 ? (uint64_t)0 - (uint64_t)(-r) : (uint64_t)r;
      phase[i * M + m] = ((uint64_t)w[1] << 32) | w[2];
    }
}

// back to first_sample: zero history in the buffer the next call reads
inline int fading_rewind(dvbt_fading *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->hist[h->cur], 0, sizeof(float2) * CH_MAX_DELAY, h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  return DVBT_OK;
}

// the call's launch on stream st; the caller has checked the buffers.  0 < n <= 2^31.
inline int fading_enqueue(dvbt_fading *h, const float2 *in, long long n, float2 *out, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const int nxt = h->cur ^ 1;
  const long long n0 = (long long)h->p.first_sample + h->pos;
  const long long tile0 = n0 & ~(long long)(FD_TILE - 1);
  const unsigned cblocks = (unsigned)((n0 + n - tile0 + FD_TILE - 1) / FD_TILE);       // <= 2^21 + 1: one launch
  hipLaunchKernelGGL(fading_kernel, dim3(cblocks + FD_HIST_BLOCKS), dim3(FD_THREADS), 0, st, in, out, (const float2 *)h->hist[h->cur], h->hist[nxt].get(), n0, n,
                     tile0, cblocks, (const FadePath *)h->paths, (const FadeSin *)h->tab, h->p.n_paths, h->M);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->cur = nxt; h->pos += n;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_fading_table(const dvbt_fading_params *p, uint64_t *inc, uint64_t *phase)
{
  if (!p || !inc || !phase) return fail(DVBT_ERR_INVALID, "null argument");
  int r = fading_check_params(p); if (r) return r;
  fading_fill_table(p, inc, phase);
  return DVBT_OK;
}

extern "C" int dvbt_fading_create(const dvbt_fading_params *p, dvbt_fading **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = fading_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_fading> hold(new dvbt_fading()); dvbt_fading *const h = hold.get();   // released on every early return below
  h->p = *p; h->M = fading_sinusoids(p);
  const int M = h->M, np = p->n_paths;
  std::vector<uint64_t> inc((size_t)np * M), ph((size_t)np * M);
  fading_fill_table(p, inc.data(), ph.data());
  std::vector<FadeSin> tab((size_t)np * M);
  for (size_t k = 0; k < tab.size(); k++) { tab[k].inc = inc[k]; tab[k].ph = ph[k]; }
  std::vector<FadePath> paths(np);
  for (int i = 0; i < np; i++) paths[i] = FadePath{p->los_re[i], p->los_im[i], (float)((double)p->sigma[i] / sqrt((double)M)), p->delay[i]};
  HIPCHK(h->ord.create());
  for (int i = 0; i < 2; i++) { HIPCHK(h->hist[i].alloc(CH_MAX_DELAY)); HIPCHK(hipMemsetAsync(h->hist[i], 0, sizeof(float2) * CH_MAX_DELAY, h->ord.s)); }
  HIPCHK(h->paths.alloc(paths.size())); HIPCHK(h->tab.alloc(tab.size()));
  HIPCHK(hipMemcpyAsync(h->paths, paths.data(), sizeof(FadePath) * paths.size(), hipMemcpyHostToDevice, h->ord.s));
  HIPCHK(hipMemcpyAsync(h->tab, tab.data(), sizeof(FadeSin) * tab.size(), hipMemcpyHostToDevice, h->ord.s));
  if ((r = fading_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));              // the vectors above are read until here
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_fading_run_device(dvbt_fading *h, const void *iq_device, size_t n, void *out_device, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = check_samples(iq_device, n, out_device); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return fading_enqueue(h, (const float2 *)iq_device, (long long)n, (float2 *)out_device, (hipStream_t)stream);
}

extern "C" int dvbt_fading_run(dvbt_fading *h, const void *iq_host, size_t n, void *out_host)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = check_samples(iq_host, n, out_host); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->dout, iq_host, n * sizeof(float2), out_host, n * sizeof(float2), [&](const void *in, void *out) {
    return fading_enqueue(h, (const float2 *)in, (long long)n, (float2 *)out, h->ord.s); });
}

extern "C" int dvbt_fading_reset(dvbt_fading *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return fading_rewind(h);
}

extern "C" void dvbt_fading_destroy(dvbt_fading *h) { delete h; }
