// dvbt_rf.inc -- dvbt_rf_*: the radio hardware on either side of a channel -- the transmitter's amplifier, the oscillator's phase noise, the tuner's IQ
// imbalance and DC offset -- as one streaming handle (DESIGN.md 4i) over k_rf.hpp.  Included from dvbt_hip.hip.
//
// The block is memoryless, so all a handle carries from call to call is the number of samples it has seen (the phases are functions of first_sample + pos).
// dvbt_rf_phase_noise_tones is host arithmetic in double (tests/rfref.py::tones is the same formulas).

struct dvbt_rf {
  dvbt_rf_params p;
  RfArgs a;
  long long pos = 0;                  // samples since first_sample
  DevBuf dio;                         // staging of the host entry: the kernel runs in place on it
  CallOrder ord;                      // last: see CallOrder
};

namespace {

constexpr uint32_t RF_TAG = 0x5246504Eu;          // "RFPN": counter word 3 of the tone table's Philox blocks; the noise generator's is 0, the fading table's "FADE"

inline int rf_check_params(const dvbt_rf_params *p)
{
  if (!(p->sat_amplitude >= 0.f) || !std::isfinite(p->sat_amplitude)) return fail(DVBT_ERR_INVALID, "sat_amplitude must be a finite number >= 0");
  if (p->smoothness != 0.f && !(p->smoothness >= 0.5f && p->smoothness <= 16.f)) return fail(DVBT_ERR_INVALID, "smoothness must be 0 or in [0.5, 16]");
  if (p->n_tones < 0 || p->n_tones > DVBT_RF_MAX_TONES) return fail(DVBT_ERR_INVALID, "n_tones must be in [0, DVBT_RF_MAX_TONES]");
  double sum = 0.0;
  for (int m = 0; m < p->n_tones; m++) {
    if (!(p->tone_amp[m] >= 0.f) || !std::isfinite(p->tone_amp[m])) return fail(DVBT_ERR_INVALID, "a tone's amplitude must be a finite number >= 0");
    sum += (double)p->tone_amp[m];
  }
  if (sum > 3.141592653589793) return fail(DVBT_ERR_INVALID, "the tones' amplitudes must add up to at most pi");
  if (!std::isfinite(p->mu_re) || !std::isfinite(p->mu_im) || !std::isfinite(p->nu_re) || !std::isfinite(p->nu_im)) return fail(DVBT_ERR_INVALID, "mu and nu must be finite");
  if (!std::isfinite(p->dc_re) || !std::isfinite(p->dc_im)) return fail(DVBT_ERR_INVALID, "dc must be finite");
  if (p->first_sample < 0) return fail(DVBT_ERR_INVALID, "first_sample must be >= 0");
  return DVBT_OK;
}

// the kernel's arguments of a checked struct; a stage that the struct leaves off costs the kernel a branch
inline void rf_fill_args(const dvbt_rf_params *p, RfArgs &a)
{
  memset(&a, 0, sizeof a);
  a.has_pa = p->sat_amplitude != 0.f;
  if (a.has_pa) {
    const double sm = p->smoothness != 0.f ? (double)p->smoothness : 2.0;
    a.A = p->sat_amplitude; a.lg_a2 = (float)(2.0 * log2((double)p->sat_amplitude)); a.p = (float)sm; a.e = (float)(-1.0 / (2.0 * sm));
  }
  a.n_tones = p->n_tones;
  for (int m = 0; m < p->n_tones; m++) { a.inc[m] = p->tone_inc[m]; a.ph[m] = p->tone_phase[m]; a.amp[m] = p->tone_amp[m]; }
  const bool mu0 = p->mu_re == 0.f && p->mu_im == 0.f;             // a zeroed struct is the identity
  a.mu_re = mu0 ? 1.f : p->mu_re; a.mu_im = p->mu_im; a.nu_re = p->nu_re; a.nu_im = p->nu_im;
  a.has_iq = !(a.mu_re == 1.f && a.mu_im == 0.f && a.nu_re == 0.f && a.nu_im == 0.f);
  a.dc_re = p->dc_re; a.dc_im = p->dc_im;
  a.has_dc = p->dc_re != 0.f || p->dc_im != 0.f;
}

// the call's launch on stream st; the caller has checked the buffers.  0 < n <= 2^31.
inline int rf_enqueue(dvbt_rf *h, const float2 *in, long long n, float2 *out, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const long long n0 = (long long)h->p.first_sample + h->pos;
  const int lead = (int)(((uintptr_t)out >> 3) & 1);
  const unsigned blocks = (unsigned)((n + lead + RF_TILE - 1) / RF_TILE);             // <= 2^21 + 1: one launch
  hipLaunchKernelGGL(rf_kernel, dim3(blocks), dim3(RF_THREADS), 0, st, in, out, n0, n, lead, h->a);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->pos += n;
  return DVBT_OK;
}

// the mask's integral over [lo, hi], segment by segment in closed form: L = l_k (f / f_k)^s on segment k
inline double rf_mask_integral(const dvbt_rf_mask *mk, double lo, double hi)
{
  double sum = 0.0;
  for (int k = 0; k + 1 < mk->n_points; k++) {
    const double fa = mk->offset_hz[k], fb = mk->offset_hz[k + 1];
    const double a = lo > fa ? lo : fa, b = hi < fb ? hi : fb;
    if (!(b > a)) continue;
    const double s = (mk->dbc_hz[k + 1] - mk->dbc_hz[k]) / (10.0 * log10(fb / fa));
    const double lk = pow(10.0, mk->dbc_hz[k] / 10.0);
    const double w = log(b / a);
    const double F = fabs(s + 1.0) < 1e-9 ? w : expm1((s + 1.0) * w) / (s + 1.0);
    sum += lk * pow(a / fa, s) * a * F;
  }
  return sum;
}

}  // namespace

extern "C" int dvbt_rf_phase_noise_tones(const dvbt_rf_mask *mk, int n_tones, uint64_t seed, uint64_t *inc, uint64_t *phase, float *amp)
{
  if (!mk || !inc || !phase || !amp) return fail(DVBT_ERR_INVALID, "null argument");
  if (n_tones < 1 || n_tones > DVBT_RF_MAX_TONES) return fail(DVBT_ERR_INVALID, "n_tones must be in [1, DVBT_RF_MAX_TONES]");
  if (mk->n_points < 2 || mk->n_points > DVBT_RF_MAX_MASK_POINTS) return fail(DVBT_ERR_INVALID, "a mask has 2 to DVBT_RF_MAX_MASK_POINTS points");
  if (!(mk->sample_rate > 0.0) || !std::isfinite(mk->sample_rate)) return fail(DVBT_ERR_INVALID, "sample_rate must be a finite number > 0");
  for (int k = 0; k < mk->n_points; k++) {
    if (!std::isfinite(mk->offset_hz[k]) || !std::isfinite(mk->dbc_hz[k])) return fail(DVBT_ERR_INVALID, "a mask point must be finite");
    if (!(mk->offset_hz[k] > (k ? mk->offset_hz[k - 1] : 0.0))) return fail(DVBT_ERR_INVALID, "the mask's offsets must be > 0 and strictly ascending");
  }
  if (mk->offset_hz[mk->n_points - 1] > mk->sample_rate / 2.0) return fail(DVBT_ERR_INVALID, "the mask's last offset must be <= sample_rate / 2");
  const int M = n_tones;
  const double f0 = mk->offset_hz[0], fl = mk->offset_hz[mk->n_points - 1], lr = log(fl / f0);
  for (int m = 0; m < M; m++) {
    const double lo = m ? f0 * exp(lr * (double)m / (double)M) : f0, hi = m + 1 < M ? f0 * exp(lr * (double)(m + 1) / (double)M) : fl;
    uint32_t w[4];
    philox4x32_10((uint32_t)m, 0u, 0u, RF_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double u = ((double)w[0] + 0.5) * 2.3283064365386963e-10;                 // 2^-32
    const double f = f0 * exp(lr * ((double)m + u) / (double)M);
    inc[m] = (uint64_t)nearbyint(ldexp(f / mk->sample_rate, 64));                    // f / sample_rate <= 1/2: at most 2^63
    phase[m] = ((uint64_t)w[1] << 32) | w[2];
    amp[m] = (float)(2.0 * sqrt(rf_mask_integral(mk, lo, hi)));
  }
  return DVBT_OK;
}

extern "C" int dvbt_rf_create(const dvbt_rf_params *p, dvbt_rf **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = rf_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_rf> hold(new dvbt_rf()); dvbt_rf *const h = hold.get();   // released on every early return below
  h->p = *p;
  rf_fill_args(p, h->a);
  HIPCHK(h->ord.create());
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_rf_run_device(dvbt_rf *h, const void *iq_device, size_t n, void *out_device, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = check_samples(iq_device, n, out_device, true); if (r) return r;   // in place is fine: the block has no delay line
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return rf_enqueue(h, (const float2 *)iq_device, (long long)n, (float2 *)out_device, (hipStream_t)stream);
}

extern "C" int dvbt_rf_run(dvbt_rf *h, const void *iq_host, size_t n, void *out_host)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = check_samples(iq_host, n, out_host, true); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->dio, h->dio, iq_host, n * sizeof(float2), out_host, n * sizeof(float2), [&](const void *in, void *out) {
    return rf_enqueue(h, (const float2 *)in, (long long)n, (float2 *)out, h->ord.s); });
}

extern "C" int dvbt_rf_reset(dvbt_rf *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  h->pos = 0;                         // nothing on the device depends on the position
  return DVBT_OK;
}

extern "C" void dvbt_rf_destroy(dvbt_rf *h) { delete h; }
