// dvbt_sounder.inc -- dvbt_sounder_*: a channel sounder -- the echo profile (power over delay) and the amplitude response of the channel, from the scattered
// pilots of fft-shifted symbol rows -- as one streaming handle (DESIGN.md 4i) over k_sounder.hpp.  It consumes rows and changes nothing.  Included from
// dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of symbols it has seen (the numbers of closed groups and runs are host arithmetic on it, so nothing waits
// for the device) and, on the device, the open group (its entries, c_0 and four ints) in two buffers written alternately (as dvbt_clock and dvbt_spectrum
// carry theirs), the open run's accumulators, likewise in two buffers, and the sums.  dvbt_sounder_read synchronises and copies on the handle's own stream,
// and changes nothing.

struct dvbt_sounder {
  dvbt_sounder_params p;
  Dims d; int Kp = 0, M = 0;
  DevMem<float> win, pref; DevMem<int16_t> cpilot;
  FftPlan twN, twM;                                // twN: its table alone, as cis(-2 pi t / N) (snd_tau); twM: the profile's transform
  DevMem<float2> carry[2]; int cur = 0;            // the open group
  DevMem<float> open[2]; int ocur = 0;             // the open run: a slab as it stands
  DevMem<double> res;                              // M + Kp doubles (the sums of |h|^2 and |E|^2), then the count of used groups (a long long)
  long long pos = 0;                               // symbols since create / reset
  double sum_w = 0.0;
  DevMem<float2> ebuf;                             // the closed groups of one launch: [SND_MAX_RUNS SND_RUN][Kp]
  DevMem<float> slabs;                             // the closed runs of one launch
  DevBuf din, dmeta;                               // staging of the host entry: the rows, the three int arrays
  CallOrder ord;                                   // last: see CallOrder
};

namespace {

constexpr long long SND_MAX_TOTAL = 1ll << 56;
constexpr size_t SND_MAX_CALL = (size_t)1 << 24;
constexpr int SND_MAX_RUNS = 256;                  // runs per launch: bounds ebuf (37 MB in 8k) and the slabs

inline int sounder_check_params(const dvbt_sounder_params *p)
{
  if (p->transmission_mode < 0 || p->transmission_mode > 1) return fail(DVBT_ERR_INVALID, "transmission_mode must be 0 (2k) or 1 (8k)");
  if (p->window < 0 || p->window > 1) return fail(DVBT_ERR_INVALID, "window must be 0 (rectangular) or 1 (Hann)");
  if (p->first_index < 0 || p->first_index > 67) return fail(DVBT_ERR_INVALID, "first_index must be in 0..67");
  if (p->device < 0) return fail(DVBT_ERR_INVALID, "no such device");
  return DVBT_OK;
}

// the periodic window over the Kp entries (argument j / Kp) in double, rounded to float
inline std::vector<float> sounder_window(int Kp, int window)
{
  std::vector<float> w(Kp);
  for (int j = 0; j < Kp; j++) w[j] = (float)(window == 0 ? 1.0 : 0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)Kp));
  return w;
}

inline int sounder_check_call(const dvbt_sounder *h, const void *rows, const int *idx, const int *off, const int *cps, size_t nsym)
{
  if (nsym == 0) return DVBT_OK;
  if (!rows) return fail(DVBT_ERR_INVALID, "null buffer");
  if (nsym > SND_MAX_CALL) return fail(DVBT_ERR_INVALID, "nsym must be <= 2^24 per call (a longer stream continues over calls)");
  if ((long long)nsym > SND_MAX_TOTAL - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^56 symbols");
  if (misaligned8(rows)) return fail(DVBT_ERR_INVALID, "the rows must be 8-byte aligned");
  if ((((uintptr_t)idx | (uintptr_t)off | (uintptr_t)cps) & 3) != 0) return fail(DVBT_ERR_INVALID, "the int arrays must be 4-byte aligned");
  return DVBT_OK;
}

inline void sounder_extract(dvbt_sounder *h, const SndArgs &a, long long s_first, int nsym, long long g_base, float2 *carry_out, long long g_open,
                            bool copy_old, hipStream_t st)
{
  hipLaunchKernelGGL(sounder_extract_kernel, dim3((unsigned)(nsym + (copy_old ? 1 : 0))), dim3(SND_EXTRACT_THREADS), 0, st, a, s_first, nsym, g_base,
                     (float2 *)h->ebuf, carry_out, g_open, copy_old ? 1 : 0, (const int16_t *)h->cpilot, (const float *)h->pref, (const float2 *)h->twN.tw);
}

// the call's launches on stream st; the caller has checked the buffers.  0 < n <= 2^24.
inline int sounder_enqueue(dvbt_sounder *h, const float2 *rows, const int *idx, const int *off, const int *cps, int n, hipStream_t st)
{
  const int M = h->M, Kp = h->Kp;
  SndArgs a;
  a.N = h->d.N; a.K = h->d.K; a.Kp = Kp; a.M = M; a.zl = h->d.zl; a.n_cp = h->d.n_cp; a.first_index = h->p.first_index;
  a.n = n; a.pos0 = h->pos; a.rows = rows; a.idx = idx; a.off = off; a.cps = cps; a.carry_in = h->carry[h->cur];
  const long long pos1 = h->pos + n, ga = h->pos / 4, gb = pos1 / 4;       // the call closes the groups [ga, gb)
  const bool had_open = (h->pos % 4) != 0, has_open = (pos1 % 4) != 0;
  const bool to_open = gb > ga && (gb % SND_RUN) != 0;
  const int nxt = h->cur ^ 1, onxt = h->ocur ^ 1;
  const size_t words = snd_slab_words(M, Kp);
  HIPCHK(h->ord.join(st));
  if (gb > ga) {
    const long long r0 = ga / SND_RUN, r1 = (gb - 1) / SND_RUN;            // the call's runs: r0 .. r1
    double *const res = h->res;
    for (long long r = r0; r <= r1; r += SND_MAX_RUNS) {
      const int runs = (int)std::min<long long>(SND_MAX_RUNS, r1 - r + 1);
      const long long g_lo = std::max(r * SND_RUN, ga), g_hi = std::min((r + runs) * SND_RUN, gb);
      const long long s_lo = std::max(4 * g_lo, h->pos);
      sounder_extract(h, a, s_lo, (int)(4 * g_hi - s_lo), g_lo, nullptr, -1, had_open && g_lo == ga, st);
      HIPCHK(hipGetLastError());
      if (a.N == 2048)
        hipLaunchKernelGGL((sounder_profile_kernel<1024 / FFT_THREADS, (569 + FFT_THREADS - 1) / FFT_THREADS>), dim3((unsigned)runs), dim3(FFT_THREADS), h->twM.lds(),
                           st, a, (const float2 *)h->ebuf, g_lo, r, ga, gb, (const float *)h->win, (const float2 *)h->twM.tw, (const float *)h->open[h->ocur],
                           (float *)h->open[onxt], (float *)h->slabs);
      else
        hipLaunchKernelGGL((sounder_profile_kernel<4096 / FFT_THREADS, (2273 + FFT_THREADS - 1) / FFT_THREADS>), dim3((unsigned)runs), dim3(FFT_THREADS), h->twM.lds(),
                           st, a, (const float2 *)h->ebuf, g_lo, r, ga, gb, (const float *)h->win, (const float2 *)h->twM.tw, (const float *)h->open[h->ocur],
                           (float *)h->open[onxt], (float *)h->slabs);
      HIPCHK(hipGetLastError());
      const int closed = runs - ((r + runs - 1 == r1 && to_open) ? 1 : 0);
      if (closed > 0) {
        hipLaunchKernelGGL(sounder_fold_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, (const float *)h->slabs, (int)words, closed, res,
                           (long long *)(res + M + Kp));
        HIPCHK(hipGetLastError());
      }
    }
  }
  if (has_open) {
    const long long s_lo = std::max(4 * gb, h->pos);
    sounder_extract(h, a, s_lo, (int)(pos1 - s_lo), gb, (float2 *)h->carry[nxt], gb, had_open && gb == ga, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(h->ord.mark(st));
  if (has_open) h->cur = nxt;
  if (to_open) h->ocur = onxt;
  h->pos = pos1;
  return DVBT_OK;
}

// back to the state after create: the sums zeroed (the open group and the open run are not read before they are written again)
inline int sounder_rewind(dvbt_sounder *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->res, 0, sizeof(double) * ((size_t)h->M + h->Kp + 1), h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_sounder_create(const dvbt_sounder_params *p, dvbt_sounder **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = sounder_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_sounder> hold(new dvbt_sounder()); dvbt_sounder *const h = hold.get();   // released on every early return below
  h->p = *p;
  h->d = make_dims(1, 0, 0, 0, p->transmission_mode);
  if (!h->d.valid || FFT_THREADS != 512) return fail(DVBT_ERR_INVALID, "the sounder's kernels are laid out for workgroups of 512");
  const int N = h->d.N, Kp = (h->d.K - 1) / 3 + 1, M = N / 2;
  h->Kp = Kp; h->M = M;
  const std::vector<float> w = sounder_window(Kp, p->window);
  for (int j = 0; j < Kp; j++) h->sum_w += (double)w[j];
  const std::vector<int> c = cpilot_table(h->d);
  const std::vector<int16_t> c16(c.begin(), c.end());
  if ((r = upload(w, h->win)) || (r = h->twN.build(N)) || (r = h->twM.build(M)) || (r = upload(c16, h->cpilot)) ||
      (r = upload(pilot_ref_table(h->d), h->pref))) return r;
  const void *fn = N == 2048 ? (const void *)sounder_profile_kernel<1024 / FFT_THREADS, (569 + FFT_THREADS - 1) / FFT_THREADS>
                             : (const void *)sounder_profile_kernel<4096 / FFT_THREADS, (2273 + FFT_THREADS - 1) / FFT_THREADS>;
  if ((r = set_lds(fn, h->twM.lds()))) return r;
  HIPCHK(h->ord.create());
  const size_t words = snd_slab_words(M, Kp);
  for (int i = 0; i < 2; i++) {
    HIPCHK(h->carry[i].alloc(snd_carry_float2(Kp))); HIPCHK(hipMemsetAsync(h->carry[i], 0, sizeof(float2) * snd_carry_float2(Kp), h->ord.s));
    HIPCHK(h->open[i].alloc(words)); HIPCHK(hipMemsetAsync(h->open[i], 0, sizeof(float) * words, h->ord.s));
  }
  HIPCHK(h->ebuf.alloc((size_t)SND_MAX_RUNS * SND_RUN * Kp));
  HIPCHK(h->slabs.alloc((size_t)SND_MAX_RUNS * words));
  HIPCHK(h->res.alloc((size_t)M + Kp + 1));
  if ((r = sounder_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_sounder_push_device(dvbt_sounder *h, const void *rows_dev, const int *idx_dev, const int *off_dev, const int *cps_dev, size_t nsym,
                                        void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = sounder_check_call(h, rows_dev, idx_dev, off_dev, cps_dev, nsym); if (r) return r;
  if (nsym == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return sounder_enqueue(h, (const float2 *)rows_dev, idx_dev, off_dev, cps_dev, (int)nsym, (hipStream_t)stream);
}

extern "C" int dvbt_sounder_push(dvbt_sounder *h, const void *rows_host, const int *idx_host, const int *off_host, const int *cps_host, size_t nsym)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = sounder_check_call(h, rows_host, idx_host, off_host, cps_host, nsym); if (r) return r;
  if (nsym == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  if ((r = h->dmeta.reserve(3 * nsym * sizeof(int)))) return r;
  return staged_call(h->ord, h->din, h->din, rows_host, nsym * (size_t)h->d.N * sizeof(float2), nullptr, 0, [&](const void *in, void *) {
    int *const m = (int *)h->dmeta.p;
    const int *host[3] = {idx_host, off_host, cps_host}, *dev[3];
    for (int i = 0; i < 3; i++) {
      dev[i] = host[i] ? m + (size_t)i * nsym : nullptr;
      if (host[i]) HIPCHK(hipMemcpyAsync(m + (size_t)i * nsym, host[i], nsym * sizeof(int), hipMemcpyHostToDevice, h->ord.s));
    }
    return sounder_enqueue(h, (const float2 *)in, dev[0], dev[1], dev[2], (int)nsym, h->ord.s); });
}

extern "C" int dvbt_sounder_read(dvbt_sounder *h, dvbt_sounder_result *res, double *pdp, size_t cap_pdp, double *resp, size_t cap_resp)
{
  if (!h || !res) return fail(DVBT_ERR_INVALID, "null argument");
  const int M = h->M, Kp = h->Kp;
  if ((pdp && cap_pdp < (size_t)M) || (resp && cap_resp < (size_t)Kp)) return fail(DVBT_ERR_INVALID, "pdp takes M doubles, resp Kp");
  HIPCHK(hipSetDevice(h->p.device));
  const long long groups = h->pos / 4;
  const bool open = (groups % SND_RUN) != 0;
  const size_t words = snd_slab_words(M, Kp);
  std::vector<double> r((size_t)M + Kp + 1);
  std::vector<float> o(words, 0.f);
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemcpyAsync(r.data(), h->res, sizeof(double) * r.size(), hipMemcpyDeviceToHost, h->ord.s));
  if (open) HIPCHK(hipMemcpyAsync(o.data(), h->open[h->ocur], sizeof(float) * words, hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipStreamSynchronize(h->ord.s));
  long long used; memcpy(&used, r.data() + M + Kp, sizeof used);
  if (open) { int u; memcpy(&u, o.data() + M + Kp, sizeof u); used += u; }
  memset(res, 0, sizeof *res);
  res->symbols_pushed = h->pos; res->groups_used = used; res->groups_skipped = groups - used; res->M = M; res->Kp = Kp;
  const double norm = h->sum_w * h->sum_w;
  if (pdp) for (int b = 0; b < M; b++) pdp[b] = (open ? r[b] + (double)o[b] : r[b]) / norm;
  if (resp) for (int b = 0; b < Kp; b++) resp[b] = open ? r[M + b] + (double)o[M + b] : r[M + b];
  return DVBT_OK;
}

extern "C" int dvbt_sounder_reset(dvbt_sounder *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return sounder_rewind(h);
}

extern "C" void dvbt_sounder_destroy(dvbt_sounder *h) { delete h; }
