// dvbt_scan.inc -- dvbt_scan_*: FFT size, guard interval, symbol timing and fractional carrier offset of an unknown DVB-T signal, from the cyclic-prefix
// correlation folded at the eight candidate symbol lengths, as one streaming handle (DESIGN.md 4i) over k_scan.hpp.  It consumes a stream and changes
// nothing.  Included from dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of samples it has seen (the symbols each hypothesis has completed are host arithmetic on it, so nothing
// waits for the device) and, on the device, the samples from the oldest incomplete symbol's start on (fewer than 10240 + 8192), in two buffers written
// alternately (as dvbt_spectrum), every hypothesis' open group, likewise in two buffers, and the accumulators.  dvbt_scan_read synchronises and copies on the
// handle's own stream, evaluates on the host (dvbt_scan_evaluate: double arithmetic, no device), and changes nothing.

struct dvbt_scan {
  dvbt_scan_params p;                 // rho_min, ratio_min already resolved (0 -> the defaults)
  DevMem<float2> hist[2]; int cur = 0;
  long long hbase = 0;                // stream index of hist[cur][0]
  DevMem<float> open[2]; int ocur[SCAN_HYPS] = {0, 0, 0, 0, 0, 0, 0, 0};   // the open groups: hypothesis h's 3 S floats at 3 scan_off(h), in open[ocur[h]]
  DevMem<double> res;                 // 3 SCAN_BINS doubles laid out like `open`, then the count of non-finite samples (64 bits)
  long long pos = 0;                  // samples since create / reset
  DevBuf slabs;                       // the closed groups of one launch: floats [groups][3 S]
  DevBuf din;                         // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

namespace {

constexpr long long SCAN_MAX_TOTAL = 1ll << 56;
constexpr int SCAN_MAX_GROUPS = 512;               // groups per launch: bounds the slab buffer (60 MB at S = 10240)
constexpr double SCAN_RHO_MIN = 0.1, SCAN_RATIO_MIN = 1.5;

inline int scan_check_params(const dvbt_scan_params *p)
{
  if (!p) return fail(DVBT_ERR_INVALID, "null argument");
  if (!(p->rho_min >= 0.0 && p->rho_min <= 1.0)) return fail(DVBT_ERR_INVALID, "rho_min must be in (0, 1] (0: 0.1)");
  if (!(p->ratio_min == 0.0 || (p->ratio_min >= 1.0 && p->ratio_min <= 1e6))) return fail(DVBT_ERR_INVALID, "ratio_min must be in [1, 1e6] (0: 1.5)");
  if (p->device < 0) return fail(DVBT_ERR_INVALID, "no such device");
  return DVBT_OK;
}

// complete symbols of hypothesis hyp once `pos` samples have been pushed
inline long long scan_symbols(long long pos, int hyp) { const int N = scan_N(hyp); return pos >= N ? (pos - N) / scan_S(hyp) : 0; }

inline int scan_check_call(const dvbt_scan *h, const void *in, size_t n)
{
  int r = check_samples(in, n, in, true); if (r) return r;
  if ((long long)n > SCAN_MAX_TOTAL - h->pos) return fail(DVBT_ERR_INVALID, "a stream takes at most 2^56 samples");
  return DVBT_OK;
}

// the call's launches on stream st; the caller has checked the buffer.  0 < n <= 2^31.
inline int scan_enqueue(dvbt_scan *h, const float2 *in, long long n, hipStream_t st)
{
  const long long pos0 = h->pos, pos1 = pos0 + n;
  long long j0[SCAN_HYPS], j1[SCAN_HYPS], first = pos1;
  bool any = false;
  for (int k = 0; k < SCAN_HYPS; k++) {
    j0[k] = scan_symbols(pos0, k); j1[k] = scan_symbols(pos1, k);
    any = any || j1[k] > j0[k];
    first = std::min(first, j1[k] * scan_S(k));    // what the next call needs starts at the oldest incomplete symbol
  }
  const long long cnt = pos1 - first;              // 0 < cnt < SCAN_HIST
  if (any) { int r = h->slabs.reserve((size_t)SCAN_MAX_GROUPS * 3 * scan_S(SCAN_HYPS - 1) * sizeof(float)); if (r) return r; }
  HIPCHK(h->ord.join(st));
  double *const res = h->res;
  const float2 *const hist = h->hist[h->cur];
  hipLaunchKernelGGL(scan_count_kernel, dim3((unsigned)std::min<long long>((n + SCAN_THREADS - 1) / SCAN_THREADS, 2048)), dim3(SCAN_THREADS), 0, st, in, n,
                     (unsigned long long *)(res + 3 * (size_t)SCAN_BINS));
  HIPCHK(hipGetLastError());
  int ocur[SCAN_HYPS];
  for (int k = 0; k < SCAN_HYPS; k++) {
    ocur[k] = h->ocur[k];
    if (j1[k] == j0[k]) continue;
    const int S = scan_S(k);
    const size_t off = 3 * (size_t)scan_off(k);
    ScanArgs a;
    a.N = scan_N(k); a.S = S; a.j0 = j0[k]; a.j1 = j1[k]; a.pos0 = pos0; a.hbase = h->hbase;
    const long long g0 = j0[k] / SCAN_GROUP, g1 = (j1[k] - 1) / SCAN_GROUP;            // the call's groups: g0 .. g1
    const bool to_open = (j1[k] % SCAN_GROUP) != 0;
    const float *const oin = h->open[ocur[k]] + off; float *const oout = h->open[ocur[k] ^ 1] + off;
    for (long long g = g0; g <= g1; g += SCAN_MAX_GROUPS) {
      const int groups = (int)std::min<long long>(SCAN_MAX_GROUPS, g1 - g + 1);
      hipLaunchKernelGGL(scan_kernel, dim3((unsigned)((S + SCAN_THREADS - 1) / SCAN_THREADS), (unsigned)groups), dim3(SCAN_THREADS), 0, st, in, hist, a, g,
                         oin, oout, (float *)h->slabs.p);
      HIPCHK(hipGetLastError());
      const int closed = groups - ((g + groups - 1 == g1 && to_open) ? 1 : 0);
      if (closed > 0) {
        hipLaunchKernelGGL(scan_fold_kernel, dim3((unsigned)((3 * S + SCAN_THREADS - 1) / SCAN_THREADS)), dim3(SCAN_THREADS), 0, st,
                           (const float *)h->slabs.p, 3 * S, closed, res + off);
        HIPCHK(hipGetLastError());
      }
    }
    if (to_open) ocur[k] ^= 1;
  }
  const int nxt = h->cur ^ 1;
  hipLaunchKernelGGL(scan_carry_kernel, dim3((unsigned)((cnt + SCAN_THREADS - 1) / SCAN_THREADS)), dim3(SCAN_THREADS), 0, st, in, hist, pos0, h->hbase, first,
                     (int)cnt, (float2 *)h->hist[nxt]);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  for (int k = 0; k < SCAN_HYPS; k++) h->ocur[k] = ocur[k];
  h->cur = nxt; h->hbase = first; h->pos = pos1;
  return DVBT_OK;
}

// back to the state after create: the accumulators zeroed (the history and the open groups are not read before they are written again)
inline int scan_rewind(dvbt_scan *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->res, 0, sizeof(double) * (3 * (size_t)SCAN_BINS + 1), h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->pos = 0; h->hbase = 0;
  return DVBT_OK;
}

// the device's sums as they stand: every hypothesis' A (S pairs re, im) and E (S doubles), the open group added last, and the non-finite count
inline int scan_fetch(dvbt_scan *h, std::vector<double> A[SCAN_HYPS], std::vector<double> E[SCAN_HYPS], long long *nonfinite)
{
  std::vector<double> r(3 * (size_t)SCAN_BINS + 1);
  std::vector<float> o[2];
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemcpyAsync(r.data(), h->res, sizeof(double) * r.size(), hipMemcpyDeviceToHost, h->ord.s));
  for (int b = 0; b < 2; b++) {
    o[b].resize(3 * (size_t)SCAN_BINS);
    HIPCHK(hipMemcpyAsync(o[b].data(), h->open[b], sizeof(float) * o[b].size(), hipMemcpyDeviceToHost, h->ord.s));
  }
  HIPCHK(hipStreamSynchronize(h->ord.s));
  for (int k = 0; k < SCAN_HYPS; k++) {
    const int S = scan_S(k);
    const size_t off = 3 * (size_t)scan_off(k);
    const bool open = (scan_symbols(h->pos, k) % SCAN_GROUP) != 0;
    const double *const a = r.data() + off;
    const float *const f = o[h->ocur[k]].data() + off;
    A[k].resize(2 * (size_t)S); E[k].resize(S);
    for (int m = 0; m < S; m++) {
      A[k][2 * m] = open ? a[m] + (double)f[m] : a[m];
      A[k][2 * m + 1] = open ? a[S + m] + (double)f[S + m] : a[S + m];
      E[k][m] = open ? a[2 * S + m] + (double)f[2 * S + m] : a[2 * S + m];
    }
  }
  unsigned long long nf; memcpy(&nf, r.data() + 3 * (size_t)SCAN_BINS, sizeof nf);
  *nonfinite = (long long)nf;
  return DVBT_OK;
}

// one hypothesis' rho, symbol_start and cfo from its sums (include/dvbt_hip.h has the order of operations)
inline void scan_evaluate_one(int hyp, long long J, const double *A, const double *E, double *rho, int *start, double *cfo)
{
  *rho = 0.0; *start = 0; *cfo = 0.0;
  if (J <= 0) return;
  const int G = scan_G(hyp), S = scan_S(hyp);
  double sr = 0.0, si = 0.0, se = 0.0;
  for (int m = 0; m < S; m++) { sr = sr + A[2 * m]; si = si + A[2 * m + 1]; se = se + E[m]; }
  if (!std::isfinite(sr) || !std::isfinite(si) || !std::isfinite(se)) { *rho = std::numeric_limits<double>::quiet_NaN(); return; }
  const double mr = sr / (double)S, mi = si / (double)S;
  std::vector<double> ar(S), ai(S);
  for (int m = 0; m < S; m++) { ar[m] = A[2 * m] - mr; ai[m] = A[2 * m + 1] - mi; }
  double cr = 0.0, ci = 0.0, ph = 0.0;
  for (int k = 0; k < G; k++) { cr = cr + ar[k]; ci = ci + ai[k]; ph = ph + E[k]; }
  double best = cr * cr + ci * ci, bcr = cr, bci = ci, bph = ph;
  int bm = 0;
  for (int m = 0; m + 1 < S; m++) {
    const int t = m + G < S ? m + G : m + G - S;
    cr = (cr - ar[m]) + ar[t]; ci = (ci - ai[m]) + ai[t]; ph = (ph - E[m]) + E[t];
    const double q = cr * cr + ci * ci;
    if (q > best) { best = q; bcr = cr; bci = ci; bph = ph; bm = m + 1; }
  }
  *start = bm;
  *rho = bph > 0.0 ? std::sqrt(best) / (bph / 2.0) : 0.0;
  const double c = -std::atan2(bci, bcr) / (2.0 * M_PI);
  *cfo = c == -0.5 ? 0.5 : c;
}

}  // namespace

extern "C" int dvbt_scan_evaluate(const dvbt_scan_params *p, const int64_t symbols[8], const double *const A[8], const double *const E[8], int64_t samples,
                                  int64_t nonfinite, dvbt_scan_result *res)
{
  int r = scan_check_params(p); if (r) return r;
  if (!symbols || !A || !E || !res) return fail(DVBT_ERR_INVALID, "null argument");
  if (samples < 0 || nonfinite < 0) return fail(DVBT_ERR_INVALID, "samples and nonfinite must be >= 0");
  for (int k = 0; k < SCAN_HYPS; k++) {
    if (symbols[k] < 0) return fail(DVBT_ERR_INVALID, "symbols must be >= 0");
    if (symbols[k] > 0 && (!A[k] || !E[k])) return fail(DVBT_ERR_INVALID, "a hypothesis with symbols needs its accumulators");
  }
  const double rho_min = p->rho_min == 0.0 ? SCAN_RHO_MIN : p->rho_min, ratio_min = p->ratio_min == 0.0 ? SCAN_RATIO_MIN : p->ratio_min;
  memset(res, 0, sizeof *res);
  res->samples_pushed = samples; res->nonfinite = nonfinite;
  bool enough = true, finite = true;
  for (int k = 0; k < SCAN_HYPS; k++) {
    res->symbols[k] = symbols[k];
    scan_evaluate_one(k, symbols[k], A[k], E[k], &res->rho[k], &res->symbol_start[k], &res->cfo[k]);
    enough = enough && symbols[k] >= 8;
    finite = finite && std::isfinite(res->rho[k]);
  }
  int b = 0, ru = -1;
  for (int k = 1; k < SCAN_HYPS; k++) if (res->rho[k] > res->rho[b]) b = k;
  for (int k = 0; k < SCAN_HYPS; k++) if (k != b && (ru < 0 || res->rho[k] > res->rho[ru])) ru = k;
  res->detected = enough && finite && nonfinite == 0 && res->rho[b] >= rho_min && res->rho[b] >= ratio_min * res->rho[ru];
  res->mode = res->detected ? b >> 2 : -1;
  res->guard = res->detected ? b & 3 : -1;
  return DVBT_OK;
}

extern "C" int dvbt_scan_create(const dvbt_scan_params *p, dvbt_scan **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = scan_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_scan> hold(new dvbt_scan()); dvbt_scan *const h = hold.get();   // released on every early return below
  h->p = *p;
  if (h->p.rho_min == 0.0) h->p.rho_min = SCAN_RHO_MIN;
  if (h->p.ratio_min == 0.0) h->p.ratio_min = SCAN_RATIO_MIN;
  HIPCHK(h->ord.create());
  for (int i = 0; i < 2; i++) {
    HIPCHK(h->hist[i].alloc(SCAN_HIST)); HIPCHK(hipMemsetAsync(h->hist[i], 0, sizeof(float2) * SCAN_HIST, h->ord.s));
    HIPCHK(h->open[i].alloc(3 * (size_t)SCAN_BINS)); HIPCHK(hipMemsetAsync(h->open[i], 0, sizeof(float) * 3 * (size_t)SCAN_BINS, h->ord.s));
  }
  HIPCHK(h->res.alloc(3 * (size_t)SCAN_BINS + 1));
  if ((r = scan_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_scan_push_device(dvbt_scan *h, const void *iq_device, size_t n, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = scan_check_call(h, iq_device, n); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return scan_enqueue(h, (const float2 *)iq_device, (long long)n, (hipStream_t)stream);
}

extern "C" int dvbt_scan_push(dvbt_scan *h, const void *iq_host, size_t n)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = scan_check_call(h, iq_host, n); if (r) return r;
  if (n == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->din, iq_host, n * sizeof(float2), nullptr, 0, [&](const void *in, void *) {
    return scan_enqueue(h, (const float2 *)in, (long long)n, h->ord.s); });
}

extern "C" int dvbt_scan_accumulators(dvbt_scan *h, int hyp, double *A_re_im, double *E, int cap)
{
  if (!h || !A_re_im || !E) return fail(DVBT_ERR_INVALID, "null argument");
  if (hyp < 0 || hyp >= SCAN_HYPS) return fail(DVBT_ERR_INVALID, "hyp must be in 0 .. 7");
  if (cap < scan_S(hyp)) return fail(DVBT_ERR_INVALID, "the buffers must hold S bins");
  HIPCHK(hipSetDevice(h->p.device));
  std::vector<double> A[SCAN_HYPS], Ev[SCAN_HYPS];
  long long nf;
  int r = scan_fetch(h, A, Ev, &nf); if (r) return r;
  memcpy(A_re_im, A[hyp].data(), sizeof(double) * A[hyp].size());
  memcpy(E, Ev[hyp].data(), sizeof(double) * Ev[hyp].size());
  return DVBT_OK;
}

extern "C" int dvbt_scan_read(dvbt_scan *h, dvbt_scan_result *res)
{
  if (!h || !res) return fail(DVBT_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->p.device));
  std::vector<double> A[SCAN_HYPS], Ev[SCAN_HYPS];
  long long nf;
  int r = scan_fetch(h, A, Ev, &nf); if (r) return r;
  int64_t J[SCAN_HYPS]; const double *Ap[SCAN_HYPS], *Ep[SCAN_HYPS];
  for (int k = 0; k < SCAN_HYPS; k++) { J[k] = scan_symbols(h->pos, k); Ap[k] = A[k].data(); Ep[k] = Ev[k].data(); }
  return dvbt_scan_evaluate(&h->p, J, Ap, Ep, h->pos, nf, res);
}

extern "C" int dvbt_scan_reset(dvbt_scan *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return scan_rewind(h);
}

extern "C" void dvbt_scan_destroy(dvbt_scan *h) { delete h; }
