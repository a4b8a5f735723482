// dvbt_constellation.inc -- dvbt_constellation_*: a constellation analyser -- the I/Q density, the error cloud of every point and the signal and error sums of
// every carrier, from rows of equalised cells -- as one streaming handle (DESIGN.md 4i) over k_constellation.hpp.  It consumes rows and changes nothing.
// Included from dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of rows it has seen and, on the device, one array of 64-bit integers (the density, the point moments, the
// carrier sums, the two counts).  Integer adds commute, so nothing is carried between calls and no order is kept.  dvbt_constellation_read synchronises and
// copies on the handle's own stream, and changes nothing.

struct dvbt_constellation {
  dvbt_constellation_params p;
  int alpha = 1, H = 1, span = 2, cus = 1;
  float inv_d = 1.f;
  DevMem<unsigned long long> acc;                  // con_words(P) words: con_off_*
  long long rows = 0;                              // rows since create / reset
  DevBuf din;                                      // staging of the host entry
  CallOrder ord;                                   // last: see CallOrder
};

namespace {

constexpr long long CON_MAX_CELLS = 1ll << 33;     // per stream: 32767^2 2^33 < 2^63
constexpr size_t CON_MAX_CALL = (size_t)1 << 24;   // rows per call
constexpr int CON_MAX_BAND = 1 << 20;              // rows per workgroup: 2^20 rows of at most 2 CON_THREADS columns stay below CON_MAX_WG_CELLS

inline int constellation_check_params(const dvbt_constellation_params *p)
{
  if (p->constellation < DVBT_QPSK || p->constellation > DVBT_QAM64) return fail(DVBT_ERR_INVALID, "constellation must be 0 (QPSK), 1 (QAM16) or 2 (QAM64)");
  if (p->hierarchy < DVBT_NH || p->hierarchy > DVBT_ALPHA4) return fail(DVBT_ERR_INVALID, "hierarchy must be in 0..3");
  if (p->constellation == DVBT_QPSK && p->hierarchy != DVBT_NH) return fail(DVBT_ERR_INVALID, "QPSK is not hierarchical");
  if (p->row_length < 1 || p->row_length > 8192) return fail(DVBT_ERR_INVALID, "row_length must be in 1..8192");
  if (p->device < 0) return fail(DVBT_ERR_INVALID, "no such device");
  return DVBT_OK;
}

inline int constellation_check_call(const dvbt_constellation *h, const void *rows, size_t nrows)
{
  if (nrows == 0) return DVBT_OK;
  if (!rows) return fail(DVBT_ERR_INVALID, "null buffer");
  if (nrows > CON_MAX_CALL) return fail(DVBT_ERR_INVALID, "nrows must be <= 2^24 per call (a longer stream continues over calls)");
  if (misaligned8(rows)) return fail(DVBT_ERR_INVALID, "the rows must be 8-byte aligned");
  if ((h->rows + (long long)nrows) * h->p.row_length > CON_MAX_CELLS) return fail(DVBT_ERR_CAPACITY, "a stream takes at most 2^33 cells");
  return DVBT_OK;
}

// the launch geometry for P cells a row: k tiles of tx threads side by side (two columns each), ty rows at a time.  Of the tile counts from the fewest on,
// the one that leaves the fewest threads of a workgroup idle (1512: 3 tiles of 252 x 2; 6048: 6 tiles of 504 x 1)
inline void constellation_geometry(int P, int *tiles, int *tx, int *ty)
{
  const int pairs = (P + 1) / 2, kmin = (pairs + CON_THREADS - 1) / CON_THREADS;
  int best = 0;
  for (int k = kmin; k < kmin + 4; k++) {
    const int x = (pairs + k - 1) / k, y = CON_THREADS / x;
    if (x * y > best) { best = x * y; *tiles = k; *tx = x; *ty = y; }
  }
}

// the call's launch on stream st; the caller has checked the buffer.  0 < n <= 2^24.
inline int constellation_enqueue(dvbt_constellation *h, const float2 *rows, int n, hipStream_t st)
{
  ConArgs a;
  a.P = h->p.row_length; a.alpha = h->alpha; a.H = h->H; a.inv_d = h->inv_d; a.bin_scale = (float)(CON_GRID / (2 * h->span)); a.nrows = n;
  int tiles = 1;
  constellation_geometry(a.P, &tiles, &a.tx, &a.ty);
  // two workgroups share a CU (LDS); as many bands as fill the device once, none longer than CON_MAX_BAND rows or shorter than one pass of ty rows
  const int want = std::max(1, 2 * h->cus / tiles), least = (n + CON_MAX_BAND - 1) / CON_MAX_BAND, most = (n + a.ty - 1) / a.ty;
  const int bands = std::max(least, std::min(want, most));
  a.band = (n + bands - 1) / bands;
  const unsigned gy = (unsigned)((n + a.band - 1) / a.band);
  const bool vec = (a.P & 1) == 0 && ((uintptr_t)rows & 15) == 0;
  HIPCHK(h->ord.join(st));
  if (vec) hipLaunchKernelGGL(constellation_kernel<true>, dim3((unsigned)tiles, gy), dim3(CON_THREADS), con_lds(), st, rows, a, (unsigned long long *)h->acc);
  else hipLaunchKernelGGL(constellation_kernel<false>, dim3((unsigned)tiles, gy), dim3(CON_THREADS), con_lds(), st, rows, a, (unsigned long long *)h->acc);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(st));
  h->rows += n;
  return DVBT_OK;
}

// back to the state after create: the sums zeroed
inline int constellation_rewind(dvbt_constellation *h)
{
  HIPCHK(h->ord.drain());
  HIPCHK(hipMemsetAsync(h->acc, 0, sizeof(unsigned long long) * con_words(h->p.row_length), h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  h->rows = 0;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_constellation_create(const dvbt_constellation_params *p, dvbt_constellation **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = constellation_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_constellation> hold(new dvbt_constellation()); dvbt_constellation *const h = hold.get();   // released on every early return below
  h->p = *p;
  h->H = p->constellation == DVBT_QPSK ? 1 : p->constellation == DVBT_QAM16 ? 2 : 4;
  h->alpha = p->hierarchy == DVBT_ALPHA2 ? 2 : p->hierarchy == DVBT_ALPHA4 ? 4 : 1;
  static const int s_of[3][3] = {{2, 2, 2}, {10, 20, 52}, {42, 60, 108}};                                         // [constellation][alpha 1, 2, 4]
  h->inv_d = (float)std::sqrt((double)s_of[p->constellation][h->alpha == 1 ? 0 : h->alpha == 2 ? 1 : 2]);
  h->span = 2;
  while (h->span < h->alpha + 2 * h->H - 1) h->span *= 2;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, p->device));
  h->cus = std::max(1, prop.multiProcessorCount);
  if ((r = set_lds((const void *)constellation_kernel<true>, con_lds())) || (r = set_lds((const void *)constellation_kernel<false>, con_lds()))) return r;
  HIPCHK(h->ord.create());
  HIPCHK(h->acc.alloc(con_words(p->row_length)));
  if ((r = constellation_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_constellation_push_device(dvbt_constellation *h, const void *rows_dev, size_t nrows, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = constellation_check_call(h, rows_dev, nrows); if (r) return r;
  if (nrows == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return constellation_enqueue(h, (const float2 *)rows_dev, (int)nrows, (hipStream_t)stream);
}

extern "C" int dvbt_constellation_push(dvbt_constellation *h, const void *rows_host, size_t nrows)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = constellation_check_call(h, rows_host, nrows); if (r) return r;
  if (nrows == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->din, rows_host, nrows * (size_t)h->p.row_length * sizeof(float2), nullptr, 0, [&](const void *in, void *) {
    return constellation_enqueue(h, (const float2 *)in, (int)nrows, h->ord.s); });
}

extern "C" int dvbt_constellation_read(dvbt_constellation *h, dvbt_constellation_result *res, unsigned long long *hist, dvbt_constellation_point *points,
                                       size_t cap_points, dvbt_constellation_carrier *carriers, size_t cap_carriers)
{
  if (!h || !res) return fail(DVBT_ERR_INVALID, "null argument");
  const int P = h->p.row_length, L = 2 * h->H;
  if ((points && cap_points < (size_t)(L * L)) || (carriers && cap_carriers < (size_t)P))
    return fail(DVBT_ERR_CAPACITY, "points takes levels^2 entries, carriers row_length");
  HIPCHK(hipSetDevice(h->p.device));
  static_assert(sizeof(dvbt_constellation_point) == 6 * sizeof(long long) && sizeof(dvbt_constellation_carrier) == 3 * sizeof(long long), "the device's words");
  std::vector<unsigned long long> w(con_words(P));
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemcpyAsync(w.data(), h->acc, sizeof(unsigned long long) * w.size(), hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipStreamSynchronize(h->ord.s));
  memset(res, 0, sizeof *res);
  res->rows_pushed = h->rows; res->cells = h->rows * P;
  res->nonfinite = (long long)w[con_off_totals(P)]; res->clipped = (long long)w[con_off_totals(P) + 1];
  res->points = L * L; res->levels = L; res->alpha = h->alpha; res->span = h->span;
  if (hist) memcpy(hist, w.data(), sizeof(unsigned long long) * CON_GRID * CON_GRID);
  if (points) memcpy(points, w.data() + con_off_points(), sizeof(dvbt_constellation_point) * (size_t)(L * L));
  if (carriers) memcpy(carriers, w.data() + con_off_carriers(), sizeof(dvbt_constellation_carrier) * (size_t)P);
  return DVBT_OK;
}

extern "C" int dvbt_constellation_reset(dvbt_constellation *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return constellation_rewind(h);
}

extern "C" void dvbt_constellation_destroy(dvbt_constellation *h) { delete h; }
