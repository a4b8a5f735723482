// dvbt_ts.inc -- dvbt_ts_*: a transport-stream analyser -- the packets, flags and continuity of every PID and the timing of its PCRs, from a stream of
// 188-byte packets -- as one streaming handle (DESIGN.md 4i) over k_ts.hpp.  It consumes packets and changes nothing.  Included from dvbt_hip.hip.
//
// What a handle keeps from call to call: the number of packets it has seen and, on the device, one entry and one state per PID (TsPid, TsState) and three
// totals.  A call is worked off in batches of at most `batch` packets, three launches each (parse, tile, carry), through scratch sized once at create; the
// carry kernel is the only writer of the entries and the state, and the stream's order is the order of the launches.  dvbt_ts_read synchronises and copies
// on the handle's own stream, and changes nothing.

struct dvbt_ts {
  dvbt_ts_params p;
  int batch = 0;                                   // packets per parse / tile / carry: min(max_packets, TS_MAX_BATCH)
  DevMem<unsigned> rec, runs, rank, bitmap, tile_tot;
  DevMem<unsigned long long> pcr, totals;
  DevMem<TsPid> acc;
  DevMem<TsState> state;
  long long packets = 0;                           // since create / reset
  DevBuf din;                                      // staging of the host entry
  CallOrder ord;                                   // last: see CallOrder
};

namespace {

constexpr long long TS_MAX_STREAM = 1ll << 40;     // packets per stream
constexpr int TS_MAX_PACKETS = 1 << 24;            // dvbt_ts_params.max_packets
constexpr int TS_MAX_BATCH = 1 << 19;              // what the scratch is sized for at most: 120 bytes a packet where every packet is a run of its own

static_assert(sizeof(dvbt_ts_pid) == sizeof(TsPid) && sizeof(TsPid) == 23 * sizeof(long long), "the device's entry is the header's");
static_assert(DVBT_TS_TILE == TS_TILE && DVBT_TS_PIDS == TS_PIDS && DVBT_TS_PACKET == 188, "the header's constants");

inline int ts_check_params(const dvbt_ts_params *p)
{
  if (p->max_packets < 1 || p->max_packets > TS_MAX_PACKETS) return fail(DVBT_ERR_INVALID, "max_packets must be in 1..2^24");
  if (p->device < 0) return fail(DVBT_ERR_INVALID, "no such device");
  return DVBT_OK;
}

inline int ts_check_call(const dvbt_ts *h, const void *packets, size_t npackets)
{
  if (npackets == 0) return DVBT_OK;
  if (!packets) return fail(DVBT_ERR_INVALID, "null buffer");
  if (npackets > (size_t)TS_MAX_STREAM || h->packets + (long long)npackets > TS_MAX_STREAM) return fail(DVBT_ERR_CAPACITY, "a stream takes at most 2^40 packets");
  return DVBT_OK;
}

// the call's launches on stream st; the caller has checked the buffer.  n > 0.
inline int ts_enqueue(dvbt_ts *h, const unsigned char *packets, size_t n, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  for (size_t off = 0; off < n; off += (size_t)h->batch) {
    const int m = (int)std::min((size_t)h->batch, n - off), ntiles = (m + TS_TILE - 1) / TS_TILE;
    hipLaunchKernelGGL(ts_parse_kernel, dim3((unsigned)((m + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, packets + off * 188, m,
                       (unsigned *)h->rec, (unsigned long long *)h->pcr);
    hipLaunchKernelGGL(ts_tile_kernel, dim3((unsigned)ntiles), dim3(TS_TILE), 0, st, (const unsigned *)h->rec, (const unsigned long long *)h->pcr, m,
                       (unsigned *)h->runs, (unsigned *)h->rank, (unsigned *)h->bitmap, (unsigned *)h->tile_tot);
    hipLaunchKernelGGL(ts_carry_kernel, dim3((unsigned)((TS_PIDS + 1 + TS_CARRY_PIDS - 1) / TS_CARRY_PIDS)), dim3(TS_THREADS), 0, st, (const unsigned *)h->runs,
                       (const unsigned *)h->rank, (const unsigned *)h->bitmap, (const unsigned *)h->tile_tot, ntiles, h->packets + (long long)off,
                       (TsPid *)h->acc, (TsState *)h->state, (unsigned long long *)h->totals);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(h->ord.mark(st));
  h->packets += (long long)n;
  return DVBT_OK;
}

// back to the state after create
inline int ts_rewind(dvbt_ts *h)
{
  HIPCHK(h->ord.drain());
  hipLaunchKernelGGL(ts_init_kernel, dim3((unsigned)(TS_PIDS / TS_THREADS)), dim3(TS_THREADS), 0, h->ord.s, (TsPid *)h->acc, (TsState *)h->state,
                     (unsigned long long *)h->totals);
  HIPCHK(hipGetLastError());
  HIPCHK(h->ord.mark(h->ord.s));
  h->packets = 0;
  return DVBT_OK;
}

}  // namespace

extern "C" int dvbt_ts_create(const dvbt_ts_params *p, dvbt_ts **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = ts_check_params(p); if (r) return r;
  if ((r = need_device()) || (r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_ts> hold(new dvbt_ts()); dvbt_ts *const h = hold.get();   // released on every early return below
  h->p = *p;
  h->batch = std::min(p->max_packets, TS_MAX_BATCH);
  const size_t tiles = (size_t)(h->batch + TS_TILE - 1) / TS_TILE;
  HIPCHK(h->ord.create());
  HIPCHK(h->rec.alloc(tiles * TS_TILE));
  HIPCHK(h->pcr.alloc(tiles * TS_TILE));
  HIPCHK(h->runs.alloc(tiles * TS_TILE * TS_RUN_WORDS));
  HIPCHK(h->rank.alloc(tiles * TS_BITMAP_WORDS));
  HIPCHK(h->bitmap.alloc(tiles * TS_BITMAP_WORDS));
  HIPCHK(h->tile_tot.alloc(tiles * TS_TOTALS));
  HIPCHK(h->totals.alloc(TS_TOTALS));
  HIPCHK(h->acc.alloc(TS_PIDS));
  HIPCHK(h->state.alloc(TS_PIDS));
  if ((r = ts_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int dvbt_ts_push_device(dvbt_ts *h, const void *packets_dev, size_t npackets, void *stream)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = ts_check_call(h, packets_dev, npackets); if (r) return r;
  if (npackets == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return ts_enqueue(h, (const unsigned char *)packets_dev, npackets, (hipStream_t)stream);
}

extern "C" int dvbt_ts_push(dvbt_ts *h, const void *packets_host, size_t npackets)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  int r = ts_check_call(h, packets_host, npackets); if (r) return r;
  if (npackets == 0) return DVBT_OK;
  HIPCHK(hipSetDevice(h->p.device));
  return staged_call(h->ord, h->din, h->din, packets_host, npackets * 188, nullptr, 0, [&](const void *in, void *) {
    return ts_enqueue(h, (const unsigned char *)in, npackets, h->ord.s); });
}

extern "C" int dvbt_ts_read(dvbt_ts *h, dvbt_ts_result *res, dvbt_ts_pid *pids, size_t cap, size_t *n_pids)
{
  if (!h || !res) return fail(DVBT_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->p.device));
  std::vector<dvbt_ts_pid> all(TS_PIDS);
  unsigned long long tot[TS_TOTALS];
  HIPCHK(h->ord.join(h->ord.s));
  HIPCHK(hipMemcpyAsync(all.data(), h->acc, sizeof(dvbt_ts_pid) * TS_PIDS, hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipMemcpyAsync(tot, h->totals, sizeof tot, hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipStreamSynchronize(h->ord.s));
  size_t seen = 0;
  long long tei = 0;
  for (const dvbt_ts_pid &e : all) if (e.packets + e.tei > 0) { seen++; tei += e.tei; }
  if (pids && cap < seen) return fail(DVBT_ERR_CAPACITY, "pids takes one entry per PID seen (at most 8192)");
  memset(res, 0, sizeof *res);
  res->packets_pushed = h->packets; res->sync_errors = (long long)tot[TS_TOT_SYNC]; res->transport_errors = tei;
  res->afc_reserved = (long long)tot[TS_TOT_AFC0]; res->af_length_errors = (long long)tot[TS_TOT_AFLEN]; res->pids_seen = (long long)seen;
  if (pids) { size_t k = 0; for (const dvbt_ts_pid &e : all) if (e.packets + e.tei > 0) pids[k++] = e; }
  if (n_pids) *n_pids = seen;
  return DVBT_OK;
}

extern "C" int dvbt_ts_reset(dvbt_ts *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return ts_rewind(h);
}

extern "C" void dvbt_ts_destroy(dvbt_ts *h) { delete h; }
