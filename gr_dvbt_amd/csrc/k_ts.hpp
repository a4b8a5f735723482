// k_ts.hpp -- the transport-stream analyser's kernels (dvbt_ts.inc): PIDs, continuity and PCR timing of a stream of 188-byte packets.  include/dvbt_hip.h has
// the specification, step by step; tests/tsref.py is the same text in Python.
//
// The counts per PID are order-free; the continuity rule and the PCR pairs relate a packet to the previous packet of the same PID, wherever that one was.
// Three launches per batch of a call:
//   ts_parse_kernel   a thread per packet reads the header and, behind an adaptation field, bytes 4 .. 11 -- aligned dwords and a funnel shift, whatever the
//                     packet's byte alignment -- and writes one 32-bit record (TS_REC_*) and, where there is one, the 64-bit PCR.  Everything behind it
//                     works on these 4 .. 12 bytes per packet.
//   ts_tile_kernel    a workgroup per TS_TILE records sorts the keys `class << 10 | local index` (class = the PID of a member, 8192 + PID of a packet with the
//                     transport error flag, above both for a packet without sync or beyond the end) with a bitonic network: each thread keeps one key, the
//                     exchanges below 64 are lane shuffles, the ten above go through LDS.  Every class then forms a contiguous run in stream order, and the
//                     relations to the previous member (j), the one before (k) and the previous PCR are neighbour lookups and one max-scan.  A segmented scan
//                     (TsPart: fourteen 16-bit counts in seven words, two sums, a minimum and two maxima, all of which fit 32 bits inside a tile) leaves a
//                     run's partial sums at its last element, which writes the run (TS_RUN_*).  What needs a packet of an earlier tile stays open: the
//                     continuity verdict of the run's first two members and the pair in front of its first PCR.  The runs of a tile are dense and ascending
//                     by class; a bitmap of 16384 bits says which classes a tile holds, and a rank per bitmap word where its first run lies.
//   ts_carry_kernel   a wavefront per PID takes the batch's tiles 64 at a time, a lane each: it tests the bitmap, finds its run by its rank (the runs in front
//                     of the bitmap word's first, plus the bits below its own), resolves what the tile left open -- from the nearest lower lane that holds
//                     a run of the PID, or from the state the handle keeps per PID (TsState) -- and the lanes' sums are added by shuffles.  Lane 0 is the ONLY
//                     writer of its PID's entry and state: there is no atomic on any accumulator, and the same state carries the stream across chunks,
//                     batches and calls.  One more wavefront adds the tiles' three order-free totals.
// Nothing depends on where a tile, a batch or a call starts: every quantity is an exact integer and every relation is resolved by the same two functions
// (ts_verdict, ts_pcr_pair) whether both packets lie in one run or not.
#pragma once

namespace dvbt {

constexpr int TS_TILE = 1024;                      // DVBT_TS_TILE: packets per workgroup tile = threads of ts_tile_kernel
constexpr int TS_TILE_LOG2 = 10;
constexpr int TS_WAVES = TS_TILE / 64;
constexpr int TS_PIDS = 8192;
constexpr int TS_CLASSES = 2 * TS_PIDS;            // members' PIDs, then the PIDs of packets with the transport error flag
constexpr int TS_BITMAP_WORDS = TS_CLASSES / 32;   // per tile
constexpr int TS_THREADS = 256;                    // ts_parse_kernel, ts_carry_kernel, ts_init_kernel
constexpr long long TS_PCR_MOD = (1ll << 33) * 300;
constexpr long long TS_PCR_100MS = 2700000, TS_PCR_40MS = 1080000;

// a packet's record
constexpr unsigned TS_REC_MEMBER = 1u << 0;
constexpr int TS_REC_PID_SHIFT = 1;                // 13 bits
constexpr int TS_REC_CC_SHIFT = 14;                // 4 bits
constexpr unsigned TS_REC_PAY = 1u << 18, TS_REC_DI = 1u << 19, TS_REC_PCR = 1u << 20, TS_REC_NOSYNC = 1u << 21, TS_REC_TEI = 1u << 22, TS_REC_PUSI = 1u << 23,
                   TS_REC_SCR = 1u << 24, TS_REC_AF = 1u << 25, TS_REC_RAI = 1u << 26, TS_REC_AFC0 = 1u << 27, TS_REC_AFLEN = 1u << 28;
// the state of a PID's sequence: the last member's record (its cc and pay are read) and
constexpr unsigned TS_ST_SAME = 1u << 29, TS_ST_VALID = 1u << 30;
constexpr unsigned TS_ST_KEEP = (15u << TS_REC_CC_SHIFT) | TS_REC_PAY;

// a run, in 32-bit words
enum {
  TS_RUN_CLASS = 0 /* for whoever reads a dump: the carry finds a run by rank */, TS_RUN_N, TS_RUN_REC0, TS_RUN_REC1, TS_RUN_IDX0, TS_RUN_IDX_LAST, TS_RUN_LAST_STATE /* cc and pay of the last member; same, for a run of two or more */,
  TS_RUN_W0 /* 7 words of counts */, TS_RUN_SUM_DT = TS_RUN_W0 + 7, TS_RUN_SUM_DP, TS_RUN_MIN_DT, TS_RUN_MAX_DT, TS_RUN_MAX_DP,
  TS_RUN_HAS_PCR, TS_RUN_PCR0_IDX /* bit 31: its discontinuity indicator */, TS_RUN_PCR1_IDX, TS_RUN_PCR0 /* 2 words */, TS_RUN_PCR1 = TS_RUN_PCR0 + 2 /* 2 words */,
  TS_RUN_WORDS = TS_RUN_PCR1 + 2
};
static_assert(TS_RUN_WORDS % 2 == 0 && TS_RUN_PCR0 % 2 == 0, "the 64-bit PCRs of a run are 8-byte aligned");

// what the handle keeps per PID besides its entry
struct TsState { unsigned st, pcr_valid; unsigned long long pcr; long long pcr_index; };

// the handle's entry per PID: dvbt_ts_pid of include/dvbt_hip.h, word for word
struct TsPid {
  long long pid, packets, pusi, scrambled, payload, adaptation, discontinuity, random_access, pcr, tei, duplicates, cc_errors, first, last,
            pcr_pairs, pcr_discontinuity_signalled, pcr_over_100ms, pcr_over_40ms, sum_dt, sum_dp, min_dt, max_dt, max_dp;
};

enum { TS_TOT_SYNC = 0, TS_TOT_AFC0, TS_TOT_AFLEN, TS_TOTALS };

// ------------------------------------------------------------------ the two relations
__device__ __forceinline__ unsigned ts_cc(unsigned r) { return (r >> TS_REC_CC_SHIFT) & 15u; }
__device__ __forceinline__ unsigned ts_pid_of(unsigned r) { return (r >> TS_REC_PID_SHIFT) & 8191u; }

// same(i) of step 7, j the member in front of i (rj: its record or a state word)
__device__ __forceinline__ bool ts_same(unsigned ri, unsigned rj)
{
  return (ri & TS_REC_PAY) && (rj & TS_REC_PAY) && ts_cc(ri) == ts_cc(rj) && !(ri & TS_REC_DI);
}

// step 7 for a member i that has a j: 0 nothing or in order, 1 a duplicate, 2 a continuity error
__device__ __forceinline__ int ts_verdict(unsigned ri, unsigned rj, bool same_j)
{
  if (ts_pid_of(ri) == 8191u || (ri & TS_REC_DI)) return 0;
  if (ts_cc(ri) == ((ts_cc(rj) + ((ri & TS_REC_PAY) ? 1u : 0u)) & 15u)) return 0;
  return ts_same(ri, rj) && !same_j ? 1 : 2;
}

// step 8 for a pair (a, b): 0 signalled, 1 over 100 ms, 2 a pair, 3 a pair over 40 ms; dt where it is a pair
__device__ __forceinline__ int ts_pcr_pair(unsigned long long pcr_a, unsigned long long pcr_b, bool di_b, long long *dt)
{
  if (di_b) return 0;
  long long d = (long long)pcr_b - (long long)pcr_a;              // |d| < 2 M
  if (d < 0) d += TS_PCR_MOD;
  if (d < 0) d += TS_PCR_MOD;
  if (d >= TS_PCR_MOD) d -= TS_PCR_MOD;
  *dt = d;
  return d > TS_PCR_100MS ? 1 : d > TS_PCR_40MS ? 3 : 2;
}

// ------------------------------------------------------------------ parse
__device__ __forceinline__ unsigned ts_funnel(unsigned lo, unsigned hi, unsigned shift_bits)
{
  return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> shift_bits);
}

__global__ __launch_bounds__(TS_THREADS) void ts_parse_kernel(const unsigned char *__restrict__ packets, int n, unsigned *__restrict__ rec,
                                                              unsigned long long *__restrict__ pcr)
{
  const int i = (int)blockIdx.x * TS_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const uintptr_t a = (uintptr_t)packets + (size_t)i * 188u;
  const unsigned *q = reinterpret_cast<const unsigned *>(a & ~(uintptr_t)3);     // q[0] holds b0; q[1 .. 3] end at or before b15: all inside the packet
  const unsigned sh = (unsigned)(a & 3u) * 8u;
  const unsigned d0 = q[0], d1 = q[1];
  const unsigned w0 = ts_funnel(d0, d1, sh);
  const unsigned b0 = w0 & 255u, b1 = (w0 >> 8) & 255u, b2 = (w0 >> 16) & 255u, b3 = w0 >> 24;
  const unsigned pid = ((b1 & 0x1fu) << 8) | b2;
  unsigned r;
  if (b0 != 0x47u) r = TS_REC_NOSYNC;
  else if (b1 >> 7) r = TS_REC_TEI | (pid << TS_REC_PID_SHIFT);
  else {
    const unsigned afc = (b3 >> 4) & 3u, pay = afc & 1u, af = afc >> 1;
    r = TS_REC_MEMBER | (pid << TS_REC_PID_SHIFT) | ((b3 & 15u) << TS_REC_CC_SHIFT);
    if (pay) r |= TS_REC_PAY;
    if ((b1 >> 6) & 1u) r |= TS_REC_PUSI;
    if (b3 >> 6) r |= TS_REC_SCR;
    if (afc == 0u) r |= TS_REC_AFC0;
    if (af) {
      r |= TS_REC_AF;
      const unsigned d2 = q[2], d3 = q[3];
      const unsigned w1 = ts_funnel(d1, d2, sh), w2 = ts_funnel(d2, d3, sh);      // b4 .. b7, b8 .. b11
      const unsigned afl = w1 & 255u, b5 = (w1 >> 8) & 255u;
      if (afl > 183u - pay) r |= TS_REC_AFLEN;
      else if (afl >= 1u) {
        if (b5 >> 7) r |= TS_REC_DI;
        if ((b5 >> 6) & 1u) r |= TS_REC_RAI;
        if ((b5 >> 4) & 1u) {
          if (afl < 7u) r |= TS_REC_AFLEN;
          else {
            const unsigned long long b6 = (w1 >> 16) & 255u, b7 = w1 >> 24, b8 = w2 & 255u, b9 = (w2 >> 8) & 255u, b10 = (w2 >> 16) & 255u, b11 = w2 >> 24;
            const unsigned long long base = (b6 << 25) | (b7 << 17) | (b8 << 9) | (b9 << 1) | (b10 >> 7);
            r |= TS_REC_PCR;
            pcr[i] = 300ull * base + (((b10 & 1u) << 8) | b11);
          }
        }
      }
    }
  }
  rec[i] = r;
}

// ------------------------------------------------------------------ tile
struct TsPart { unsigned w[7], sum_dt, sum_dp, min_dt, max_dt, max_dp; };
constexpr int TS_PART_WORDS = 12;

// a: the earlier elements
__device__ __forceinline__ TsPart ts_combine(const TsPart &a, const TsPart &b)
{
  TsPart o;
#pragma unroll
  for (int i = 0; i < 7; i++) o.w[i] = a.w[i] + b.w[i];
  o.sum_dt = a.sum_dt + b.sum_dt; o.sum_dp = a.sum_dp + b.sum_dp;
  o.min_dt = min(a.min_dt, b.min_dt); o.max_dt = max(a.max_dt, b.max_dt); o.max_dp = max(a.max_dp, b.max_dp);
  return o;
}

__device__ __forceinline__ TsPart ts_shfl_up(const TsPart &v, int d)
{
  TsPart o;
#pragma unroll
  for (int i = 0; i < 7; i++) o.w[i] = __shfl_up(v.w[i], d);
  o.sum_dt = __shfl_up(v.sum_dt, d); o.sum_dp = __shfl_up(v.sum_dp, d);
  o.min_dt = __shfl_up(v.min_dt, d); o.max_dt = __shfl_up(v.max_dt, d); o.max_dp = __shfl_up(v.max_dp, d);
  return o;
}

// inclusive scans over the workgroup's TS_TILE threads; s16: TS_WAVES ints of LDS, free again on return
__device__ __forceinline__ int ts_scan_max(int v, int *s16, int tid)
{
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v = max(v, o); }
  if (lane == 63) s16[w] = v;
  __syncthreads();
  int p = -1;
  for (int i = 0; i < w; i++) p = max(p, s16[i]);
  __syncthreads();
  return max(v, p);
}

__device__ __forceinline__ int ts_scan_count(bool flag, int *s16, int tid, int *total)
{
  const int lane = tid & 63, w = tid >> 6;
  const unsigned long long m = __ballot(flag);
  const int v = __popcll(m & (~0ull >> (63 - lane)));
  if (lane == 63) s16[w] = __popcll(m);
  __syncthreads();
  int p = 0, t = 0;
  for (int i = 0; i < TS_WAVES; i++) { const int c = s16[i]; if (i < w) p += c; t += c; }
  __syncthreads();
  *total = t;
  return v + p;
}

// tile blockIdx.x of a batch of n records: its runs at runs + tile TS_TILE TS_RUN_WORDS, the classes present in bitmap + tile TS_BITMAP_WORDS, the number of
// runs in front of a bitmap word's first in rank + tile TS_BITMAP_WORDS (written where the word has a bit), the order-free totals in tile_tot + tile TS_TOTALS
__global__ __launch_bounds__(TS_TILE) void ts_tile_kernel(const unsigned *__restrict__ rec, const unsigned long long *__restrict__ pcr, int n,
                                                          unsigned *__restrict__ runs, unsigned *__restrict__ rank, unsigned *__restrict__ bitmap,
                                                          unsigned *__restrict__ tile_tot)
{
  __shared__ unsigned s_rec[TS_TILE];              // by local index
  __shared__ unsigned s_key[TS_TILE];              // the sort's exchange, then the sorted keys
  __shared__ unsigned long long s_pcr[TS_TILE];    // by sorted position
  __shared__ unsigned s_bitmap[TS_BITMAP_WORDS];
  __shared__ int s_scan[TS_WAVES];
  __shared__ unsigned s_cnt[TS_WAVES][TS_TOTALS];
  __shared__ unsigned s_tail[TS_WAVES][TS_PART_WORDS];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t tile = blockIdx.x, g = tile * TS_TILE + (size_t)tid;
  const bool inside = g < (size_t)n;

  unsigned key;
  {
    const unsigned r = inside ? rec[g] : 0u;
    s_rec[tid] = r;
    if (tid < TS_BITMAP_WORDS) s_bitmap[tid] = 0u;
    const unsigned cls = !inside ? 0x3fffffu : (r & TS_REC_NOSYNC) ? (unsigned)TS_CLASSES : ts_pid_of(r) + ((r & TS_REC_TEI) ? (unsigned)TS_PIDS : 0u);
    key = (cls << TS_TILE_LOG2) | (unsigned)tid;
    const unsigned long long m0 = __ballot((r & TS_REC_NOSYNC) != 0u), m1 = __ballot((r & TS_REC_AFC0) != 0u), m2 = __ballot((r & TS_REC_AFLEN) != 0u);
    if (lane == 0) { s_cnt[wave][TS_TOT_SYNC] = (unsigned)__popcll(m0); s_cnt[wave][TS_TOT_AFC0] = (unsigned)__popcll(m1); s_cnt[wave][TS_TOT_AFLEN] = (unsigned)__popcll(m2); }
  }
  __syncthreads();
  if (tid < TS_TOTALS) {
    unsigned t = 0u;
    for (int i = 0; i < TS_WAVES; i++) t += s_cnt[i][tid];
    tile_tot[tile * TS_TOTALS + tid] = t;
  }

  // the bitonic network: thread tid keeps element tid
  for (int k = 2; k <= TS_TILE; k <<= 1) {
    for (int j = k >> 1; j >= 1; j >>= 1) {
      unsigned other;
      if (j >= 64) {
        s_key[tid] = key;
        __syncthreads();
        other = s_key[tid ^ j];
        __syncthreads();
      } else other = (unsigned)__shfl_xor((int)key, j);
      const bool keep_min = ((tid & j) == 0) == ((tid & k) == 0);
      key = keep_min ? min(key, other) : max(key, other);
    }
  }
  s_key[tid] = key;
  __syncthreads();

  const unsigned cls = key >> TS_TILE_LOG2, li = key & (TS_TILE - 1);
  const bool live = cls < (unsigned)TS_CLASSES, member = cls < (unsigned)TS_PIDS;
  const unsigned key_prev = tid >= 1 ? s_key[tid - 1] : 0u, key_next = tid + 1 < TS_TILE ? s_key[tid + 1] : 0u;
  const bool head = live && (tid == 0 || (key_prev >> TS_TILE_LOG2) != cls);
  const bool tail = live && (tid == TS_TILE - 1 || (key_next >> TS_TILE_LOG2) != cls);
  const unsigned r = live ? s_rec[li] : 0u;
  const unsigned r_prev = tid >= 1 ? s_rec[key_prev & (TS_TILE - 1)] : 0u;                   // of sorted position tid - 1, whatever its run
  const bool prev_member = tid >= 1 && (key_prev >> TS_TILE_LOG2) < (unsigned)TS_PIDS;
  const bool has_pcr = member && (r & TS_REC_PCR);
  if (has_pcr) s_pcr[tid] = pcr[tile * TS_TILE + li];
  if (head) atomicOr(&s_bitmap[cls >> 5], 1u << (cls & 31u));                                // once per run

  const int run_start = ts_scan_max(head ? tid : -1, s_scan, tid);                           // (meaningful where live: the live elements come first)
  int n_runs;
  const int run_index = ts_scan_count(head, s_scan, tid, &n_runs) - 1;
  const int pcr_before = ts_scan_max(prev_member && (r_prev & TS_REC_PCR) ? tid - 1 : -1, s_scan, tid);   // the last position in front of tid with a PCR
  const int pcr_last = has_pcr ? tid : pcr_before;
  if (head && (tid == 0 || (key_prev >> (TS_TILE_LOG2 + 5)) != (cls >> 5))) rank[tile * TS_BITMAP_WORDS + (cls >> 5)] = (unsigned)run_index;   // the word's first run
  const int rr = tid - run_start;                                                            // position in the run
  // (the scans' barriers stand between the writes of s_pcr, s_bitmap and their reads below)

  TsPart v;
#pragma unroll
  for (int i = 0; i < 7; i++) v.w[i] = 0u;
  v.sum_dt = 0u; v.sum_dp = 0u; v.min_dt = 0xffffffffu; v.max_dt = 0u; v.max_dp = 0u;
  bool same_i = false;
  unsigned *const run = runs + (tile * TS_TILE + (size_t)(live ? run_index : 0)) * TS_RUN_WORDS;
  if (live) v.w[0] = 1u;
  if (member) {
    v.w[0] |= (r & TS_REC_PUSI) ? 1u << 16 : 0u;
    v.w[1] = ((r & TS_REC_SCR) ? 1u : 0u) | ((r & TS_REC_PAY) ? 1u << 16 : 0u);
    v.w[2] = ((r & TS_REC_AF) ? 1u : 0u) | ((r & TS_REC_DI) ? 1u << 16 : 0u);
    v.w[3] = ((r & TS_REC_RAI) ? 1u : 0u) | (has_pcr ? 1u << 16 : 0u);
    if (rr >= 1) same_i = ts_same(r, r_prev);
    if (rr >= 2) {
      const unsigned r_k = s_rec[s_key[tid - 2] & (TS_TILE - 1)];
      const int c = ts_verdict(r, r_prev, ts_same(r_prev, r_k));
      v.w[4] = c == 1 ? 1u : c == 2 ? 1u << 16 : 0u;
    }
    if (has_pcr) {
      if (pcr_before >= run_start) {
        long long dt = 0;
        const int c = ts_pcr_pair(s_pcr[pcr_before], s_pcr[tid], (r & TS_REC_DI) != 0u, &dt);
        if (c == 0) v.w[5] = 1u << 16;
        else if (c == 1) v.w[6] = 1u;
        else {
          const unsigned dp = li - (s_key[pcr_before] & (TS_TILE - 1));
          v.w[5] = 1u;
          if (c == 3) v.w[6] = 1u << 16;
          v.sum_dt = (unsigned)dt; v.min_dt = (unsigned)dt; v.max_dt = (unsigned)dt; v.sum_dp = dp; v.max_dp = dp;
        }
      } else {                                                                               // the run's first PCR: its pair is the carry's
        run[TS_RUN_PCR0_IDX] = li | ((r & TS_REC_DI) ? 1u << 31 : 0u);
        *reinterpret_cast<unsigned long long *>(run + TS_RUN_PCR0) = s_pcr[tid];
      }
    }
  }

  // the segmented scan: inside a wavefront by shuffles, across wavefronts through their last lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const TsPart o = ts_shfl_up(v, d);
    if (lane >= d && tid - d >= run_start) v = ts_combine(o, v);
  }
  if (lane == 63) {
#pragma unroll
    for (int i = 0; i < 7; i++) s_tail[wave][i] = v.w[i];
    s_tail[wave][7] = v.sum_dt; s_tail[wave][8] = v.sum_dp; s_tail[wave][9] = v.min_dt; s_tail[wave][10] = v.max_dt; s_tail[wave][11] = v.max_dp;
  }
  __syncthreads();
  if (tail) {
    for (int q = wave - 1; q >= 0 && q >= (run_start >> 6); --q) {                           // the run's part in wavefront q ends at its last lane
      TsPart o;
#pragma unroll
      for (int i = 0; i < 7; i++) o.w[i] = s_tail[q][i];
      o.sum_dt = s_tail[q][7]; o.sum_dp = s_tail[q][8]; o.min_dt = s_tail[q][9]; o.max_dt = s_tail[q][10]; o.max_dp = s_tail[q][11];
      v = ts_combine(o, v);
    }
    const unsigned key0 = s_key[run_start];
    run[TS_RUN_CLASS] = cls;
    run[TS_RUN_N] = (unsigned)(rr + 1);
    run[TS_RUN_REC0] = s_rec[key0 & (TS_TILE - 1)];
    run[TS_RUN_REC1] = rr >= 1 ? s_rec[s_key[run_start + 1] & (TS_TILE - 1)] : 0u;
    run[TS_RUN_IDX0] = key0 & (TS_TILE - 1);
    run[TS_RUN_IDX_LAST] = li;
    run[TS_RUN_LAST_STATE] = (r & TS_ST_KEEP) | (same_i ? TS_ST_SAME : 0u) | TS_ST_VALID;
#pragma unroll
    for (int i = 0; i < 7; i++) run[TS_RUN_W0 + i] = v.w[i];
    run[TS_RUN_SUM_DT] = v.sum_dt; run[TS_RUN_SUM_DP] = v.sum_dp; run[TS_RUN_MIN_DT] = v.min_dt; run[TS_RUN_MAX_DT] = v.max_dt; run[TS_RUN_MAX_DP] = v.max_dp;
    const bool run_pcr = member && pcr_last >= run_start;
    run[TS_RUN_HAS_PCR] = run_pcr ? 1u : 0u;
    if (run_pcr) {
      run[TS_RUN_PCR1_IDX] = s_key[pcr_last] & (TS_TILE - 1);
      *reinterpret_cast<unsigned long long *>(run + TS_RUN_PCR1) = s_pcr[pcr_last];
    }
  }
  if (tid < TS_BITMAP_WORDS) bitmap[tile * TS_BITMAP_WORDS + tid] = s_bitmap[tid];
}

// ------------------------------------------------------------------ carry
// the run of class `cls` in tile t, present by the bitmap word `word`: its rank among the tile's runs
__device__ __forceinline__ const unsigned *ts_run_of(const unsigned *__restrict__ runs, const unsigned *__restrict__ rank, size_t t, unsigned cls, unsigned word)
{
  const unsigned slot = rank[t * TS_BITMAP_WORDS + (cls >> 5)] + (unsigned)__popc(word & ((1u << (cls & 31u)) - 1u));
  return runs + (t * TS_TILE + slot) * TS_RUN_WORDS;
}

// what a lane gathers of its PID over its tiles: order-free once the edges are resolved
struct TsLane {
  unsigned long long packets, pusi, scrambled, payload, adaptation, discontinuity, random_access, pcr, tei, duplicates, cc_errors, pcr_pairs,
                     pcr_discontinuity_signalled, pcr_over_100ms, pcr_over_40ms, sum_dt, sum_dp;
  unsigned long long min_dt, first;                // ~0: unset
  unsigned long long max_dt, max_dp;
  long long last;                                  // -1: unset
};

// one member of a run's head against the state in front of it
__device__ __forceinline__ void ts_carry_member(unsigned ri, unsigned &st, TsLane &a)
{
  const bool valid = (st & TS_ST_VALID) != 0u, same_i = valid && ts_same(ri, st);
  if (valid) {
    const int c = ts_verdict(ri, st, (st & TS_ST_SAME) != 0u);
    if (c == 1) a.duplicates += 1; else if (c == 2) a.cc_errors += 1;
  }
  st = (ri & TS_ST_KEEP) | (same_i ? TS_ST_SAME : 0u) | TS_ST_VALID;
}

__device__ __forceinline__ unsigned long long ts_wave_sum(unsigned long long v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ unsigned long long ts_wave_min(unsigned long long v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned long long ts_wave_max(unsigned long long v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}

constexpr int TS_CARRY_PIDS = TS_THREADS / 64;     // wavefronts, one PID each, per workgroup

// A wavefront per PID p < TS_PIDS (and one more for the totals), `base` the stream index of the batch's first packet.  The wavefront takes the batch's tiles
// 64 at a time, lane l the tile c0 + l.  What a run needs of the stream in front of it is little: for the verdicts of its first two members the state
// (cc, pay, same) behind the PID's previous run, and `same` behind a run of ONE member needs (cc, pay) of the run before that and nothing older; for the pair
// in front of its first PCR the previous run with a PCR.  So a lane fetches both from the nearest lower lane that holds one (two shuffles for the state, in
// turn, and one for the PCR), the lowest lanes from the state the wavefront carries from chunk to chunk, and everything else is sums, minima and maxima
// over the lanes.  Lane 0 is the only writer of the PID's entry and state.
__global__ __launch_bounds__(TS_THREADS) void ts_carry_kernel(const unsigned *__restrict__ runs, const unsigned *__restrict__ rank,
                                                              const unsigned *__restrict__ bitmap, const unsigned *__restrict__ tile_tot, int ntiles,
                                                              long long base, TsPid *__restrict__ acc, TsState *__restrict__ state,
                                                              unsigned long long *__restrict__ totals)
{
  const int lane = (int)threadIdx.x & 63;
  const int p = (int)blockIdx.x * TS_CARRY_PIDS + ((int)threadIdx.x >> 6);
  if (p > TS_PIDS) return;
  if (p == TS_PIDS) {
    unsigned long long t[TS_TOTALS] = {0ull, 0ull, 0ull};
    for (int i = lane; i < ntiles; i += 64)
      for (int k = 0; k < TS_TOTALS; k++) t[k] += tile_tot[(size_t)i * TS_TOTALS + k];
    for (int k = 0; k < TS_TOTALS; k++) {
      const unsigned long long sum = ts_wave_sum(t[k]);
      if (lane == 0 && sum) totals[k] += sum;
    }
    return;
  }
  const unsigned cls_tei = (unsigned)(TS_PIDS + p);
  const unsigned long long lower = (1ull << lane) - 1ull;
  TsState s = state[p];                            // the same in every lane
  TsLane a = {};
  a.min_dt = ~0ull; a.first = ~0ull; a.last = -1;
  bool touched = false;                            // the same in every lane
  for (int c0 = 0; c0 < ntiles; c0 += 64) {
    const int t = c0 + lane;
    const bool in = t < ntiles;
    const unsigned wm = in ? bitmap[(size_t)t * TS_BITMAP_WORDS + (p >> 5)] : 0u, wt = in ? bitmap[(size_t)t * TS_BITMAP_WORDS + (cls_tei >> 5)] : 0u;
    const bool hm = (wm >> (p & 31)) & 1u, ht = (wt >> (cls_tei & 31u)) & 1u;
    if (ht) a.tei += ts_run_of(runs, rank, (size_t)t, cls_tei, wt)[TS_RUN_N];
    const unsigned long long mask = __ballot(hm);
    if (!mask) continue;
    touched = true;
    const long long tile_base = base + (long long)t * TS_TILE;
    unsigned nrun = 0u, rec0 = 0u, rec1 = 0u, last = 0u, has_pcr = 0u, di0 = 0u;
    unsigned long long pcr0 = 0ull, pcr1 = 0ull;
    long long index0 = 0, index1 = 0;
    if (hm) {
      const unsigned *run = ts_run_of(runs, rank, (size_t)t, (unsigned)p, wm);
      nrun = run[TS_RUN_N]; rec0 = run[TS_RUN_REC0]; rec1 = run[TS_RUN_REC1]; last = run[TS_RUN_LAST_STATE]; has_pcr = run[TS_RUN_HAS_PCR];
      const unsigned long long first = (unsigned long long)(tile_base + run[TS_RUN_IDX0]);
      a.first = first < a.first ? first : a.first;
      a.last = tile_base + run[TS_RUN_IDX_LAST];                                             // (a lane's tiles ascend)
      const unsigned w0 = run[TS_RUN_W0], w1 = run[TS_RUN_W0 + 1], w2 = run[TS_RUN_W0 + 2], w3 = run[TS_RUN_W0 + 3], w4 = run[TS_RUN_W0 + 4],
                     w5 = run[TS_RUN_W0 + 5], w6 = run[TS_RUN_W0 + 6];
      a.packets += w0 & 0xffffu; a.pusi += w0 >> 16; a.scrambled += w1 & 0xffffu; a.payload += w1 >> 16; a.adaptation += w2 & 0xffffu;
      a.discontinuity += w2 >> 16; a.random_access += w3 & 0xffffu; a.pcr += w3 >> 16; a.duplicates += w4 & 0xffffu; a.cc_errors += w4 >> 16;
      a.pcr_pairs += w5 & 0xffffu; a.pcr_discontinuity_signalled += w5 >> 16; a.pcr_over_100ms += w6 & 0xffffu; a.pcr_over_40ms += w6 >> 16;
      a.sum_dt += run[TS_RUN_SUM_DT]; a.sum_dp += run[TS_RUN_SUM_DP];
      if (run[TS_RUN_MIN_DT] != 0xffffffffu && run[TS_RUN_MIN_DT] < a.min_dt) a.min_dt = run[TS_RUN_MIN_DT];
      if (run[TS_RUN_MAX_DT] > a.max_dt) a.max_dt = run[TS_RUN_MAX_DT];
      if (run[TS_RUN_MAX_DP] > a.max_dp) a.max_dp = run[TS_RUN_MAX_DP];
      if (has_pcr) {
        const unsigned i0 = run[TS_RUN_PCR0_IDX];
        di0 = i0 >> 31;
        index0 = tile_base + (long long)(i0 & 0x7fffffffu); index1 = tile_base + (long long)run[TS_RUN_PCR1_IDX];
        pcr0 = *reinterpret_cast<const unsigned long long *>(run + TS_RUN_PCR0); pcr1 = *reinterpret_cast<const unsigned long long *>(run + TS_RUN_PCR1);
      }
    }
    // the state in front of my run: the nearest lower lane's, or the carried one
    const unsigned long long below = mask & lower;
    const int from = below ? 63 - __clzll((long long)below) : -1;
    const unsigned front_rec = (unsigned)__shfl((int)last, from < 0 ? 0 : from);             // its cc and pay are final; its `same` only for a run of two or more
    if (hm && nrun == 1u) {
      const unsigned front = from >= 0 ? front_rec : s.st;
      last = (rec0 & TS_ST_KEEP) | ((front & TS_ST_VALID) && ts_same(rec0, front) ? TS_ST_SAME : 0u) | TS_ST_VALID;
    }
    const unsigned front_st = (unsigned)__shfl((int)last, from < 0 ? 0 : from);              // now final in every lane
    if (hm) {
      unsigned st = from >= 0 ? front_st : s.st;
      ts_carry_member(rec0, st, a);
      if (nrun >= 2u) ts_carry_member(rec1, st, a);
    }
    // the PCR in front of my run's first
    const unsigned long long pmask = __ballot(hm && has_pcr), pbelow = pmask & lower;
    const int pfrom = pbelow ? 63 - __clzll((long long)pbelow) : -1;
    const unsigned long long pcr_in = __shfl(pcr1, pfrom < 0 ? 0 : pfrom);
    const long long index_in = __shfl(index1, pfrom < 0 ? 0 : pfrom);
    if (hm && has_pcr && (pfrom >= 0 || s.pcr_valid)) {
      long long dt = 0;
      const int c = ts_pcr_pair(pfrom >= 0 ? pcr_in : s.pcr, pcr0, di0 != 0u, &dt);
      if (c == 0) a.pcr_discontinuity_signalled += 1;
      else if (c == 1) a.pcr_over_100ms += 1;
      else {
        const unsigned long long dp = (unsigned long long)(index0 - (pfrom >= 0 ? index_in : s.pcr_index)), udt = (unsigned long long)dt;
        a.pcr_pairs += 1; a.sum_dt += udt; a.sum_dp += dp;
        if (c == 3) a.pcr_over_40ms += 1;
        a.min_dt = udt < a.min_dt ? udt : a.min_dt; a.max_dt = udt > a.max_dt ? udt : a.max_dt; a.max_dp = dp > a.max_dp ? dp : a.max_dp;
      }
    }
    // what the next chunk finds in front of it
    s.st = (unsigned)__shfl((int)last, 63 - __clzll((long long)mask));
    if (pmask) {
      const int top = 63 - __clzll((long long)pmask);
      s.pcr_valid = 1u; s.pcr = __shfl(pcr1, top); s.pcr_index = __shfl(index1, top);
    }
  }
  const unsigned long long tei = ts_wave_sum(a.tei);
  if (!touched && !tei) return;
  TsLane r;
  r.packets = ts_wave_sum(a.packets); r.pusi = ts_wave_sum(a.pusi); r.scrambled = ts_wave_sum(a.scrambled); r.payload = ts_wave_sum(a.payload);
  r.adaptation = ts_wave_sum(a.adaptation); r.discontinuity = ts_wave_sum(a.discontinuity); r.random_access = ts_wave_sum(a.random_access);
  r.pcr = ts_wave_sum(a.pcr); r.duplicates = ts_wave_sum(a.duplicates); r.cc_errors = ts_wave_sum(a.cc_errors); r.pcr_pairs = ts_wave_sum(a.pcr_pairs);
  r.pcr_discontinuity_signalled = ts_wave_sum(a.pcr_discontinuity_signalled); r.pcr_over_100ms = ts_wave_sum(a.pcr_over_100ms);
  r.pcr_over_40ms = ts_wave_sum(a.pcr_over_40ms); r.sum_dt = ts_wave_sum(a.sum_dt); r.sum_dp = ts_wave_sum(a.sum_dp);
  r.min_dt = ts_wave_min(a.min_dt); r.first = ts_wave_min(a.first); r.max_dt = ts_wave_max(a.max_dt); r.max_dp = ts_wave_max(a.max_dp);
  r.last = (long long)ts_wave_max((unsigned long long)(a.last + 1)) - 1;
  if (lane != 0) return;
  TsPid e = acc[p];
  e.packets += (long long)r.packets; e.pusi += (long long)r.pusi; e.scrambled += (long long)r.scrambled; e.payload += (long long)r.payload;
  e.adaptation += (long long)r.adaptation; e.discontinuity += (long long)r.discontinuity; e.random_access += (long long)r.random_access;
  e.pcr += (long long)r.pcr; e.tei += (long long)tei; e.duplicates += (long long)r.duplicates; e.cc_errors += (long long)r.cc_errors;
  e.pcr_pairs += (long long)r.pcr_pairs; e.pcr_discontinuity_signalled += (long long)r.pcr_discontinuity_signalled;
  e.pcr_over_100ms += (long long)r.pcr_over_100ms; e.pcr_over_40ms += (long long)r.pcr_over_40ms; e.sum_dt += (long long)r.sum_dt; e.sum_dp += (long long)r.sum_dp;
  if (r.first != ~0ull && e.first < 0) e.first = (long long)r.first;
  if (r.last >= 0) e.last = r.last;
  if (r.min_dt != ~0ull && (e.min_dt < 0 || (long long)r.min_dt < e.min_dt)) e.min_dt = (long long)r.min_dt;
  if ((long long)r.max_dt > e.max_dt) e.max_dt = (long long)r.max_dt;
  if ((long long)r.max_dp > e.max_dp) e.max_dp = (long long)r.max_dp;
  acc[p] = e;
  if (touched) state[p] = s;
}

// the state after create
__global__ __launch_bounds__(TS_THREADS) void ts_init_kernel(TsPid *__restrict__ acc, TsState *__restrict__ state, unsigned long long *__restrict__ totals)
{
  const int p = (int)blockIdx.x * TS_THREADS + (int)threadIdx.x;
  if (p < TS_TOTALS) totals[p] = 0ull;
  if (p >= TS_PIDS) return;
  TsPid a = {};
  a.pid = p; a.first = -1; a.min_dt = -1;
  acc[p] = a;
  TsState s = {0u, 0u, 0ull, 0ll};
  state[p] = s;
}

}  // namespace dvbt
