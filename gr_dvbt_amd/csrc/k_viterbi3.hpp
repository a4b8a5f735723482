// k_viterbi3.hpp -- A7 (viterbi_decoder): depuncture + K=7 Viterbi + traceback, the dominant kernel of the chain.
// Add-compare-select butterflies on DPP lane exchanges (no LDS crossbar, no ds_bpermute in the inner loop), TWO cells
// per VGPR on packed 16-bit arithmetic (v_pk_add_i16 / v_pk_sub_i16 / v_pk_max_i16).
//
// Mapping: one wavefront decodes FOUR chunks, a chunk owns one DPP row (16 lanes); every lane holds 4 of the 64 path
// metrics as the four 16-bit halves of two VGPRs.  The trellis is updated IN PLACE: the butterfly (i, i+32) -> (2i, 2i+1)
// is computed by the two cells that hold states i and i+32, each keeping one output, so after a step the cell that held
// state s holds state rotl6(s): cell c holds state rotl6(c, u mod 6) at relative step u.  The two cells of a butterfly
// differ in exactly one bit of the cell index, which walks 5,4,3,2,1,0,5,... with the step.  Cell index
//     c = r(VGPR 0/1) : h(half 0/1) : a3 a2 a1 a0,   physical lane-in-row = (a0 + 2*a1) ^ (7*a2) ^ (8*a3)
// so the six exchanges are: VGPR swap (free), half swap (one v_alignbit), and four DPP controls (row_ror:8,
// row_half_mirror, quad_perm[2,3,0,1], quad_perm[1,0,3,2]).
//
// Branch metrics enter as delta = 2*(agreements - disagreements) of the butterfly's label with the received pair:
// X = M + delta (own), Y = M - delta (offered to the partner), new = max(X, Y_partner); this is the reference's m0..m3
// (d_viterbi.c:503-506) up to an offset common to all 64 states, which the renormalisation removes anyway.
//
// A 16-bit cell = (2M + bias) << 8 | path byte.
//  * metric field (8 bits, signed): M in units of half an agreement, bias = 1 when the cell holds an upper state
//    (i+32): compares are strict and reproduce the reference's tie rule (d_viterbi.c:508-521).  For a K=7 code
//    the spread of the 64 metrics is bounded by 6 steps x the per-step range: 2M+bias spans <= 49, whenever the offset
//    was last removed.  The best field never decreases: of the best state's two outgoing branches (complementary
//    labels) one has delta >= 0; and it rises by at most 4 per step (|delta| <= 4).  Every V3_RENORM_EVERY = 6 windows
//    the best field is set back to T = V3_RENORM_BEST = -72 (the reference subtracts the minimum at every output only
//    to keep ITS 8-bit metrics from wrapping, :728-732; any common offset changes no compare), so s steps later every
//    field lies in [T - 49, T + 1 + 4s] and the candidates X, Y of a step in [T - 53, T + 5 + 4s]: with s <= 48 that
//    is [-125, 125], inside int8 (the static_asserts at V3_RENORM_BEST; eight windows would need 310 values and do
//    not fit, so six is the longest cadence that divides V3_BLK).  A decoder starts with every field at T, as if
//    behind a renormalisation.  tests/test_viterbi_renorm_model.py runs the recurrence in exact integers.
//  * path byte (8 bits): the content of the reference's path byte of the survivor -- the state at the window start
//    (kept as that state's cell storage index, bits 5:0) and the two oldest inputs of the window (= top two bits of
//    the state after step 6, stamped there, bits 7:6).  It rides along with the metric through v_pk_max (metric
//    fields never tie).  In the LDS ring a hop is one v_bfi: origin = byte & 63, inserted under the next row's offset (v3_hop).
//  * the tie-break bits are armed THREE STEPS AT A TIME.  Whether a cell holds an upper state at a step depends on one bit of its
//    index, a different one at every step, and the two cells of a butterfly differ in exactly the bit of the current step.  So the
//    biases of the next three steps can be written together into bits 6, 7, 8 (the earliest step in the lowest bit; bits 7:6 of
//    the path byte are free until the stamp of the window's 6th step): at the first step the two candidates agree in bits 8 and 7
//    and differ in bit 6, whichever wins carries the right bits 8 and 7 into the next step, where bit 7 decides and the stale
//    bit 6 below it cannot; and so on.  The deltas have zeros in bits 8:0, so the adds leave the three bits alone.  A window of 8
//    steps re-arms after steps 3, 6 (with the stamp), 7 and 8 (with the origin of the next window): 4 v_and_or instead of 8.
// Per step (two VGPRs, four cells): ONE v_perm (the branch-metric deltas of all four cells out of one word of four class deltas: register 1 has register 0's deltas, their
// negatives, or -- phases 1 and 5, where a register's two cells share a class -- the other half of the permuted word, read through op_sel; v3_step), and per VGPR pk_add,
// pk_sub, the exchange (a v_mov_dpp at four of the six phases, free at the other two), pk_max, and on every second step a v_and_or: 9.33 instructions per step, 2.33 per cell
// (the second v_perm that phases 1 and 5 issued until round 11 made it 9.67).
//
// The instruction budget, as compiled (tools/vit_window_count.py on the device assembly; tests/test_viterbi_isa_budget.py holds it): a window is 77 VALU instructions for
// its eight steps, 1 for the path-byte word and 10.8 for its end (key and argmax 10, the renormalisation's 5 every sixth window; 12.5 = 90.5 in all while it ran every second) = 88.8, plus its address arithmetic; a traceback hop is 2 per chain (one row back, one v_bfi).  A block of
// V3_BLK windows of viterbi3_kernel<24, 72, 1> is straight-line code: windows 0-11 with the previous block's 2 x 23 hops, the start of its chains' output and the calls' bytes
// 97.6 per window (106.8 before the ring became one array of the workgroup; 95.7 while the calls' bytes were assembled behind the block), the other blocks of twelve 91.5 and
// 87.9 (94.0 as a loop of six), staging and the chains' start ~240 per block (~270 with the output before round 8): 2,458 instructions per block of 24 windows measured
// (SQ_INSTS_VALU; 2,472 in round 7, 2,727 before it).  Since rounds 9 and 10 (the shortcut below; the renormalisation every sixth window): the hop-free windows 0-11 86.3 per window, with
// hops 94.7, windows 12-23 90.2 (88.0 / 96.3 / 91.8 with the renormalisation every second window; tests/test_viterbi_isa_renorm.py holds them), 2,361 per block measured (2,400 in round 9).  Since round 11 (one v_perm per step at every phase: 74.7 for a window's eight steps instead of 77.3; the ring's row masked once per
// group of eight windows instead of once per window, v3_fwd_window): 83.7 / 92.0 / 85.8 (tests/test_viterbi_isa_perm.py), 2,275 per block measured.  Every stamp is one v_and_or_b32 (the lane constants are kept opaque, v3_init_lane).
// Since round 13 the work OUTSIDE the windows (staging, the chains' set-up, the decision: ~240 of the 2,275): staging's index chain walks two steps per link through the pair table
// (v3_init_lut: six ds_read_b64 for twelve ds_read_b32), the received bits are compacted with constant masks per constellation (v3_compact) and the block's 16-byte load needs no
// 64-bit compare inside the wave-uniform bounds l_first .. l_last (stage_load) -- the stretch between the loop header and the first window 471 -> 412 VALU as compiled, all paths
// counted (tests/test_viterbi_isa_outside.py), 2,216 per block measured (SQ_INSTS_VALU 1,726.6 M -> 1,681.5 M per launch), the windows as they were; LDS 80,896 B per workgroup.
// What the count alone did not buy, the order of the LDS reads did: a hop's read and its use stand three and five steps apart (v3_fwd_window), and a window's
// step words are loaded one window ahead (v3_fwd_six) -- the wavefront, one of two on its SIMD, no longer waits out the LDS latency 70 times per block.  The same holds around
// the windows since round 8: staging computes a lane's twelve table indices first, issues the twelve look-ups back to back behind one wait and stores the words as three
// ds_write_b128 (stage_words); the best states the chains start from are read at the top of the iteration and used behind staging (bests_read / trace_init); the chains' last
// path bytes are read together in the hop slot behind the last hop and the calls' bytes leave where that hop would be merged, under an exec mask without a branch
// (v3_trace_read / v3_trace_store): as compiled, two s_waitcnt lgkmcnt(0) between the loop header and the first window (the compacted bits, the first window's step words; the batch of look-ups
// is met by three partial waits, one per wide store) instead of fifteen, and none on the spot behind the last hop instead of two (tests/test_viterbi_isa_staging.py).
//
// The traceback's shortcut (round 9).  On a stream the code copes with all chains walk the same path: the chain started at window jj passes window jj - 1 at the state that window's
// own chain starts from (its best state), and its ntraceback - 1 hops re-derive what bests[] already holds.  With Z(w) = the storage index of window w's best state (trace_init's
// T.z, low six bits) and link(w) = ((tab[row(w)][Z(w)] & 63) == Z(w - 1)) -- one hop from w's best state lands on w - 1's -- a chain whose links hold for every w in
// [jj - (ntraceback - 2), jj] stands at Z(jj - (ntraceback - 1)) behind its hops, and the call's byte is what v3_trace_store makes of that window's path byte at its own best state:
// the very byte the walk reaches, so no decoded byte can change (tests/test_viterbi_shortcut_model.py).  The decision is taken once per iteration of the block loop, wave-uniform,
// in front of the windows: every link of the block whose chains start (24 windows x the wavefront's live decoders, one ballot) and every link of the block before it (the previous
// iteration's verdict) -- more than any chain needs, and enough for every ntraceback.  Z(jj - 1) is the neighbouring lane's Z(jj) (one DPP row shift); the first hop's reads ride
// on staging's waits (link_reads: behind the compacted bits' reads, met by the waits of the table look-ups; LDS returns in order); where the shortcut is taken the path bytes at the
// best states of the windows the chains end in are read and the calls' bytes leave under the chains' exec masks before the first window, and the iteration runs the hop-free
// windows.  Where a link fails the chains walk as before; where no chain of the wavefront ends in a call (warm-up, idle tails) nothing is walked at all.  The hop block it replaces is 12 x (94.7 - 86.3) = 100 instructions and
// 46 + 2 dependent LDS round trips.
// V3Aux.debug bit 1 (dvbt_rx_set_viterbi_walk) switches the shortcut off; the MODE 1 decoders count both kinds of iteration (ctl[V3_CTL_SHORT]).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <string.h>
#include "dvbt_tables.hpp"
#include "k_backend.hpp"

namespace dvbt {

// host side: the decoder's parameters for one configuration (viterbi_decoder_impl.cc:61-65,95-124,149-153)
inline VitParams make_vit_params(const Dims &d, int bsize, int chunk_bytes)
{
  VitParams v; memset(&v, 0, sizeof v);
  v.m = d.m; v.k = d.k; v.n = d.n; v.plen = d.plen; v.ntb = d.ntb; v.bsize = bsize;
  v.d_nsymbols = bsize * d.n / d.m; v.d_nbits = 2 * d.k * bsize;
  v.chunk_bytes = chunk_bytes > 0 ? chunk_bytes : 768; v.payload = d.payload; v.warm = 72;   // (= V3_WARM, declared below)
  memcpy(v.punct, d.punct, 16); memcpy(v.prefix, d.prefix, 16);
  v.punct_mask = 0; v.prefix_nib = 0;
  for (int i = 0; i < d.plen; i++) { v.punct_mask |= (unsigned)d.punct[i] << i; v.prefix_nib |= (unsigned long long)d.prefix[i] << (4 * i); }
  v.magic_plen = ~0ull / (unsigned)d.plen + 1; v.magic_m = ~0ull / (unsigned)d.m + 1; v.magic_n = ~0ull / (unsigned)d.n + 1;
  for (int i = 0; i < 64; i++) v.punct_rep |= (unsigned long long)d.punct[i % d.plen] << i;
  v.magic16_plen = (65536u + (unsigned)d.plen - 1) / (unsigned)d.plen;
  return v;
}

#define DPP_XOR1 0xB1              /* quad_perm [1,0,3,2] */
#define DPP_XOR2 0x4E              /* quad_perm [2,3,0,1] */
#define DPP_HALF_MIRROR 0x141      /* lane i <-> 7-i inside each half row: logical bit a2 */
#define DPP_ROR8 0x128             /* row_ror:8: lane i <-> i^8 */
#define DPP_MIRROR 0x140

__device__ __forceinline__ int rotl6(int c, int p) { return ((c << p) | (c >> (6 - p))) & 63; }

#ifndef V3_WGW_N
#define V3_WGW_N 4
#endif
constexpr int V3_WGW = V3_WGW_N;    // wavefronts per workgroup: independent (no barrier), each with its own slice of the LDS arrays.  Alone on the machine one-wave and
                                   // four-wave workgroups decode equally fast (3.63 / 3.70 ms); four waves make the workgroup 79 KB of LDS, the size of the symbol kernel's
                                   // (76 KB), so that with several segments in flight a retiring workgroup of either kernel makes room for one of the other and the two
                                   // kernels share the CUs instead of queueing: 4.42 against 4.53 ms per step (bench.py --pipeline 3)
#ifndef V3_EXP
#define V3_EXP 0                   // tools/vit_kbench.hip only, never the product library (cost attribution; the output is wrong for bits 1..8, 256):
                                   // 1 no traceback, 2 no window end, 4 no path-byte store, 8 stage once, 16 record every wavefront's SIMD and
                                   // lifetime, 32 alternate s_setprio window by window, 64 s_nop after every step, 128 s_sleep per window,
                                   // 256 step words from registers (no LDS read in the loop)
#endif
constexpr int V3_WARM = 72;        // warm-up windows before a chunk's first byte (the default; dvbt_rx_params.viterbi_warm_windows selects the WARM = 0 instantiation, which reads VitParams.warm)
constexpr int V3_WARM_MAX = 1152;  // the largest warm-up the parameter accepts
static_assert(V3_WARM == 72, "make_vit_params (above) presets VitParams.warm to the default");
constexpr int V3_BLK = 24;         // windows per forward block (a multiple of 3, the phase cycle, and of V3_RENORM_EVERY: every block ends right behind a renormalisation)
constexpr int V3_RENORM_EVERY = 6; // windows between two renormalisations: the last window of every group of six sets the best metric field back to V3_RENORM_BEST
constexpr int V3_RENORM_BEST = -72; // (even: bit 8 of a cell is the tie-break bit).  The range note in the header, as arithmetic:
static_assert(V3_BLK % V3_RENORM_EVERY == 0, "a block of windows ends right behind a renormalisation: equal states are equal registers at a block's top (proof, repair, carried state)");
static_assert(V3_RENORM_BEST % 2 == 0, "the renormalisation leaves bit 8 of the cells alone");
static_assert(V3_RENORM_BEST - 49 - 4 >= -128, "lowest candidate of a step: the best field never decreases, the spread is at most 49, |delta| <= 4");
static_assert(V3_RENORM_BEST + 1 + 4 * 8 * V3_RENORM_EVERY + 4 <= 127, "highest candidate of a step: the best field rises by at most 4 per step, 8 steps per window");
constexpr int V3_RINGW = 64;       // windows kept in the LDS ring (power of two, >= 2*V3_BLK - 12 + max ntraceback - 1: the traceback of a
                                   // block runs during the first 12 windows of the next one).  20 KB of LDS per wavefront = 2 wavefronts
                                   // per SIMD.  A 32-window ring with traceback groups of six windows (3 wavefronts per SIMD) was built and
                                   // measured in round 2: +14 % instructions for -7 % cycles per instruction, 4.33 ms against 4.03 ms
                                   // (tools/experiments/viterbi_w3_ring32.patch, profiles/r02_viterbi_attribution.json)
constexpr int V3_WAVES_PER_CU = 4 * 2; // wavefronts resident per CU (LDS: 2 per SIMD)
constexpr int V3_CBW = 17;         // words of compacted received bits per decoder and block (192 steps need <= 384 + 23 bits)

typedef short v3pk __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v3pk pk(int x) { return __builtin_bit_cast(v3pk, x); }
__device__ __forceinline__ int ipk(v3pk x) { return __builtin_bit_cast(int, x); }
__device__ __forceinline__ int pk_add(int a, int b) { return ipk(pk(a) + pk(b)); }
__device__ __forceinline__ int pk_sub(int a, int b) { return ipk(pk(a) - pk(b)); }
__device__ __forceinline__ int pk_max(int a, int b) { return ipk(__builtin_elementwise_max(pk(a), pk(b))); }
__device__ __forceinline__ int pk_min(int a, int b) { return ipk(__builtin_elementwise_min(pk(a), pk(b))); }
// DPP read with bound_ctrl: every control used here reads a valid lane, and with full row/bank masks the compiler
// then needs no "old" value (no extra v_mov before the v_mov_dpp)
template <int CTRL> __device__ __forceinline__ int dppb(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
// a constant the compiler must keep in a VGPR (v_and_or_b32 takes one literal at most)
__device__ __forceinline__ int vconst(int c) { int x; asm("v_mov_b32 %0, %1" : "=v"(x) : "s"(c)); return x; }
// max of a's halves with b's halves SWAPPED (the half exchange of phase 1 rides on the op_sel of the VOP3P encoding)
__device__ __forceinline__ int pk_max_swap(int a, int b) { int r; asm("v_pk_max_i16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b)); return r; }
// a's halves plus / minus ONE half of b, the same for both (HI: b's high half, else its low one): the phases 1 and 5 keep the deltas of the two registers in the two halves of
// one word (v3_step).  No clamp; not volatile, the scheduler moves them like the compiler's own packed adds
template <bool HI> __device__ __forceinline__ int pk_add_half(int a, int b)
{
  int r;
  if (HI) asm("v_pk_add_u16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
  else asm("v_pk_add_u16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <bool HI> __device__ __forceinline__ int pk_sub_half(int a, int b)
{
  int r;
  if (HI) asm("v_pk_sub_i16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
  else asm("v_pk_sub_i16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

struct V3Lane {
  unsigned sel[6];      // v_perm selectors out of the step word: [0, d(class of register 0's lo cell), 0, d(class of its hi cell)], register 1 lives on the same word (v3_step);
                        // at the phases 1 and 5, where a register's halves share their class: [0, d(class of register 0), 0, d(class of register 1)]
  int bias8[6][2];      // tie-break bit of phase P at bit 8 of both halves (1 = the cell holds an upper state at that phase)
  int kc[3][2];         // (63 - state of the two cells) | (the cell holds a LOWER state) << 8, at window ends (phase 0,2,4)
  int org[2];           // storage index of the two cells, at the path-byte position (bits 5:0)
  int arm_mid[3][2];    // window starting at phase 0,2,4: biases of its steps 3,4,5 at bits 6,7,8              (after the 3rd step)
  int arm_b2[3][2];     // top two bits of the cells' states after the 6th step at bits 7:6 | bias of step 6 at bit 8 (after the 6th step)
  int arm_org[3][2];    // NEXT window starting at phase 0,2,4: org | biases of its steps 0,1,2 at bits 6,7,8     (after the last step)
};

// storage index of a cell in the path-byte table: z = physical lane * 4 + 2r + h (a lane's four bytes are one word)
__device__ __forceinline__ int v3_phys(int a) { const int a2 = (a >> 2) & 1; return (a & 8) | (a2 << 2) | ((a & 3) ^ (a2 ? 3 : 0)); }
__device__ __forceinline__ int v3_log(int p) { const int q = p & 7, a2 = (q >> 2) & 1; return (p & 8) | (a2 << 2) | ((q ^ (a2 ? 7 : 0)) & 3); }
__device__ __forceinline__ int v3_cell_of_z(int z) { return ((z & 2) << 4) | ((z & 1) << 4) | v3_log(z >> 2); }
__device__ __forceinline__ int v3_z_of_cell(int c) { return v3_phys(c & 15) * 4 + ((c >> 5) & 1) * 2 + ((c >> 4) & 1); }

// 1 when cell (r, h, a) holds an upper state (state bit 5 set) at phase P: the state is rotl6(cell, P), its bit 5 is cell bit (5 - P)
__device__ __forceinline__ int v3_upper(int P, int r, int h, int a) { const int c = (r << 5) | (h << 4) | a; return (c >> (5 - P)) & 1; }
// label class of cell (r, h, a) at phase P = the byte of the step word its delta comes from
__device__ __forceinline__ unsigned v3_class(int P, int r, int h, int a)
{
  const int c = (r << 5) | (h << 4) | a, i = rotl6(c, P) & 31;
  const int c0 = ((i >> 2) ^ (i >> 1) ^ i) & 1;                       // parity(2i & 0x4f)
  const int c1 = ((i >> 4) ^ (i >> 2) ^ (i >> 1)) & 1;                // parity(2i & 0x6d)
  return (unsigned)(c0 | (c1 << 1));
}
__device__ inline void v3_init_lane(int pl, V3Lane &L)
{
  const int a = v3_log(pl);
  for (int P = 0; P < 6; P++) {
    // the two bytes of the selector: register 0's two halves -- or, at the phases 1 and 5, the two registers: cell bit 4 (the half) sits on state bit 5 resp. 3 there, which
    // neither parity reads, so a register's halves share their class, and register 1's is register 0's ^ 1 resp. ^ 2 (tests/test_viterbi_opsel_model.py)
    const bool regs = P == 1 || P == 5;
    L.sel[P] = 0x0c | (v3_class(P, 0, 0, a) << 8) | (0x0cu << 16) | ((regs ? v3_class(P, 1, 0, a) : v3_class(P, 0, 1, a)) << 24);
  }
  for (int r = 0; r < 2; r++) {
    for (int P = 0; P < 6; P++) L.bias8[P][r] = (v3_upper(P, r, 0, a) << 8) | (v3_upper(P, r, 1, a) << 24);
    L.org[r] = (pl * 4 + 2 * r) | ((pl * 4 + 2 * r + 1) << 16);     // bits 5:0 of the path byte
    for (int e = 0; e < 3; e++) {
      const int P0 = 2 * e;
      const int s0 = rotl6((r << 5) | a, P0), s1 = rotl6((r << 5) | 16 | a, P0);
      L.kc[e][r] = ((63 - s0) | ((63 - s1) << 16)) | (L.bias8[P0][r] ^ 0x01000100);
      const int b2 = ((s0 >> 4) << 6) | (((s1 >> 4) << 6) << 16);   // top two bits of the cells' states at phase P0, at bits 7:6 of the path byte
      // a window that starts at phase P0: step u runs at phase (P0 + u) % 6
      L.arm_mid[e][r] = (L.bias8[(P0 + 3) % 6][r] >> 2) | (L.bias8[(P0 + 4) % 6][r] >> 1) | L.bias8[(P0 + 5) % 6][r];
      L.arm_org[e][r] = L.org[r] | (L.bias8[P0][r] >> 2) | (L.bias8[P0 + 1][r] >> 1) | L.bias8[(P0 + 2) % 6][r];
      // after the 6th step of a window that started at phase P0 the phase is P0 again: the stamp and the bias of the 7th step
      L.arm_b2[e][r] = b2 | L.bias8[P0][r];
    }
  }
  // Some of these operands are the same in every lane (bias8[0], bias8[1] and what is built from them alone): left visible, the compiler folds them into literals and a
  // stamp becomes v_and_b32 + v_or_b32 with one literal each.  Kept opaque they stay in VGPRs and every stamp is one v_and_or_b32 (see vconst)
  for (int r = 0; r < 2; r++) {
    for (int P = 0; P < 6; P++) asm("" : "+v"(L.bias8[P][r]));
    for (int e = 0; e < 3; e++) { asm("" : "+v"(L.kc[e][r])); asm("" : "+v"(L.arm_mid[e][r])); asm("" : "+v"(L.arm_b2[e][r])); asm("" : "+v"(L.arm_org[e][r])); }
  }
}

// ST: what happens to the tie-break bits after the step (see the header): 0 nothing (the bits armed earlier serve the next step too);
// 3 = the window's 3rd step: the biases of steps 4..6 are armed; 1 = the 6th step: the two oldest inputs are stamped into the path byte
// together with the bias of the 7th; 4 = the 7th step: the bias of the 8th; 2 = the last step: raw[] keeps the survivors' path bytes for the
// table, v gets the origin stamp of the next window and the biases of its first three steps in the same v_and_or
template <int P, int ST> __device__ __forceinline__ void v3_step(int (&v)[2], unsigned W, const V3Lane &L, int (&raw)[2])
{
  int X[2], Y[2], mx[2];
  // The label class of a cell depends on bits 0,1,2,4 of its state (parity taps 0x4f, 0x6d without the MSB).  The
  // VGPR index is cell bit 5 = state bit (5+P)%6: at phases 0 and 4 (state bits 5, 3) both VGPRs have the same
  // deltas, at phases 2 and 3 (state bits 1, 2: both parities flip) VGPR 1 has the negated ones.  At phases 1 and 5 (state bits 0, 4: one parity flips) VGPR 1 has
  // another class, but there the two cells of a VGPR share theirs (the half, cell bit 4, is state bit 5 resp. 3): the one permute delivers [0, d(VGPR 0), 0, d(VGPR 1)]
  // and each VGPR's add and subtract read their half of it for both cells (op_sel) -- one v_perm per step at every phase.
  const int D0 = (int)__builtin_amdgcn_perm(0u, W, L.sel[P]);
  if (P == 1 || P == 5) {
    X[0] = pk_add_half<false>(v[0], D0); Y[0] = pk_sub_half<false>(v[0], D0);
    X[1] = pk_add_half<true>(v[1], D0); Y[1] = pk_sub_half<true>(v[1], D0);
  } else {
    X[0] = pk_add(v[0], D0); Y[0] = pk_sub(v[0], D0);
    if (P == 0 || P == 4) { X[1] = pk_add(v[1], D0); Y[1] = pk_sub(v[1], D0); }
    else { X[1] = pk_sub(v[1], D0); Y[1] = pk_add(v[1], D0); }
  }
  if (P == 0) { mx[0] = pk_max(X[0], Y[1]); mx[1] = pk_max(X[1], Y[0]); }
  else if (P == 1) { mx[0] = pk_max_swap(X[0], Y[0]); mx[1] = pk_max_swap(X[1], Y[1]); }
  else {
#pragma unroll
    for (int r = 0; r < 2; r++)
      mx[r] = pk_max(X[r], P == 2 ? dppb<DPP_ROR8>(Y[r]) : P == 3 ? dppb<DPP_HALF_MIRROR>(Y[r]) : P == 4 ? dppb<DPP_XOR2>(Y[r]) : dppb<DPP_XOR1>(Y[r]));
  }
  constexpr int PN = (P + 1) % 6;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (ST == 0) v[r] = mx[r];
    else if (ST == 3) v[r] = (mx[r] & (int)0xfe3ffe3f) | L.arm_mid[((PN + 3) % 6) / 2][r];       // the window started at phase PN - 3
    else if (ST == 1) v[r] = (mx[r] & (int)0xfe3ffe3f) | L.arm_b2[PN / 2][r];                    // PN = the phase the window started at
    else if (ST == 4) v[r] = (mx[r] & (int)0xfefffeff) | L.bias8[PN][r];
    else { raw[r] = mx[r]; v[r] = (mx[r] & (int)0xfe00fe00) | L.arm_org[PN / 2][r]; }
  }
}

// (the 8 steps of a window that starts at phase P0 = 0, 2, 4 are written out in v3_fwd_window; v arrives with the origin stamp in its path bytes)
#if V3_EXP & 64
#define V3_YIELD() asm volatile("s_nop 3" ::: "memory")
#else
#define V3_YIELD()
#endif

// halves of a packed register as sign-extended 32-bit values
__device__ __forceinline__ int lo16(int x) { return (x << 16) >> 16; }
__device__ __forceinline__ int hi16(int x) { return x >> 16; }
template <int CTRL> __device__ __forceinline__ int max_dpp(int v) { return max(v, dppb<CTRL>(v)); }   // folds into v_max_i32_dpp
template <int CTRL> __device__ __forceinline__ int min_dpp(int v) { return min(v, dppb<CTRL>(v)); }

// end of a window: best state = first index of the maximum metric (d_viterbi.c:699-711) and, when asked, the
// renormalisation.  PE = phase after the window.  Key of a cell = (2M + bias ^ 1) << 8 | 63 - state: among equal M the
// cells holding a lower state win over the upper ones, then the smaller state (the flag sits in L.kc); one v_and_or per VGPR.
// Returns the key's low byte (63 - best state in bits 5:0) in every lane of the row.
template <int PE, bool RENORM> __device__ __forceinline__ int v3_window_end(int (&v)[2], const V3Lane &L)
{
  const int kp = pk_max((v[0] & (int)0xfe00fe00) | L.kc[PE / 2][0], (v[1] & (int)0xfe00fe00) | L.kc[PE / 2][1]);
  int k = max(lo16(kp), hi16(kp));
  k = max_dpp<DPP_XOR1>(k); k = max_dpp<DPP_XOR2>(k); k = max_dpp<DPP_HALF_MIRROR>(k); k = max_dpp<DPP_MIRROR>(k);
  if (RENORM) {
    // any offset common to the 64 metrics will do (the reference subtracts the minimum, d_viterbi.c:728-732, only to keep
    // its 8-bit metrics from wrapping): the maximum is already here, so the best metric is set to V3_RENORM_BEST -- the
    // spread is at most 49, so the field restarts inside [BEST - 49, BEST + 1], and until the next renormalisation,
    // 8 * V3_RENORM_EVERY steps on, only its upper end moves: by at most 4 per step (the range note in the header)
    const unsigned sub = (unsigned)((k & ~0x1ff) - V3_RENORM_BEST * 256);   // (2 M_best - BEST) at the metric position; bias and path byte untouched
    const int mn = (int)__builtin_amdgcn_perm(sub, sub, 0x01000100u);
    v[0] = pk_sub(v[0], mn); v[1] = pk_sub(v[1], mn);
  }
  return k;
}

// Two traceback chains per lane: the calls (windows) pl and 16+pl of one block of a decoder.
// The ring of path bytes is ONE array of the workgroup, [window][wavefront][decoder][cell z]: a window's row is V3_ROW<NW> = NW * 256 bytes, the wavefront and the decoder sit
// in bits 9:6 of the byte offset, below the window and above the cell.  A chain's offset into it is then a bit field of one register, and a hop needs no base address.
template <int NW> constexpr int V3_ROW = NW * 4 * 64;                              // bytes per window of the ring
template <int NW> constexpr int V3_RMASK = (V3_RINGW * V3_ROW<NW> - 1) & ~63;      // window | wavefront | decoder in a byte offset (NW = 4: 0xffc0, the ring is 64 KB)
struct V3Trace {
  int z[2];             // current cell: byte offset into the ring = window row | wavefront | decoder | storage index
  int wsh[2];           // ring row of the window whose table is read next (x V3_ROW; counts down past zero: only the bits of V3_RMASK are used) | wavefront << 8 | decoder << 6
  int osh[2];           // (6 - phase at the start of the window a chain ends in) mod 6: the rotation of v3_trace_store, a constant of the lane
  unsigned long long ok[2];   // the lanes of the wavefront whose chain q ends in a call of the chunk (v3_trace_store's exec mask)
  int oend[2];          // the chunk's end for the calls this chain takes (no call: INT_MIN)
  int ob[2];            // output byte of the call, relative to the chunk's first byte
};
// one hop of both chains: state = path_byte >> 2 in the reference's layout (d_viterbi.c:717) = the low six bits here.
// Two VALU instructions per chain: one row back, and the v_bfi that takes window, wavefront and decoder from wsh and the origin (bits 5:0) from the path byte -- the ring's wrap
// is the mask.  (Written as asm: from the C expression the compiler re-derives the row from the chain's start and masks both sides, four instructions.)
// The two halves of a hop are separate so that the forward pass can put add-compare-select steps between the read and the use of the path byte.
__device__ __forceinline__ void v3_hop_read(const V3Trace &T, const unsigned char *tab, unsigned (&t)[2])
{
#pragma unroll
  for (int q = 0; q < 2; q++) t[q] = tab[T.z[q]];                    // z is the whole offset into the ring
}
template <int NW> __device__ __forceinline__ void v3_hop_merge(V3Trace &T, const unsigned (&t)[2])
{
#pragma unroll
  for (int q = 0; q < 2; q++) {
    T.wsh[q] -= V3_ROW<NW>;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(T.z[q]) : "s"(V3_RMASK<NW>), "v"(T.wsh[q]), "v"(t[q]));
  }
}
template <int NW> __device__ __forceinline__ void v3_hop(V3Trace &T, const unsigned char *tab) { unsigned t[2]; v3_hop_read(T, tab, t); v3_hop_merge<NW>(T, t); }
// the decoded byte of a call: (state at the start of the last window of the chain) << 2 | its two oldest inputs.  The read of the chain's last path byte and its use are separate
// (v3_hop_read / v3_hop_merge likewise): the forward pass issues both chains' reads together behind the last hop and assembles the bytes a window or more later.
__device__ __forceinline__ void v3_trace_read(const V3Trace &T, const unsigned char *tab, unsigned (&t)[2])
{
#pragma unroll
  for (int q = 0; q < 2; q++) t[q] = tab[T.z[q]];
}
// outb = where the chunk's first byte goes.  The cell of storage index z is rotr6(z ^ 12 * (bit 4 of z), 2) (v3_cell_of_z) and the window starts at phase oph = (8w) % 6, so the
// state << 2 is the doubled six bits shifted by osh = (6 - oph) % 6 -- seven instructions per chain, none of them under the store's exec mask
template <bool MASKED> __device__ __forceinline__ void v3_trace_store(const V3Trace &T, const unsigned (&t)[2], uint8_t *outb)
{
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const unsigned zz = (t[q] ^ (((t[q] >> 4) & 1u) * 12u)) & 63u;
    unsigned by = (((zz | (zz << 6)) >> T.osh[q]) & 0xfcu) | (t[q] >> 6);
    if (MASKED) {
      // the store under the lanes' ok as exec mask, without a branch: around a conditional store the compiler keeps an s_cbranch_execz, and the twelve windows would no
      // longer be one basic block for the scheduler (and for tools/vit_window_count.py).  What this relies on: T.ok[q] is a ballot taken with all 64 lanes live, in wave-uniform
      // control flow (trace_init), and so is this place -- exec is all ones on entry and the group puts back what it found; the group is the only user of exec here (the compiler
      // sees one opaque instruction, nothing can be scheduled into it).  The compiler does not count the store in its vmcnt bookkeeping: an uncounted store in flight can only make
      // a later s_waitcnt vmcnt(N) wait longer, never shorter, and nothing reads the byte back.  The "memory" clobber keeps the store in source order against the kernel's other
      // memory operations; it is a scheduling barrier at the two places per block where a store stands (the end of window 11 for ntraceback 24).
      unsigned long long sv;
      asm volatile("s_and_saveexec_b64 %0, %1\n\tglobal_store_byte %2, %3, off\n\ts_mov_b64 exec, %0" : "=&s"(sv) : "s"(T.ok[q]), "v"(outb + T.ob[q]), "v"(by) : "memory", "scc");
    } else if ((T.ok[q] >> (threadIdx.x & 63)) & 1) outb[T.ob[q]] = (unsigned char)by;
  }
}
__device__ __forceinline__ void v3_trace_out(const V3Trace &T, const unsigned char *tab, uint8_t *outb) { unsigned t[2]; v3_trace_read(T, tab, t); v3_trace_store<false>(T, t, outb); }

// window jb + W0 + V6 of a decoder (jb: the block's first window, W0 = 0, 6, 12, 18 the group of six): it starts at phase (8 V6) % 6 = 0,2,4,0,2,4; the last window of the six
// (V6 == V3_RENORM_EVERY - 1) renormalises.  HOPS: two traceback hops of the previous block's calls ride along (their LDS latency
// hides under the add-compare-select work).
// Which hops exist is a compile-time fact (HOP0 + 2 V6 (+1) < NTB - 1 with NTB = ntraceback, a template parameter of the
// kernel): the window stays one straight-line block, with the dependent LDS reads spread over it (below).
__device__ __forceinline__ void v3_load_words(const unsigned *wp_, unsigned (&W)[8])
{
  const uint4 *wp = reinterpret_cast<const uint4 *>(wp_);
  const uint4 t0 = wp[0], t1 = wp[1];
  W[0] = t0.x; W[1] = t0.y; W[2] = t0.z; W[3] = t0.w; W[4] = t1.x; W[5] = t1.y; W[6] = t1.z; W[7] = t1.w;
}
// tabw = the ring at this lane's word of a row (wavefront, decoder, 4 x lane in row)
// W = the window's eight step words, already in registers; PREF: the next window's (they follow in wrow) are loaded into Wn at the start of this one, a window ahead of their use
// The read of the chains' last path byte takes the slot of the hop that would follow the last one (FINA / FINB), and the calls' bytes are assembled and written where that hop
// would be merged, three or five steps later (outb: v3_trace_store)
template <int V6, int W0, bool HOPS, int HOP0, int NTB, int NW, bool PREF> __device__ __forceinline__ void v3_fwd_window(int (&v)[2], const V3Lane &L, const unsigned *wrow, unsigned char *tab, unsigned char *tabw,
                                                                                           unsigned char *bests, int jb, int dd, int pl, V3Trace &T, unsigned (&W)[8], unsigned (&Wn)[8], uint8_t *outb)
{
  // a window's two hops are dependent LDS reads: the first is issued here and used behind the window's 3rd step, where the second is issued, which is used behind the last step
  // (the compiler keeps the source order: written as read + use in one place they end up 1 to 5 instructions apart, and the wavefront waits out the LDS latency 46 times a block)
  constexpr bool HOPA = HOPS && HOP0 + 2 * V6 < NTB - 1, HOPB = HOPS && HOP0 + 2 * V6 + 1 < NTB - 1;
  constexpr bool FINA = HOPS && HOP0 + 2 * V6 == NTB - 1, FINB = HOPS && HOP0 + 2 * V6 + 1 == NTB - 1;
  unsigned th[2], tout[2];
  if (HOPA) v3_hop_read(T, tab, th);
  if (FINA) v3_trace_read(T, tab, tout);
  // The window's row of the ring.  A block starts at a multiple of eight windows and the ring holds a multiple of eight, so the ring can wrap only between two groups of eight
  // windows of the block: one masked row per group, the window's place in its group a constant (an immediate offset of the ds_write).  Written as (jb + WB) & (V3_RINGW - 1) the
  // compiler masks every window behind the block's eighth on its own and pays two address instructions per window (the path-byte word's, the best state's)
  constexpr int WB = W0 + V6;
  static_assert(V3_BLK % 8 == 0 && V3_RINGW % 8 == 0, "jb % 8 == 0: the ring's wrap falls between two groups of eight windows");
  const int jr = ((jb + (WB & ~7)) & (V3_RINGW - 1)) + (WB & 7);
#if V3_EXP & 256
  for (int i = 0; i < 8; i++) { W[i] = (unsigned)((jb + W0) * 0x01010101 + i * 0x00020406 + pl); asm volatile("" : "+v"(W[i])); }   // no LDS read in the loop
#else
  if (PREF) v3_load_words(wrow + (V6 + 1) * 8, Wn);
#endif
  constexpr int P0 = (8 * V6) % 6;
  int raw[2];
#if V3_EXP & 32
  if (V6 & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);   // alternate the wavefront's issue priority window by window
#endif
#if V3_EXP & 128
  __builtin_amdgcn_s_sleep(1);
#endif
  v3_step<(P0 + 0) % 6, 0>(v, W[0], L, raw); V3_YIELD(); v3_step<(P0 + 1) % 6, 0>(v, W[1], L, raw); V3_YIELD(); v3_step<(P0 + 2) % 6, 3>(v, W[2], L, raw); V3_YIELD();
  if (HOPA) { v3_hop_merge<NW>(T, th); if (HOPB) v3_hop_read(T, tab, th); }
  if (FINB) v3_trace_read(T, tab, tout);
  if (FINA) v3_trace_store<true>(T, tout, outb);
  v3_step<(P0 + 3) % 6, 0>(v, W[3], L, raw); V3_YIELD(); v3_step<(P0 + 4) % 6, 0>(v, W[4], L, raw); V3_YIELD(); v3_step<(P0 + 5) % 6, 1>(v, W[5], L, raw); V3_YIELD();
  v3_step<(P0 + 6) % 6, 4>(v, W[6], L, raw); V3_YIELD(); v3_step<(P0 + 7) % 6, 2>(v, W[7], L, raw);
  if (HOPB) v3_hop_merge<NW>(T, th);
  if (FINB) v3_trace_store<true>(T, tout, outb);
  // the four path bytes of this lane's cells = one word of the table (storage index z = 4*lane + 2r + h)
  if (!(V3_EXP & 4)) *reinterpret_cast<unsigned *>(tabw + jr * V3_ROW<NW>) = __builtin_amdgcn_perm((unsigned)raw[1], (unsigned)raw[0], 0x06040200u);
  if (V3_EXP & 2) { if (raw[0] == 0x12345) bests[jr] = 1; return; }
  const int s = v3_window_end<(P0 + 2) % 6, V6 == V3_RENORM_EVERY - 1>(v, L);
  bests[dd * V3_RINGW + jr] = (unsigned char)s;                    // low byte of the key (63 - best state in bits 5:0); all 16 lanes of the row write the same byte
}
static_assert(V3_RENORM_EVERY == 6, "v3_fwd_six is the group of windows that ends in a renormalisation (V6 = 0..5)");
// six windows; Wa arrives with the first window's step words and leaves with those of the window behind the six (MORE: there is one in this block)
template <int W0, bool HOPS, int HOP0, int NTB, int NW, bool MORE> __device__ __forceinline__ void v3_fwd_six(int (&v)[2], const V3Lane &L, const unsigned *wrow, unsigned char *tab, unsigned char *tabw,
                                                                                  unsigned char *bests, int jb, int dd, int pl, V3Trace &T, unsigned (&Wa)[8], unsigned (&Wb)[8], uint8_t *outb)
{
  v3_fwd_window<0, W0, HOPS, HOP0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb); v3_fwd_window<1, W0, HOPS, HOP0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wb, Wa, outb);
  v3_fwd_window<2, W0, HOPS, HOP0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb); v3_fwd_window<3, W0, HOPS, HOP0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wb, Wa, outb);
  v3_fwd_window<4, W0, HOPS, HOP0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb); v3_fwd_window<5, W0, HOPS, HOP0, NTB, NW, MORE>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wb, Wa, outb);
}

// A chunk = vp.chunk_bytes decoded bytes; it is decoded by an independent decoder that starts `warm` windows early
// from equal metrics (all V3_RENORM_BEST) and runs ntraceback-1 windows past its end.  Per block of 24 windows:
//   staging   depuncture (viterbi_decoder_impl.cc:241-256) + delta packing for 192 steps x 4 decoders.  The row
//             loads the input bytes of its decoder (one 16-byte load per lane, issued one block ahead) and compacts
//             the m valid bits of every byte into a bit stream in LDS; every lane then owns 12 consecutive steps:
//             it places itself in the puncture period with small-integer arithmetic relative to the row's base (one
//             64-bit locate per row), takes the period's keep-mask for its 24 symbol positions and a 32-bit window
//             of the bit stream, and emits one word of four class deltas per step, two steps per look-up in the 256-entry pair table;
//   forward   24 windows of add-compare-select (v3_fwd_window), path bytes into the LDS ring;
//   traceback of the PREVIOUS block's 24 calls x 4 decoders (d_viterbi.c:714-724), lane = (decoder, call): its
//             dependent LDS reads are interleaved into the first 12 windows of the forward pass.
#if V3_EXP & 16
__device__ unsigned long long *v3_dbg;     // tools/vit_kbench.hip: (hw id, start, end in 100 MHz ticks) per wavefront
#endif

// ---- The chunk decoders ARE the reference's one streaming decoder (viterbi_decoder_impl.cc:192-324, d_viterbi.c:680-735), by construction: proof + repair.
// A decoder's whole state at the top of a block of windows is its two registers of cells: the block starts at phase 0 right behind a renormalisation (best metric field = V3_RENORM_BEST) and the
// low nine bits of a cell are a function of the lane and the phase alone (v3_step, ST == 2) -- two decoders over the same input whose registers are EQUAL there make identical
// decisions from there on.  With B a multiple of V3_BLK the decoder of chunk c stands at the top of a block when it reaches its chunk's first window (relative window warm) and
// so does its predecessor, B windows further into its own run: both store their registers (MODE 1).  Per chunk c three slots of 32 words:
//   own[c]   the state, at the chunk's first window, of the decoder whose bytes fill chunk c
//   pred[c]  the state there of the decoder whose bytes fill chunk c - 1
//   fix[c]   (repair) the state there of a repaired chunk c - 1 where it is not pred[c]
// Chunk 0 starts the stream (or is handed the streaming decoder's state: the single block carries it from call to call), so own[c] == pred[c] for every c >= 1 proves, by induction,
// that every byte is the streaming decoder's.  viterbi_check_kernel lists the chunks where the two differ (their survivors had not merged inside the warm-up: none in 83,000 on
// streams the code can cope with, one in a few hundred on a collapsed channel or the hierarchical modes' degenerate input); viterbi_repair_kernel decodes each of them again from
// pred[c] (MODE 2: no warm-up, one chunk, in parallel) and compares the state it reaches at the next chunk's first window with pred[c + 1] -- equal: the chain holds (whoever
// filled chunk c + 1 started from, or was checked against, that state).  Not equal (the repaired decoder and the unproven one have not merged over a whole chunk: never observed)
// the chunk behind is flagged and viterbi_repair_seq_kernel, one decoder, walks on from there in stream order until its state is the own[] of the chunk it arrives at.  The host
// reads no verdict: the launches are unconditional and return at once when there is nothing to do.
constexpr int V3_SLOT = 32;          // words per state slot (16 lanes x 2 registers)
constexpr int V3_CTL_CHUNKS = 0;     // ctl words: chunks of the launch
constexpr int V3_CTL_MISMATCH = 1;   //            chunks the first check could not prove (= decoded again)
constexpr int V3_CTL_CONFLICT = 2;   //            chunks left to the sequential pass
constexpr int V3_CTL_UNPROVEN = 3;   //            chunks that are not proven after the repair (the final check; -1: not run)
constexpr int V3_CTL_SEQ = 4;        //            chunks the sequential pass decoded
constexpr int V3_CTL_ACC = 8;        //            [8..10] chunks, mismatches, sequential decodes summed over the launches since the owner cleared them
constexpr int V3_CTL_SHORT = 12;     //            [12..15] two 64-bit counters, never cleared by a kernel: iterations (blocks of windows, per wavefront) of the MODE 1 decoders whose
                                     //            calls' bytes left by the shortcut, and iterations whose chains walked
constexpr int V3_CTL_HDR = 16;       // ... then the list of mismatching chunks (cap words), then the conflict flags (cap words)
struct V3Aux {
  int *snap;                         // 3 slots per chunk (own, pred, fix), cap + 2 chunks
  int *ctl;
  long long cap;                     // chunks the buffers hold
  long long grid0;                   // absolute index of chunk 0's first byte (the single block: where the carried state stands, <= the first byte of the call)
  const int *carry_in;               // the streaming decoder's state at grid0 (null: chunk 0 warms up like the others -- it starts the stream)
  int *carry_out; int carry_rel;     // the last chunk's decoder leaves its state carry_rel windows into its chunk (a multiple of V3_BLK; carry_out null: no)
  int debug;                         // test hook (dvbt_rx_params.viterbi_verify = 4): bit 0 = every repaired chunk flags the chunk behind it as if its decoder had not arrived in
                                     // pred[] (the flag / fix[] hand-over to the sequential pass is otherwise reached only by inputs nobody has seen);
                                     // bit 1 (V3_DEBUG_WALK, dvbt_rx_set_viterbi_walk) = every traceback chain walks all its hops, the shortcut over chained best states is never taken
};
constexpr int V3_DEBUG_WALK = 2;
__device__ __forceinline__ int *v3_own(const V3Aux &ax, long long c) { return ax.snap + (3 * c) * V3_SLOT; }
__device__ __forceinline__ int *v3_pred(const V3Aux &ax, long long c) { return ax.snap + (3 * c + 1) * V3_SLOT; }
__device__ __forceinline__ int *v3_fix(const V3Aux &ax, long long c) { return ax.snap + (3 * c + 2) * V3_SLOT; }
inline size_t v3_snap_words(long long cap) { return (size_t)(cap + 2) * 3 * V3_SLOT; }
inline size_t v3_ctl_words(long long cap) { return (size_t)V3_CTL_HDR + 2 * (size_t)(cap + 2); }

struct V3Lds { unsigned char *tab; unsigned *wbuf; unsigned char *bests; const uint2 *lut; int wv; };   // tab: the workgroup's ring; wbuf, bests: the wavefront's; wv: the wavefront
// the label-class deltas of a step as a function of e = (keep flags of its two symbols) << 2 | next two received bits: the step word
__device__ __forceinline__ unsigned v3_step_word(int e)
{
  // deltas of the four label classes, doubled (a step with one punctured symbol keeps the bias bit free):
  // class 0: u0+u1 | class 1 (c0=1): -u0+u1 | class 2 (c1=1): u0-u1 | class 3: -u0-u1, u = +1/-1 for a received 0/1, 0 if erased
  const int k0 = (e >> 2) & 1, k1 = (e >> 3) & 1, t1 = (e >> 1) & 1, t0 = e & 1;
  const int u0 = k0 ? 1 - 2 * t1 : 0, u1 = k1 ? 1 - 2 * (k0 ? t0 : t1) : 0;
  const unsigned d0 = (unsigned)(2 * (u0 + u1)) & 0xff, d1 = (unsigned)(2 * (-u0 + u1)) & 0xff;
  const unsigned d2 = (unsigned)(2 * (u0 - u1)) & 0xff, d3 = (unsigned)(2 * (-u0 - u1)) & 0xff;
  return d0 | (d1 << 8) | (d2 << 16) | (d3 << 24);
}
// The pair table: TWO steps per look-up.  Key = (keep flags of the two steps' four symbols) << 4 | next four received bits (the oldest on top); the entry holds the first
// step's word, and the second step's behind the bits the first one consumed (one per kept symbol).  256 entries of 8 bytes; every wavefront writes all of them, the same
// values, before its first use (a wavefront's LDS operations execute in order): staging's index chain is six links long instead of twelve, and a link costs what it did
// (tests/test_viterbi_pair_table_model.py restates the entry and the chain)
constexpr int V3_PAIRS = 256;
__device__ __forceinline__ void v3_init_lut(uint2 *lut, int lane)
{
#pragma unroll
  for (int j = 0; j < V3_PAIRS / 64; j++) {
    const int e = lane + 64 * j, k4 = e >> 4, t = e & 15;
    const int used = __popc(k4 & 3);                               // received bits the first step consumes
    lut[e] = make_uint2(v3_step_word(((k4 & 3) << 2) | (t >> 2)), v3_step_word((k4 & 12) | (((t << used) >> 2) & 3)));
  }
}

// The M valid bits (the low ones) of each of a dword's four input bytes as one field of 4 M bits, byte 0 -- the first in memory -- most significant: what
//   ((d & mk) << 3 M) | (((d >> 8) & mk) << 2 M) | (((d >> 16) & mk) << M) | ((d >> 24) & mk),  mk = (1 << M) - 1
// gives, folded pairwise with constant masks: bytes 0 and 1 (2 and 3) into the low 2 M bits of each half, then the two halves.  Whatever a byte holds above its M bits is dropped
// (tests/test_viterbi_compact_host.py compiles this for the host and compares it with the formula)
template <int M> __device__ __forceinline__ unsigned v3_compact(unsigned d)
{
  constexpr unsigned c2 = ((1u << M) - 1) * 0x00010001u;           // the M bits of byte 0 and of byte 2
  const unsigned t = ((d & c2) << M) | ((d >> 8) & c2);            // [byte 2 : byte 3] at bit 16, [byte 0 : byte 1] at bit 0
  return ((t & ((1u << (2 * M)) - 1)) << (2 * M)) | (t >> 16);
}
// (end of v3_compact)
// 16 bytes of the input at a 4-byte aligned address kept as an integer (stage_load): a global load (through a generic pointer it would be a flat one, which also counts as an LDS
// operation in the wavefront's waits)
typedef unsigned v3u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 v3_load16(unsigned long long addr)
{
  const v3u4 t = *(const __attribute__((address_space(1))) v3u4 *)addr;
  return make_uint4(t.x, t.y, t.z, t.w);
}

// One decoder per DPP row over [b0, min(b0 + B, total_out)), the wavefront's four rows in step.
// MODE 0: the plain chunk decoder.  MODE 1: the same, and it leaves own[] / pred[] (own, predn: this lane's two words of the slots; inject: the state chunk 0 is handed at its
// first window instead of what its warm-up produced).  MODE 2: from the state in v, no warm-up (WARM is ignored); endv = the state at the next chunk's first window.
// WARM: the warm-up in windows as a compile-time constant (the default instantiation: V3_WARM), or 0: taken from vp.warm (any multiple of V3_BLK up to V3_WARM_MAX).
template <int NTB, int WARM, int MODE, int NW>
__device__ __forceinline__ void v3_decode(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long total_steps, long long total_out, const VitParams &vp,
                                          long long in_base, long long out_lo, long long b0, bool dec_active, const V3Lds &S, const V3Lane &L, int (&v)[2], int (&endv)[2],
                                          int *own, int *predn, const int *inject, int *carry, int carry_rel, int debug, unsigned long long *shortcut)
{
  unsigned char *const tab = S.tab; unsigned *const wbuf = S.wbuf; unsigned char *const bests = S.bests; const uint2 *const lut = S.lut;
  // compacted received bits per decoder (MSB first): V3_CBW words at the head of the decoder's wbuf row.  stage_words reads them (every
  // lane its two words) before the wavefront writes the block's step words over them, and the previous block's step words are dead by
  // then; a wavefront's LDS operations execute in order.  The overlay keeps the workgroup at 20,224 B of LDS per wavefront (19,712 + its share of the pair table): eight wavefronts per CU
  // (two wavefronts per SIMD) with room to spare
  unsigned *const cbits = wbuf;
  constexpr int V3_CBS = V3_BLK * 8;                                               // stride between the decoders' bit streams
  static_assert(V3_CBW <= V3_CBS, "bit stream does not fit the step-word row");
  const int lane = threadIdx.x & 63, dd = lane >> 4, pl = lane & 15;
  const int rowl = S.wv * 256 + dd * 64;                           // wavefront | decoder in a ring offset
  unsigned char *const tabw = tab + rowl + pl * 4;
  const int B = vp.chunk_bytes, m = vp.m;
  constexpr int ntb = NTB;                                         // == vp.ntb (the host picks the instantiation)
  const long long b1 = (b0 + B < total_out) ? b0 + B : total_out;
  const int warm = MODE == 2 ? 0 : WARM > 0 ? WARM : vp.warm;
  const long long w0 = b0 + 2 - warm;                              // absolute window of relative window 0
  const int J = ((warm + B + ntb - 1 + V3_BLK - 1) / V3_BLK) * V3_BLK;
  const long long n_in_bytes = (total_steps * 2 / vp.plen * vp.n + vp.m - 1) / vp.m;   // input bytes that exist
  const int nload = ((384 + 2 * m - 2) / m + 3 + 15) / 16;         // lanes whose 16 bytes a block can need (13, 7, 5)

  // what the traceback compares and addresses per block, as 32-bit offsets from the chunk's first byte (the 64-bit arithmetic is done once, here)
  uint8_t *const outb = out + (b0 - out_lo);
  const int ob_end = !dec_active ? INT_MIN : (int)(b1 - b0 > INT_MIN / 2 ? b1 - b0 : INT_MIN / 2);      // a call is written when ob_lo <= its byte < ob_end[chain]
  const int ob_lo = MODE != 1 || out_lo <= b0 ? 0 : (int)(out_lo - b0 < INT_MAX / 2 ? out_lo - b0 : INT_MAX / 2);
  const long long tb0 = 8 * (w0 - 1) - 2;                          // real step index of step 0 of block 0 (may be < 0)
  constexpr int BLKBITS = 2 * 8 * V3_BLK;                          // depunctured bits per block
  const int inc_q = BLKBITS / vp.plen, inc_ph = BLKBITS - inc_q * vp.plen;   // a block's advance in puncture periods (once per decoder)
  const unsigned magic16_m = (65536u + (unsigned)m - 1) / (unsigned)m;       // x / m for x < 65536 / m

  // The blocks of this wavefront's four decoders whose 8 * V3_BLK steps are all real steps of the stream are jb = u_first .. u_last (a block reaches before the stream's start only
  // in the warm-up of the stream's first chunk, past its end only in its last chunks, and an idle decoder has none): everywhere else staging needs no clamp, and the test is scalar
  int u_first, u_last;
  {
    const long long r = total_steps - 8 * V3_BLK - tb0;
    int first = tb0 >= 0 ? 0 : (int)((-tb0 + 7) >> 3 < J ? (-tb0 + 7) >> 3 : J), last = !dec_active || r < 0 ? -1 : (int)(r >> 3 < J ? r >> 3 : J);
    u_first = max(max(__builtin_amdgcn_readlane(first, 0), __builtin_amdgcn_readlane(first, 16)), max(__builtin_amdgcn_readlane(first, 32), __builtin_amdgcn_readlane(first, 48)));
    u_last = min(min(__builtin_amdgcn_readlane(last, 0), __builtin_amdgcn_readlane(last, 16)), min(__builtin_amdgcn_readlane(last, 32), __builtin_amdgcn_readlane(last, 48)));
  }
  // A second pair of block bounds, for staging's loads: in the blocks jb = l_first .. l_last every one of the nload 16-byte loads of all four rows lies inside the input that exists,
  // [in_base, n_in_bytes) -- the load is then one address and one global_load_dwordx4 under dec_active && pl < nload.  A row's block starts in byte y(t) = rb(2 t) / m of the
  // stream, t = max(tb0 + 8 jb, 0) its first step and rb(p) = (p / plen) n + pfx(p % plen) the received bits in front of depunctured bit p; its lanes read
  // [A, A + 16 nload) with A = the address in + (y - in_base) rounded down to four bytes.  With a = in & 3 and N = n_in_bytes - in_base:
  //   A >= in                   <=>  y - in_base >= (4 - a) & 3                                   =: dmin
  //   A + 16 nload <= in + N    <=>  y - in_base <= ((N + a - 16 nload) & ~3) + 3 - a             =: dmax   (N + a - 16 nload >= 0; otherwise no block)
  // y is monotone in jb, so each side is one threshold on jb.  rb is inverted in whole puncture periods: rb(p) >= R for p >= ((R - 1) / n + 1) plen and rb(p) <= R for
  // p <= (R / n) plen -- up to plen depunctured bits (seven steps, less than a window) on the safe side of the exact threshold, so a bound is the exact one or one block
  // inside it (tests/test_viterbi_load_bounds_model.py).  Outside the bounds the lanes test their bytes themselves, as they always did.
  const unsigned long long in_addr = (unsigned long long)(uintptr_t)in;
  const int ld_lanes = dec_active ? nload : 0;                     // the lanes of the row that load: one compare, one exec region
  int l_first, l_last;
  {
    const int a = (int)(in_addr & 3ull);
    const long long H = n_in_bytes - in_base + a - 16 * nload;
    const long long Rlo = (in_base + ((4 - a) & 3)) * m;                             // y >= in_base + dmin  <=>  rb >= Rlo
    const long long Rhi = (in_base + (H & ~3ll) + 3 - a + 1) * m - 1;                // y <= in_base + dmax  <=>  rb <= Rhi
    int first = 0, last = J;                                                       // (a decoder that does not exist loads nothing)
    if (dec_active) {
      if (Rlo > 0) {
        const unsigned long long p = (__umul64hi((unsigned long long)(Rlo - 1), vp.magic_n) + 1) * (unsigned)vp.plen;
        const long long w = ((long long)((p + 1) >> 1) - tb0 + 7) >> 3;            // the first window at or behind step p / 2
        first = w <= 0 ? 0 : w >= J ? J : (((int)w + V3_BLK - 1) / V3_BLK) * V3_BLK;
      }
      if (H < 0 || Rhi < 0) last = -1;
      else {
        const unsigned long long p = __umul64hi((unsigned long long)Rhi, vp.magic_n) * (unsigned)vp.plen;
        const long long w = ((long long)(p >> 1) - tb0) >> 3;                      // the last window whose first step is at or in front of step p / 2
        last = w < 0 ? -1 : w >= J ? J : ((int)w / V3_BLK) * V3_BLK;
      }
    }
    l_first = max(max(__builtin_amdgcn_readlane(first, 0), __builtin_amdgcn_readlane(first, 16)), max(__builtin_amdgcn_readlane(first, 32), __builtin_amdgcn_readlane(first, 48)));
    l_last = min(min(__builtin_amdgcn_readlane(last, 0), __builtin_amdgcn_readlane(last, 16)), min(__builtin_amdgcn_readlane(last, 32), __builtin_amdgcn_readlane(last, 48)));
  }
  // ---- staging, first half: where block jb starts in the input (row-uniform) and the load of its bytes.  The blocks are staged in order: behind a block whose step 0 is a real
  // step the position advances by BLKBITS depunctured bits -- ph0, the byte and bo0 are carried with small integers; the 64-bit locate runs for a decoder's first block, and for
  // the blocks of a decoder that starts before the stream does (the clamp below), in which case the whole wavefront takes it.
  // pfx(ph) = received bits of a period before its phase ph (VitParams.prefix): the kept symbols below ph -- one v_bfe + v_bcnt where the nibble table takes a 64-bit shift
  auto pfx = [&](int ph) { return (int)__popc(vp.punct_mask & ((1u << ph) - 1u)); };
  // The byte the row's block starts in is carried as its address pb = in + (byte - in_base), a 64-bit integer that advances with the block (it may lie in front of `in` or
  // behind the last byte: nothing is read through it outside [in, in + n_in_bytes - in_base)).  The lanes read 16 bytes each from pb rounded down to four bytes
  int ph0 = 0, pf0 = 0, bo0 = 0, off = 0; unsigned long long pb = 0; uint4 q = make_uint4(0, 0, 0, 0);   // pf0 = pfx(ph0), carried with it
  auto stage_load = [&](int jb) {
    const long long tb = tb0 + (long long)jb * 8;                  // real step index of block step 0 (may be < 0)
    if (jb > 0 && jb - V3_BLK >= u_first) {                         // (the block before starts at a real step in all four decoders)
      const int pf_old = pf0;
      ph0 += inc_ph;
      const int wrap = ph0 >= vp.plen ? 1 : 0;
      ph0 -= wrap ? vp.plen : 0;
      pf0 = pfx(ph0);
      const int r = bo0 + (inc_q + wrap) * vp.n + pf0 - pf_old;       // received bits from the old byte's first bit (0 <= r < 1024)
      const int dby = (int)(((unsigned)r * magic16_m) >> 16);
      bo0 = r - dby * m; pb += (unsigned)dby;
    } else {
      const unsigned long long pbit = 2ull * (unsigned long long)(tb > 0 ? tb : 0);
      const unsigned long long pq = __umul64hi(pbit, vp.magic_plen);
      ph0 = (int)(pbit - pq * (unsigned)vp.plen); pf0 = pfx(ph0);
      const unsigned long long rb = pq * (unsigned)vp.n + (unsigned)pf0;
      const unsigned long long by = __umul64hi(rb, vp.magic_m);
      pb = in_addr + (by - (unsigned long long)in_base); bo0 = (int)(rb - by * (unsigned)m);
    }
    off = (int)((unsigned)pb & 3u);
    const unsigned long long la = (pb & ~3ull) + (unsigned)(pl * 16);   // 4-byte aligned address of this lane's 16 bytes
    q = make_uint4(0, 0, 0, 0);
    if (__builtin_expect(jb >= l_first && jb <= l_last, 1)) {       // every lane's 16 bytes exist (wave-uniform): no lane compares a 64-bit position
      if (pl < ld_lanes) q = v3_load16(la);
    } else if (pl < ld_lanes) {
      const long long src = (long long)(la - in_addr) + in_base;   // the bytes' index in the stream
      if (src >= in_base && src + 16 <= n_in_bytes) q = v3_load16(la);
      else {
        // byte by byte.  Which of the sixteen exist is settled once, in 64 bits: the bytes [e0, e1) -- a byte then costs two 32-bit compares with a constant, not two 64-bit
        // ones behind a 64-bit add (sixteen copies of this stand in the middle of every iteration's code)
        const long long d0 = in_base - src, d1 = n_in_bytes - src;
        const int e0 = d0 < 0 ? 0 : d0 > 16 ? 16 : (int)d0, e1 = d1 < 0 ? 0 : d1 > 16 ? 16 : (int)d1;
        const uint8_t *const pbyte = in + (src - in_base);
        unsigned w[4] = {0, 0, 0, 0};
        for (int i = 0; i < 16; i++) {
          const unsigned bv = (i >= e0 && i < e1) ? pbyte[i] : 0;
          w[i >> 2] |= bv << (8 * (i & 3));
        }
        q = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  };
  // ---- staging, second half: bit compaction and the step words of block jb
  auto stage_words = [&](int jb, auto &&mid) {
    {
      // m is wave-uniform: each of the three exclusive branches compacts with constant masks and shifts (v3_compact)
      unsigned *cb = cbits + dd * V3_CBS;
      if (pl < nload) {
        if (m == 2) cb[pl] = (v3_compact<2>(q.x) << 24) | (v3_compact<2>(q.y) << 16) | (v3_compact<2>(q.z) << 8) | v3_compact<2>(q.w);
        else if (m == 4) { cb[2 * pl] = (v3_compact<4>(q.x) << 16) | v3_compact<4>(q.y); cb[2 * pl + 1] = (v3_compact<4>(q.z) << 16) | v3_compact<4>(q.w); }
        else {
          const unsigned g0 = v3_compact<6>(q.x), g1 = v3_compact<6>(q.y), g2 = v3_compact<6>(q.z), g3 = v3_compact<6>(q.w);
          cb[3 * pl] = (g0 << 8) | (g1 >> 16); cb[3 * pl + 1] = (g1 << 16) | (g2 >> 8); cb[3 * pl + 2] = (g2 << 24) | g3;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    constexpr int SPL = V3_BLK * 8 / 16;                           // steps per lane
    const long long tb = tb0 + (long long)jb * 8;
    const int ub0 = pl * SPL;
    // a block that lies inside the stream, of a decoder that exists: every step is real.  Otherwise (a decoder's blocks around the stream's start and end) the wavefront clamps
    int lo = 0, hi = SPL;                                          // leading steps before the stream start; end of the real steps
    int x = ph0 + 2 * ub0;                                         // depunctured-bit offset of the first real step from the row base
    if (jb < u_first || jb > u_last) {
      const long long tbr = tb > 0 ? tb : 0;
      const long long t = tb + ub0;
      if (t < 0) lo = (-t < SPL) ? (int)(-t) : SPL;
      const long long rem = total_steps - t;
      hi = !dec_active ? 0 : rem <= 0 ? 0 : rem < SPL ? (int)rem : SPL;
      if (hi < lo) hi = lo;
      x = ph0 + 2 * (int)((t + lo) - tbr);
      if (x < 0) x = 0;
    }
    const int dq = (int)(((unsigned)x * vp.magic16_plen) >> 16);
    const int ph = x - dq * vp.plen;
    const int pos = off * m + bo0 + dq * vp.n + pfx(ph) - pf0;
    const unsigned kmask = ((unsigned)(vp.punct_rep >> ph) << (2 * lo)) & (((1u << (2 * hi)) - 1u) & ~((1u << (2 * lo)) - 1u));
    const unsigned *cb = cbits + dd * V3_CBS;
    const unsigned cw0 = cb[pos >> 5], cw1 = cb[(pos >> 5) + 1];
    mid();                                                         // (LDS returns in order: what is read here has arrived when the look-ups below have)
    unsigned win = (unsigned)(((((unsigned long long)cw0) << 32) | cw1) >> (32 - (pos & 31)));
    // the twelve table indices first (one VALU chain on win), then the twelve look-ups back to back behind ONE wait, then the lane's 48 bytes as three 16-byte stores.  Written as
    // look-up + store per step, the compiler keeps that order (the table and the step words are members of one LDS object) and the wavefront waits out twelve LDS round trips in a row
    // (two steps per link and per look-up: the pair table, v3_init_lut)
    unsigned idx[SPL / 2], sw[SPL];
#pragma unroll
    for (int i = 0; i < SPL / 2; i++) {
      const unsigned k4 = (kmask >> (4 * i)) & 15u;                 // keep flags of the two steps' four symbols
      idx[i] = (k4 << 4) | (win >> 28);
      win <<= __popc(k4);                                          // consume one received bit per kept symbol
    }
#pragma unroll
    for (int i = 0; i < SPL / 2; i++) { const uint2 w2 = lut[idx[i]]; sw[2 * i] = w2.x; sw[2 * i + 1] = w2.y; }
    static_assert(SPL % 4 == 0, "a lane's step words are whole 16-byte groups (its offset dd * 768 + pl * 48 bytes is 16-byte aligned)");
    uint4 *const wdst = reinterpret_cast<uint4 *>(wbuf + dd * (V3_BLK * 8) + ub0);
#pragma unroll
    for (int i = 0; i < SPL / 4; i++) wdst[i] = make_uint4(sw[4 * i], sw[4 * i + 1], sw[4 * i + 2], sw[4 * i + 3]);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  };
  // ---- traceback chains of the block that starts at window jp
  // (a block starts at a multiple of 3 windows, so the phases a chain meets depend on the lane alone)
  // The bit shuffles between a state and a cell's storage index depend, beside the path byte, on the lane alone: z(cell) = rotl6(cell, 2) ^ 12 * (cell bit 2) (v3_z_of_cell) and
  // cell = rotr6(state, phase), so z = R ^ 12 * (R bit 4) with R = rotl6(state, 2 - phase) -- one shift by a constant of the lane (tsh, osh: computed once per kernel)
  V3Trace T;
  int tsh[2];                                                      // (phase after the window a chain starts in + 4) % 6, that phase = (8 jj + 8) % 6 = 2 * ((jj + 1) % 3)
  int tsh_e[2];                                                    // the same for the window the chain ends in (jj - (ntb - 1))
#pragma unroll
  for (int c = 0; c < 2; c++) {
    tsh_e[c] = (2 * ((c * 16 + pl + 1 + 3 * ntb - (ntb - 1)) % 3) + 4) % 6;
    T.oend[c] = c * 16 + pl < V3_BLK ? ob_end : INT_MIN; tsh[c] = (2 * ((c * 16 + pl + 1) % 3) + 4) % 6; T.osh[c] = (6 - 2 * ((c * 16 + pl + 3 * ntb - (ntb - 1)) % 3)) % 6;
  }
  static_assert(V3_BLK % 3 == 0, "phases per lane");
  // the best states the chains of the block at window jp start from.  The block is complete when it ends: the reads are issued at the top of the next iteration, ahead of
  // staging, and used behind it (trace_init) -- their round trip hides under the staging arithmetic
  auto bests_read = [&](int jp, unsigned (&bb)[2]) {
#pragma unroll
    for (int c = 0; c < 2; c++) bb[c] = bests[dd * V3_RINGW + ((jp + c * 16 + pl) & (V3_RINGW - 1))];
  };
  // storage index of the best state's cell from the byte in bests (63 - best state = ~state in six bits): R = rotl6(bb, .) ^ 63, and 63 ^ 12 * (1 - bit) = 51 ^ 12 * bit
  auto z_of_best = [](unsigned b, int sh) { const unsigned R = (b | (b << 6)) >> sh; return (R ^ 51u ^ (((R >> 4) & 1u) * 12u)) & 63u; };
  auto trace_init = [&](int jp, const unsigned (&bb)[2]) {
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int jj = jp + c * 16 + pl;
      T.ob[c] = jj - (warm + ntb - 1);
      T.ok[c] = __builtin_amdgcn_ballot_w64(T.ob[c] >= ob_lo && T.ob[c] < T.oend[c]);          // (a chain that is not ok runs all the same, over whatever the ring holds: every read is masked into the ring)
      T.wsh[c] = jj * V3_ROW<NW> + rowl;
      T.z[c] = (int)z_of_best(bb[c], tsh[c]) | (T.wsh[c] & V3_RMASK<NW>);
    }
  };
  // ---- the shortcut (see the header): the best states of the windows in front of the chains' starts and of the windows the chains end in are read with bb at the top of the
  // iteration; behind the compacted bits' reads (stage_words' `mid`) the chains are set up and four path bytes are read: the first hop's (tl: it tells whether the hop from
  // window jj's best state lands on window jj - 1's) and the one at the best state of the window the chain ends in (te: the call's byte when every link holds)
  unsigned bb[2], be[2], tl[2], te[2];
  int zp[2], zcarry = 0;                                           // zp: Z(jj - 1) in the low six bits; zcarry (lane 0 of a row): Z of the last window of the block before
  auto bests_read_ends = [&](int jp) {
#pragma unroll
    for (int c = 0; c < 2; c++) be[c] = bests[dd * V3_RINGW + ((jp + c * 16 + pl - (ntb - 1)) & (V3_RINGW - 1))];
  };
  // Z(jj - 1) is the neighbouring lane's Z(jj): one row shift.  Lane 0 has no neighbour: its chain 1 (window jp + 16) takes chain 0's lane 15 (row_ror:1 as the value the shift
  // leaves in place), its chain 0 the Z of window jp - 1 = the previous iteration's chain 1 of lane 7 (row_ror:9, kept in zcarry)
  auto link_reads = [&](int jp) {
    trace_init(jp, bb);
    zp[0] = __builtin_amdgcn_update_dpp(zcarry, T.z[0], 0x111, 0xf, 0xf, false);                     // row_shr:1
    zp[1] = __builtin_amdgcn_update_dpp(dppb<0x121>(T.z[0]), T.z[1], 0x111, 0xf, 0xf, false);
#pragma unroll
    for (int c = 0; c < 2; c++) tl[c] = tab[T.z[c]];
    zcarry = dppb<0x129>(T.z[1]);
  };
  // the path byte at the best state of the window a chain ends in: read only where the shortcut is taken
  auto end_reads = [&]() {
#pragma unroll
    for (int c = 0; c < 2; c++) te[c] = tab[(int)z_of_best(be[c], tsh_e[c]) | ((T.wsh[c] - (ntb - 1) * V3_ROW<NW>) & V3_RMASK<NW>)];
  };
  // all 24 links of the block at jp hold in every decoder of the wavefront that still has calls to deliver (chain 1 of the lanes 8..15 has no window in the block).  A decoder
  // whose block starts behind its last call -- an idle one, or the stream's last chunk beside longer ones: its windows lie past the stream's end and chain up with nothing -- has
  // none in any later block either, so its links are nobody's
  auto links_hold = [&](int jp) {
    const bool fails = jp - (warm + ntb - 1) < ob_end && ((((tl[0] ^ (unsigned)zp[0]) & 63u) != 0) || (pl < V3_BLK - 16 && ((tl[1] ^ (unsigned)zp[1]) & 63u) != 0));
    return __builtin_amdgcn_ballot_w64(fails) == 0;
  };
  bool ok_prev = false;                                            // the links of the block before the one whose chains start now
  unsigned n_short = 0, n_walk = 0;

  stage_load(0);
  for (int jb = 0; jb < J; jb += V3_BLK) {
    if (MODE == 1 && dec_active) {                                 // (wave-uniform but for dec_active and the pointers)
      if (jb == warm) { if (inject) { v[0] = inject[0]; v[1] = inject[1]; } own[0] = v[0]; own[1] = v[1]; }
      if (jb == warm + B) { predn[0] = v[0]; predn[1] = v[1]; }   // the NEXT chunk's first window, seen by its predecessor
      if (carry && jb == warm + carry_rel) { carry[0] = v[0]; carry[1] = v[1]; }
    }
    if (MODE == 2) {
      if (jb == 0 && dec_active) { own[0] = v[0]; own[1] = v[1]; }
      if (jb == B) { endv[0] = v[0]; endv[1] = v[1]; }
      if (carry && dec_active && jb == carry_rel) { carry[0] = v[0]; carry[1] = v[1]; }
    }
    bests_read(jb - V3_BLK, bb);                                   // (block 0: whatever the ring holds, unused)
    bests_read_ends(jb - V3_BLK);
    if (!(V3_EXP & 8) || jb == 0) stage_words(jb, [&]() { link_reads(jb - V3_BLK); });
    else link_reads(jb - V3_BLK);
    if (jb + V3_BLK < J && !(V3_EXP & 8)) stage_load(jb + V3_BLK);                  // the bytes of the next block travel during this block's forward pass
    // The decision, once per iteration and wave-uniform.  A chain started at window jj walks through the windows jj - 1 .. jj - (ntb - 1); where every hop lands on the best state
    // of the window it reaches, the chain ends at the best state of window jj - (ntb - 1) and its byte is te.  The chains of this block need the links of the windows
    // jj - (ntb - 2) .. jj: this block's and the one's before (more than needed, and enough for every ntraceback).  Nothing is walked either where no chain ends in a call.
    // (bests_read_ends, trace_init and link_reads run in every iteration, jb == 0 and the switched-off decoder included: over whatever the ring and bests[] hold, every index
    // masked into the ring; only te is read on the fast branch alone.  Block 0's link(0) compares with a zcarry nobody set and block 0 has no verdict (jb > 0 below), so the first
    // iteration that can be fast is jb = 72: the blocks at 24 and 48 both seen.)
    const bool ok_cur = jb > 0 && links_hold(jb - V3_BLK);
    const bool ends = (T.ok[0] | T.ok[1]) != 0;
    const bool fast = ok_cur && ok_prev && !(debug & V3_DEBUG_WALK) && !(V3_EXP & 1);
    ok_prev = ok_cur;
    const bool tr = jb > 0 && !fast && ends && !(V3_EXP & 1);
    if (fast && ends) { end_reads(); v3_trace_store<true>(T, te, outb); n_short++; }
    if (tr) n_walk++;
    const unsigned *wrow = wbuf + dd * (V3_BLK * 8);
    unsigned Wa[8], Wb[8];                                         // the step words of the current and of the next window
    v3_load_words(wrow, Wa);
    if (tr) {
      v3_fwd_six<0, true, 0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb);
      v3_fwd_six<6, true, 12, NTB, NW, true>(v, L, wrow + 48, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb);
    } else {
      v3_fwd_six<0, false, 0, NTB, NW, true>(v, L, wrow, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb);
      v3_fwd_six<6, false, 0, NTB, NW, true>(v, L, wrow + 48, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb);
    }
    static_assert(V3_BLK == 24, "the second half of the block is written out: two groups of six windows, straight-line like the first half");
    static_assert(NTB - 1 < 24, "the chains' last read takes a hop slot of the first twelve windows");
    v3_fwd_six<12, false, 0, NTB, NW, true>(v, L, wrow + 96, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb);
    v3_fwd_six<18, false, 0, NTB, NW, false>(v, L, wrow + 144, tab, tabw, bests, jb, dd, pl, T, Wa, Wb, outb);
  }
  // the last block's calls
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  bests_read(J - V3_BLK, bb);
  trace_init(J - V3_BLK, bb);
  for (int h = 0; h < ntb - 1; h++) v3_hop<NW>(T, tab);
  v3_trace_out(T, tab, outb);
  if (MODE == 1 && shortcut && lane == 0) { atomicAdd(shortcut, (unsigned long long)n_short); atomicAdd(shortcut + 1, (unsigned long long)n_walk); }
}

// One object, the ring first: it is the kernel's only LDS variable, so the ring starts at LDS offset 0 and a ring offset IS the ds address (a hop adds no base).  Nothing depends
// on that for correctness: wherever the object lies, its address is a constant that folds into the ds instructions' offset field.
template <int NW> struct V3Shared {
  alignas(16) unsigned char tab[V3_RINGW * V3_ROW<NW>];     // path bytes: [window][wavefront][decoder][cell z]  (the ppresult ring)
  alignas(16) unsigned wbuf[NW][4 * V3_BLK * 8];            // step words: [wavefront][decoder][step in block]
  unsigned char bests[NW][4 * V3_RINGW];                    // best state per window
  uint2 lut[V3_PAIRS];                                      // (keep flags of two steps, next four received bits) -> the two step words (v3_init_lut)
};
static_assert(sizeof(V3Shared<4>) == 80896, "79 KiB: two workgroups are 158 of a CU's 160 KiB");
static_assert(sizeof(V3Shared<4>) <= 81920 && V3_RMASK<4> == 0xffc0 && V3_RMASK<1> == 0x3fc0, "two four-wave workgroups per CU beside the symbol kernel's 76 KB");
#define V3_LDS_DECL(NW) __shared__ V3Shared<NW> sh_;
#define V3_LDS(NW, wv) V3Lds{sh_.tab, sh_.wbuf[wv], sh_.bests[wv], sh_.lut, wv}

// MODE 0 / 1 (see v3_decode).  MODE 0: out_lo is also the index of chunk 0's first byte (the block API's former layout); MODE 1: ax.grid0 is, out_lo the first byte that is written.
template <int NTB, int WARM = V3_WARM, int MODE = 0> __global__ __launch_bounds__(64 * V3_WGW) void viterbi3_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const RxState *st,
                                                      long long steps_fixed, VitParams vp, V3Aux ax, long long in_base, long long out_lo)
{
  V3_LDS_DECL(V3_WGW)
  const int wv = V3_WGW > 1 ? (int)(threadIdx.x >> 6) : 0;
  const V3Lds S = V3_LDS(V3_WGW, wv);
  const int lane = threadIdx.x & 63, dd = lane >> 4, pl = lane & 15;
  const long long total_steps = st ? st->n_vit_steps : steps_fixed;
  const long long total_out = total_steps / 8 - vp.ntb;
  const int B = vp.chunk_bytes;
  if (MODE == 1 && blockIdx.x == 0 && threadIdx.x == 0) {        // the counters of the passes behind this launch
    ax.ctl[V3_CTL_MISMATCH] = 0; ax.ctl[V3_CTL_CONFLICT] = 0; ax.ctl[V3_CTL_UNPROVEN] = -1; ax.ctl[V3_CTL_SEQ] = 0;
  }
  const long long grid0 = MODE == 1 ? ax.grid0 : out_lo;
  const long long chunk0 = ((long long)blockIdx.x * V3_WGW + wv) * 4;
  if (grid0 + chunk0 * B >= total_out) return;                    // whole wavefront idle
  const long long c = chunk0 + dd, b0 = grid0 + c * B;            // this lane's decoder
  const bool dec_active = b0 < total_out;
  v3_init_lut(sh_.lut, lane);
#if V3_EXP & 16
  const unsigned long long dbg_t0 = wall_clock64();
#endif
  V3Lane L; v3_init_lane(pl, L);
  // equal metrics, origin stamp of window 0, tie-break bits of its first three steps.  The metric byte of both halves starts at V3_RENORM_BEST, where a renormalisation
  // would have left the best: the first one comes V3_RENORM_EVERY windows on, and from 0 the field would pass 127 before it
  constexpr int v3_start = (int)(((unsigned)(V3_RENORM_BEST & 0xff) << 8) * 0x00010001u);
  int v[2] = {L.arm_org[0][0] | v3_start, L.arm_org[0][1] | v3_start}, endv[2];
  int *own = nullptr, *predn = nullptr, *carry = nullptr; const int *inject = nullptr;
  if (MODE == 1) {
    own = v3_own(ax, c) + 2 * pl; predn = v3_pred(ax, c + 1) + 2 * pl;
    if (c == 0 && ax.carry_in) inject = ax.carry_in + 2 * pl;
    if (ax.carry_out && b0 + B >= total_out) carry = ax.carry_out + 2 * pl;      // the launch's last chunk
  }
  v3_decode<NTB, WARM, MODE, V3_WGW>(in, out, total_steps, total_out, vp, in_base, out_lo, b0, dec_active, S, L, v, endv, own, predn, inject, carry, ax.carry_rel, ax.debug,
                                     MODE == 1 ? reinterpret_cast<unsigned long long *>(ax.ctl + V3_CTL_SHORT) : nullptr);
#if V3_EXP & 16
  if (lane == 0) {
    unsigned id, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long *d = v3_dbg + 3 * ((long long)blockIdx.x * V3_WGW + wv);
    d[0] = (id & 0xffffu) | ((xcc & 0xfu) << 16); d[1] = dbg_t0; d[2] = wall_clock64();
  }
#endif
}

__device__ __forceinline__ long long v3_nchunks(long long total_out, long long grid0, int B) { return total_out > grid0 ? (total_out - grid0 + B - 1) / B : 0; }
__device__ __forceinline__ bool v3_slots_equal(const int *a_, const int *b_)
{
  const int4 *a = reinterpret_cast<const int4 *>(a_), *b = reinterpret_cast<const int4 *>(b_);      // 32 words = 8 x int4 per slot
  bool same = true;
#pragma unroll
  for (int i = 0; i < 8; i++) { const int4 x = a[i], y = b[i]; same = same && x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w; }
  return same;
}

// pass 0: the chunks c >= 1 whose own[c] is not pred[c] go on the list (ctl[V3_CTL_MISMATCH] of them), the conflict flags are cleared.
// pass 1 (the final check, dvbt_rx_params.viterbi_verify): they are counted in ctl[V3_CTL_UNPROVEN] (zero behind the repair passes, by construction).
__global__ __launch_bounds__(256) void viterbi_check_kernel(V3Aux ax, const RxState *st, long long steps_fixed, VitParams vp, int pass)
{
  const long long total_steps = st ? st->n_vit_steps : steps_fixed;
  const long long nch = v3_nchunks(total_steps / 8 - vp.ntb, ax.grid0, vp.chunk_bytes);
  if (blockIdx.x == 0 && threadIdx.x == 0) { ax.ctl[V3_CTL_CHUNKS] = (int)(nch < INT_MAX ? nch : INT_MAX); if (pass == 1) ax.ctl[V3_CTL_UNPROVEN] = 0; }
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x + 1;
  if (c >= nch || c > ax.cap) return;
  const bool same = v3_slots_equal(v3_own(ax, c), v3_pred(ax, c));
  if (pass == 0) {
    ax.ctl[V3_CTL_HDR + (ax.cap + 2) + c] = 0;
    if (!same) ax.ctl[V3_CTL_HDR + atomicAdd(ax.ctl + V3_CTL_MISMATCH, 1)] = (int)c;
  }
}
// (the final check's count needs its zero before any thread adds to it: a second kernel rather than a grid-wide handshake)
__global__ __launch_bounds__(256) void viterbi_count_kernel(V3Aux ax, const RxState *st, long long steps_fixed, VitParams vp)
{
  const long long total_steps = st ? st->n_vit_steps : steps_fixed;
  const long long nch = v3_nchunks(total_steps / 8 - vp.ntb, ax.grid0, vp.chunk_bytes);
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x + 1;
  if (c >= nch || c > ax.cap) return;
  if (!v3_slots_equal(v3_own(ax, c), v3_pred(ax, c))) atomicAdd(ax.ctl + V3_CTL_UNPROVEN, 1);
}

// every lane of the row: do the row's 16 lanes hold the same two words in a and b?
__device__ __forceinline__ bool v3_row_equal(const int (&a)[2], const int (&b)[2], int dd)
{
  const unsigned long long ne = __ballot(a[0] != b[0] || a[1] != b[1]);
  return ((ne >> (16 * dd)) & 0xffffull) == 0;
}

// The parallel repair pass: one decoder (row) per listed chunk, from pred[c], over that chunk alone.  `rows` decoder rows work through the list, this wavefront's first is row0.
template <int NTB, int NW> __device__ __forceinline__ void v3_repair_rows(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long total_steps, const VitParams &vp, const V3Aux &ax,
                                                                  long long in_base, long long out_lo, const V3Lds &S, const V3Lane &L, long long rows, long long row0, int n)
{
  const int lane = threadIdx.x & 63, dd = lane >> 4, pl = lane & 15;
  const long long total_out = total_steps / 8 - vp.ntb;
  const int B = vp.chunk_bytes;
  const long long nch = v3_nchunks(total_out, ax.grid0, B);
  for (long long i0 = row0; i0 < n; i0 += rows) {
    const bool act = i0 + dd < n;
    const long long c = act ? ax.ctl[V3_CTL_HDR + i0 + dd] : 1;
    const long long b0 = ax.grid0 + c * B;
    int v[2], endv[2] = {0, 0};
    { const int *p = v3_pred(ax, c) + 2 * pl; v[0] = p[0]; v[1] = p[1]; }
    int *carry = (act && ax.carry_out && b0 + B >= total_out) ? ax.carry_out + 2 * pl : nullptr;
    v3_decode<NTB, 0, 2, NW>(in, out, total_steps, total_out, vp, in_base, out_lo, b0, act && b0 < total_out, S, L, v, endv, v3_own(ax, c) + 2 * pl, nullptr, nullptr, carry, ax.carry_rel, ax.debug, nullptr);
    int pn[2] = {endv[0], endv[1]};
    if (act && c + 1 < nch) { const int *p = v3_pred(ax, c + 1) + 2 * pl; pn[0] = p[0]; pn[1] = p[1]; }
    if (!v3_row_equal(endv, pn, dd) || ((ax.debug & 1) && act && c + 1 < nch)) {   // the repaired decoder does not arrive where the unproven one did: the sequential pass goes on from here
      int *f = v3_fix(ax, c + 1) + 2 * pl; f[0] = endv[0]; f[1] = endv[1];
      if (pl == 0) { ax.ctl[V3_CTL_HDR + (ax.cap + 2) + c + 1] = 1; atomicAdd(ax.ctl + V3_CTL_CONFLICT, 1); }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");          // (the next round's staging overwrites this round's LDS)
  }
}
template <int NTB> __global__ __launch_bounds__(64 * V3_WGW) void viterbi_repair_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const RxState *st,
                                                      long long steps_fixed, VitParams vp, V3Aux ax, long long in_base, long long out_lo)
{
  V3_LDS_DECL(V3_WGW)
  const int n = ax.ctl[V3_CTL_MISMATCH];
  const int wv = V3_WGW > 1 ? (int)(threadIdx.x >> 6) : 0;
  const long long rows = (long long)gridDim.x * V3_WGW * 4, row0 = ((long long)blockIdx.x * V3_WGW + wv) * 4;
  if (row0 >= n) return;
  const V3Lds S = V3_LDS(V3_WGW, wv);
  v3_init_lut(sh_.lut, threadIdx.x & 63);
  V3Lane L; v3_init_lane(threadIdx.x & 15, L);
  v3_repair_rows<NTB, V3_WGW>(in, out, st ? st->n_vit_steps : steps_fixed, vp, ax, in_base, out_lo, S, L, rows, row0, n);
}

// The sequential pass: ONE decoder walks the flagged chunks in stream order.  From fix[c] it decodes chunk c; where the state it reaches at chunk c + 1 is own[c + 1] the bytes behind
// are the streaming decoder's already, otherwise it goes on through chunk c + 1.  force (a test hook, dvbt_rx_params.viterbi_verify = 3: the parallel pass is not launched): every
// chunk whose own[] is not pred[] is taken, from pred[].  One wavefront, its first row.
template <int NTB, int NW> __device__ __forceinline__ void v3_seq_walk(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long total_steps, const VitParams &vp, const V3Aux &ax,
                                                               long long in_base, long long out_lo, const V3Lds &S, const V3Lane &L, int force)
{
  const int lane = threadIdx.x & 63, dd = lane >> 4, pl = lane & 15;
  if (lane == 0) { ax.ctl[V3_CTL_ACC] += ax.ctl[V3_CTL_CHUNKS]; ax.ctl[V3_CTL_ACC + 1] += ax.ctl[V3_CTL_MISMATCH]; }   // (the last pass of every repairing launch)
  if (!force && ax.ctl[V3_CTL_CONFLICT] == 0) return;
  const long long total_out = total_steps / 8 - vp.ntb;
  const int B = vp.chunk_bytes;
  long long nch = v3_nchunks(total_out, ax.grid0, B);
  if (nch > ax.cap) nch = ax.cap;
  const int *cflag = ax.ctl + V3_CTL_HDR + (ax.cap + 2);
  int done = 0;
  long long pos = 0;                                                 // everything up to and including chunk pos is the streaming decoder's
  for (;;) {
    // the next chunk behind pos that is flagged (64 candidates per round, one per lane)
    long long cn = -1;
    for (long long c0 = pos + 1; c0 < nch && cn < 0; c0 += 64) {
      const long long c = c0 + lane;
      bool hit = false;
      if (c < nch) hit = cflag[c] != 0 || (force && !v3_slots_equal(v3_own(ax, c), v3_pred(ax, c)));
      const unsigned long long b = __ballot(hit);
      if (b) cn = c0 + __builtin_ctzll(b);
    }
    if (cn < 0) break;
    long long c = cn;
    int v[2];
    { const int *p = (cflag[c] ? v3_fix(ax, c) : v3_pred(ax, c)) + 2 * pl; v[0] = p[0]; v[1] = p[1]; }
    for (;;) {
      const long long b0 = ax.grid0 + c * B;
      const bool act = dd == 0;
      int st0[2] = {v[0], v[1]}, endv[2] = {0, 0};
      if (act) { int *p = v3_pred(ax, c) + 2 * pl; p[0] = v[0]; p[1] = v[1]; }
      int *carry = (act && ax.carry_out && b0 + B >= total_out) ? ax.carry_out + 2 * pl : nullptr;
      v3_decode<NTB, 0, 2, NW>(in, out, total_steps, total_out, vp, in_base, out_lo, b0, act, S, L, st0, endv, v3_own(ax, c) + 2 * pl, nullptr, nullptr, carry, ax.carry_rel, ax.debug, nullptr);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      done++;
      if (c + 1 >= nch) { pos = nch; break; }
      int on[2]; { const int *p = v3_own(ax, c + 1) + 2 * pl; on[0] = p[0]; on[1] = p[1]; }
      const bool eq = (__ballot(on[0] != endv[0] || on[1] != endv[1]) & 0xffffull) == 0;
      if (act) { int *p = v3_pred(ax, c + 1) + 2 * pl; p[0] = endv[0]; p[1] = endv[1]; }
      if (eq) { pos = c + 1; break; }
      c++; v[0] = endv[0]; v[1] = endv[1];
    }
  }
  if (lane == 0) { ax.ctl[V3_CTL_SEQ] = done; ax.ctl[V3_CTL_ACC + 2] += done; }
}
template <int NTB> __global__ __launch_bounds__(64) void viterbi_repair_seq_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const RxState *st,
                                                      long long steps_fixed, VitParams vp, V3Aux ax, long long in_base, long long out_lo, int force)
{
  V3_LDS_DECL(1)
  const V3Lds S = V3_LDS(1, 0);
  v3_init_lut(sh_.lut, threadIdx.x & 63);
  V3Lane L; v3_init_lane(threadIdx.x & 15, L);
  v3_seq_walk<NTB, 1>(in, out, st ? st->n_vit_steps : steps_fixed, vp, ax, in_base, out_lo, S, L, force);
}

// Check, parallel repair (16 decoder rows) and sequential pass in ONE launch of one workgroup, for launches of few chunks (V3_FIX_SMALL): the lock periods of a walk, the single
// block's calls, short pieces -- where three launches that mostly find nothing to do cost more than they compute (BASELINE config 5 at the prescribed noise: 121 Viterbi launches
// per 16 superframes).  The same passes in the same order; the workgroup's barriers stand where the launch boundaries stood.
constexpr long long V3_FIX_SMALL = 1024;
template <int NTB> __global__ __launch_bounds__(64 * V3_WGW) void viterbi_fix_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const RxState *st,
                                                      long long steps_fixed, VitParams vp, V3Aux ax, long long in_base, long long out_lo, int force)
{
  V3_LDS_DECL(V3_WGW)
  const int wv = V3_WGW > 1 ? (int)(threadIdx.x >> 6) : 0;
  const long long total_steps = st ? st->n_vit_steps : steps_fixed;
  const long long nch = v3_nchunks(total_steps / 8 - vp.ntb, ax.grid0, vp.chunk_bytes);
  if (threadIdx.x == 0) ax.ctl[V3_CTL_CHUNKS] = (int)(nch < INT_MAX ? nch : INT_MAX);
  for (long long c = 1 + threadIdx.x; c < nch && c <= ax.cap; c += 64 * V3_WGW) {
    ax.ctl[V3_CTL_HDR + (ax.cap + 2) + c] = 0;
    if (!v3_slots_equal(v3_own(ax, c), v3_pred(ax, c))) ax.ctl[V3_CTL_HDR + atomicAdd(ax.ctl + V3_CTL_MISMATCH, 1)] = (int)c;
  }
  __threadfence(); __syncthreads();
  const int n = *(volatile int *)(ax.ctl + V3_CTL_MISMATCH);
  const V3Lds S = V3_LDS(V3_WGW, wv);
  v3_init_lut(sh_.lut, threadIdx.x & 63);
  V3Lane L; v3_init_lane(threadIdx.x & 15, L);
  if (!force && n > 0) v3_repair_rows<NTB, V3_WGW>(in, out, total_steps, vp, ax, in_base, out_lo, S, L, 4 * V3_WGW, 4 * wv, n);
  __threadfence(); __syncthreads();
  if (wv == 0) v3_seq_walk<NTB, V3_WGW>(in, out, total_steps, vp, ax, in_base, out_lo, S, L, force);
}

}  // namespace dvbt
