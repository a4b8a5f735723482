// k_txblocks.hpp -- the transmit blocks of gr-dvbt one at a time (dvbt_txblocks.inc), one launch per call each.
//
//   txb_dispersal_kernel      energy_dispersal: sync bytes rewritten, bytes 1..187 XOR the PRBS of their place in the 8-packet group
//   txb_rs_enc_kernel         reed_solomon_enc: RS(204,188) parity, one lane per packet (the remainder register of tx_outer_kernel)
//   txb_conv_int_kernel       convolutional_interleaver: out[t] = x[t - I M (t mod I)], the last (I-1) M I input bytes carried on the device
//   txb_inner_coder_kernel    inner_coder: every output byte (one m-bit symbol) from 7-bit windows of the info stream, the last input byte carried
//   txb_bit_int_kernel        bit_inner_interleaver (non-hierarchical): bit e of output word w = bit kinv[e] of input word H_e(w) of its 126-word block
//   txb_map_kernel            dvbt_map: label -> constellation point
//   txb_refsig_kernel<N>      reference_signals: one workgroup per OFDM symbol, the symbol built in LDS, written out in frequency order
//
// Byte streams are read byte by byte (their offsets in a flowgraph buffer are arbitrary); every output is written with 4-, 8- or 16-byte
// vector stores, so the entries require outputs aligned to that.  Lanes of a wavefront touch consecutive words in every global access.
#pragma once
#include "k_tx.hpp"

namespace dvbt {

constexpr int TXB_THREADS = 256;

// ---------------------------------------------------------------- energy_dispersal (energy_dispersal_impl.cc:106-141)
// in: the call's packets from the sync byte on (any alignment); out: npk * 188 bytes (npk a multiple of 8), 16-byte aligned.
// Lane i writes output bytes [16 i, 16 i + 16): packet p = b / 188 of the call, g = p mod 8 its place in the group.
__global__ __launch_bounds__(TXB_THREADS) void txb_dispersal_kernel(const uint8_t *__restrict__ in, long long nvec,
                                                                   const uint8_t *__restrict__ prbs, uint4 *__restrict__ out)
{
  const long long i = (long long)blockIdx.x * TXB_THREADS + threadIdx.x;
  if (i >= nvec) return;
  uint32_t w[4];
  for (int j = 0; j < 4; j++) {
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
      const long long o = i * 16 + j * 4 + b;
      const long long p = o / 188;
      const int k = (int)(o - p * 188), g = (int)(p & 7);
      const uint8_t d = k == 0 ? (g == 0 ? 0xB8 : 0x47) : (uint8_t)(in[o] ^ prbs[g * 188 + k]);
      v |= (uint32_t)d << (8 * b);
    }
    w[j] = v;
  }
  out[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------- reed_solomon_enc (reed_solomon_enc_impl.cc:66-99, reed_solomon.cc:216-244)
// in: npk packets of 188 bytes, out: npk packets of 204 bytes, both 4-byte aligned.  Lane = packet; the remainder register is 16 bytes,
// one step is  fb = d ^ reg[0];  reg = (reg >> 8 bits) ^ enc_tab[fb]  (enc_tab: rs_encoder_rows).
__global__ __launch_bounds__(TX_OUTER_PK) void txb_rs_enc_kernel(const uint8_t *__restrict__ in, long long npk, const uint4 *__restrict__ enc_tab,
                                                                uint8_t *__restrict__ dst)
{
  __shared__ uint4 tab[256];
  __shared__ __attribute__((aligned(16))) uint32_t pk[TX_OUTER_PK * 47];
  __shared__ uint4 par[TX_OUTER_PK];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * TX_OUTER_PK;
  const int n = (int)(npk - p0 < TX_OUTER_PK ? npk - p0 : TX_OUTER_PK);
  for (int i = tid; i < 256; i += TX_OUTER_PK) tab[i] = enc_tab[i];
  const uint32_t *src = (const uint32_t *)(in + p0 * 188);
  for (int i = tid; i < n * 47; i += TX_OUTER_PK) pk[i] = src[i];
  __syncthreads();
  if (tid < n) {
    const uint8_t *b = (const uint8_t *)pk + tid * 188;
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    for (int k = 0; k < 188; k++) {
      const uint4 t = tab[(b[k] ^ r0) & 0xff];
      r0 = ((r0 >> 8) | (r1 << 24)) ^ t.x; r1 = ((r1 >> 8) | (r2 << 24)) ^ t.y;
      r2 = ((r2 >> 8) | (r3 << 24)) ^ t.z; r3 = (r3 >> 8) ^ t.w;
    }
    par[tid] = make_uint4(r0, r1, r2, r3);
  }
  __syncthreads();
  uint32_t *out = (uint32_t *)(dst + p0 * 204);
  for (int i = tid; i < n * 51; i += TX_OUTER_PK) {
    const int p = i / 51, w = i - p * 51;
    const uint4 pr = par[p];
    out[i] = w < 47 ? pk[p * 47 + w] : (w == 47 ? pr.x : w == 48 ? pr.y : w == 49 ? pr.z : pr.w);
  }
}

// ---------------------------------------------------------------- convolutional_interleaver (convolutional_interleaver_impl.cc:73-82)
// Branch j = t mod I is a FIFO of M j bytes: out[t] = x[t - I M (t mod I)], x[< 0] from the history (the last H = (I-1) M I input bytes of
// the stream so far, zero at the start).  Lanes [0, nw) write output words (nbytes is a multiple of I * blocks; out 4-byte aligned); the
// lanes behind them write hist_out = the last H bytes of (hist_in ++ in), the next call's history (ping-pong: hist_in is not overwritten).
__global__ __launch_bounds__(TXB_THREADS) void txb_conv_int_kernel(const uint8_t *__restrict__ in, long long nbytes, int I, int IM,
                                                                  const uint8_t *__restrict__ hist_in, int H, uint8_t *__restrict__ hist_out,
                                                                  uint32_t *__restrict__ out)
{
  const long long nw = nbytes >> 2;
  const long long i = (long long)blockIdx.x * TXB_THREADS + threadIdx.x;
  if (i < nw) {
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
      const long long t = i * 4 + b;
      const long long s = t - (long long)IM * (int)(t % I);
      v |= (uint32_t)(s >= 0 ? in[s] : hist_in[H + s]) << (8 * b);
    }
    out[i] = v;
    return;
  }
  const long long j = i - nw;                       // history byte j: stream byte (nbytes - H + j) of (hist_in ++ in)
  if (j >= H) return;
  const long long s = nbytes - H + j;
  hist_out[j] = s >= 0 ? in[s] : hist_in[H + s];
}

// ---------------------------------------------------------------- inner_coder (inner_coder_impl.cc:33-121, :206-266)
struct TxbCoderParams {
  int m, k, n;
  uint8_t cmap[8];            // coded bit o of a puncture period: info bit (cmap >> 1) of the period, x (0) or y (1) output
};
// nsym output bytes (a multiple of 4; out 4-byte aligned) from nbytes input bytes (any alignment).  Info bit t of the call is bit 7 - (t mod 8)
// of in[t / 8]; bits in front of the call come from *prev_in, the last input byte of the stream so far (0 at the start: the encoder's zero
// register).  Lane 0 writes *prev_out, the next call's (ping-pong: prev_in is not overwritten).
__global__ __launch_bounds__(TXB_THREADS) void txb_inner_coder_kernel(const uint8_t *__restrict__ in, long long nbytes, long long nsym,
                                                                     TxbCoderParams p, const uint8_t *__restrict__ prev_in, uint8_t *__restrict__ prev_out,
                                                                     uint32_t *__restrict__ out)
{
  const long long i = (long long)blockIdx.x * TXB_THREADS + threadIdx.x;
  if (i == 0) *prev_out = nbytes > 0 ? in[nbytes - 1] : *prev_in;
  if (i >= (nsym >> 2)) return;
  const uint8_t prev = *prev_in;
  uint32_t v = 0;
  for (int b = 0; b < 4; b++) {
    const long long q = i * 4 + b;
    int s = 0;
    for (int e = 0; e < p.m; e++) {
      const long long c = q * p.m + e;                          // coded bit of the call
      const long long per = c / p.n;
      const int o = (int)(c - per * p.n);
      const long long t = per * p.k + (p.cmap[o] >> 1);         // info bit of the call
      const long long G = t + 2;                                // bit t - 6, counted from the MSB of the byte in front of the call
      const long long i0 = (G >> 3) - 1;                        // input byte holding it (-1: prev)
      const int sh = (int)(G & 7);
      const unsigned hi = i0 < 0 ? prev : in[i0];
      const unsigned lo = i0 + 1 < nbytes ? in[i0 + 1] : 0u;
      const unsigned win = ((((hi << 8) | lo)) >> (9 - sh)) & 0x7f;   // bit 6 = info bit t - 6 ... bit 0 = info bit t
      s = (s << 1) | (int)(__popc(win & ((p.cmap[o] & 1) ? 0x6Du : 0x4Fu)) & 1);   // G1 = 171, G2 = 133 (octal)
    }
    v |= (uint32_t)s << (8 * b);
  }
  out[i] = v;
}

// ---------------------------------------------------------------- bit_inner_interleaver, non-hierarchical (bit_inner_interleaver_impl.cc:120-184)
struct TxbBitParams {
  int m;
  uint8_t kinv[6];            // bit e of an output word comes from bit kinv[e] (MSB first) of its input word
  uint8_t hoff[6];            // row e reads input word (w + hoff[e]) mod 126 of the block (H_e(w))
};
// nbytes (a multiple of 126 and of 4; out 4-byte aligned)
__global__ __launch_bounds__(TXB_THREADS) void txb_bit_int_kernel(const uint8_t *__restrict__ in, long long nbytes, TxbBitParams p,
                                                                 uint32_t *__restrict__ out)
{
  const long long i = (long long)blockIdx.x * TXB_THREADS + threadIdx.x;
  if (i >= (nbytes >> 2)) return;
  uint32_t v = 0;
  for (int b = 0; b < 4; b++) {
    const long long q = i * 4 + b;
    const long long blk = q / 126;
    const int w = (int)(q - blk * 126);
    const uint8_t *src = in + blk * 126;
    int s = 0;
    for (int e = 0; e < p.m; e++) {
      int wi = w + p.hoff[e]; if (wi >= 126) wi -= 126;
      s = (s << 1) | ((src[wi] >> (p.m - 1 - p.kinv[e])) & 1);
    }
    v |= (uint32_t)s << (8 * b);
  }
  out[i] = v;
}

// ---------------------------------------------------------------- dvbt_map (dvbt_map_impl.cc:154-171)
// npairs label pairs -> npairs float4 (two cfloat each; out 16-byte aligned).  points: the 64-entry table of Tables::build_inner(gain).
__global__ __launch_bounds__(TXB_THREADS) void txb_map_kernel(const uint8_t *__restrict__ in, long long npairs, const float2 *__restrict__ points,
                                                             float4 *__restrict__ out)
{
  __shared__ float2 pt[64];
  if (threadIdx.x < 64) pt[threadIdx.x] = points[threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * TXB_THREADS + threadIdx.x;
  if (i >= npairs) return;
  const float2 a = pt[in[2 * i] & 63], b = pt[in[2 * i + 1] & 63];
  out[i] = make_float4(a.x, a.y, b.x, b.y);
}

// ---------------------------------------------------------------- reference_signals (reference_signals_impl.cc:1127-1186, :1289-1314)
struct TxbRefParams {
  int payload, zl, K, n_tps;
  long long S0;               // stream index of the call's first symbol
  int nsym;
  int npil[TX_NCLASS];
};
inline size_t txb_refsig_lds_bytes(int N) { return (size_t)N * sizeof(float2); }
// in: nsym items of payload cfloat; out: nsym items of N cfloat (16-byte aligned), zeros left and right, carriers c at zl + c.
template <int N>
__global__ __launch_bounds__(FFT_THREADS) void txb_refsig_kernel(const float2 *__restrict__ in, TxbRefParams p, TxTables T, float4 *__restrict__ out)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float2 *x = reinterpret_cast<float2 *>(smem_raw);
  const int tid = threadIdx.x, ls = blockIdx.x;
  if (ls >= p.nsym) return;
  const long long sg = p.S0 + ls;
  const int si = (int)(sg % 68), fi = (int)((sg / 68) & 3);
  const int cls = si == 0 ? 4 : (si & 3);
  for (int f = tid; f < N; f += FFT_THREADS) x[f] = make_float2(0.f, 0.f);
  __syncthreads();
  const float2 *src = in + (size_t)ls * p.payload;
  const uint16_t *pay = T.pay + (size_t)cls * p.payload;
  for (int q = tid; q < p.payload; q += FFT_THREADS) x[p.zl + pay[q]] = src[q];
  const uint16_t *pil = T.pil + (size_t)cls * TX_PIL_MAX;
  for (int i = tid; i < p.npil[cls]; i += FFT_THREADS) { const int c = pil[i]; x[p.zl + c] = make_float2(T.pref[c], 0.f); }
  const float sgn = T.tps_sign[fi * 68 + si];
  for (int i = tid; i < p.n_tps; i += FFT_THREADS) x[p.zl + T.tps[i]] = make_float2(sgn * T.tps_base[i], 0.f);
  __syncthreads();
  float4 *o = out + (size_t)ls * (N / 2);
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  for (int f = tid; f < N / 2; f += FFT_THREADS) o[f] = x4[f];
}

}  // namespace dvbt
