// k_tx.hpp -- the DVB-T modulator (transport stream -> OFDM baseband) as two launches per call.
//
//   tx_outer_kernel        energy dispersal + RS(204,188) parity, one lane per packet; one extra workgroup carries the RS history
//                          of the previous call to the front of this call's buffer
//   tx_symbol_kernel<N>    one workgroup per OFDM symbol: Forney gather, convolutional encoder + puncturing, bit and symbol
//                          interleavers, mapping, pilots and TPS, inverse FFT, cyclic prefix, scale
//
// Each symbol is independent once its place in the stream is known: its info bits are bits [s ibits, (s+1) ibits) of the byte-
// interleaved stream, whose byte i is rs[i - 204 (i mod 12)] (zero before the stream start; convolutional_interleaver_impl.cc:73-82),
// and the encoder's state is the 6 bits in front of them (inner_coder_impl.cc:33-48).  Every symbol starts at puncture phase 0
// because ibits is a whole number of puncture periods.  Reference chain: apps/dvbt_tx_demo*.grc.
#pragma once
#include <stdint.h>
#include "k_fft.hpp"

namespace dvbt {

constexpr int TX_OUTER_PK = 128;          // packets (= lanes) per workgroup of tx_outer_kernel
constexpr int TX_NCLASS = 5;              // carrier classes: symbol_index mod 4, plus symbol_index == 0 (see dvbt_tx.inc: tx_carrier_classes)
constexpr int TX_PIL_MAX = 1024;          // pilot carriers per class (8k: 568 + 1 scattered, 177 continual)

// ---------------------------------------------------------------- outer coder
// blocks [0, nblk): TX_OUTER_PK packets each.  TS packets -> dst[hist + 204 p ...]: byte 0 = 0xB8 for the first packet of every
// group of 8 (counted from the start of the whole TS: group phase g = (pk0 + p) mod 8), 0x47 otherwise; bytes 1..187 XOR the
// PRBS (energy_dispersal_impl.cc:106-141); then the 16 parity bytes of RS(255,239) shortened by 51 (reed_solomon.cc:216-244): the
// remainder register is 16 bytes, one step is  fb = d ^ reg[0];  reg = (reg >> 8 bits) ^ enc_tab[fb].
// block nblk: dst[0, hist) = prev[prev_len - hist, prev_len), the last `hist` RS bytes of the stream so far.
__global__ __launch_bounds__(TX_OUTER_PK) void tx_outer_kernel(const uint8_t *__restrict__ ts, long long npk, long long pk0,
                                                               const uint8_t *__restrict__ prbs, const uint4 *__restrict__ enc_tab,
                                                               const uint8_t *__restrict__ prev, long long prev_len, int hist,
                                                               uint8_t *__restrict__ dst)
{
  __shared__ uint4 tab[256];
  __shared__ uint8_t seq[1504];
  __shared__ __attribute__((aligned(16))) uint32_t pk[TX_OUTER_PK * 47];      // the workgroup's packets, dispersed in place
  __shared__ uint4 par[TX_OUTER_PK];
  const int tid = threadIdx.x;
  const long long nblk = (npk + TX_OUTER_PK - 1) / TX_OUTER_PK;
  if ((long long)blockIdx.x == nblk) {                                          // history of the previous call (hist and prev_len are multiples of 4)
    const uint32_t *src = (const uint32_t *)(prev + prev_len - hist);
    for (int i = tid; i < hist / 4; i += TX_OUTER_PK) ((uint32_t *)dst)[i] = src[i];
    return;
  }
  const long long p0 = (long long)blockIdx.x * TX_OUTER_PK;
  const int n = (int)(npk - p0 < TX_OUTER_PK ? npk - p0 : TX_OUTER_PK);
  for (int i = tid; i < 256; i += TX_OUTER_PK) tab[i] = enc_tab[i];
  for (int i = tid; i < 1504; i += TX_OUTER_PK) seq[i] = prbs[i];
  const uint32_t *src = (const uint32_t *)(ts + p0 * 188);
  for (int i = tid; i < n * 47; i += TX_OUTER_PK) pk[i] = src[i];
  __syncthreads();
  if (tid < n) {
    uint8_t *b = (uint8_t *)pk + tid * 188;
    const int g = (int)((pk0 + p0 + tid) & 7);
    const uint8_t *q = seq + g * 188;
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;                                  // reg[0..15], little-endian: reg[0] = low byte of r0
    for (int k = 0; k < 188; k++) {
      const uint8_t d = k == 0 ? (g == 0 ? 0xB8 : 0x47) : (uint8_t)(b[k] ^ q[k]);
      b[k] = d;
      const uint4 t = tab[(d ^ r0) & 0xff];
      r0 = ((r0 >> 8) | (r1 << 24)) ^ t.x; r1 = ((r1 >> 8) | (r2 << 24)) ^ t.y;
      r2 = ((r2 >> 8) | (r3 << 24)) ^ t.z; r3 = (r3 >> 8) ^ t.w;
    }
    par[tid] = make_uint4(r0, r1, r2, r3);
  }
  __syncthreads();
  uint32_t *out = (uint32_t *)(dst + hist + p0 * 204);
  for (int i = tid; i < n * 51; i += TX_OUTER_PK) {                           // 204 bytes = 47 data words + 4 parity words per packet
    const int p = i / 51, w = i - p * 51;
    const uint4 pr = par[p];
    out[i] = w < 47 ? pk[p * 47 + w] : (w == 47 ? pr.x : w == 48 ? pr.y : w == 49 ? pr.z : pr.w);
  }
}

// ---------------------------------------------------------------- symbol kernel
struct TxSymParams {
  int N, cp, payload, m, k, n, zl, K, n_tps;
  long long ibits;
  long long S0;               // stream index of the call's first symbol
  long long base;             // stream index of the RS byte at rs[0]
  long long rs_len;           // bytes valid in rs
  int nsym;
  float scale;
  int npil[TX_NCLASS];
  uint8_t cmap[8];            // coded bit o of a puncture period: info bit (cmap >> 1) of the period, x (0) or y (1) output
  uint8_t kinv[6];            // bit interleaver: bit e of an output word comes from bit kinv[e] (MSB first) of its input word
  uint8_t hoff[6];            // bit interleaver: row e reads input word (w + hoff[e]) mod 126 of the block (H_e(w))
  uint32_t nmagic;            // ceil(2^32 / n): c / n = umulhi(c, nmagic) for every coded bit index c < 2^16
};
struct TxTables {
  const float2 *tw; const uint16_t *H, *Hinv; const float2 *points;
  const uint16_t *pay;        // [TX_NCLASS][payload] payload carriers, ascending
  const uint16_t *pil;        // [TX_NCLASS][TX_PIL_MAX] continual + scattered pilot carriers
  const float *pref;          // [K] pilot value +-4/3
  const uint16_t *tps;        // [n_tps] TPS carriers
  const float *tps_base;      // [n_tps] 2 (0.5 - w_k)
  const float *tps_sign;      // [4][68] (-1)^(tps_f[1] + .. + tps_f[s])
};

// the dynamic LDS of tx_symbol_kernel: the FFT's workspace, then the carrier labels
inline size_t tx_symbol_lds_bytes(int N, int payload) { return fft_lds_bytes(N) + (size_t)payload + 16; }

// the inverse DFT through the forward one: swap(FFT(swap(X))) = IFFT(X) unnormalised (swap(z) = i conj(z)), exact in the swaps.
template <int N>
__global__ __launch_bounds__(FFT_THREADS) void tx_symbol_kernel(const uint8_t *__restrict__ rs, TxSymParams p, TxTables T,
                                                                float2 *__restrict__ out, float2 *__restrict__ carriers)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const FftWork w = fft_work(smem_raw, N);
  float2 *const x = w.x;
  uint8_t *word = w.end;                                        // [payload] symbol-interleaved carrier labels
  uint8_t *il = smem_raw;                                       // the symbol's interleaved bytes (aliases x until the carriers are placed)
  const int tid = threadIdx.x, ls = blockIdx.x;
  if (ls >= p.nsym) return;
  const long long sg = p.S0 + ls;
  const int si = (int)(sg % 68), fi = (int)((sg / 68) & 3);
  fft_work_fill(w, N, T.tw, tid);

  // gather: interleaved bytes gb0 .. last, gb0 one byte in front of the first info bit (the encoder's 6-bit history)
  const long long Bg = sg * p.ibits;
  const long long gb0 = (Bg >> 3) - 1;
  const int nA = (int)(((Bg + p.ibits - 1) >> 3) - gb0 + 1);
  for (int i = tid; i <= nA; i += FFT_THREADS) {
    const long long gi = gb0 + i;
    uint8_t v = 0;
    if (gi >= 0 && i < nA) {
      const long long j = gi - 204 * (gi % 12) - p.base;      // convolutional_interleaver: branch gi mod 12 delays by 17 (gi mod 12) x 12 bytes
      if (gi - 204 * (gi % 12) >= 0 && j >= 0 && j < p.rs_len) v = rs[j];
    }
    il[i] = v;                                                  // il[nA] = 0: the window read below may touch it
  }
  __syncthreads();

  // encode + puncture + pack m bits + bit interleaver + symbol interleaver: lane q builds output word q of the bit interleaver
  const int m = p.m, k = p.k, n = p.n;
  const bool odd = si & 1;
  for (int q = tid; q < p.payload; q += FFT_THREADS) {
    const int blk = q / 126, wq = q - blk * 126;
    int v = 0;
    for (int e = 0; e < m; e++) {
      int wi = wq + p.hoff[e]; if (wi >= 126) wi -= 126;
      const int c = m * (blk * 126 + wi) + p.kinv[e];           // coded bit of the symbol
      const int per = (int)__umulhi((unsigned)c, p.nmagic), o = c - per * n;
      const int t = per * k + (p.cmap[o] >> 1);                 // info bit of the symbol
      const int G = (int)(Bg & 7) + 2 + t;                      // position of info bit t - 6 in il[], counted from the MSB of il[0] (bit 8 gb0 of the stream)
      const int i0 = G >> 3, sh = G & 7;
      const unsigned w16 = ((unsigned)il[i0] << 8) | il[i0 + 1];
      const unsigned win = (w16 >> (9 - sh)) & 0x7f;             // bit 6 = info bit t - 6 ... bit 0 = info bit t
      const unsigned bit = __popc(win & ((p.cmap[o] & 1) ? 0x6Du : 0x4Fu)) & 1;   // G1 = 171, G2 = 133 (octal)
      v = (v << 1) | (int)bit;
    }
    word[odd ? T.Hinv[q] : T.H[q]] = (uint8_t)v;                 // symbol_inner_interleaver_impl.cc:182-195
  }
  __syncthreads();

  // carriers into the IFFT input: carrier c lands at frequency index f = zl + c, IFFT bin (f + N/2) mod N (shift=True)
  const int cls = si == 0 ? 4 : (si & 3);
  const int K1 = p.zl, K2 = p.zl + p.K;
  for (int f = tid; f < N; f += FFT_THREADS)
    if (f < K1 || f >= K2) x[fpad((f + N / 2) & (N - 1))] = make_float2(0.f, 0.f);
  const uint16_t *pay = T.pay + (size_t)cls * p.payload;
  for (int q = tid; q < p.payload; q += FFT_THREADS)
    x[fpad((p.zl + pay[q] + N / 2) & (N - 1))] = cswap(T.points[word[q]]);
  const uint16_t *pil = T.pil + (size_t)cls * TX_PIL_MAX;
  for (int i = tid; i < p.npil[cls]; i += FFT_THREADS) {
    const int c = pil[i];
    x[fpad((p.zl + c + N / 2) & (N - 1))] = make_float2(0.f, T.pref[c]);
  }
  const float sgn = T.tps_sign[fi * 68 + si];
  for (int i = tid; i < p.n_tps; i += FFT_THREADS)
    x[fpad((p.zl + T.tps[i] + N / 2) & (N - 1))] = make_float2(0.f, sgn * T.tps_base[i]);
  __syncthreads();
  if (carriers) {
    float2 *cr = carriers + (size_t)ls * N;
    for (int f = tid; f < N; f += FFT_THREADS) cr[f] = cswap(x[fpad((f + N / 2) & (N - 1))]);
    __syncthreads();                                            // the FFT's first pass overwrites x in place
  }

  fft_dif_lds(w, N, tid);

  // cyclic prefix first, then the body; time sample t = swap(FFT output bin t)
  const int cp = p.cp;
  float2 *o = out + (size_t)ls * (N + cp);
  const float sc = p.scale;
  for (int j = tid; j < N + cp; j += FFT_THREADS) {
    const int t = j < cp ? N - cp + j : j - cp;
    const float2 v = x[fpad(fft_pos_of_bin(t, N))];
    o[j] = make_float2(sc * v.y, sc * v.x);
  }
}

}  // namespace dvbt
