// The index arithmetic of gr_dvbt_amd/csrc/k_fft.hpp on the CPU (tests/test_fft_index_host.py builds this with g++ and runs it; the header's device part is not compiled and no HIP runtime call is made).
// For every size the dvbt_fft block takes:
//   fft_pos_of_bin(., N) is a permutation of 0 .. N - 1, and it is the digit reversal over the pass radices of fft_dif_lds, restated here independently:
//     the radices by the rule "16 while the span allows, then 4 and/or 2", position p = digits d_0 d_1 .. (most significant first, radix r_i) holds the bin
//     k = d_0 + r_0 d_1 + r_0 r_1 d_2 + ...;
//   fpad is strictly increasing on 0 .. N - 1 and the padded image fits N + N / 32 entries;
//   fft_lds_bytes(N) is the padded image (N + N / 32 = fpad(N - 1) + 2 entries), the coarse table (max(N / 128, 1)) and 128 fine entries, 8 bytes each.
#include <cstdio>
#include <vector>
#include "k_fft.hpp"

static std::vector<int> radices(int N)
{
  std::vector<int> r;
  int L = N;
  while (L >= 16) { r.push_back(16); L /= 16; }
  if (L >= 4) { r.push_back(4); L /= 4; }
  if (L == 2) r.push_back(2);
  return r;
}

int main()
{
  int errors = 0, sizes = 0;
  for (int N = 64; N <= 8192; N *= 2, sizes++) {
    const std::vector<int> rad = radices(N);
    std::vector<int> pos_of_k(N, -1);
    for (int p = 0; p < N; p++) {
      int span = N, weight = 1, k = 0;
      for (int r : rad) { span /= r; const int dgt = (p / span) % r; k += dgt * weight; weight *= r; }
      pos_of_k[k] = p;
    }
    std::vector<int> seen(N, 0);
    int e = 0;
    for (int k = 0; k < N; k++) {
      const int p = dvbt::fft_pos_of_bin(k, N);
      if (p < 0 || p >= N || seen[p]++) { e++; continue; }             // a permutation
      if (p != pos_of_k[k]) e++;                                         // the digit reversal
    }
    for (int a = 1; a < N; a++) if (dvbt::fpad(a) <= dvbt::fpad(a - 1)) e++;
    if (dvbt::fpad(0) != 0 || dvbt::fpad(N - 1) + 1 > N + N / 32) e++;
    const int nc = N / 128 > 1 ? N / 128 : 1;
    if (dvbt::fft_lds_bytes(N) != (size_t)(dvbt::fpad(N - 1) + 2 + nc + 128) * 8) e++;
    printf("N %d: radices", N);
    for (int r : rad) printf(" %d", r);
    printf(", %zu bytes, %d errors\n", dvbt::fft_lds_bytes(N), e);
    errors += e;
  }
  printf("%d sizes, %d errors\n", sizes, errors);
  return errors ? 1 : 0;
}
