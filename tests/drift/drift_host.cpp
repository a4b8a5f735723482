// CPU check of gr_dvbt_amd/csrc/k_drift.hpp (the closed form of the reference's float phase accumulator) against the literal accumulator
// (ofdm_sym_acquisition_impl.cc:285-309 restated: float phase, double increment, one addition per sample, float wrap constants).
// usage: drift_host N cp nsym eps jitter seed [options]  ->  prints: literal_wander sequential_residual parallel_residual parallel_entry_error
//        (and on stderr: how far the last two rounds of the fixed point were apart, as a phase, and whether the recurrence was taken)
// options:
//   --eps-file FILE   the epsilon of every call from a text file (one value per line, at least nsym) instead of the generator; sw still from the seed
//   --mixed           increments of both signs: epsilon uniform in +-1.7 jitter around ZERO (eps is ignored) -- for the block path, which takes any increment
//   --sw-out K        the switch position of call K lies outside its call (N + cp + 5): the literal accumulator then keeps incA[K] through the whole call
//   --dump FILE       the literal accumulator only (neither the closed form nor the replay of the kernels' scheme is run: they are outside their domain for
//                     mixed signs); prints literal_wander and writes FILE: int32 N, cp, nsym, nb | int32 sw[nsym] | double incA[nsym] | double incB[nsym] |
//                     float entry[nsym] (the accumulator's value at every call entry) | double lit[nsym][nb] (the deviation at the steps 32 k + 17)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <cmath>
#include <vector>
#include <algorithm>
#include "../../gr_dvbt_amd/csrc/k_drift_math.hpp"
using namespace dvbt;

static double wrapd(double x) { x = fmod(x + M_PI, 2 * M_PI); if (x < 0) x += 2 * M_PI; return x - M_PI; }

int main(int argc, char **argv)
{
  if (argc < 7) return 2;
  const int N = atoi(argv[1]), cp = atoi(argv[2]), nsym = atoi(argv[3]), L = N + cp;
  const double eps0 = atof(argv[4]), jit = atof(argv[5]); unsigned seed = (unsigned)atoi(argv[6]);
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xffffff) / 16777216.0 - 0.5; };
  const char *dump = nullptr, *eps_file = nullptr; bool mixed = false; int sw_out = -1;
  for (int i = 7; i < argc; i++) {
    if (!strcmp(argv[i], "--mixed")) mixed = true;
    else if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else if (!strcmp(argv[i], "--eps-file") && i + 1 < argc) eps_file = argv[++i];
    else if (!strcmp(argv[i], "--sw-out") && i + 1 < argc) sw_out = atoi(argv[++i]);
    else return 2;
  }
  if (nsym < 1 || N < 32 || cp < 1) return 2;
  std::vector<float> eps(nsym + 2); std::vector<int> sw(nsym);
  for (auto &e : eps) e = (float)((mixed ? 0.0 : eps0) + jit * 3.4 * rnd());
  for (auto &w : sw) w = cp - 1 + (int)(20 * rnd());
  if (eps_file) {
    std::ifstream f(eps_file); double v; int n = 0;
    while (n < nsym && (f >> v)) eps[n++] = (float)v;
    if (n < nsym) { fprintf(stderr, "drift_host: %s holds %d values, %d needed\n", eps_file, n, nsym); return 2; }
  }
  if (sw_out >= 0 && sw_out < nsym) sw[sw_out] = L + 5;
  std::vector<double> incA(nsym), incB(nsym);
  for (int s = 0; s < nsym; s++) { incA[s] = s == 0 ? 0.0 : -(double)eps[s - 1] / N; incB[s] = -(double)eps[s] / N; }
  // ---- literal accumulator: deviation from the exact line at the steps 32 k + 17 of every call, and the phase at every call entry
  const int nb = N / 32;
  std::vector<double> lit((size_t)nsym * nb), lit_entry(nsym), ex_entry(nsym);
  {
    float ph = 0.f; double ex = 0.0;
    for (int s = 0; s < nsym; s++) {
      lit_entry[s] = ph; ex_entry[s] = ex;
      double inc = incA[s];
      for (int i = 0; i < L; i++) {
        if (i == sw[s]) inc = incB[s];
        ph = (float)((double)ph + inc); ex += inc;
        while (ph > (float)M_PI) ph -= (float)(2.0 * M_PI);
        while (ph < (float)(-M_PI)) ph += (float)(2.0 * M_PI);
        if (i < N && (i & 31) == 16) lit[(size_t)s * nb + (i >> 5)] = wrapd(wrapd((double)ph - ex) - wrapd(lit_entry[s] - ex_entry[s]));
      }
    }
  }
  if (dump) {
    double worst = 0; for (double v : lit) worst = std::max(worst, fabs(v));
    FILE *f = fopen(dump, "wb");
    if (!f) return 3;
    const int hdr[4] = {N, cp, nsym, nb};
    std::vector<float> ent_f(nsym); for (int s = 0; s < nsym; s++) ent_f[s] = (float)lit_entry[s];
    bool ok = fwrite(hdr, sizeof hdr, 1, f) == 1 && fwrite(sw.data(), sizeof(int), nsym, f) == (size_t)nsym && fwrite(incA.data(), sizeof(double), nsym, f) == (size_t)nsym &&
              fwrite(incB.data(), sizeof(double), nsym, f) == (size_t)nsym && fwrite(ent_f.data(), sizeof(float), nsym, f) == (size_t)nsym &&
              fwrite(lit.data(), sizeof(double), lit.size(), f) == lit.size();
    ok = fclose(f) == 0 && ok;
    printf("%.3e\n", worst);
    return ok ? 0 : 3;
  }
  auto delta_of = [&](int s, double ent, std::vector<double> &out) {   // what drift_table_kernel computes
    const double phsw = drift_advance(incA[s], ent, sw[s]);
    for (int k = 0; k < nb; k++) {
      const int n = 32 * k + 17;
      double phi, exact;
      if (n <= sw[s]) { phi = drift_advance(incA[s], ent, n); exact = n * incA[s]; }
      else { phi = drift_advance(incB[s], phsw, n - sw[s]); exact = sw[s] * incA[s] + (n - sw[s]) * incB[s]; }
      out[k] = (phi - ent) - exact;
    }
  };
  // ---- sequential use of the closed form (exact recurrence over the calls)
  double worst_lit = 0, worst_seq = 0, worst_par = 0, worst_ent = 0;
  std::vector<double> d(nb);
  {
    double ent = 0.0;
    for (int s = 0; s < nsym; s++) {
      delta_of(s, ent, d);
      for (int k = 0; k < nb; k++) { worst_seq = std::max(worst_seq, fabs(d[k] - lit[(size_t)s * nb + k])); worst_lit = std::max(worst_lit, fabs(lit[(size_t)s * nb + k])); }
      ent = drift_advance(incB[s], drift_advance(incA[s], ent, sw[s]), L - sw[s]);
    }
  }
  // ---- the scheme of the kernels: tables per run, three rounds of (evaluate d_r at the previous iterate, prefix sum); the last two rounds compared as phases
  //      (drift_round_kernel<2>); where they differ, the recurrence over the runs on the same tables (drift_seq_kernel)
  {
    const bool neg = incB[0] < 0;
    std::vector<DriftTab> tab(nsym);
    for (int r = 0; r < nsym; r++) drift_build(incB[r], tab[r].q, tab[r].tc);
    std::vector<double> ex_run(nsym), S(nsym, 0.0), S_old(nsym, 0.0), dd(nsym, 0.0), phi_seq;
    for (int r = 0; r < nsym; r++) ex_run[r] = ex_entry[r] + sw[r] * incA[r];
    const double A0 = drift_T(tab[0].q, tab[0].tc, neg, 0.0);
    auto phi_run = [&](int r, bool first) {
      if (r == 0) return 0.0;
      if (!phi_seq.empty()) return phi_seq[r];
      if (first) return ex_run[r];
      return drift_Tinv(tab[r - 1].q, tab[r - 1].tc, neg, A0 + ((double)r * L + sw[r] - sw[0]) - S[r - 1]);
    };
    for (int it = 0; it < 3; it++) {
      for (int r = 1; r < nsym; r++) { const double phi = phi_run(r, it == 0); dd[r] = drift_T(tab[r - 1].q, tab[r - 1].tc, neg, phi) - drift_T(tab[r].q, tab[r].tc, neg, phi); }
      S_old = S;
      double acc = 0.0; for (int r = 0; r < nsym; r++) { acc += dd[r]; S[r] = acc; }
    }
    double apart = 0.0, A = 0.0;
    for (int r = 1; r < nsym; r++) A += drift_jump(tab[r - 1].q, tab[r].q);
    for (int r = 0; r < nsym; r++) apart = std::max(apart, fabs(S[r] - S_old[r]) * 1.25 * fabs(incB[r]));
    const bool seq = apart * (1.0 + 1.5 * A) > DRIFT_SETTLED;
    if (seq) {
      phi_seq.assign(nsym, 0.0);
      for (int r = 0; r + 1 < nsym; r++)
        phi_seq[r + 1] = drift_Tinv(tab[r].q, tab[r].tc, neg, drift_T(tab[r].q, tab[r].tc, neg, phi_seq[r]) + (double)(L + sw[r + 1] - sw[r]));
    }
    fprintf(stderr, "rounds apart %.3e rad, jumps %.3e, recurrence %d\n", apart, A, seq ? 1 : 0);
    for (int s = 0; s < nsym; s++) {
      double ent = 0.0;
      if (s > 0) { const double phr = phi_run(s - 1, false); ent = drift_Tinv(tab[s - 1].q, tab[s - 1].tc, neg, drift_T(tab[s - 1].q, tab[s - 1].tc, neg, phr) + (L - sw[s - 1])); }
      worst_ent = std::max(worst_ent, fabs(wrapd(ent - lit_entry[s])));
      delta_of(s, ent, d);
      for (int k = 0; k < nb; k++) worst_par = std::max(worst_par, fabs(d[k] - lit[(size_t)s * nb + k]));
    }
  }
  printf("%.3e %.3e %.3e %.3e\n", worst_lit, worst_seq, worst_par, worst_ent);
  return 0;
}
