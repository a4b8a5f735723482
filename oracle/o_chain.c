/* o_chain.c -- the RX flowgraph of apps/dvbt_rx_demo*.grc, stage after stage, in the
 * "one item per general_work call" scheduling regime.
 * TEST INFRASTRUCTURE (see dvbt_oracle.h): used by tests/ as the checker and by bench.py's
 * cpu_baseline leg as the timed CPU port.
 *
 * A lost CP lock is followed the way the reference follows it (ofdm_sym_acquisition_impl.cc:545-559: half a window
 * consumed, full search again, sync_start on the next item): demod_reference_signals hunts the superframe start again
 * (demod_reference_signals_impl.cc:115-136) and drops the items in between; the superframe_start tag resets the Viterbi
 * decoder, which also drops the input bytes between its last whole block and the tag (viterbi_decoder_impl.cc:213-229:
 * every call handles whole blocks from the previous reset on, so the remainder in front of the tag is what is consumed
 * undecoded); the byte de-interleaver drops the bytes in front of the tag that do not fill a pair of items and keeps its
 * FIFOs (convolutional_deinterleaver_impl.cc:109-120); reed_solomon_dec goes on; energy_descramble re-searches the NSYNC
 * whenever the byte at its offset is not one at the start of a call (energy_descramble_impl.cc:121-141), in calls of the
 * minimum size (4 items visible, 2 consumed).  Returns the number of lock periods that delivered items, minus one
 * ("truncated" in the Python binding: 0 for a run with a single lock). */
#include "dvbt_oracle.h"
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double now(void)
{ struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

int o_rx_run(const o_cfg *c, const ocf *iq, size_t nsamples, float snr_db, int bsize,
             int rs_compat, o_rx_taps *t)
{ return o_rx_run_cut(c, iq, nsamples, snr_db, bsize, rs_compat, 0, t); }

/* sym_off > 0: the segment continues a cut stream (include/dvbt_hip.h: dvbt_rx_set_cut) whose first superframe start
 * lies sym_off OFDM symbols (a multiple of 272) before this segment's.  This is NOT reference behaviour (the reference
 * has no notion of a cut): it is the checker of the product's cut mode and of gr_dvbt_amd/multi.py -- block, delay and
 * item roundings are taken in stream coordinates, and the TS starts at the first NSYNC and runs in whole 8-packet
 * groups to the end of the RS words. */
int o_rx_run_cut(const o_cfg *c, const ocf *iq, size_t nsamples, float snr_db, int bsize,
                 int rs_compat, long long sym_off, o_rx_taps *t)
{
  const int N = c->N, cp = c->cp, P = c->payload;
  int truncated = 0;
  double t0;
  size_t max_sym = nsamples / (size_t)(N + cp) + 2;
  for (int i = 0; i < 10; i++) t->t_stage[i] = 0;
  t->acq_n = t->fft_n = t->eq_n = t->sym_n = t->vit_n = t->deint_n = t->rs_n = t->ts_n = 0;
  t->first_out_symbol = -1; t->n_acquired = 0; t->rs_fail = t->rs_corr = 0;

  /* ---- A1 acquisition */
  ocf *acq = malloc(sizeof(ocf) * (size_t)N * max_sym);
  unsigned char *sync_tag = calloc(max_sym, 1);
  size_t nacq = 0, pos = 0;
  {
    t0 = now();
    o_acq *a = o_acq_new(c, snr_db);
    int pending = 0;
    /* forecast :474-481 asks for 2N+cp; 16 more keeps the +-8 tracking window in range */
    while (pos + (size_t)(2 * N + cp) + 16 <= nsamples && nacq < max_sym) {
      int consumed, sync, cps; float eps;
      o_acq_set_avail(a, (long long)(nsamples - pos));
      int produced = o_acq_work_hist(a, iq + pos, (long long)pos, acq + nacq * (size_t)N, &consumed, &sync, &cps, &eps);
      if (sync) pending = 1;
      if (produced) {
        sync_tag[nacq] = (unsigned char)pending; pending = 0;
        if (t->cp_start && nacq < t->meta_cap) t->cp_start[nacq] = cps;
        if (t->epsilon && nacq < t->meta_cap) t->epsilon[nacq] = eps;
        if (t->call_pos && nacq < t->meta_cap) t->call_pos[nacq] = (long long)pos;
        if (t->sync_flag && nacq < t->meta_cap) t->sync_flag[nacq] = sync_tag[nacq];
        nacq++;
      }
      pos += (size_t)consumed;
    }
    o_acq_free(a);
    t->t_stage[0] = now() - t0;
  }
  t->n_acquired = (int)nacq;
  if (t->acq_out) { size_t n = nacq < t->acq_cap ? nacq : t->acq_cap; memcpy(t->acq_out, acq, sizeof(ocf) * N * n); t->acq_n = n; }

  /* ---- A2 FFT */
  ocf *fft = malloc(sizeof(ocf) * (size_t)N * (nacq + 1));
  t0 = now();
  for (size_t s = 0; s < nacq; s++) o_fft_forward_shift(N, acq + s * (size_t)N, fft + s * (size_t)N);
  t->t_stage[1] = now() - t0;
  free(acq);
  if (t->fft_out) { size_t n = nacq < t->fft_cap ? nacq : t->fft_cap; memcpy(t->fft_out, fft, sizeof(ocf) * N * n); t->fft_n = n; }

  /* ---- A3 demod (needs item j and j+1: forecast :88-94) */
  size_t nout = 0;
  enum { O_MAX_PERIODS = 64 };
  size_t per_start[O_MAX_PERIODS + 1]; int nper = 0;
  ocf *eq = malloc(sizeof(ocf) * (size_t)P * (nacq + 1));
  int *symidx = malloc(sizeof(int) * (nacq + 1));
  {
    t0 = now();
    o_demod *d = o_demod_new(c);
    for (size_t j = 0; j + 1 < nacq; j++) {
      int sf, si, info[8];
      int produced = o_demod_work(d, fft + j * (size_t)N, eq + nout * (size_t)P, sync_tag[j], &sf, &si, info);
      if (t->sym_index && j < t->meta_cap) t->sym_index[j] = si;
      if (t->freq_offset && j < t->meta_cap) t->freq_offset[j] = info[0];
      if (t->sf_flag && j < t->meta_cap) t->sf_flag[j] = (unsigned char)(sf ? 1 : (produced ? 2 : 0));
      if (sf) {
        if (t->first_out_symbol < 0) t->first_out_symbol = (int)j; else truncated++;
        if (nper < O_MAX_PERIODS) per_start[nper++] = nout;        /* output item at which this lock period starts */
      }
      if (produced) symidx[nout++] = si;
    }
    o_demod_free(d);
    t->t_stage[2] = now() - t0;
  }
  free(fft); free(sync_tag);
  if (t->eq_out) { size_t n = nout < t->eq_cap ? nout : t->eq_cap; memcpy(t->eq_out, eq, sizeof(ocf) * P * n); t->eq_n = n; }

  /* ---- A4..A6 demap, symbol de-interleave, bit de-interleave */
  unsigned char *b0 = malloc((size_t)P * (nout + 1)), *b1 = malloc((size_t)P * (nout + 1)), *b2 = malloc((size_t)P * (nout + 1));
  {
    ocf *points = malloc(sizeof(ocf) * c->csize); o_constellation(c, 1.0f, points);
    int *H = malloc(sizeof(int) * P); o_sym_H(c, H);
    t0 = now();
    o_demap(c, points, eq, b0, (size_t)P * nout);
    t->t_stage[3] = now() - t0; t0 = now();
    for (size_t s = 0; s < nout; s++) o_sym_interleave(c, H, b0 + s * P, b1 + s * P, symidx[s], 0);
    t->t_stage[4] = now() - t0; t0 = now();
    /* hierarchical modes: two outputs; port 0 (HP) is what the flowgraphs connect to the Viterbi decoder, which unpacks d_m bits of every byte whatever
     * the stream carries (viterbi_decoder_impl.cc:93,236-243: its config knows no priority streams) */
    if (c->hierarchy != O_NH) {
      unsigned char *lp = malloc((size_t)P * (nout + 1));
      o_bit_deinterleave_hier(c, b1, b2, lp, (size_t)P * nout);
      if (t->bitdeint_lp_out) { size_t n = nout < t->sym_cap ? nout : t->sym_cap; memcpy(t->bitdeint_lp_out, lp, (size_t)P * n); }
      free(lp);
    } else
    o_bit_deinterleave(c, b1, b2, (size_t)P * nout);
    t->t_stage[5] = now() - t0;
    free(points); free(H);
  }
  free(eq); free(symidx);
  {
    size_t n = nout < t->sym_cap ? nout : t->sym_cap;
    if (t->demap_out) memcpy(t->demap_out, b0, (size_t)P * n);
    if (t->symdeint_out) memcpy(t->symdeint_out, b1, (size_t)P * n);
    if (t->bitdeint_out) memcpy(t->bitdeint_out, b2, (size_t)P * n);
    t->sym_n = n;
  }
  free(b0); free(b1);

  /* ---- A7 Viterbi */
  size_t vit_cap = (size_t)P * nout * c->m * c->k / (8 * c->n) + 64;
  unsigned char *vit = malloc(vit_cap);
  t0 = now();
  const long long ibits = (long long)P * c->m * c->k / c->n;            /* decoded bits per OFDM symbol */
  const long long d_nsym = (long long)bsize * c->n / c->m;
  /* every lock period is a stream of its own for the decoder (reset at the superframe_start tag); what it delivers in front
   * of the next tag is cut to whole pairs of de-interleaver items (the tag realigns that block's input) */
  size_t nvit = 0;
  long long nb_g = 0;
  per_start[nper] = nout;
  for (int pi = 0; pi < nper; pi++) {
    const long long n_sym_p = (long long)(per_start[pi + 1] - per_start[pi]);
    const long long off_p = pi == 0 ? sym_off : 0;                   /* a cut stream's offset belongs to its first period */
    const long long nblocks_g = (off_p + n_sym_p) * P / d_nsym;      /* viterbi_decoder_impl.cc:198 in stream coordinates */
    long long nin_l = nblocks_g * d_nsym - off_p * P;
    if (nin_l < 0) nin_l = 0;
    size_t nv = o_viterbi_decode_n(c, b2 + per_start[pi] * (size_t)P, (size_t)nin_l, vit + nvit);
    nb_g = nblocks_g * (long long)c->k * bsize / 8 - o_vit_ntraceback(c->code_rate);
    if (nb_g < 0) nb_g = 0;
    if (pi + 1 < nper) nv = o_conv_deint_taken_before_tag(nv);          /* convolutional_deinterleaver_impl.cc:109-120 */
    nvit += nv;
  }
  if (nper > 1) nb_g = (long long)nvit;                              /* several periods: the item count below follows the concatenated stream */
  t->t_stage[6] = now() - t0;
  free(b2);
  if (t->vit_out) { size_t n = nvit < t->vit_cap ? nvit : t->vit_cap; memcpy(t->vit_out, vit, n); t->vit_n = n; }

  /* ---- A8 byte de-interleave: items of 12*136 bytes, output multiple of 2 (:55-61) */
  const long long items_g = (nb_g / 1632) & ~1ll;
  long long nwords_l = items_g * 8 - sym_off * ibits / (8 * 204);
  if (nwords_l < 0) nwords_l = 0;
  if ((size_t)nwords_l * 204 > nvit) nwords_l = (long long)(nvit / 204);   /* cannot happen; keeps the reads in bounds */
  size_t nitems = (size_t)nwords_l / 8;                  /* whole items (all of them unless the segment continues a cut stream) */
  const size_t nwords = (size_t)nwords_l;
  t->stream_rs_items = items_g; t->ts_first_packet = 0;
  unsigned char *dei = malloc(nwords * 204 + 1);
  t0 = now();
  o_conv_deinterleave(vit, dei, nwords * 204);
  t->t_stage[7] = now() - t0;
  free(vit);
  if (t->deint_out) { size_t n = nwords * 204 < t->deint_cap ? nwords * 204 : t->deint_cap; memcpy(t->deint_out, dei, n); t->deint_n = n; }

  /* ---- A9 RS */
  unsigned char *rso = malloc(nwords * 188 + 1);
  {
    o_rs rs; o_rs_init(&rs);
    t0 = now();
    o_rs_dec_block(&rs, dei, rso, nwords, rs_compat, &t->rs_fail, &t->rs_corr);
    t->t_stage[8] = now() - t0;
  }
  free(dei);
  if (t->rs_out) { size_t n = nwords * 188 < t->rs_cap ? nwords * 188 : t->rs_cap; memcpy(t->rs_out, rso, n); t->rs_n = n; }

  /* ---- next: energy descramble */
  if (t->ts_out) {
    unsigned char *tso = malloc(nwords * 188 + 1);
    t0 = now();
    size_t n;
    if (sym_off > 0) {
      size_t q = 0;
      while (q < nwords && rso[q * 188] != 0xB8) q++;
      n = q < nwords ? o_energy_descramble_groups(rso + q * 188, (nwords - q) / 8, tso) : 0;
      t->ts_first_packet = (long long)q;
    } else {
      size_t q = 0;                                       /* what o_energy_descramble locks on: the first NSYNC, 16 packets at a time */
      while (q < nitems * 8 && rso[q * 188] != 0xB8) q++;
      t->ts_first_packet = (long long)q;
      n = o_energy_descramble(rso, nitems, tso);
    }
    t->t_stage[9] = now() - t0;
    if (n > t->ts_cap) n = t->ts_cap;
    memcpy(t->ts_out, tso, n); t->ts_n = n;
    free(tso);
  }
  free(rso);
  return truncated;
}
