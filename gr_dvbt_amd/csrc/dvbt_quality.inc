// dvbt_quality.inc -- dvbt_rx_enable_quality / dvbt_rx_quality (include/dvbt_hip.h): a pass of its own over what a finished segment left on the device
// (k_quality.hpp).  Nothing here is part of enqueue, of a captured graph or of the streaming entry; with quality never enabled every launch of the chain
// is the one it was.  Included from dvbt_hip.hip.

static int quality_buffers(dvbt_rx *h)
{
  if (!h->q_sym) HIPCHK(h->q_sym.alloc((size_t)h->max_calls + 1));
  if (!h->q_mer) HIPCHK(h->q_mer.alloc(2));
  if (!h->q_cnt) HIPCHK(h->q_cnt.alloc(4));
  return DVBT_OK;
}

extern "C" int dvbt_rx_enable_quality(dvbt_rx *h, int enable)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  if (h->pending) return fail(DVBT_ERR_STATE, "dvbt_rx_enable_quality: a segment is in flight (dvbt_rx_segment_finish first)");
  HIPCHK(hipSetDevice(h->prm.device));
  drop_graphs(h);
  if (enable) {
    // the equalised carriers alone: a non-null eq selects the symbol kernel's TAPS instantiation (as a soft-decision handle does); its other taps stay null
    if (!h->eq) { HIPCHK(h->eq.alloc((size_t)h->max_calls * h->d.payload)); h->q_eq_serial = h->seg_serial; }   // (no segment so far has written it)
    return quality_buffers(h);
  }
  // the debug taps (dvbt_rx_enable_taps: acq_tap stands for them) and the soft demapper keep eq for themselves
  if (!h->prm.soft_decision && !h->acq_tap) h->eq.reset();
  return DVBT_OK;
}

static unsigned quality_grid(long long items)
{
  long long g = (items + Q_THREADS - 1) / Q_THREADS;
  return (unsigned)(g < 1 ? 1 : g > (long long)Q_MAX_GRID ? (long long)Q_MAX_GRID : g);
}

// the measurement's launches on stream s; what == 0: all, 1..4: that kernel alone (dvbt_debug_quality_time).  Sizes of 0 launch nothing.
struct QualityPlan { long long mer_symbols = 0, first_out = 0, n_in = 0, n_vit_ch = 0, n_vit = 0, n_words = 0; };
static void quality_launch(dvbt_rx *h, hipStream_t s, const QualityPlan &q, int what)
{
  const int P = h->d.payload;
  if (q.mer_symbols > 0 && (what == 0 || what == 1))
    hipLaunchKernelGGL(quality_mer_kernel, dim3((unsigned)q.mer_symbols), dim3(Q_THREADS), 0, s, (const float2 *)(h->eq + (size_t)q.first_out * P),
                       (const uint8_t *)(h->labels + (size_t)q.first_out * P), (const float2 *)h->T.points, P, h->q_sym.get());
  if (q.mer_symbols > 0 && (what == 0 || what == 2))
    hipLaunchKernelGGL(quality_sum_kernel, dim3(1), dim3(Q_THREADS), 0, s, (const float2 *)h->q_sym, (int)q.mer_symbols, h->q_mer.get());
  if (q.n_vit_ch >= 2 && (what == 0 || what == 3))
    hipLaunchKernelGGL(quality_channel_kernel, dim3(quality_grid((q.n_vit_ch + 7) / 8)), dim3(Q_THREADS), 0, s, (const uint8_t *)h->bitdeint, q.n_in, (const uint8_t *)h->vit,
                       q.n_vit_ch, h->vp, h->q_cnt.get());
  if (q.n_words > 0 && (what == 0 || what == 4))
    hipLaunchKernelGGL(quality_rs_kernel, dim3(quality_grid(q.n_words * 47)), dim3(Q_THREADS), 0, s, (const uint8_t *)h->vit, q.n_vit, (const uint8_t *)h->rs_out, q.n_words,
                       h->q_cnt.get() + 2);
}

static int quality_plan(dvbt_rx *h, const char *who, QualityPlan &q, int &flags)
{
  if (h->d.hierarchy != 0) return fail(DVBT_ERR_INVALID, std::string(who) + ": hierarchical modes are not measured (the decoder's input is degenerate there)");
  if (h->prm.soft_decision) return fail(DVBT_ERR_STATE, std::string(who) + ": a soft-decision handle keeps neither labels nor the decoder's hard input");
  if (h->cut.stream_symbol_offset != 0 || h->cut.start_delay_symbols != 0 || h->cut.descr_call_phase != 0)
    return fail(DVBT_ERR_STATE, std::string(who) + ": the handle decodes a piece of a cut stream (dvbt_rx_set_cut)");
  if (h->pending) return fail(DVBT_ERR_STATE, std::string(who) + ": a segment is in flight (dvbt_rx_segment_finish first)");
  if (!h->have_last) return fail(DVBT_ERR_STATE, std::string(who) + ": no finished segment");
  const dvbt_rx_report &r = h->last;
  flags = 0;
  q = QualityPlan();
  const bool have_eq = h->eq && h->seg_serial > h->q_eq_serial;         // allocated, and a segment has run since
  if (!have_eq) flags |= 1;
  // the front-end buffers (eq, labels, the decoder's input) hold the last lock period alone: they describe the segment only when that period is the whole of it,
  // i.e. its decoded bytes are the segment's Viterbi stream from byte 0
  const bool one = r.n_lock_periods == 1 && r.first_out_symbol >= 0 && h->st_host->n_vit_bytes == r.n_viterbi_bytes;
  if (r.n_lock_periods > 1 || (r.n_lock_periods == 1 && !one)) flags |= 2;
  if (one) {
    q.first_out = r.first_out_symbol;
    if (have_eq) q.mer_symbols = r.n_out_symbols > 0 ? r.n_out_symbols : 0;
    q.n_in = (long long)(r.n_out_symbols > 0 ? r.n_out_symbols : 0) * h->d.payload;
    q.n_vit_ch = r.n_viterbi_bytes;
  }
  q.n_vit = r.n_viterbi_bytes;
  q.n_words = r.n_rs_bytes / 188;
  return DVBT_OK;
}

extern "C" int dvbt_rx_quality(dvbt_rx *h, dvbt_rx_quality_report *out)
{
  if (!h || !out) return fail(DVBT_ERR_INVALID, "null argument");
  QualityPlan q; int flags = 0;
  int r = quality_plan(h, "dvbt_rx_quality", q, flags); if (r) return r;
  HIPCHK(hipSetDevice(h->prm.device));
  if ((r = quality_buffers(h))) return r;
  hipStream_t s = h->own_stream;
  HIPCHK(hipMemsetAsync(h->q_mer, 0, 2 * sizeof(double), s));
  HIPCHK(hipMemsetAsync(h->q_cnt, 0, 4 * sizeof(unsigned long long), s));
  quality_launch(h, s, q, 0);
  HIPCHK(hipGetLastError());
  double mer[2]; unsigned long long cnt[4];
  HIPCHK(hipMemcpyAsync(mer, h->q_mer, sizeof mer, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(cnt, h->q_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  memset(out, 0, sizeof *out);
  if (q.mer_symbols > 0) { out->mer_carriers = q.mer_symbols * h->d.payload; out->mer_signal = mer[0]; out->mer_error = mer[1]; }
  if (q.n_vit_ch >= 2) { out->channel_bits = (int64_t)cnt[0]; out->channel_bit_errors = (int64_t)cnt[1]; }
  out->post_bits = 1504 * q.n_words; out->post_bit_errors = (int64_t)cnt[2];
  out->rs_fail_words = h->last.rs_fail_words; out->rs_corrected_symbols = h->last.rs_corrected_symbols; out->n_lock_periods = h->last.n_lock_periods;
  out->flags = flags;
  return DVBT_OK;
}

// measurement hook (tools/quality_bench.py): every kernel of dvbt_rx_quality alone on the finished segment's buffers, `warmup` launches and then `iters` timed ones
// between two HIP events each.  ms: [4][iters] (mer, sum, channel, rs; a kernel the segment gives nothing to do stays 0); bytes_read[4]: what each reads.
extern "C" int dvbt_debug_quality_time(dvbt_rx *h, int warmup, int iters, float *ms, int64_t *bytes_read)
{
  if (!h || !ms || !bytes_read || warmup < 0 || iters < 1 || iters > 1000) return fail(DVBT_ERR_INVALID, "null argument, or iters outside [1, 1000]");
  QualityPlan q; int flags = 0;
  int r = quality_plan(h, "dvbt_debug_quality_time", q, flags); if (r) return r;
  HIPCHK(hipSetDevice(h->prm.device));
  if ((r = quality_buffers(h))) return r;
  hipStream_t s = h->own_stream;
  Event a, b; HIPCHK(a.create()); HIPCHK(b.create());
  const long long P = h->d.payload;
  bytes_read[0] = q.mer_symbols * P * 9 + 512; bytes_read[1] = q.mer_symbols * 8;
  // the channel kernel reads the decoded bytes and the input bytes their steps' kept bits lie in
  bytes_read[2] = q.n_vit_ch >= 2 ? q.n_vit_ch + std::min(q.n_in, q.n_vit_ch * 8 * h->d.n / ((long long)h->d.k * h->d.m) + 1) : 0;
  bytes_read[3] = q.n_words * (188 + 188);
  const bool has[4] = {q.mer_symbols > 0, q.mer_symbols > 0, q.n_vit_ch >= 2, q.n_words > 0};
  for (int k = 0; k < 4; k++)
    for (int i = -warmup; i < iters; i++) {
      if (i >= 0) ms[k * iters + i] = 0.f;
      if (!has[k]) continue;
      HIPCHK(hipEventRecord(a, s));
      quality_launch(h, s, q, k + 1);
      HIPCHK(hipEventRecord(b, s));
      HIPCHK(hipEventSynchronize(b));
      float t = 0.f; HIPCHK(hipEventElapsedTime(&t, a, b));
      if (i >= 0) ms[k * iters + i] = t;
    }
  HIPCHK(hipGetLastError());
  return DVBT_OK;
}

// test hooks: upload, one kernel, download
extern "C" int dvbt_debug_quality_channel(int constellation, int code_rate, const uint8_t *in_host, int64_t n_in, const uint8_t *vit_host, int64_t n_vit, int64_t *bits, int64_t *errors)
{
  if (!in_host || !vit_host || !bits || !errors) return fail(DVBT_ERR_INVALID, "null argument");
  const Dims d = make_dims(constellation, 0, code_rate, 0, 0);
  if (!d.valid) return fail(DVBT_ERR_INVALID, "bad DVB-T parameters");
  if (n_in < 0 || n_vit < 0 || n_in > (1ll << 30) || n_vit > (1ll << 30)) return fail(DVBT_ERR_INVALID, "n_in and n_vit must lie in [0, 2^30]");
  int r = need_device(); if (r) return r;
  const VitParams vp = make_vit_params(d, 768, 768);
  DevMem<uint8_t> din, dvit; DevMem<unsigned long long> cnt;
  HIPCHK(din.alloc((size_t)n_in + 64)); HIPCHK(dvit.alloc((size_t)n_vit + 64)); HIPCHK(cnt.alloc(2));
  if (n_in) HIPCHK(hipMemcpy(din, in_host, (size_t)n_in, hipMemcpyHostToDevice));
  if (n_vit) HIPCHK(hipMemcpy(dvit, vit_host, (size_t)n_vit, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(cnt, 0, 2 * sizeof(unsigned long long)));
  if (n_vit >= 2)
    hipLaunchKernelGGL(quality_channel_kernel, dim3(quality_grid((n_vit + 7) / 8)), dim3(Q_THREADS), 0, nullptr, (const uint8_t *)din, (long long)n_in, (const uint8_t *)dvit,
                       (long long)n_vit, vp, cnt.get());
  HIPCHK(hipGetLastError());
  unsigned long long c[2];
  HIPCHK(hipMemcpy(c, cnt, sizeof c, hipMemcpyDeviceToHost));
  *bits = (int64_t)c[0]; *errors = (int64_t)c[1];
  return DVBT_OK;
}

extern "C" int dvbt_debug_quality_post(const uint8_t *vit_host, int64_t n_vit, const uint8_t *rs_host, int64_t n_words, int64_t *bits, int64_t *errors)
{
  if (!vit_host || !rs_host || !bits || !errors) return fail(DVBT_ERR_INVALID, "null argument");
  if (n_vit < 0 || n_words < 0 || n_vit > (1ll << 30) || n_words > (1ll << 30) / 188) return fail(DVBT_ERR_INVALID, "n_vit and 188 n_words must lie in [0, 2^30]");
  int r = need_device(); if (r) return r;
  DevMem<uint8_t> dvit, drs; DevMem<unsigned long long> cnt;
  HIPCHK(dvit.alloc((size_t)n_vit + 64)); HIPCHK(drs.alloc((size_t)n_words * 188 + 64)); HIPCHK(cnt.alloc(1));
  if (n_vit) HIPCHK(hipMemcpy(dvit, vit_host, (size_t)n_vit, hipMemcpyHostToDevice));
  if (n_words) HIPCHK(hipMemcpy(drs, rs_host, (size_t)n_words * 188, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(cnt, 0, sizeof(unsigned long long)));
  if (n_words > 0)
    hipLaunchKernelGGL(quality_rs_kernel, dim3(quality_grid(n_words * 47)), dim3(Q_THREADS), 0, nullptr, (const uint8_t *)dvit, (long long)n_vit, (const uint8_t *)drs,
                       (long long)n_words, cnt.get());
  HIPCHK(hipGetLastError());
  unsigned long long c = 0;
  HIPCHK(hipMemcpy(&c, cnt, sizeof c, hipMemcpyDeviceToHost));
  *bits = 1504 * n_words; *errors = (int64_t)c;
  return DVBT_OK;
}
