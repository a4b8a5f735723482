// dvbt_tx.inc -- dvbt_tx_*: the modulator of apps/dvbt_tx_demo*.grc (energy_dispersal .. reference_signals, fft_vxx(reverse, shift),
// cyclic prefixer, multiply_const) as one streaming handle (DESIGN.md 4i) over k_tx.hpp.  Included from dvbt_hip.hip.
//
// A handle modulates one transport stream.  What it carries from call to call: the stream's packet
// count (the dispersal group phase), the symbols emitted so far (symbol_index / frame_index, and where the next symbol's bits start),
// and -- on the device -- the last `hist` RS-coded bytes: the byte interleaver's memory (11 x 204 bytes), the info bits
// that did not fill a symbol yet and the encoder's 6-bit history all lie in that window.  The output length follows from the
// packet counts alone, so dvbt_tx_run_device only enqueues.

namespace {

// TPS word of frame f (code rate HP = d.code_rate): reference_signals_impl.cc:883-916 (format_tps_data), BCH(67,53) parity :352-382 (generate_bch_code)
inline void tx_tps_word(const Dims &d, int code_rate_lp, int include_cell_id, int cell_id, int frame_index, int w0, uint8_t *t)
{
  auto set_bits = [&](int start, int stop, unsigned data) { for (int i = start; i >= stop; i--) { t[i] = data & 1; data >>= 1; } };
  memset(t, 0, 68);
  set_bits(0, 0, (unsigned)w0);
  set_bits(16, 1, (frame_index % 2) ? 0xca11 : 0x35ee);
  set_bits(22, 17, include_cell_id ? 0x1f : 0x17);
  set_bits(24, 23, (unsigned)frame_index);
  set_bits(26, 25, (unsigned)d.constellation);
  set_bits(29, 27, (unsigned)d.hierarchy);
  set_bits(32, 30, (unsigned)d.code_rate);
  set_bits(35, 33, (unsigned)code_rate_lp);
  set_bits(37, 36, (unsigned)d.guard);
  set_bits(39, 38, (unsigned)d.mode);
  set_bits(47, 40, (unsigned)cell_id);
  unsigned reg = 0;                                   // 60 leading zeros, then bits 1..53
  for (int i = 0; i < 113; i++) {
    const unsigned b = i < 60 ? 0 : t[1 + (i - 60)];
    const unsigned fb = 1 & (b ^ reg);
    reg >>= 1;
    reg |= fb << 13;
    reg ^= (fb << 12) ^ (fb << 11) ^ (fb << 9) ^ (fb << 8) ^ (fb << 7) ^ (fb << 5) ^ (fb << 4);
  }
  for (int i = 0; i < 14; i++) t[54 + i] = 1 & (reg >> i);
}

// Carrier classes as pilot_gen::update_output walks the carriers (reference_signals_impl.cc:1127-1186): a scattered pilot where
// k == 3 (symbol_index mod 4) + 12 sp, with sp wrapping at n_spilot + 1 on symbol_index 0 and at n_spilot otherwise (advance_spilot);
// continual pilots and TPS carriers from their tables.  Class c < 4: symbol_index mod 4 == c, symbol_index != 0; class 4: symbol_index 0.
struct TxClasses { std::vector<uint16_t> pay, pil; int npil[TX_NCLASS]; };
inline int tx_carrier_classes(const Dims &d, TxClasses &out)
{
  const std::vector<int> cpl = cpilot_table(d), tps = tps_table(d);
  out.pay.assign((size_t)TX_NCLASS * d.payload, 0); out.pil.assign((size_t)TX_NCLASS * TX_PIL_MAX, 0);
  for (int cls = 0; cls < TX_NCLASS; cls++) {
    const int si = cls == 4 ? 0 : cls == 0 ? 4 : cls;
    int sp = 0, cpi = 0, tpi = 0, pc = 0, np = 0;
    const int sp_size = d.n_sp + (si == 0 ? 1 : 0);
    for (int k = 0; k < d.K; k++) {
      bool payload = true, pilot = false;
      if (k == 3 * (si % 4) + 12 * sp) { sp = (sp + 1) % sp_size; pilot = true; payload = false; }
      if (k == cpl[cpi]) { cpi = (cpi + 1) % (int)cpl.size(); pilot = true; payload = false; }
      if (k == tps[tpi]) { tpi = (tpi + 1) % (int)tps.size(); pilot = false; payload = false; }
      if (pilot) { if (np == TX_PIL_MAX) return fail(DVBT_ERR_INVALID, "pilot table overflow"); out.pil[(size_t)cls * TX_PIL_MAX + np++] = (uint16_t)k; }
      if (payload) { if (pc == d.payload) return fail(DVBT_ERR_INVALID, "payload carrier table overflow"); out.pay[(size_t)cls * d.payload + pc++] = (uint16_t)k; }
    }
    if (pc != d.payload) return fail(DVBT_ERR_INVALID, "payload carrier table size mismatch");
    out.npil[cls] = np;
  }
  return DVBT_OK;
}

// TPS carriers, their base values 2 (0.5 - w_k) (w_k from the sign of the pilot reference) and the sign of symbol s in frame f: DBPSK over
// the bits 1..s of the frame's TPS word (format_tps_data is re-run every symbol; the word changes only with frame_index)
struct TxTps { std::vector<uint16_t> car; std::vector<float> base, sign; };
inline void tx_tps_tables(const Dims &d, int code_rate_lp, int include_cell_id, int cell_id, const std::vector<float> &pref, TxTps &out)
{
  const std::vector<int> tpsc = tps_table(d);
  out.car.assign(tpsc.begin(), tpsc.end());
  out.base.resize(tpsc.size()); out.sign.resize(4 * 68);
  for (size_t i = 0; i < tpsc.size(); i++) out.base[i] = (float)(2 * (0.5 - (pref[tpsc[i]] < 0.f ? 1 : 0)));
  const int w0 = pref[0] < 0.f ? 1 : 0;
  for (int f = 0; f < 4; f++) {
    uint8_t t[68];
    tx_tps_word(d, code_rate_lp, include_cell_id, cell_id, f, w0, t);
    float sg = 1.f;
    for (int s = 0; s < 68; s++) { if (s > 0 && t[s]) sg = -sg; out.sign[f * 68 + s] = sg; }
  }
}

// the RS encoder's feedback rows enc[fb][i] = fb g_(15 - i): row fb is XORed into the 16-byte remainder register, reg[0] first
inline std::vector<uint8_t> rs_encoder_rows()
{
  std::vector<uint8_t> div = rs_division_table(), enc(256 * 16);
  for (int b = 0; b < 256; b++) for (int i = 0; i < 16; i++) enc[b * 16 + i] = div[b * 16 + 15 - i];
  return enc;
}

}  // namespace

struct dvbt_tx {
  dvbt_tx_params p;
  Dims d;
  Tables T;                           // twiddles, symbol interleaver H / H^-1, constellation points
  TxSymParams sp;
  TxTables tt;                        // views into T and the tables below
  DevMem<uint8_t> prbs, enc_tab;
  DevMem<uint16_t> pay, pil, tps;
  DevMem<float> pref, tps_base, tps_sign;
  DevMem<uint8_t> rs[2]; int cur = 0;                     // RS buffers: [history | this call's packets], ping-pong from call to call
  int hist = 0;
  long long packets = 0, symbols = 0, last_np = 0, last_nsym = 0;
  long long max_sym = 0;
  DevMem<float2> carriers;
  DevMem<uint8_t> dts; DevBuf diq;                       // staging of the host entry
  CallOrder ord;                      // last: see CallOrder
};

static long long tx_symbols_after(const dvbt_tx *h, long long npackets)
{ return (h->packets + npackets) * 1632 / h->d.info_bits_per_symbol - h->symbols; }

// back to the start of a stream: zero history in the buffer the next call reads
static int tx_rewind(dvbt_tx *h)
{
  HIPCHK(h->ord.drain());
  h->packets = h->symbols = h->last_np = h->last_nsym = 0;
  HIPCHK(hipMemsetAsync(h->rs[h->cur], 0, (size_t)h->hist, h->ord.s));
  HIPCHK(h->ord.mark(h->ord.s));
  return DVBT_OK;
}

extern "C" int dvbt_tx_create(const dvbt_tx_params *p, dvbt_tx **out)
{
  if (!p || !out) return fail(DVBT_ERR_INVALID, "null argument");
  *out = nullptr;
  int r = need_device(); if (r) return r;
  Dims d = make_dims(p->constellation, p->hierarchy, p->code_rate, p->guard_interval, p->transmission_mode);
  if (!d.valid) return fail(DVBT_ERR_INVALID, "bad DVB-T parameters");
  if (!(p->scale > 0.f) || !std::isfinite(p->scale)) return fail(DVBT_ERR_INVALID, "scale must be a finite number > 0");
  if (p->max_packets < 1 || p->max_packets > (size_t)1 << 24) return fail(DVBT_ERR_INVALID, "max_packets must be in [1, 2^24]");
  if (p->first_packet < 0) return fail(DVBT_ERR_INVALID, "first_packet must be >= 0");
  if (p->include_cell_id < 0 || p->include_cell_id > 1 || p->cell_id < 0 || p->cell_id > 0xffff) return fail(DVBT_ERR_INVALID, "bad cell id parameters");
  if (p->keep_carriers < 0 || p->keep_carriers > 1) return fail(DVBT_ERR_INVALID, "keep_carriers must be 0 or 1");
  if ((r = use_device(p->device))) return r;

  std::unique_ptr<dvbt_tx> hold(new dvbt_tx()); dvbt_tx *const h = hold.get();   // released on every early return below
  h->p = *p; h->d = d; h->T.d = d;
  HIPCHK(h->ord.create());
  if ((r = h->T.fft.build(d.N))) return r;
  if ((r = h->T.build_inner(1.0f))) return r;

  // outer coder tables: the PRBS of one dispersal group and the RS encoder's feedback rows
  if ((r = upload(energy_prbs(), h->prbs))) return r;
  if ((r = upload(rs_encoder_rows(), h->enc_tab))) return r;

  // carriers, pilot values, TPS
  TxClasses cl;
  if ((r = tx_carrier_classes(d, cl))) return r;
  if ((r = upload(cl.pay, h->pay))) return r; if ((r = upload(cl.pil, h->pil))) return r;
  const std::vector<float> pref = pilot_ref_table(d);
  if ((r = upload(pref, h->pref))) return r;
  TxTps tp;
  tx_tps_tables(d, d.code_rate, p->include_cell_id, p->cell_id, pref, tp);
  const std::vector<uint16_t> &t16 = tp.car;
  if ((r = upload(tp.car, h->tps))) return r; if ((r = upload(tp.base, h->tps_base))) return r; if ((r = upload(tp.sign, h->tps_sign))) return r;

  // symbol kernel parameters
  TxSymParams &sp = h->sp;
  memset(&sp, 0, sizeof sp);
  sp.N = d.N; sp.cp = d.cp; sp.payload = d.payload; sp.m = d.m; sp.k = d.k; sp.n = d.n; sp.zl = d.zl; sp.K = d.K; sp.n_tps = (int)t16.size();
  sp.ibits = d.info_bits_per_symbol; sp.scale = p->scale;
  for (int c = 0; c < TX_NCLASS; c++) sp.npil[c] = cl.npil[c];
  for (int j = 0, o = 0; j < d.k; j++) {                 // inner_coder_impl.cc:225-254: x then y of every info bit, kept where the puncture vector says 1
    if (d.punct[2 * j]) sp.cmap[o++] = (uint8_t)(j << 1);
    if (d.punct[2 * j + 1]) sp.cmap[o++] = (uint8_t)((j << 1) | 1);
  }
  for (int kk = 0; kk < d.m; kk++) {                     // bit_inner_interleaver_impl.cc:137-176: bit kk of input word i goes to row e = perm(kk)
    const int e = (kk / (d.m / 2)) + 2 * (kk % (d.m / 2));
    sp.kinv[e] = (uint8_t)kk;
  }
  static const uint8_t hoff[6] = {0, 63, 105, 42, 21, 84};
  memcpy(sp.hoff, hoff, 6);
  sp.nmagic = (uint32_t)((((uint64_t)1 << 32) + d.n - 1) / d.n);
  TxTables &tt = h->tt;
  tt.tw = h->T.fft.tw; tt.H = h->T.H; tt.Hinv = h->T.Hinv; tt.points = h->T.points; tt.pay = h->pay; tt.pil = h->pil; tt.pref = h->pref;
  tt.tps = h->tps; tt.tps_base = h->tps_base; tt.tps_sign = h->tps_sign;

  // buffers: RS history covers the interleaver's 2244 bytes plus the bits of a symbol not yet emitted (+ the 6 in front of them)
  h->hist = (2244 + d.info_bits_per_symbol / 8 + 3 + 15) & ~15;
  const size_t rs_bytes = (size_t)h->hist + p->max_packets * 204;
  for (int i = 0; i < 2; i++) { HIPCHK(h->rs[i].alloc(rs_bytes + 64)); HIPCHK(hipMemsetAsync(h->rs[i], 0, rs_bytes + 64, h->ord.s)); }
  h->max_sym = ((long long)p->max_packets * 1632 + d.info_bits_per_symbol - 1) / d.info_bits_per_symbol;
  if (p->keep_carriers) HIPCHK(h->carriers.alloc((size_t)h->max_sym * d.N + 8));
  if ((r = set_lds(d.N == 8192 ? (const void *)tx_symbol_kernel<8192> : (const void *)tx_symbol_kernel<2048>, tx_symbol_lds_bytes(d.N, d.payload)))) return r;
  if ((r = tx_rewind(h))) return r;
  HIPCHK(hipStreamSynchronize(h->ord.s));
  *out = hold.release();
  return DVBT_OK;
}

extern "C" int64_t dvbt_tx_samples_for(const dvbt_tx *h, size_t npackets)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  return tx_symbols_after(h, (long long)npackets) * (h->d.N + h->d.cp);
}

// the call's two launches on stream st; the caller has checked the capacities
static int tx_enqueue(dvbt_tx *h, const void *ts, long long np, void *iq, long long nsym, hipStream_t st)
{
  HIPCHK(h->ord.join(st));
  const int nxt = h->cur ^ 1;
  const long long nblk = (np + TX_OUTER_PK - 1) / TX_OUTER_PK;
  hipLaunchKernelGGL(tx_outer_kernel, dim3((unsigned)(nblk + 1)), dim3(TX_OUTER_PK), 0, st, (const uint8_t *)ts, np, (long long)h->p.first_packet + h->packets,
                     (const uint8_t *)h->prbs, (const uint4 *)h->enc_tab.get(), (const uint8_t *)h->rs[h->cur], (long long)h->hist + h->last_np * 204, h->hist, h->rs[nxt]);
  HIPCHK(hipGetLastError());
  if (nsym > 0) {
    TxSymParams sp = h->sp;
    sp.S0 = h->symbols; sp.base = h->packets * 204 - h->hist; sp.rs_len = h->hist + np * 204; sp.nsym = (int)nsym;
    float2 *car = h->p.keep_carriers ? h->carriers : nullptr;
    const size_t lds = tx_symbol_lds_bytes(h->d.N, h->d.payload);
    if (h->d.N == 8192) hipLaunchKernelGGL(tx_symbol_kernel<8192>, dim3((unsigned)nsym), dim3(FFT_THREADS), lds, st, (const uint8_t *)h->rs[nxt], sp, h->tt, (float2 *)iq, car);
    else hipLaunchKernelGGL(tx_symbol_kernel<2048>, dim3((unsigned)nsym), dim3(FFT_THREADS), lds, st, (const uint8_t *)h->rs[nxt], sp, h->tt, (float2 *)iq, car);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(h->ord.mark(st));
  h->cur = nxt; h->packets += np; h->symbols += nsym; h->last_np = np; h->last_nsym = nsym;
  return DVBT_OK;
}

// DVBT_ERR_CAPACITY / DVBT_ERR_INVALID leave the stream where it was
static int tx_check(dvbt_tx *h, const void *ts, size_t npackets, const void *iq, size_t cap_samples, long long &nsym)
{
  if (npackets > h->p.max_packets) return fail(DVBT_ERR_CAPACITY, "npackets > max_packets");
  nsym = tx_symbols_after(h, (long long)npackets);
  if ((size_t)nsym * (size_t)(h->d.N + h->d.cp) > cap_samples) return fail(DVBT_ERR_CAPACITY, "cap_samples is smaller than the call's output (dvbt_tx_samples_for)");
  if ((npackets && !ts) || (nsym && !iq)) return fail(DVBT_ERR_INVALID, "null buffer");
  if (((uintptr_t)ts & 3) || ((uintptr_t)iq & 7)) return fail(DVBT_ERR_INVALID, "the TS buffer must be 4-byte aligned, the sample buffer 8-byte aligned");
  return DVBT_OK;
}

extern "C" int dvbt_tx_run_device(dvbt_tx *h, const void *ts_device, size_t npackets, void *iq_device, size_t cap_samples, void *stream, size_t *nsamples)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  long long nsym;
  int r = tx_check(h, ts_device, npackets, iq_device, cap_samples, nsym); if (r) return r;
  if (nsamples) *nsamples = 0;
  if (npackets == 0) { h->last_nsym = 0; return DVBT_OK; }
  HIPCHK(hipSetDevice(h->p.device));
  r = tx_enqueue(h, ts_device, (long long)npackets, iq_device, nsym, (hipStream_t)stream); if (r) return r;
  if (nsamples) *nsamples = (size_t)nsym * (size_t)(h->d.N + h->d.cp);
  return DVBT_OK;
}

extern "C" int dvbt_tx_run(dvbt_tx *h, const void *ts_host, size_t npackets, void *iq_host, size_t cap_samples, size_t *nsamples)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  long long nsym;
  int r = tx_check(h, ts_host, npackets, iq_host, cap_samples, nsym); if (r) return r;
  if (nsamples) *nsamples = 0;
  if (npackets == 0) { h->last_nsym = 0; return DVBT_OK; }
  HIPCHK(hipSetDevice(h->p.device));
  const size_t nout = (size_t)nsym * (size_t)(h->d.N + h->d.cp);
  if (!h->dts) HIPCHK(h->dts.alloc(h->p.max_packets * 188 + 64));
  HIPCHK(h->ord.join(h->ord.s));
  r = h->diq.reserve(nout * sizeof(float2)); if (r) return r;
  HIPCHK(hipMemcpyAsync(h->dts, ts_host, npackets * 188, hipMemcpyHostToDevice, h->ord.s));
  r = tx_enqueue(h, h->dts, (long long)npackets, h->diq.p, nsym, h->ord.s); if (r) return r;
  if (nout) HIPCHK(hipMemcpyAsync(iq_host, h->diq.p, nout * sizeof(float2), hipMemcpyDeviceToHost, h->ord.s));
  HIPCHK(hipStreamSynchronize(h->ord.s));
  if (nsamples) *nsamples = nout;
  return DVBT_OK;
}

extern "C" int64_t dvbt_tx_read_carriers(dvbt_tx *h, void *dst_host, size_t cap_bytes)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  if (!h->p.keep_carriers) return fail(DVBT_ERR_STATE, "the handle was created without keep_carriers");
  const size_t bytes = (size_t)h->last_nsym * h->d.N * sizeof(float2);
  if (!dst_host) return (int64_t)bytes;
  if (cap_bytes < bytes) return fail(DVBT_ERR_CAPACITY, "cap_bytes is smaller than the last call's carriers");
  HIPCHK(h->ord.drain());
  if (bytes) HIPCHK(hipMemcpy(dst_host, h->carriers, bytes, hipMemcpyDeviceToHost));
  return (int64_t)bytes;
}

extern "C" int dvbt_tx_reset(dvbt_tx *h)
{
  if (!h) return fail(DVBT_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->p.device));
  return tx_rewind(h);
}

extern "C" void dvbt_tx_destroy(dvbt_tx *h) { delete h; }
