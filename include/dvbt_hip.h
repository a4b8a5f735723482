/*
 * dvbt_hip.h -- C ABI of libdvbt_hip.so: the MI355X (gfx950) DVB-T receive hot path
 * behind the gr::dvbt block interfaces of BogdanDIA/gr-dvbt.
 *
 * Plain C: opaque handles, POD parameter structs that carry exactly the arguments of the
 * reference's X::make(...), caller-owned in/out buffers (host memory unless a function
 * says "_device"), explicit sideband struct instead of GNU Radio stream tags.
 *
 * One triple per reference block (create / forecast / work / destroy) + the segment API
 * that runs the whole chain device-resident.  Each entry cites the reference interface
 * it replaces (paths relative to the gr-dvbt tree).
 *
 * Threading: like a GNU Radio block, a handle must not be used from two threads at once.
 * Errors: functions return >= 0 (items produced / DVBT_OK) or a negative dvbt_status.
 * The reference never reports errors (SURVEY 8b "Error conventions"); RS failures are
 * likewise silent here (bytes pass through), and are only counted in the report.
 */
#ifndef DVBT_HIP_H
#define DVBT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DVBT_OK = 0,
  DVBT_ERR_INVALID = -1,      /* bad parameter */
  DVBT_ERR_NO_DEVICE = -2,    /* no HIP device / kernel image not loadable: there is NO CPU fallback */
  DVBT_ERR_HIP = -3,          /* a HIP runtime call failed (message via dvbt_last_error) */
  DVBT_ERR_CAPACITY = -4,     /* caller buffer or handle capacity too small */
  DVBT_ERR_STATE = -5         /* call sequence violates the block's contract */
} dvbt_status;

/* enums: include/dvbt/dvbt_config.h:34-75 (values double as TPS field encodings).  Every function takes them as int.  A
 * translation unit that also includes gr-dvbt's dvbt/dvbt_config.h (the GNU Radio block shells, gr_dvbt_amd/host/gr) defines
 * DVBT_HIP_NO_ENUMS first: that header puts the same type names into the global namespace (:160-167). */
#ifndef DVBT_HIP_NO_ENUMS
typedef enum { DVBT_QPSK = 0, DVBT_QAM16 = 1, DVBT_QAM64 = 2 } dvbt_constellation_t;
typedef enum { DVBT_NH = 0, DVBT_ALPHA1, DVBT_ALPHA2, DVBT_ALPHA4 } dvbt_hierarchy_t;
typedef enum { DVBT_C1_2 = 0, DVBT_C2_3, DVBT_C3_4, DVBT_C5_6, DVBT_C7_8 } dvbt_code_rate_t;
typedef enum { DVBT_T2k = 0, DVBT_T8k = 1 } dvbt_transmission_mode_t;
typedef enum { DVBT_G1_32 = 0, DVBT_G1_16, DVBT_G1_8, DVBT_G1_4 } dvbt_guard_interval_t;
#endif
#define DVBT_AUTO (-1)   /* dvbt_rx_stream_params.rx.constellation / hierarchy / code_rate: take it from the stream's TPS word */

/* sideband: replaces the stream tags of SURVEY Appendix D */
typedef enum { DVBT_TAG_SYNC_START = 1, DVBT_TAG_SUPERFRAME_START = 2, DVBT_TAG_SYMBOL_INDEX = 3 } dvbt_tag_key;
typedef struct { int64_t rel_offset; int32_t key; int32_t value; } dvbt_tag;   /* offset in items, relative to the call's first item */
typedef struct {
  const dvbt_tag *in_tags; int n_in_tags;      /* tags visible in the input window */
  dvbt_tag *out_tags; int out_cap; int n_out_tags;  /* tags the block attaches to its output */
  int n_consumed;                              /* what the block would pass to consume_each() */
} dvbt_sideband;

/* Every block has two work entries.  dvbt_<blk>_work takes HOST buffers, like gr::block::general_work: it copies in, computes, copies
 * out and synchronises.  dvbt_<blk>_work_device takes DEVICE pointers (hipMalloc'd; same item layout) and a hipStream_t (NULL: the
 * device's default stream, on which blocks chained without an explicit stream are ordered): it only enqueues, so adjacent HIP blocks of a flowgraph hand items to each other without crossing PCIe.
 * Tags still travel through the host-side dvbt_sideband.  Two blocks must know data-dependent counts before they return and
 * therefore read a few bytes back and synchronise the stream once per call (ofdm_sym_acquisition: items produced / samples consumed;
 * demod_reference_signals: which items passed the superframe hunt, and their symbol indices); energy_descramble reads the 16 sync
 * positions of its window (NSYNC search).  The others return counts that follow from the call's sizes and tags alone.  A handle is
 * driven through one of the two entries for its whole life (the history of the streaming blocks lives on the device either way). */
const char *dvbt_last_error(void);
/* device buffers for hosts that do not link the HIP runtime themselves (a GNU Radio block shell, gr_dvbt_amd/host/rx_flowgraph_example.cpp):
 * hipMalloc / hipFree / hipMemcpy (synchronous) / hipStreamSynchronize (stream NULL: the whole device) */
void *dvbt_device_malloc(size_t bytes);
void  dvbt_device_free(void *p);
int   dvbt_copy_to_device(void *dst_device, const void *src_host, size_t bytes);
int   dvbt_copy_to_host(void *dst_host, const void *src_device, size_t bytes);
int   dvbt_synchronize(void *stream);
/* page-lock a host buffer that will be handed to the host-pointer entries again and again (hipHostRegister / hipHostUnregister): a GNU Radio shell registers
 * its input and output buffers once (they live as long as the flowgraph); dvbt_<blk>_work (and dvbt_rx_stream_push for calls of 2 MB and more) then let the DMA engines read and write
 * them directly instead of staging every item through a pinned buffer of the handle (one host memcpy each way).  Buffers that are not registered work as before. */
int   dvbt_host_register(void *p, size_t bytes);
int   dvbt_host_unregister(void *p);
int dvbt_device_count(void);                   /* HIP devices visible; <=0 means the library cannot run */
const char *dvbt_version(void);

/* ------------------------------------------------------------------ derived constants
 * replaces dvbt_config::dvbt_config (lib/dvbt_config.cc:94-250, include/dvbt/dvbt_config.h:95-139) */
typedef struct {
  int fft_length, cp_length, Kmax, payload_length, zeros_on_left, m, cr_k, cr_n;
  float norm;
  int ntraceback;                              /* lib/viterbi_decoder_impl.cc:95-124 */
  int info_bits_per_symbol;
} dvbt_dims;
int dvbt_get_dims(int constellation, int hierarchy, int code_rate, int guard_interval,
                  int transmission_mode, dvbt_dims *out);

/* ------------------------------------------------------------------ A1 ofdm_sym_acquisition
 * replaces ofdm_sym_acquisition::make(blocks, fft_length, occupied_tones, cp_length, snr)
 * (include/dvbt/ofdm_sym_acquisition.h:49) and general_work/forecast
 * (lib/ofdm_sym_acquisition_impl.cc:474-481,489-568).  in: cfloat stream; out: items of N cfloat.
 * Unlike the reference (<=1 item per call) a call may produce up to noutput_items items;
 * n_consumed = (N+cp) per symbol attempted. */
typedef struct { int blocks, fft_length, occupied_tones, cp_length; float snr; } dvbt_ofdm_sym_acquisition_params;
typedef struct dvbt_ofdm_sym_acquisition dvbt_ofdm_sym_acquisition;
int  dvbt_ofdm_sym_acquisition_create(const dvbt_ofdm_sym_acquisition_params *p, dvbt_ofdm_sym_acquisition **out);
int  dvbt_ofdm_sym_acquisition_forecast(const dvbt_ofdm_sym_acquisition *h, int noutput_items, int *ninput_required);
int  dvbt_ofdm_sym_acquisition_work(dvbt_ofdm_sym_acquisition *h, int noutput_items, int ninput_items,
                                    const void *in, void *out, dvbt_sideband *sb);
int  dvbt_ofdm_sym_acquisition_work_device(dvbt_ofdm_sym_acquisition *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                            dvbt_sideband *sb, void *stream);
void dvbt_ofdm_sym_acquisition_destroy(dvbt_ofdm_sym_acquisition *h);

/* ------------------------------------------------------------------ A2 forward FFT (stock fft_vxx in the flowgraph)
 * replaces gr::fft::fft_vcc(fft_size, forward=True, rectangular, shift=True)
 * (apps/dvbt_rx_demo*.grc block fft_vxx_0). items of N cfloat in and out.
 * forward = 0 (shift = 1): fft_vcc(fft_size, forward=False, shift=True) of apps/dvbt_tx_demo*.grc -- the input halves swapped, then
 * out[t] = sum_k in'[k] e^{+2 pi i t k / N}, unnormalised.  shift = 0 is refused. */
typedef struct { int fft_size; int forward; int shift; } dvbt_fft_params;
typedef struct dvbt_fft dvbt_fft;
int  dvbt_fft_create(const dvbt_fft_params *p, dvbt_fft **out);
int  dvbt_fft_forecast(const dvbt_fft *h, int noutput_items, int *ninput_required);
int  dvbt_fft_work(dvbt_fft *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_fft_work_device(dvbt_fft *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                           dvbt_sideband *sb, void *stream);
void dvbt_fft_destroy(dvbt_fft *h);

/* ------------------------------------------------------------------ A3 demod_reference_signals
 * replaces demod_reference_signals::make(itemsize, ninput, noutput, constellation, hierarchy,
 * code_rate_HP, code_rate_LP, guard_interval, transmission_mode, include_cell_id, cell_id)
 * (include/dvbt/demod_reference_signals.h:50-54); general_work lib/demod_reference_signals_impl.cc:97-150.
 * in: items of ninput cfloat (needs noutput_items+1 visible); out: items of noutput cfloat.
 * Emits SUPERFRAME_START once and SYMBOL_INDEX per produced item. */
typedef struct { int itemsize, ninput, noutput, constellation, hierarchy, code_rate_hp, code_rate_lp,
                 guard_interval, transmission_mode, include_cell_id, cell_id; } dvbt_demod_reference_signals_params;
typedef struct dvbt_demod_reference_signals dvbt_demod_reference_signals;
int  dvbt_demod_reference_signals_create(const dvbt_demod_reference_signals_params *p, dvbt_demod_reference_signals **out);
int  dvbt_demod_reference_signals_forecast(const dvbt_demod_reference_signals *h, int noutput_items, int *ninput_required);
int  dvbt_demod_reference_signals_work(dvbt_demod_reference_signals *h, int noutput_items, int ninput_items,
                                       const void *in, void *out, dvbt_sideband *sb);
int  dvbt_demod_reference_signals_work_device(dvbt_demod_reference_signals *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                               dvbt_sideband *sb, void *stream);
void dvbt_demod_reference_signals_destroy(dvbt_demod_reference_signals *h);

/* ------------------------------------------------------------------ A4 dvbt_demap
 * replaces dvbt_demap::make(nsize, constellation, hierarchy, transmission, gain)
 * (include/dvbt/dvbt_demap.h:50); general_work lib/dvbt_demap_impl.cc:217-240. cfloat x nsize -> u8 x nsize */
typedef struct { int nsize, constellation, hierarchy, transmission_mode; float gain; } dvbt_demap_params;
typedef struct dvbt_demap dvbt_demap;
int  dvbt_demap_create(const dvbt_demap_params *p, dvbt_demap **out);
int  dvbt_demap_forecast(const dvbt_demap *h, int noutput_items, int *ninput_required);
int  dvbt_demap_work(dvbt_demap *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_demap_work_device(dvbt_demap *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                             dvbt_sideband *sb, void *stream);
void dvbt_demap_destroy(dvbt_demap *h);

/* ------------------------------------------------------------------ A5 symbol_inner_interleaver
 * replaces symbol_inner_interleaver::make(ninput, transmission, direction)
 * (include/dvbt/symbol_inner_interleaver.h:50-51); general_work lib/symbol_inner_interleaver_impl.cc:161-219.
 * direction 0 (RX) needs one SYMBOL_INDEX tag per item; direction 1 (TX) counts internally. */
typedef struct { int nsize, transmission_mode, direction; } dvbt_symbol_inner_interleaver_params;
typedef struct dvbt_symbol_inner_interleaver dvbt_symbol_inner_interleaver;
int  dvbt_symbol_inner_interleaver_create(const dvbt_symbol_inner_interleaver_params *p, dvbt_symbol_inner_interleaver **out);
int  dvbt_symbol_inner_interleaver_forecast(const dvbt_symbol_inner_interleaver *h, int noutput_items, int *ninput_required);
int  dvbt_symbol_inner_interleaver_work(dvbt_symbol_inner_interleaver *h, int noutput_items, int ninput_items,
                                        const void *in, void *out, dvbt_sideband *sb);
int  dvbt_symbol_inner_interleaver_work_device(dvbt_symbol_inner_interleaver *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                                dvbt_sideband *sb, void *stream);
void dvbt_symbol_inner_interleaver_destroy(dvbt_symbol_inner_interleaver *h);

/* ------------------------------------------------------------------ A6 bit_inner_deinterleaver
 * replaces bit_inner_deinterleaver::make(nsize, constellation, hierarchy, transmission)
 * (include/dvbt/bit_inner_deinterleaver.h:50-51); general_work lib/bit_inner_deinterleaver_impl.cc:120-184.
 * Non-hierarchical: one output stream (work / work_device).  Hierarchical (ALPHA1 / 2 / 4; io_signature (1, 2)): two output streams, the high-priority
 * bytes (2 bits each) and the low-priority ones (:148-184): work_hier / work_hier_device; work / work_device then deliver output 0 alone, as a flowgraph
 * that connects only the first port gets it.  Two things of the reference's hierarchical branch are not reproducible and are defined here: the bits it
 * reads from behind its bit matrix (64-QAM, low-priority bytes i >= 84 of a block, row 5: undefined behaviour there) are 0; hierarchical QPSK is rejected
 * (the reference's constructor divides by d_v - 2 = 0). */
typedef struct { int nsize, constellation, hierarchy, transmission_mode; } dvbt_bit_inner_deinterleaver_params;
typedef struct dvbt_bit_inner_deinterleaver dvbt_bit_inner_deinterleaver;
int  dvbt_bit_inner_deinterleaver_create(const dvbt_bit_inner_deinterleaver_params *p, dvbt_bit_inner_deinterleaver **out);
int  dvbt_bit_inner_deinterleaver_forecast(const dvbt_bit_inner_deinterleaver *h, int noutput_items, int *ninput_required);
int  dvbt_bit_inner_deinterleaver_work(dvbt_bit_inner_deinterleaver *h, int noutput_items, int ninput_items,
                                       const void *in, void *out, dvbt_sideband *sb);
int  dvbt_bit_inner_deinterleaver_work_device(dvbt_bit_inner_deinterleaver *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                               dvbt_sideband *sb, void *stream);
int  dvbt_bit_inner_deinterleaver_work_hier(dvbt_bit_inner_deinterleaver *h, int noutput_items, int ninput_items,
                                            const void *in, void *out_hp, void *out_lp, dvbt_sideband *sb);
int  dvbt_bit_inner_deinterleaver_work_hier_device(dvbt_bit_inner_deinterleaver *h, int noutput_items, int ninput_items, const void *in_device,
                                                   void *out_hp_device, void *out_lp_device, dvbt_sideband *sb, void *stream);
void dvbt_bit_inner_deinterleaver_destroy(dvbt_bit_inner_deinterleaver *h);

/* ------------------------------------------------------------------ A7 viterbi_decoder
 * replaces viterbi_decoder::make(constellation, hierarchy, coderate, bsize, S0, SK)
 * (include/dvbt/viterbi_decoder.h:51-52); general_work lib/viterbi_decoder_impl.cc:192-324 and the
 * SSE2 kernels lib/d_viterbi.c:461-576,680-735.  u8 stream (m bits per byte) -> u8 stream.
 * noutput_items must be a multiple of bsize*k/8 (set_output_multiple, :141). A SUPERFRAME_START tag
 * at rel_offset 0 resets the decoder; at rel_offset>0 the call consumes up to the tag and returns 0 (:213-229).
 * Unlike the reference (file-scope static state) any number of instances may coexist. */
/* what the Viterbi stage's proof + repair passes did (dvbt_rx_params.viterbi_verify; dvbt_rx_viterbi_proof, dvbt_viterbi_decoder_proof) */
typedef struct {
  int64_t chunks;             /* chunk decoders of the launch */
  int64_t decoded_again;      /* chunks the warm-up alone did not prove (decoded again by the parallel repair pass) */
  int64_t sequential;         /* chunks the sequential pass decoded (a repaired decoder that had not merged with the unproven one after a whole chunk: never observed) */
  int64_t not_proven;         /* chunks that are not proven when the launch ends: the final check's count (viterbi_verify >= 1), -1 when it did not run */
} dvbt_viterbi_proof;
typedef struct { int constellation, hierarchy, code_rate, bsize, S0, SK; } dvbt_viterbi_decoder_params;
typedef struct dvbt_viterbi_decoder dvbt_viterbi_decoder;
int  dvbt_viterbi_decoder_create(const dvbt_viterbi_decoder_params *p, dvbt_viterbi_decoder **out);
int  dvbt_viterbi_decoder_forecast(const dvbt_viterbi_decoder *h, int noutput_items, int *ninput_required);
int  dvbt_viterbi_decoder_work(dvbt_viterbi_decoder *h, int noutput_items, int ninput_items,
                               const void *in, void *out, dvbt_sideband *sb);
int  dvbt_viterbi_decoder_work_device(dvbt_viterbi_decoder *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                       dvbt_sideband *sb, void *stream);
/* the chunk decoders' warm-up for the single block (see dvbt_rx_params.viterbi_warm_windows): 0 = the default 72 windows, else a multiple of 24 in [48, 576].
 * Speed only: the block proves and repairs every launch and carries the streaming decoder's state from call to call (dvbt_rx_params.viterbi_verify). */
int  dvbt_viterbi_decoder_set_warm_windows(dvbt_viterbi_decoder *h, int windows);
/* counters of the block's proof + repair passes, summed over its calls since the last reset (chunks, decoded_again, sequential; not_proven = -1: the block runs no final check) */
int  dvbt_viterbi_decoder_proof(dvbt_viterbi_decoder *h, dvbt_viterbi_proof *out);
/* always != 0: the traceback chains of the following calls walk every hop instead of taking the shortcut over chained best states (the same bytes; tests, measurements) */
int  dvbt_viterbi_decoder_set_walk(dvbt_viterbi_decoder *h, int always);
/* test hooks.  The chunk size of the block's launches: 0 = the default 264 bytes, else a multiple of 24 in [24, 264]; adopted by the next call that carries a
 * superframe-start tag (a stream reset).  The same bytes at any size (tests/test_gpu_viterbi_handover.py) */
int  dvbt_viterbi_decoder_set_chunk_bytes(dvbt_viterbi_decoder *h, int bytes);
/* test hook: dvbt_rx_params.viterbi_verify (-1 .. 4) for the block's launches from the next stream reset on, 0 = the default.  With a mode >= 1 dvbt_viterbi_decoder_proof reports the
 * last launch's final check in not_proven */
int  dvbt_viterbi_decoder_set_verify(dvbt_viterbi_decoder *h, int mode);
/* test hook, read-only and blocking: the 16 header words of the last launch's control block (chunks, decoded again, left to the sequential pass, not proven,
 * decoded by the sequential pass, ..., the sums at [8..10], the shortcut's counters at [12..15]) */
int  dvbt_viterbi_decoder_last_ctl(dvbt_viterbi_decoder *h, int out[16]);
/* out[0], out[1]: blocks of 24 windows, per wavefront, whose bytes left by the shortcut / whose chains walked, since the block was created */
int  dvbt_viterbi_decoder_shortcut(dvbt_viterbi_decoder *h, long long out[2]);
void dvbt_viterbi_decoder_destroy(dvbt_viterbi_decoder *h);

/* ------------------------------------------------------------------ A8 convolutional_deinterleaver
 * replaces convolutional_deinterleaver::make(nsize(blocks), I, M)
 * (include/dvbt/convolutional_deinterleaver.h:49); general_work lib/convolutional_deinterleaver_impl.cc:93-150.
 * u8 stream -> items of I*blocks bytes; noutput_items must be even (set_output_multiple(2)). */
typedef struct { int blocks, I, M; } dvbt_convolutional_deinterleaver_params;
typedef struct dvbt_convolutional_deinterleaver dvbt_convolutional_deinterleaver;
int  dvbt_convolutional_deinterleaver_create(const dvbt_convolutional_deinterleaver_params *p, dvbt_convolutional_deinterleaver **out);
int  dvbt_convolutional_deinterleaver_forecast(const dvbt_convolutional_deinterleaver *h, int noutput_items, int *ninput_required);
int  dvbt_convolutional_deinterleaver_work(dvbt_convolutional_deinterleaver *h, int noutput_items, int ninput_items,
                                           const void *in, void *out, dvbt_sideband *sb);
int  dvbt_convolutional_deinterleaver_work_device(dvbt_convolutional_deinterleaver *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                                   dvbt_sideband *sb, void *stream);
void dvbt_convolutional_deinterleaver_destroy(dvbt_convolutional_deinterleaver *h);

/* ------------------------------------------------------------------ A9 reed_solomon_dec
 * replaces reed_solomon_dec::make(p, m, gfpoly, n, k, t, s, blocks)
 * (include/dvbt/reed_solomon_dec.h:49); general_work lib/reed_solomon_dec_impl.cc:77-116 and
 * reed_solomon::rs_decode lib/reed_solomon.cc:246-489. items of blocks*(n-s) -> blocks*(k-s) bytes.
 * Only the DVB parameter set (2,8,0x11d,255,239,8,51) is accepted.
 * oracle_compat = 1 reproduces the as-compiled reference quirk (SURVEY 8c last row / B-1). */
typedef struct { int p, m, gfpoly, n, k, t, s, blocks; int oracle_compat; } dvbt_reed_solomon_dec_params;
typedef struct dvbt_reed_solomon_dec dvbt_reed_solomon_dec;
int  dvbt_reed_solomon_dec_create(const dvbt_reed_solomon_dec_params *p, dvbt_reed_solomon_dec **out);
int  dvbt_reed_solomon_dec_forecast(const dvbt_reed_solomon_dec *h, int noutput_items, int *ninput_required);
int  dvbt_reed_solomon_dec_work(dvbt_reed_solomon_dec *h, int noutput_items, int ninput_items,
                                const void *in, void *out, dvbt_sideband *sb);
int  dvbt_reed_solomon_dec_work_device(dvbt_reed_solomon_dec *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                        dvbt_sideband *sb, void *stream);
void dvbt_reed_solomon_dec_destroy(dvbt_reed_solomon_dec *h);

/* ------------------------------------------------------------------ next row: energy_descramble
 * replaces energy_descramble::make(nblocks) (lib/energy_descramble_impl.cc:108-174).
 * items of 8*188 bytes -> u8 stream. */
typedef struct { int nblocks; } dvbt_energy_descramble_params;
typedef struct dvbt_energy_descramble dvbt_energy_descramble;
int  dvbt_energy_descramble_create(const dvbt_energy_descramble_params *p, dvbt_energy_descramble **out);
int  dvbt_energy_descramble_forecast(const dvbt_energy_descramble *h, int noutput_items, int *ninput_required);
int  dvbt_energy_descramble_work(dvbt_energy_descramble *h, int noutput_items, int ninput_items,
                                 const void *in, void *out, dvbt_sideband *sb);
int  dvbt_energy_descramble_work_device(dvbt_energy_descramble *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                         dvbt_sideband *sb, void *stream);
void dvbt_energy_descramble_destroy(dvbt_energy_descramble *h);

/* ------------------------------------------------------------------ next row 2: front-of-chain resample + scale
 * replaces the stock blocks in front of the path in apps/dvbt_rx_demo*.grc:
 *   rational_resampler_xxx_0 (gr::filter rational_resampler_ccc, interp 64, decim 70, taps none, fbw none)
 *   blocks_multiply_const_vxx_0 (complex const 0.0022097087 @2k, 0.00055242272 @8k)
 * cfloat stream at the file rate (10 Msps) -> cfloat stream at the OFDM elementary rate (64/7 Msps), scaled.
 * GNU Radio (gr-filter, gr-fft) is a third-party dependency that is absent from the reference tree and not version
 * pinned: the taps are designed as the 3.7 series does for taps=None (interp/decim reduced by their gcd, fractional_bw
 * 0.4, Kaiser beta 7 windowed sinc: 1149 taps, 32 branches of 36 for 64/70); parity unpinned, float-tolerance tap.
 * scale = 1.0f for the resampler alone.  forecast/work follow rational_resampler_base (noutput*decim/interp + history). */
typedef struct { int interpolation, decimation; float scale; } dvbt_resampler_params;
typedef struct dvbt_resampler dvbt_resampler;
int  dvbt_resampler_create(const dvbt_resampler_params *p, dvbt_resampler **out);
int  dvbt_resampler_forecast(const dvbt_resampler *h, int noutput_items, int *ninput_required);
int  dvbt_resampler_work(dvbt_resampler *h, int noutput_items, int ninput_items,
                         const void *in, void *out, dvbt_sideband *sb);
int  dvbt_resampler_work_device(dvbt_resampler *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                dvbt_sideband *sb, void *stream);
int  dvbt_resampler_get_taps(const dvbt_resampler *h, float *taps, int cap, int *interpolation, int *decimation);  /* returns the tap count */
void dvbt_resampler_destroy(dvbt_resampler *h);

/* ================================================================== the transmit blocks, one at a time
 * The blocks of apps/dvbt_tx_demo*.grc and of the per-block apps (energy_dispersal.grc, rs_encode.grc, dvbt_map.grc, symbol_inner_interleaver.grc,
 * dvbt_tx.grc), each with the create / forecast / work / work_device / destroy of the receive blocks.  With symbol_inner_interleaver(direction = 1) and
 * fft(forward = 0) above, every HIP block of the TX chain has an entry; vector_to_stream, the cyclic prefixer and multiply_const are stock GNU Radio.
 * The stateful blocks (convolutional_interleaver, inner_coder, reference_signals) keep their state in the handle; a refused call (DVBT_ERR_INVALID)
 * leaves it as it was, and the next good call continues the stream.  Byte outputs of the device entries must be 4-byte aligned, cfloat outputs
 * 16-byte aligned (vector stores); byte inputs may sit anywhere.  Only energy_dispersal synchronises in work_device: it reads its SYNC window back. */

/* ------------------------------------------------------------------ T1 energy_dispersal
 * replaces energy_dispersal::make(nblocks) (include/dvbt/energy_dispersal.h); forecast and general_work lib/energy_dispersal_impl.cc:86-141.
 * u8 stream -> items of nblocks*8*188 bytes.  forecast: 8*189*nblocks*noutput_items bytes (one spare byte per packet for the SYNC search).
 * Every call searches its first 188 bytes for 0x47: none there -> 0 items, n_consumed = 188; found at `index` -> the items behind it,
 * n_consumed = index + nblocks*1504*items.  The PRBS restarts with every group of 8 packets; sync bytes are written as 0xB8 (first packet of a
 * group) and 0x47 (the others) whatever the input holds (the reference only prints "Malformed MPEG-TS").  Defined here, not reproduced: a call
 * that sees fewer bytes than its output needs produces what fits (the reference reads past its window); with fewer than 188 bytes and no sync
 * it consumes nothing, with a sync but not one item behind it it consumes the bytes in front of the sync.
 * work_device copies the 188-byte window back to the host and synchronises `stream` once per call before it enqueues (the search decides what
 * is consumed), like energy_descramble. */
typedef struct { int nblocks; } dvbt_energy_dispersal_params;
typedef struct dvbt_energy_dispersal dvbt_energy_dispersal;
int  dvbt_energy_dispersal_create(const dvbt_energy_dispersal_params *p, dvbt_energy_dispersal **out);
int  dvbt_energy_dispersal_forecast(const dvbt_energy_dispersal *h, int noutput_items, int *ninput_required);
int  dvbt_energy_dispersal_work(dvbt_energy_dispersal *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_energy_dispersal_work_device(dvbt_energy_dispersal *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                       dvbt_sideband *sb, void *stream);
void dvbt_energy_dispersal_destroy(dvbt_energy_dispersal *h);

/* ------------------------------------------------------------------ T2 reed_solomon_enc
 * replaces reed_solomon_enc::make(p, m, gfpoly, n, k, t, s, blocks) (include/dvbt/reed_solomon_enc.h); general_work
 * lib/reed_solomon_enc_impl.cc:66-99 and reed_solomon::rs_encode lib/reed_solomon.cc:216-244.  items of blocks*(k-s) -> blocks*(n-s) bytes.
 * Only the DVB parameter set (2,8,0x11d,255,239,8,51) is accepted, as by reed_solomon_dec.  Input and output 4-byte aligned (device). */
typedef struct { int p, m, gfpoly, n, k, t, s, blocks; } dvbt_reed_solomon_enc_params;
typedef struct dvbt_reed_solomon_enc dvbt_reed_solomon_enc;
int  dvbt_reed_solomon_enc_create(const dvbt_reed_solomon_enc_params *p, dvbt_reed_solomon_enc **out);
int  dvbt_reed_solomon_enc_forecast(const dvbt_reed_solomon_enc *h, int noutput_items, int *ninput_required);
int  dvbt_reed_solomon_enc_work(dvbt_reed_solomon_enc *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_reed_solomon_enc_work_device(dvbt_reed_solomon_enc *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                       dvbt_sideband *sb, void *stream);
void dvbt_reed_solomon_enc_destroy(dvbt_reed_solomon_enc *h);

/* ------------------------------------------------------------------ T3 convolutional_interleaver
 * replaces convolutional_interleaver::make(nsize(blocks), I, M) (include/dvbt/convolutional_interleaver.h); work
 * lib/convolutional_interleaver_impl.cc:73-82.  A sync_interpolator: items of I*blocks bytes -> u8 stream.  noutput_items must be a multiple of
 * I*blocks (else DVBT_ERR_INVALID); returns bytes, n_consumed = items.  out[t] = x[t - I*M*(t mod I)] over the whole stream, x[< 0] = 0: branch j
 * is the reference's FIFO of M*j bytes, initially zero.  The handle keeps the last (I-1)*M*I input bytes on the device.  Any I >= 1, M >= 0 with
 * I*blocks a multiple of 4. */
typedef struct { int blocks, I, M; } dvbt_convolutional_interleaver_params;
typedef struct dvbt_convolutional_interleaver dvbt_convolutional_interleaver;
int  dvbt_convolutional_interleaver_create(const dvbt_convolutional_interleaver_params *p, dvbt_convolutional_interleaver **out);
int  dvbt_convolutional_interleaver_forecast(const dvbt_convolutional_interleaver *h, int noutput_items, int *ninput_required);
int  dvbt_convolutional_interleaver_work(dvbt_convolutional_interleaver *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_convolutional_interleaver_work_device(dvbt_convolutional_interleaver *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                                dvbt_sideband *sb, void *stream);
void dvbt_convolutional_interleaver_destroy(dvbt_convolutional_interleaver *h);

/* ------------------------------------------------------------------ T4 inner_coder
 * replaces inner_coder::make(ninput, noutput, constellation, hierarchy, code_rate) (include/dvbt/inner_coder.h); the mother code and puncturing
 * lib/inner_coder_impl.cc:33-121, forecast and general_work :206-266.  u8 stream -> items of noutput bytes, one m-bit symbol per byte (MSB first).
 * forecast = n_consumed = noutput_items*noutput*k*m/(ninput*8*n) bytes.  noutput_items must be a multiple of 4 (set_output_multiple(4), :172;
 * else DVBT_ERR_INVALID); a call with fewer input bytes produces the largest multiple of 4 items they cover.  noutput % 1512 != 0 is refused (the
 * reference asserts it).  Defined here: ninput must be 1 -- the reference's input items are bytes whatever ninput is (:138) while its consume_each
 * divides by ninput.  hierarchy only selects m's table row; the code rate is code_rate (HP).  The encoder's register (the last 6 info bits) is
 * carried on the device from call to call, starting at zero. */
typedef struct { int ninput, noutput, constellation, hierarchy, code_rate; } dvbt_inner_coder_params;
typedef struct dvbt_inner_coder dvbt_inner_coder;
int  dvbt_inner_coder_create(const dvbt_inner_coder_params *p, dvbt_inner_coder **out);
int  dvbt_inner_coder_forecast(const dvbt_inner_coder *h, int noutput_items, int *ninput_required);
int  dvbt_inner_coder_work(dvbt_inner_coder *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_inner_coder_work_device(dvbt_inner_coder *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                  dvbt_sideband *sb, void *stream);
void dvbt_inner_coder_destroy(dvbt_inner_coder *h);

/* ------------------------------------------------------------------ T5 bit_inner_interleaver
 * replaces bit_inner_interleaver::make(nsize, constellation, hierarchy, transmission) (include/dvbt/bit_inner_interleaver.h); the
 * non-hierarchical branch of general_work lib/bit_inner_interleaver_impl.cc:120-184.  items of nsize bytes (m bits each) -> nsize bytes.
 * nsize must be a multiple of 252 (whole 126-word blocks, 4-byte output words; the payloads 1512 and 6048 are).  hierarchy != NH is refused
 * with DVBT_ERR_INVALID: the reference's hierarchical branch writes d_b[k][v*i/2] beyond its d_b[v][126] matrix, and for 16-QAM writes no
 * low-priority bit at all -- undefined behaviour, not reproducible. */
typedef struct { int nsize, constellation, hierarchy, transmission_mode; } dvbt_bit_inner_interleaver_params;
typedef struct dvbt_bit_inner_interleaver dvbt_bit_inner_interleaver;
int  dvbt_bit_inner_interleaver_create(const dvbt_bit_inner_interleaver_params *p, dvbt_bit_inner_interleaver **out);
int  dvbt_bit_inner_interleaver_forecast(const dvbt_bit_inner_interleaver *h, int noutput_items, int *ninput_required);
int  dvbt_bit_inner_interleaver_work(dvbt_bit_inner_interleaver *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_bit_inner_interleaver_work_device(dvbt_bit_inner_interleaver *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                            dvbt_sideband *sb, void *stream);
void dvbt_bit_inner_interleaver_destroy(dvbt_bit_inner_interleaver *h);

/* ------------------------------------------------------------------ T6 dvbt_map
 * replaces dvbt_map::make(nsize, constellation, hierarchy, transmission, gain) (include/dvbt/dvbt_map.h); lib/dvbt_map_impl.cc:44-171.
 * items of nsize labels -> nsize cfloat: make_constellation_points scaled by gain * norm, with the hierarchy's alpha (ALPHA1/2/4 accepted).
 * nsize must be even (two points per 16-byte store); labels are taken modulo 64. */
typedef struct { int nsize, constellation, hierarchy, transmission_mode; float gain; } dvbt_map_params;
typedef struct dvbt_map dvbt_map;
int  dvbt_map_create(const dvbt_map_params *p, dvbt_map **out);
int  dvbt_map_forecast(const dvbt_map *h, int noutput_items, int *ninput_required);
int  dvbt_map_work(dvbt_map *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_map_work_device(dvbt_map *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                          dvbt_sideband *sb, void *stream);
void dvbt_map_destroy(dvbt_map *h);

/* ------------------------------------------------------------------ T7 reference_signals
 * replaces reference_signals::make(itemsize, ninput, noutput, constellation, hierarchy, code_rate_HP, code_rate_LP, guard_interval,
 * transmission_mode, include_cell_id, cell_id) (include/dvbt/reference_signals.h); pilot_gen::update_output lib/reference_signals_impl.cc:1127-1186
 * and general_work :1289-1314.  items of ninput cfloat (the payload) -> items of noutput cfloat (the FFT length): zeros left and right, payload in
 * carrier order, scattered and continual pilots, TPS (the word re-formatted every symbol).  itemsize must be 8, ninput the payload length and
 * noutput the FFT length of the mode.  symbol_index and frame_index start at 0 and are carried in the handle. */
typedef struct { int itemsize, ninput, noutput, constellation, hierarchy, code_rate_hp, code_rate_lp,
                 guard_interval, transmission_mode, include_cell_id, cell_id; } dvbt_reference_signals_params;
typedef struct dvbt_reference_signals dvbt_reference_signals;
int  dvbt_reference_signals_create(const dvbt_reference_signals_params *p, dvbt_reference_signals **out);
int  dvbt_reference_signals_forecast(const dvbt_reference_signals *h, int noutput_items, int *ninput_required);
int  dvbt_reference_signals_work(dvbt_reference_signals *h, int noutput_items, int ninput_items, const void *in, void *out, dvbt_sideband *sb);
int  dvbt_reference_signals_work_device(dvbt_reference_signals *h, int noutput_items, int ninput_items, const void *in_device, void *out_device,
                                        dvbt_sideband *sb, void *stream);
void dvbt_reference_signals_destroy(dvbt_reference_signals *h);

/* ------------------------------------------------------------------ segment API: the whole chain, device resident
 * One segment = a contiguous run of baseband samples (complex64 at the OFDM elementary rate,
 * i.e. the input of ofdm_sym_acquisition in apps/dvbt_rx_demo*.grc).  The segment is processed
 * exactly as the flowgraph would process it from a cold start (acquire, hunt the superframe
 * start, decode), every stage in HBM; the only host<->device traffic is the input (unless
 * already on the device) and the decoded bytes + report. */
typedef struct {
  int constellation, hierarchy, code_rate, guard_interval, transmission_mode, include_cell_id, cell_id;
  float snr_db;            /* ofdm_sym_acquisition snr, 30 in every demo flowgraph */
  int viterbi_bsize;       /* 768 in every demo flowgraph */
  int rs_oracle_compat;    /* see dvbt_reed_solomon_dec_params */
  int descramble;          /* 1: also run energy_descramble and return TS */
  size_t max_samples;      /* capacity: device buffers are sized for this many input samples */
  int device;              /* HIP device ordinal */
  int viterbi_chunk_bytes; /* 0 = default; decoded bytes per wavefront-chunk */
  int resample_interp, resample_decim;   /* 0,0: the segment is already at the OFDM elementary rate (the north-star tap).
                                            64,70: the segment is the 10 Msps file format; resample + scale run first on the device */
  float front_scale;       /* multiply_const of the flowgraph (used only with resampling; 0 = 1.0) */
  int soft_decision;       /* 0: the reference's hard-decision demapper and Viterbi decoder (the parity path).  1: soft decisions (gr-dvbt's TODO.txt:25-26, never
                              built there): per coded bit an 8-bit max-log likelihood ratio weighted with the carrier's channel power, de-interleaved as soft
                              values, decoded by a soft-input Viterbi decoder; everything behind the decoder unchanged.  No reference exists for it: identical
                              TS on a clean loopback, 2-3 dB of gain at the waterfall (tests/test_gpu_soft.py); the chain takes about 1.6x the hard chain's time.
                              The DEMAP / SYMDEINT / BITDEINT taps are not filled in this mode. */
  int hier_stream;         /* hierarchical modes (hierarchy = ALPHA1 / 2 / 4): which output of bit_inner_deinterleaver feeds the Viterbi decoder: 0 = port 0, the
                              high-priority stream (what a flowgraph that connects the block's first output gets), 1 = port 1, the low-priority stream.
                              The decoder behind it is the reference's: it unpacks d_m bits of every byte whatever the stream carries
                              (lib/viterbi_decoder_impl.cc:93,236-243), so -- as with gr-dvbt itself -- no transport stream comes out of a hierarchical
                              transmission; what is reproduced is every block's output */
  int launch_graph;        /* 1: the ~30 launches of dvbt_rx_segment_enqueue_device are captured in a HIP graph the first time a (segment pointer, length, stream, cut) is
                              seen and replayed as ONE graph launch afterwards (a receiver that works through a resident ring of segments sees the same few
                              over and over).  The graph holds what the launch sequence holds: every size that depends on the data lives in the device-side
                              state block, the grids are worst case.  Not used while stage timing is on (dvbt_rx_enable_timing) or with a resampler in front. */
  int front_priority;      /* 1: dvbt_rx_segment_enqueue_device launches a segment's front end (acquisition .. inner de-interleavers) on a stream of the handle's own
                              with the device's highest priority and joins the caller's stream in front of the Viterbi decoder.  With several segments in flight the
                              front end of segment k + 1 then gets the workgroup slots that segment k's decoder gives up instead of queueing behind them
                              (DESIGN.md 8).  Same kernels, same order within a segment, same bytes. */
  int viterbi_warm_windows;/* 0: the default (72).  The Viterbi decoder runs as independent chunk decoders, each started `warm-up` windows (8 trellis steps = one decoded byte
                              each) in front of its chunk from all-zero metrics; a chunk's decoder IS the streaming decoder of lib/d_viterbi.c from the window on at which
                              its state equals its predecessor's -- inside the warm-up or not depends on the INPUT (of 83,000 chunk starts none is late at a pre-Viterbi bit
                              error rate of 1 %, rate 7/8, SURVEY 8d's prescribed level; two at 2 %; about one in a few hundred on a collapsed channel, >= 3 %, and on the
                              hierarchical modes' degenerate decoder input, for up to ~125 windows: tools/hier_warmup.py).  Since round 6 this parameter
                              moves SPEED only: the launch proves every chunk and decodes the late ones again (viterbi_verify below), so the bytes are the streaming
                              decoder's at any warm-up.  A multiple of 24 in [48, 1152]: that many windows instead of 72 (fewer chunks to decode again, more windows per
                              chunk: 144 costs +2.4 % of the decoder's time at the headline's chunk size, 288 +7.9 %).  Hard-decision decoder. */
  int viterbi_verify;      /* The Viterbi stage is the reference's ONE streaming decoder (viterbi_decoder_impl.cc:192-324, d_viterbi.c:680-735) by construction: every chunk
                              decoder leaves its state (64 path metrics + tie-break bits: two registers per lane) as it stands at its chunk's first window, its
                              predecessor leaves its own at the same window; equal states make equal decisions from there on (oracle/o_viterbi.c::o_viterbi_decode_snap +
                              tests/test_viterbi_boundary_proof_model.py hold the criterion on the CPU), and chunk 0 starts the stream.  A checker lists the chunks whose
                              two states differ, a repair pass decodes each of them again from its predecessor's state (no warm-up needed), and where a repaired decoder
                              does not arrive in the state the next chunk was checked against, one sequential decoder walks on in stream order.  All on the device, the
                              host reads no verdict; the passes return at once when every chunk is proven (the usual case: three small launches, +2 % of the decoder).
                                0  (default) proof + repair;  1  the same plus a final check whose count dvbt_rx_viterbi_check / dvbt_rx_viterbi_proof report (0 by
                                construction);  2  proof only, nothing decoded again: the count says how many chunks the warm-up alone does not prove (statistics);
                                3  test hook: the sequential pass does all the repairs;  4  test hook: every repaired chunk hands the chunk behind it to the sequential pass;  -1  the plain chunk decoders (no states, no passes: equal to the streaming decoder
                                where the warm-up suffices, as until round 5).
                              Chunk sizes are rounded up to a multiple of 24 (unless -1).  Hard-decision decoder; every entry (segment API, streaming entry, hierarchical
                              modes -- which ran ONE decoder on one wavefront until round 5).  The single viterbi_decoder block does the same and carries the state from call to call. */
} dvbt_rx_params;

typedef struct {
  int32_t status;              /* 0 ok; bit0: initial acquisition failed; bit1: CP tracking lost;
                                  bit2: no superframe start found;
                                  bit4: the stream's TPS disagrees with the configured parameters (tps_mismatch);
                                  bit7: a segment that continues a cut stream (dvbt_rx_set_cut) lost the CP lock: its Viterbi stream was laid out from its own
                                  lock periods, the cut offset does not apply to its counts (stream_symbol_offset is reported as 0): do not stitch it;
                                  bit8: dvbt_rx_segment_run gave up walking the segment's lock periods (more than 1024 periods or 4096 searches): the rest is not decoded */
  int32_t n_symbols;           /* OFDM symbols acquired */
  int32_t first_out_symbol;    /* symbol at which superframe_start fired, -1 if none */
  int32_t n_out_symbols;       /* symbols passed downstream */
  int32_t cp_start0;           /* d_cp_start after initial acquisition */
  int32_t first_call;          /* general_work call (window of N+cp samples) in which the initial acquisition succeeded */
  int64_t n_viterbi_bytes;
  int64_t n_rs_items;          /* items of 8 codewords */
  int64_t n_rs_bytes;          /* RS words decoded x 188 (= n_rs_items*1504 unless the segment continues a cut stream) */
  int64_t n_ts_bytes;          /* after energy_descramble (0 when descramble==0) */
  int32_t rs_fail_words, rs_corrected_symbols;
  int64_t resume_sample;       /* status bit1 (lock lost): sample of the caller's segment (at the OFDM elementary rate) at which the reference
                                  would start re-acquiring: the call that lost the lock consumes half a window (N+cp)/2; else 0.
                                  dvbt_rx_segment_run restarts there by itself while no superframe start has been found yet (the
                                  start-up transient of a segment that begins with more than one window of silence). */
  int64_t segment_offset;      /* sample of the caller's segment (OFDM elementary rate) at which the reported decode started: 0 unless
                                  dvbt_rx_segment_run restarted; cp_start0, first_call and the CP_START tap count from here */
  /* cut streams (dvbt_rx_set_cut) */
  int64_t stream_symbol_offset; /* the cut's offset, echoed */
  int64_t ts_first_packet;     /* index, among this segment's RS words, of the first packet of the TS tap */
  int64_t stream_rs_items;     /* items of 8 RS words a chain over the whole stream has produced up to this segment's end */
  /* transmission parameters as signalled by the stream (TODO.txt:25-28 "TPS auto-detection"): the TPS word of a frame that passed the
   * BCH check (reference_signals_impl.cc:385-425), decoded per the layout of format_tps_data (:883-916).  The values use the enums above
   * (they double as the TPS encodings).  status bit 4 is raised when they disagree with the handle's parameters: the segment is still
   * decoded as configured (the reference does not look at them either), but its bytes are then meaningless. */
  uint64_t tps_bits;           /* bit i = s_i; s1-s16 (sync word), s23-s24 (frame number) and s54-s67 (parity) cleared */
  int32_t tps_valid;           /* 1: a BCH-valid TPS frame was received and the fields below are set */
  int32_t tps_length_indicator, tps_constellation, tps_hierarchy, tps_code_rate_hp, tps_code_rate_lp,
          tps_guard_interval, tps_transmission_mode, tps_cell_id;
  int32_t tps_mismatch;        /* bit0 constellation, bit1 hierarchy, bit2 HP code rate, bit3 guard interval, bit4 transmission mode differ */
  /* lock periods (dvbt_rx_segment_run / _run_device follow the reference through every loss of the CP lock inside the segment) */
  int32_t n_lock_periods;      /* periods that found a superframe start and delivered items; > 1: the front-end fields above (n_symbols,
                                  first_out_symbol, cp_start0, first_call, segment_offset, the debug taps) describe the LAST one, the stream
                                  fields (n_viterbi_bytes .. n_ts_bytes, the VITERBI/DEINT/RS/TS taps) the whole segment */
  int32_t total_symbols;       /* OFDM symbols acquired over all lock periods */
} dvbt_rx_report;

typedef enum {
  DVBT_TAP_ACQ = 0,        /* cfloat[n_symbols][N]     output of A1 */
  DVBT_TAP_FFT = 1,        /* cfloat[n_symbols][N]     output of A2 (like ACQ/DEMAP/SYMDEINT/DEINT a debug tap: dvbt_rx_enable_taps first) */
  DVBT_TAP_EQ = 2,         /* cfloat[n_out_symbols][payload]  output of A3 (the float-tolerance tap; written only after dvbt_rx_enable_taps) */
  DVBT_TAP_DEMAP = 3,      /* u8[n_out_symbols][payload] */
  DVBT_TAP_SYMDEINT = 4,
  DVBT_TAP_BITDEINT = 5,
  DVBT_TAP_VITERBI = 6,    /* u8[n_viterbi_bytes] */
  DVBT_TAP_DEINT = 7,      /* u8[n_rs_bytes/188*204] */
  DVBT_TAP_RS = 8,         /* u8[n_rs_bytes] */
  DVBT_TAP_TS = 9,         /* u8[n_ts_bytes] */
  DVBT_TAP_CP_START = 10,  /* i32[n_symbols] */
  DVBT_TAP_SYMBOL_INDEX = 11, /* i32[n_symbols - 1] */
  DVBT_TAP_FREQ_OFFSET = 12, /* i32[n_symbols - 1]  integer carrier offset found for each demodulated symbol (reference_signals_impl.cc:715-744) */
  DVBT_TAP_BITDEINT_LP = 13, /* u8[n_out_symbols][payload]  hierarchical modes: the bit de-interleaver's second output (BITDEINT holds the first) */
  DVBT_TAP_SOFT = 14,      /* i8[n_out_symbols][payload * m]  soft-decision mode: the log-likelihood ratio of every coded bit in the decoder's input order (behind both
                              inner de-interleavers); > 0: the bit is more likely 0.  The EQ tap is its input (always filled in this mode) ... */
  DVBT_TAP_BITDEINT_LOG = 16, /* u8[...]  dvbt_rx_enable_taps(h, 2): the Viterbi decoder's input of every lock period (dvbt_rx_period_taps says where) */
  DVBT_TAP_CSI = 15        /* f32[n_out_symbols][payload]  ... together with the channel state of every carrier, 1 / |interpolated equaliser gain|^2 */
} dvbt_tap;

typedef struct dvbt_rx dvbt_rx;
int  dvbt_rx_create(const dvbt_rx_params *p, dvbt_rx **out);
/* Cut streams (the path shards over independent baseband segments).  A long stream is cut near superframe
 * boundaries; every piece is decoded as a segment of its own (other handle, stream or GPU).  A piece that does not hold the
 * beginning of the stream begins a pre-roll before the superframe start it is to deliver (long enough for CP lock and one
 * whole TPS frame) and declares, before it is enqueued, how many OFDM symbols lie between the stream's FIRST superframe
 * start (where the reference's chain starts decoding: demod_reference_signals_impl.cc:118-136) and its own: a multiple of
 * 272.  The library then takes the Viterbi block count (viterbi_decoder_impl.cc:198), the ntraceback delay and the even
 * item count of the byte de-interleaver (convolutional_deinterleaver_impl.cc:55-61) in stream coordinates, and the TS tap
 * starts at the piece's first NSYNC and runs in whole 8-packet groups to the end of its RS words (no two-item hold-back,
 * energy_descramble_impl.cc:139-141: that belongs to the stream's end).  The first RS words of a piece mix the
 * de-interleaver's zero fill with data, as at a stream start: the piece before delivers those packets (post-roll).
 * gr_dvbt_amd/multi.py (plan_cuts / stitch_ts) holds the host side: concatenating the trimmed pieces gives, byte for byte,
 * the TS of one chain over the whole stream.  offset 0 (the default) = the piece holds the beginning of the stream. */
typedef struct {
  int64_t stream_symbol_offset;
  /* the two fields below are what the streaming entry (dvbt_rx_stream_*) knows about the stream a piece continues; 0 / 0 = the plain cut above.
   * start_delay_symbols (0..271): the piece delivers from this many OFDM symbols BEHIND the superframe start its own pilot engine finds.  The reference's
   * demodulator re-hunts the superframe start after a lost CP lock on counters that went on counting through the gap (lib/demod_reference_signals_impl.cc:115-136,
   * the pilot engine's members live on): when no whole TPS frame lies between the new lock and the counters' next "frame d_fi_start, symbol 0", it declares the
   * start there -- a whole number of symbols off the transmitted grid -- and decodes from that symbol until the next loss.  Pieces that continue such a lock
   * period must start where the reference's chain counts from.
   * descr_call_phase: 1 + (first packet of the whole-stream descrambler's two-item calls, mod 16, counted in this piece's RS words); 0 = unknown.  When known
   * the piece checks that every such call inside it finds its NSYNC (lib/energy_descramble_impl.cc:121-141 re-searches otherwise) and reports the outcome
   * to the streaming entry, which then follows the descrambler call by call. */
  int32_t start_delay_symbols;
  int32_t descr_call_phase;
} dvbt_rx_cut;
int  dvbt_rx_set_cut(dvbt_rx *h, const dvbt_rx_cut *cut);   /* applies to the segments enqueued afterwards */
/* iq: host pointer to nsamples complex64 (copied to the device first) */
int  dvbt_rx_segment_run(dvbt_rx *h, const void *iq_host, size_t nsamples, dvbt_rx_report *report);
/* the same for a segment that is already in device memory (stream: a hipStream_t or NULL).  Like dvbt_rx_segment_run it is synchronous
 * and follows the reference through every loss of the CP lock inside the segment (ofdm_sym_acquisition_impl.cc:545-559: half a window
 * consumed, full search again; demod_reference_signals hunts the superframe start again, :115-136; the Viterbi decoder is reset at the
 * new start and the byte de-interleaver realigned, viterbi_decoder_impl.cc:213-229, convolutional_deinterleaver_impl.cc:109-120; the
 * descrambler re-searches its NSYNC, energy_descramble_impl.cc:121-141).  dvbt_rx_segment_enqueue_device below never waits for the
 * device: it decodes the segment's FIRST lock period and reports where the lock ended (status bit 1, resume_sample). */
int  dvbt_rx_segment_run_device(dvbt_rx *h, const void *iq_device, size_t nsamples, void *stream, dvbt_rx_report *report);
/* iq_device: device pointer (hipMalloc'd, e.g. a torch tensor's data_ptr). stream: a hipStream_t or NULL.
 * Asynchronous w.r.t. the host: enqueue only.  Use dvbt_rx_segment_finish to wait and fetch the report. */
int  dvbt_rx_segment_enqueue_device(dvbt_rx *h, const void *iq_device, size_t nsamples, void *stream);
int  dvbt_rx_segment_finish(dvbt_rx *h, dvbt_rx_report *report);
/* the CP-lock periods the last dvbt_rx_segment_run / _run_device walked through (ofdm_sym_acquisition alone, in stream order): where the
 * search that found the lock started, the call and d_cp_start of the initial acquisition, how many symbols the lock held.  A period with
 * n_symbols == 0 is a peak that the tracking search of the same call already missed (ofdm_sym_acquisition_impl.cc:503-559).  Returns the
 * number of periods (may exceed cap). */
typedef struct {
  int64_t offset;             /* sample of the segment (OFDM elementary rate) at which this search began */
  int32_t first_call;         /* window (of N+cp samples, from offset) in which the initial acquisition found its peak */
  int32_t cp_start0;          /* d_cp_start of that call */
  int32_t n_symbols;          /* items the lock delivered before it was lost (or the segment ended) */
  int32_t first_out_symbol;   /* 1 + symbol of the period at which superframe_start fired, 0 if it delivered nothing downstream */
} dvbt_lock_period;
/* what the proof + repair passes of the handle's last launch of the Viterbi decoder did (see dvbt_rx_params.viterbi_verify) */
int  dvbt_rx_viterbi_proof(dvbt_rx *h, dvbt_viterbi_proof *out);
/* the same counters summed over every launch of the handle's decoder since it was created (a synchronous run launches the decoder once per lock period); not_proven = -1 */
int  dvbt_rx_viterbi_proof_total(dvbt_rx *h, dvbt_viterbi_proof *out);
/* always != 0: the Viterbi decoder's traceback chains walk every hop instead of taking the shortcut over chained best states (the same bytes); drops the captured graphs */
int  dvbt_rx_set_viterbi_walk(dvbt_rx *h, int always);
/* out[0], out[1]: blocks of 24 windows, per wavefront, whose bytes left by the shortcut / whose chains walked, since the handle was created (viterbi_verify >= 0) */
int  dvbt_rx_viterbi_shortcut(dvbt_rx *h, long long out[2]);
/* (chunks, not_proven) of the same; needs the final check (viterbi_verify >= 1) */
int  dvbt_rx_viterbi_check(dvbt_rx *h, int64_t *chunks, int64_t *unproven);
int  dvbt_rx_lock_periods(dvbt_rx *h, dvbt_lock_period *out, int cap);
/* how the handle's lock-period walks ran so far: acquisition-only passes through the one-launch tracker (acq_small_kernel: look-ahead windows of up to
 * small_max_calls calls, the tracking metric in chunks of small_chunk_calls calls -- 16 for a short guard interval down to 2 for cp = 2048, what fits the LDS) and
 * through the general kernels (long windows, periods the one-launch tracker handed back) */
typedef struct { int64_t small_passes, general_passes; int32_t small_chunk_calls, small_max_calls; } dvbt_walk_stats;
int  dvbt_rx_walk_stats(dvbt_rx *h, dvbt_walk_stats *out);
/* copy a tap of the last finished segment to host memory; returns bytes written */
int64_t dvbt_rx_read_tap(dvbt_rx *h, int tap, void *dst_host, size_t cap_bytes);
/* device pointer of a tap's buffer (for RCCL gathers of the decoded packets) */
void *dvbt_rx_tap_device_ptr(dvbt_rx *h, int tap);
/* average device time in ms of the named stage over the segments finished since the last
 * dvbt_rx_enable_timing(h, 1) (HIP events on the segment's stream); stage names: "acq","fft","demod","inner","viterbi","rs","total".
 * dvbt_rx_enable_timing(h, 2): events around the decoder only ("viterbi"; the other names return -1) -- an event record holds an otherwise
 * idle stream for ~6 us, seven of them are 1 % of a step that runs alone.  0 switches the events off. */
double dvbt_rx_stage_ms(dvbt_rx *h, const char *stage);
int  dvbt_rx_enable_timing(dvbt_rx *h, int enable);
/* allocate (1) / free (0) the debug-only taps ACQ, DEMAP, SYMDEINT, DEINT; the other taps are
 * pipeline buffers and always readable.  Call before the segment whose taps are wanted.
 * 2: the same plus the per-lock-period log of the Viterbi decoder's input (dvbt_rx_period_taps): the BITDEINT tap holds the LAST period of a
 * segment that lost its lock, the log keeps every period's (synchronous entries dvbt_rx_segment_run / _run_device). */
int  dvbt_rx_enable_taps(dvbt_rx *h, int enable);
/* one entry per lock period of the last synchronous run that reached the Viterbi decoder, in stream order: where its decoder input lies in the
 * log (DVBT_TAP_BITDEINT_LOG) and where its decoded bytes lie in the VITERBI tap */
typedef struct { int64_t bitdeint_offset, bitdeint_bytes, viterbi_offset, viterbi_bytes; } dvbt_period_tap;
int  dvbt_rx_period_taps(dvbt_rx *h, dvbt_period_tap *out, int cap);   /* returns the number of entries */
/* Blind signal-quality measurement of the last finished segment (INTEGRATION.md "Signal quality"): a pass of its own over what the segment left on the device,
 * launched by dvbt_rx_quality alone -- never part of the chain's launch sequence.  MER = 10 log10(mer_signal / mer_error) over the equalised payload carriers
 * against the constellation point of the demapper's own decision; channel_*: the decoder's output re-encoded against the decoder's input (pre-Viterbi);
 * post_*: what the RS decoder changed in the 188 data bytes of every word (post-Viterbi; words it gave up on add nothing). */
typedef struct {
  int64_t mer_carriers;  double mer_signal, mer_error;          /* mer_carriers == 0: not measured */
  int64_t channel_bits, channel_bit_errors;                     /* channel_bits == 0: not measured */
  int64_t post_bits, post_bit_errors;
  int32_t rs_fail_words, rs_corrected_symbols, n_lock_periods, flags;  /* echoed from the report; flags bit0: EQ not enabled, bit1: more than one lock period */
} dvbt_rx_quality_report;
/* 1: allocate the equalised-carrier buffer (8 bytes per payload carrier of max_samples; the symbol kernel then runs its instantiation that writes it) and the
 * result buffers; 0: free it unless dvbt_rx_enable_taps or soft mode holds it.  Call before the segment to be measured.  DVBT_ERR_STATE while a segment is pending. */
int  dvbt_rx_enable_quality(dvbt_rx *h, int enable);
/* Behind dvbt_rx_segment_finish / _run / _run_device and before the next enqueue (else DVBT_ERR_STATE): launches the measurement on the handle's own stream,
 * synchronises and fills *out.  Without dvbt_rx_enable_quality the MER is not measured (flags bit0).  A segment of more than one lock period: MER and channel
 * figures not measured (flags bit1; the front-end buffers hold the last period only), post_* over the whole segment.  DVBT_ERR_INVALID for a hierarchical
 * handle, DVBT_ERR_STATE for a soft-decision handle or one with a cut set (dvbt_rx_set_cut). */
int  dvbt_rx_quality(dvbt_rx *h, dvbt_rx_quality_report *out);
void dvbt_rx_destroy(dvbt_rx *h);

/* ------------------------------------------------------------------ streaming entry: the whole chain behind push / pull
 * What a C++ host (one gr::block whose work() takes cfloat and gives TS bytes, gr_dvbt_amd/host/gr/rx_hip_impl.cc) needs to decode a
 * stream of any length at the segment API's speed: samples are pushed in calls of ANY size (complex64 at the OFDM elementary rate, the
 * input of ofdm_sym_acquisition in apps/dvbt_rx_demo*.grc), the library batches them into pieces of whole superframes with the pre- and
 * post-roll of SURVEY 8e (one CP lock + one whole TPS frame in front of a piece's first superframe boundary, the byte de-interleaver's
 * fill and the distance to the next NSYNC behind its last one), decodes every piece device resident on one of two internal chains (the
 * next piece's samples are copied in while the previous one decodes), trims the pieces and delivers the TS in order.  The bytes are
 * exactly those of ONE chain over the whole stream (dvbt_rx_segment_run on all samples at once; tests/test_gpu_stream.py), i.e. what the
 * reference's flowgraph writes to its file sink: this is gr_dvbt_amd/multi.py's plan_cuts / stitch_plan inside the library.
 * segment_superframes: superframes a piece owns (0 = 16; device memory ~ 2 x (segment_superframes + 3) superframes of samples + the
 * chains' own buffers).  rx.max_samples, rx.resample_* are ignored / must be 0 (no resampler in front).
 * A piece is decoded once the stream is known to go on far enough for the next piece to stand on its own (one superframe + 76 symbols behind its begin), so the
 * TS lags the input by about segment_superframes + 1 superframes.
 * A lost CP lock: the stream follows the reference through it, byte for byte (tests/test_gpu_stream.py, tests/test_gpu_stream_loss.py: dropouts, noise bursts,
 * BASELINE config 5 at 9 dB).  While no lock period is established -- at the stream's beginning and from a piece in which the lock is lost -- the stream is WALKED
 * window by window (the lock-period walk of dvbt_rx_segment_run with the blocks' state carried from window to window: the peak detector's average, the pilot engine's
 * counters that go on counting through the gap, the byte de-interleaver's alignment and contents, the descrambler's call phase), synchronously; once a lock period
 * has held for two superframes behind its superframe start the stream goes back to pieces, cut on the superframe grid the reference's chain counts on -- also when
 * that grid is a whole number of symbols off the transmitted one (a superframe start declared on stale counters, lib/demod_reference_signals_impl.cc:115-136: the
 * reference decodes garbage from there to the next loss, and so does the stream).  status bit 1 reports the loss; dvbt_rx_stream_trace tells what was done.
 * Sharded streams (world > 1): a rank walks a lost lock to the end of its own piece's samples; the result is the single chain's whenever the reference's chain is
 * back in a lock period on the transmitted grid in front of the next piece's first superframe start and its descrambler has found its NSYNC again on the epoch's
 * own 16-packet call grid (status bit 5 otherwise: the other ranks cannot know).  A stream that never establishes a lock period (config 5 at 9 dB) is walked by
 * every rank and delivered by rank 0.
 * At the lock's edge a piece's fresh acquisition may drop -- or not find -- a lock that the chain before it has seen hold; the piece is then started again behind
 * that loss (a few symbols later; the walk takes over beyond six): it is not a loss of the stream and is not reported as one.
 * Memory per stream object (S = segment_superframes, sf = one superframe of samples = 272 (N + cp) x 8 bytes: 18.4 MB at 8k, 4.6 MB at 2k, guard 1/32):
 *   device: per chain (two by default, `chains`) a sample buffer of (S + 3.7) sf + the chain's own buffers (~0.55 x a sample buffer; x 2.2 in soft-decision mode);
 *   S = 16 at 8k: 2 x 362 MB + 2 x ~200 MB.  The first lost lock adds two walk buffers of twice a sample buffer each (2 x 725 MB at S = 16, 8k), and the buffers behind the
 *   walking chain's Viterbi decoder grow to what a window of that size can lay out (three more buffers of ~2.2 x a piece's decoded bytes: +115 MB at S = 16, 8k QAM64 7/8).
 *   A walk's window is bounded by those buffers: a lock that holds for more than two pieces and a threshold of samples (2 x the sample buffer + (STREAM_PRE + 272) symbols)
 *   without ever reaching a superframe start -- no decodable TPS word: nothing the reference would deliver either -- is cut: the walk starts afresh two superframes back, status bits
 *   2 and 5 are raised and dvbt_rx_stream_trace says so.  With device output (dvbt_rx_stream_set_device_output) a piece's packets are handed over in the chain's TS buffer and the chain
 *   takes a spare one: up to one more TS buffer (~0.25 x a sample buffer) per piece whose packets wait for an exchange step;
 *   page-locked host: the TS ring (ts_ring_bytes, default 96 MB; a consumer that falls further behind is served from the heap) and 32 MB of staging for host
 *   pushes below 2 MB; both taken at create (page-locking them takes ~10 ms: set-up, not the first piece's latency).
 * Threading: like every handle, one thread at a time. */
/* TPS auto-configuration (gr-dvbt's TODO.txt:28 "Autodetect transmission params"): rx.constellation, rx.hierarchy and / or rx.code_rate = DVBT_AUTO.  The
 * transmission mode and the guard interval must be given (the front end is built from them); everything else the stream says itself: the head of the stream
 * (two TPS frames and a margin: 160 symbols + one window) is held back, a probe chain reads a BCH-valid TPS word out of it (lib/reference_signals_impl.cc:385-425,
 * field layout :883-916), the chains are built for what it names and the head is replayed into them -- the TS is that of a stream created with those
 * parameters (tests/test_gpu_tps.py).  While no valid word has been seen the look-ahead doubles (up to four attempts); then push fails with DVBT_ERR_STATE. */
typedef struct {
  dvbt_rx_params rx; int segment_superframes;
  /* sharding over the GPUs of a node, one stream object per process / GPU: every rank is pushed the SAME stream; piece k >= 1 belongs to rank
   * k % world, which alone copies its samples to the device and decodes it (piece 0, the plan, is decoded by every rank and delivered by rank 0).  A rank
   * pulls its own packets with their index in the stream (dvbt_rx_stream_pull_chunk); all ranks' chunks ordered by that index are the single chain's TS:
   * gathering them is the design's one exchange step (RCCL over xGMI in bench.py / gr_dvbt_amd/multi.py).  world = 0 or 1: no sharding. */
  int rank, world;
  /* page-locked ring the decoded TS waits in until it is pulled (0 = 96 MB, ~24 s of the fastest DVB-T transport stream); a consumer that falls further behind
   * than this -- and a stream that cannot have the ring -- is served from heap chunks; dvbt_rx_stream_set_device_output gives it back */
  int64_t ts_ring_bytes;
  /* 1: the samples handed to dvbt_rx_stream_push_device are BORROWED, not copied: the stream remembers where they are and reads them there -- a piece that lies in one
   * contiguous stretch of the caller's memory is decoded in place, a piece across two stretches and the windows of a walk are gathered when they are needed.  The caller keeps
   * the samples valid and unchanged until dvbt_rx_stream_info.samples_released has passed them (a ring of segments resident in HBM does).  dvbt_rx_stream_push (host memory)
   * is refused on such a stream; not together with DVBT_AUTO.  0: every push copies (the default: the caller's buffer is free when the call returns). */
  int borrow_device_pushes;
  /* chains (handle + sample buffer + HIP stream) of the stream object: 0 = 2 (the default), or 2 .. 4.  The pieces take them in turn; `chains - 1` pieces decode while the next one
   * fills, and the small latency-bound kernels of the later pieces run in the gaps of the earlier pieces' decoders (the segment API's "several segments in flight"):
   * 4 chains: 4.3 instead of 4.5 ms per 64-superframe piece at the headline workload -- for twice the device memory (every chain has its sample buffer and its buffers behind the
   * decoder; the walk's buffers hold `chains` sample buffers and a threshold).  Same bytes. */
  int chains;
} dvbt_rx_stream_params;
typedef struct {
  int32_t status;              /* dvbt_rx_report.status bits of the pieces, OR-ed (bit 1 only when the lock was lost inside a piece) | bit 5: a piece
                                  delivered fewer packets than its span of the stream | bit 6: a piece's sync byte was not where the stream's packet
                                  count puts it */
  int32_t pieces_in_flight, finished;
  int64_t samples_pushed, ts_bytes_decoded, ts_bytes_ready, ts_bytes_pulled;
  int64_t first_superframe_call;   /* call (window of N+cp samples) of the stream's first superframe start, -1 before it is known */
  int64_t first_ts_packet;         /* RS word (counted from that superframe start) of the first TS packet, -1 before it is known */
  int32_t constellation, hierarchy, code_rate;   /* the parameters the chains run with; -1 while they are being detected (DVBT_AUTO) */
  int32_t auto_configured;         /* 1: they were taken from the stream's TPS word */
  int64_t samples_released;        /* borrow_device_pushes: the stream will not read samples in front of this stream position again (else = samples_pushed) */
  int32_t in_walk;                 /* 1: no lock period is established (the stream's beginning, or behind a lost CP lock): the stream is being walked window by window */
} dvbt_rx_stream_info;
typedef struct dvbt_rx_stream dvbt_rx_stream;
int  dvbt_rx_stream_create(const dvbt_rx_stream_params *p, dvbt_rx_stream **out);
/* iq_host: nsamples complex64 in host memory; they have left the caller's buffer when the call returns (the decode has not finished) */
int  dvbt_rx_stream_push(dvbt_rx_stream *s, const void *iq_host, size_t nsamples);
/* the same for samples in device memory, ordered behind `stream` (a hipStream_t or NULL); the caller keeps them valid until that copy has run */
int  dvbt_rx_stream_push_device(dvbt_rx_stream *s, const void *iq_device, size_t nsamples, void *stream);
/* TS bytes that are ready, in stream order, up to cap; never waits for the device before dvbt_rx_stream_finish.  Returns the bytes written */
int64_t dvbt_rx_stream_pull(dvbt_rx_stream *s, void *ts_host, size_t cap);
/* one contiguous run of this rank's packets (never across two pieces) and the index of its first packet in the stream's TS (packet 0 = the first packet
 * the single chain delivers is *first_packet == first_ts_packet of dvbt_rx_stream_info): what a sharded stream's ranks exchange.  cap >= 188 */
int64_t dvbt_rx_stream_pull_chunk(dvbt_rx_stream *s, void *ts_host, size_t cap, int64_t *first_packet);
/* end of the stream: decodes what is left (energy_descramble's two-item hold-back and the block roundings apply here, as at the end of
 * the reference's run) and waits for it; pull then drains the rest */
int  dvbt_rx_stream_finish(dvbt_rx_stream *s);
int  dvbt_rx_stream_status(const dvbt_rx_stream *s, dvbt_rx_stream_info *info);
/* what the stream did, as text: one line per walk window, per epoch that was established, per piece that left its epoch (a lost CP lock) or whose descrambler
 * had to be followed on the host; returns the trace's length (the text is cut to cap - 1 characters, 0-terminated).  Bounded at 64 KB. */
int64_t dvbt_rx_stream_trace(const dvbt_rx_stream *s, char *dst, size_t cap);
/* the Viterbi stage's proof + repair passes (dvbt_rx_params.viterbi_verify: the stream's chains run them like every handle) summed over the stream's launches so far */
int  dvbt_rx_stream_viterbi_proof(const dvbt_rx_stream *s, dvbt_viterbi_proof *out);
void dvbt_rx_stream_destroy(dvbt_rx_stream *s);

/* ------------------------------------------------------------------ the exchange step of a sharded stream
 * north_star: "C++ host code ... a single RCCL gather of decoded TS packets over xGMI".  One process per GPU; every process creates a dvbt_rx_stream with its
 * rank / world, is pushed the same stream and decodes its own pieces (no data-path collective).  Per step, dvbt_rx_stream_gather moves every rank's next run
 * of finished packets to `root` in ONE group of ncclSend / ncclRecv on device buffers (a gather of fixed-stride slots: 64-byte header {first packet index,
 * byte count, drained flag, error flag} + packets, the layout of gr_dvbt_amd/multi.py; the headers go to every rank in the same group) and hands root the runs
 * with their packet indices; ordered by that index they are the single chain's TS.  librccl.so is opened with dlopen at first use (no link-time dependency).  The communicator can come from here
 * (dvbt_rccl_unique_id on one rank, its 128 bytes carried to the others by the host -- a file, a socket, MPI --, then dvbt_rccl_comm_create everywhere:
 * ncclGetUniqueId / ncclCommInitRank), so a host needs no RCCL headers.  gr_dvbt_amd/host/rx_multi_example.cpp is such a host. */
typedef struct dvbt_rccl_comm dvbt_rccl_comm;
int  dvbt_rccl_unique_id(void *id128_out);                                    /* 128 bytes */
int  dvbt_rccl_comm_create(const void *id128, int rank, int world, int device, dvbt_rccl_comm **out);   /* collective over the `world` processes */
void dvbt_rccl_comm_destroy(dvbt_rccl_comm *c);
typedef struct { int64_t first_packet; int64_t nbytes; int64_t offset; } dvbt_gather_chunk;   /* rank r's run: packet index in the stream's TS, bytes, where they sit in ts_host */
/* The step, asynchronous and double-buffered (what a host that wants the exchange behind its decode calls; bench.py's Python path does the same with
 * torch.distributed).  dvbt_rx_stream_set_device_output (before the first push): the decoded TS stays in device memory (a ring of ring_bytes, 0 = 64 MB; pull /
 * pull_chunk then refuse; a piece's packets wait in the very buffer they were decoded into, ring_bytes holds the walk's smaller runs) and a step copies its run device to
 * device into the send slot -- no PCIe hop on any rank but the root's one download (none with DVBT_GATHER_DEVICE, below).
 * dvbt_rx_stream_gather_enqueue: collective (the same root and slot_packets on every rank; a rank gives at most slot_packets packets per step); issues ONE group of
 * ncclSend / ncclRecv on the communicator's own HIP stream -- the slot to the root, the 64-byte header to every rank -- and returns at once; at most two steps in
 * flight.  dvbt_rx_stream_gather_wait: the oldest step in flight.  root: ts_host (cap >= world * slot_packets * 188) receives the runs in rank order, chunks[world]
 * describes them; returns the bytes written.  Others: ts_host / chunks may be NULL; returns 0.  *all_done (every rank, from the headers of the same step) = 1 once
 * every rank's stream is finished and drained.  A rank that fails in front of a step's group sends an empty slot with an error flag: the step completes
 * everywhere and fails on every rank (DVBT_ERR_STATE) -- no rank is left waiting.  Receive space is allocated on the root only. */
int  dvbt_rx_stream_set_device_output(dvbt_rx_stream *s, size_t ring_bytes);
int  dvbt_rx_stream_gather_enqueue(dvbt_rx_stream *s, dvbt_rccl_comm *c, int root, int slot_packets);
int64_t dvbt_rx_stream_gather_wait(dvbt_rx_stream *s, dvbt_rccl_comm *c, void *ts_host, size_t cap, dvbt_gather_chunk *chunks, int *all_done);
/* root, after a wait with ts_host = NULL: the runs stay where the step's download put them -- chunks[r].offset then counts from this page-locked buffer (valid
 * until the second next wait): a root that writes the packets on needs no copy of its own (at the headline rate the TS is ~15 GB/s).  The download copies, per
 * rank, the header and the bytes the header declares -- not the slot. */
const void *dvbt_rccl_step_buffer(const dvbt_rccl_comm *c);
/* The step that leaves the runs in the ROOT'S DEVICE MEMORY (north_star: the clock ends at "last TS byte resident on rank 0"): dvbt_rx_stream_gather_enqueue_ex with
 * DVBT_GATHER_DEVICE downloads nothing but the 64-byte headers; dvbt_rx_stream_gather_wait (ts_host = NULL) describes the runs in chunks[], offsets counted from
 * dvbt_rccl_step_device_buffer (device pointer, valid until the second next wait).  flags = 0: dvbt_rx_stream_gather_enqueue.  Same flags on every rank. */
#define DVBT_GATHER_DEVICE 1
int  dvbt_rx_stream_gather_enqueue_ex(dvbt_rx_stream *s, dvbt_rccl_comm *c, int root, int slot_packets, int flags);
const void *dvbt_rccl_step_device_buffer(const dvbt_rccl_comm *c);
/* the exchange buffers for steps of slot_packets packets towards root (flags as above: without DVBT_GATHER_DEVICE the root also gets its page-locked mirror).  The
 * enqueue calls it itself; called first, on every rank, it moves an allocation failure in front of the first step (inside a step such a failure becomes an error-flag
 * slot sent from the stream's sample buffer, so that no rank waits -- see dvbt_rccl.inc) */
int  dvbt_rccl_comm_reserve(dvbt_rccl_comm *c, int root, int slot_packets, int flags);
/* the two at once (blocking): one group and one synchronisation per step */
int64_t dvbt_rx_stream_gather(dvbt_rx_stream *s, dvbt_rccl_comm *c, int root, int slot_packets, void *ts_host, size_t cap, dvbt_gather_chunk *chunks, int *all_done);

/* ------------------------------------------------------------------ the modulator: transport stream -> OFDM baseband
 * replaces the chain of apps/dvbt_tx_demo*.grc: energy_dispersal, reed_solomon_enc, convolutional_interleaver, inner_coder, bit_inner_interleaver,
 * symbol_inner_interleaver(direction=1), dvbt_map, reference_signals, fft_vxx(forward=False, shift=True), the cyclic prefixer and multiply_const(scale).
 * A handle modulates ONE transport stream delivered over any number of calls of any number of 188-byte packets.  Each call emits every whole OFDM symbol
 * (N + cp cfloat samples, cyclic prefix first) that the packets received so far make possible; the outputs of all calls, concatenated, are the output of one
 * modulator run over the whole stream: floor(P * 1632 / info_bits_per_symbol) symbols for P packets.  The handle carries the dispersal group phase, the byte
 * interleaver's memory, the info bits that did not fill a symbol, the encoder's history and symbol_index / frame_index from call to call.  The encoder and the
 * interleaver start from zero, symbol_index and frame_index from 0; first_packet sets only the phase of the 8-packet dispersal groups.  Hierarchical modes
 * (hierarchy = ALPHA1/2/4) change the constellation's alpha and the TPS word; the bit interleaver is the non-hierarchical one (a single stream).
 * DVBT_ERR_CAPACITY (npackets > max_packets, or cap_samples < the call's output) and DVBT_ERR_INVALID leave the stream's state unchanged.  One thread per handle;
 * calls on different streams are ordered by the handle (an event).  There is no CPU path: without a GPU dvbt_tx_create returns DVBT_ERR_NO_DEVICE. */
typedef struct {
  int constellation, hierarchy, code_rate, guard_interval, transmission_mode, include_cell_id, cell_id;
  float scale;            /* multiply_const behind the cyclic prefixer (apps/dvbt_tx_demo*.grc: 0.0022097087); must be > 0 */
  size_t max_packets;     /* capacity of one call (at most 2^24) */
  int64_t first_packet;   /* index of the first packet in the whole TS: sets only the phase of the 8-packet dispersal groups */
  int keep_carriers;      /* 1: keep the last call's frequency-domain frames for dvbt_tx_read_carriers */
  int device;
} dvbt_tx_params;
typedef struct dvbt_tx dvbt_tx;
int     dvbt_tx_create(const dvbt_tx_params *p, dvbt_tx **out);
int64_t dvbt_tx_samples_for(const dvbt_tx *h, size_t npackets);   /* samples the NEXT call with npackets will produce */
/* host buffers: synchronous */
int     dvbt_tx_run(dvbt_tx *h, const void *ts_host, size_t npackets, void *iq_host, size_t cap_samples, size_t *nsamples);
/* device buffers (ts_device 4-byte aligned, iq_device 8-byte aligned): enqueues on `stream` (NULL: the default stream) and returns; *nsamples is known without
 * waiting for the device */
int     dvbt_tx_run_device(dvbt_tx *h, const void *ts_device, size_t npackets, void *iq_device, size_t cap_samples, void *stream, size_t *nsamples);
/* keep_carriers: the last call's IFFT input, cfloat[nsym][N] in frequency order (carrier c at index zeros_on_left + c), unscaled; returns the bytes
 * (dst_host NULL: the bytes it would copy); waits for the call */
int64_t dvbt_tx_read_carriers(dvbt_tx *h, void *dst_host, size_t cap_bytes);
int     dvbt_tx_reset(dvbt_tx *h);      /* back to the start of a stream */
void    dvbt_tx_destroy(dvbt_tx *h);

/* ------------------------------------------------------------------ test hooks (used by tests/ only)
 * the two peak detectors of the acquisition's trackers (lib/ofdm_sym_acquisition_impl.cc:72-146 restated sample by sample, and the wavefront-wide form the
 * sequential trackers run) on n cases of 16 metric values + a carried d_avg each: out[4k] npk, out[4k+1] position (-1: none) of the first, out[4k+2..3]
 * of the second; avg_out[2k], avg_out[2k+1]: d_avg after the window */
int dvbt_debug_peak_detect(const float *lambda_host, const float *avg_host, int n, int32_t *out_host, float *avg_out_host);
/* the streaming entry's host-side follower of energy_descramble (lib/energy_descramble_impl.cc:121-141; csrc/dvbt_stream.inc::descr_walk), which a stream uses wherever the
 * descrambler re-searches its NSYNC: rs = nitems items of 1504 bytes as they leave reed_solomon_dec; the follower is called once per entry of windows[] (items visible so
 * far, ascending: the state it carries from window to window is what is under test) and reports the calls it delivers as runs of (first packet, packets) in runs[2 k],
 * runs[2 k + 1].  Returns the number of runs, or a negative error.  No device needed. */
int64_t dvbt_debug_descr_follow(const uint8_t *rs, size_t nitems, const int64_t *windows, int nwindows, int64_t *runs, size_t cap_runs);
/* the exchange step's world > 1 logic on ONE device (RCCL refuses two ranks on a device, a test box has one): a loopback transport whose ranks are threads of one process -- a send
 * is a posted message, a receive copies device to device behind the sender's stream, a group ends when everything posted has been taken.  *group: NULL on the first call (created and
 * returned), the returned value for the other ranks.  dvbt_rccl_debug_fail_steps: the communicator's next n steps behave as if their exchange buffers could not be allocated (the
 * error-flag slot, sent from the stream's sample buffer).  tests/test_gpu_rccl.py::test_exchange_step_world_2_over_the_loopback_transport */
int dvbt_rccl_comm_create_loopback(void **group, int rank, int world, int device, dvbt_rccl_comm **out);
int dvbt_rccl_debug_fail_steps(dvbt_rccl_comm *c, int n);
/* the soft-input decoder's kernel alone (csrc/k_soft4.hpp) on n_soft host soft values (int8, the decoder's input order; a multiple of the constellation's m): chunk size B,
 * nsteps steps per decoder and `grid` workgroups as given instead of planned.  out_host[0 .. out_cap) was 0xA5 on the device before the launch; the kernel writes
 * total_steps / 8 - ntraceback bytes.  DVBT_ERR_INVALID, nothing launched, for what the planner cannot produce: B outside [64, 304], nsteps not a multiple of 48 in
 * [256 + 8 B + max(8 ntraceback, 128), 2928], grid outside [1, 2048], out_cap < total_steps / 8.  tests/test_gpu_soft_kernels.py */
int dvbt_debug_soft_viterbi(int constellation, int code_rate, const int8_t *soft_host, int64_t n_soft, int64_t total_steps, int B, int nsteps, int grid,
                            uint8_t *out_host, size_t out_cap);
/* the soft demapper's two kernels (csrc/k_soft.hpp: the scatter table of both inner de-interleavers, then the demapper) on nsym host symbols: eq cfloat[nsym][P],
 * csi float[nsym][P], parity[s] = symbol index & 1; out_host int8[nsym][P m], the soft values in the decoder's input order */
int dvbt_debug_soft_demap(int constellation, int transmission_mode, const void *eq_host, const float *csi_host, const int32_t *parity_host, int nsym, int8_t *out_host);
/* the segment chain's outer stage alone (byte de-interleaver + RS with its defer list and second pass + sync bitmap + descrambler: the launches of enqueue_tail in
 * csrc/dvbt_hip.hip, and the range form stream_rs_range of csrc/dvbt_stream.inc) on n_bytes host-supplied bytes of a Viterbi stream, uploaded into the handle's own
 * buffers (grown as the streaming entry grows them).  The RS, TS and DEINT buffers (the last when the taps are enabled), the sync bitmap and the run list are 0xA5 up to
 * their capacity before the launches.  Afterwards dvbt_rx_read_tap(DEINT / RS / TS) deliver the counts reported here; dvbt_debug_outer_read reads any of the buffers
 * up to its capacity.  mode:
 *   DVBT_OUTER_SEGMENT  enqueue_tail on a stream whose length the host knows (n_bytes / 204 words); a, b unused
 *   DVBT_OUTER_CUT      the same launches on the plan of a piece that continues a cut stream: a = n_rs_words (any value with a * 204 <= n_bytes), b = descr_call_phase
 *                       as in dvbt_rx_cut (0 = unknown, else 1 + phase)
 *   DVBT_OUTER_RANGE    stream_rs_range over the words [a, b) (a: a multiple of 64), no descrambler.  vit_host = NULL with n_bytes = 0: on the stream already in the
 *                       handle, nothing refilled, the counters carried on -- as the streaming entry's walk calls it behind every window
 * sync_host: the first sync_cap words of the bitmap (NULL: none).  DVBT_ERR_INVALID, nothing allocated or launched, for negative sizes, more than 2^30 bytes, or a plan
 * outside the uploaded stream; behind those checks DVBT_ERR_NO_DEVICE without a GPU, whatever the handle.  tests/test_gpu_outer.py */
enum { DVBT_OUTER_SEGMENT = 0, DVBT_OUTER_CUT = 1, DVBT_OUTER_RANGE = 2 };
enum { DVBT_OUTER_BUF_DEINT = 0, DVBT_OUTER_BUF_RS = 1, DVBT_OUTER_BUF_TS = 2, DVBT_OUTER_BUF_SYNC = 3, DVBT_OUTER_BUF_RUNS = 4 };
typedef struct {
  int64_t n_rs_words, n_rs_items, n_ts_bytes, ts_first_packet;
  int64_t cap_bytes;       /* capacity of the DEINT / RS / TS buffers */
  int64_t sync_cap_words;  /* ... of the bitmap, in 64-bit words */
  int64_t runs_cap;        /* ... of the run list, in runs of three int64 (source byte, destination byte, bytes) */
  int32_t rs_fail, rs_corr;
  int32_t rs_list_n;       /* words the first pass handed to the second */
  int32_t n_runs, descr_unclean, reserved;
} dvbt_outer_report;
int dvbt_debug_outer(dvbt_rx *h, int mode, const uint8_t *vit_host, int64_t n_bytes, int64_t a, int64_t b, dvbt_outer_report *report, uint64_t *sync_host, size_t sync_cap);
/* nbytes bytes from byte `offset` of one of the buffers above (DVBT_OUTER_BUF_*), within its capacity; returns the bytes copied */
int64_t dvbt_debug_outer_read(dvbt_rx *h, int buffer, int64_t offset, void *dst, size_t nbytes);

/* the kernels that reproduce the reference's float phase accumulator (csrc/k_drift.hpp) alone, on nsym host-supplied calls of a lock period: sw[s] the sample of call s
 * at which the increment switches from incA[s] to incB[s] (rad per sample), ph_base[s] the accumulator's float value at the call's entry (block path only), `status` the
 * state block's status word, N / cp any transmission mode with any of its guard intervals.  path 0: the segment path's launch sequence (enqueue's own: tables, exact
 * line, three rounds of the fixed point, the prefix and its convergence test, the recurrence where that fails, the deviations); path 1: the block path's per-call
 * kernel.  More calls are launched than nsym, as in a segment.  The scratch and delta are 0xFF bytes (NaN) on the device before the launches.  flags[4], in and out:
 * the device's flag words start as given (all 0 for a fresh handle; a second call may pass on what the first returned) and are read back behind the launches:
 * [0] the sign / validity bits drift_prep_kernel collects (cleared again by drift_exact_kernel), [1] 1 = the deviations apply, [2] 1 = negative increments, [3] 1 = the fixed point's last two rounds disagreed and the recurrence over the calls was taken.
 * delta_host float[nsym][N / 32]: the deviation (rad) of the float accumulator from the exact line at sample 32 k + 17 of call s, relative to the call's entry.
 * ms (may be NULL): the launch sequence's time between two events.  DVBT_ERR_INVALID, nothing allocated or launched, for a null pointer, nsym outside
 * [0, DVBT_DEBUG_DRIFT_MAX_CALLS] (what the hook sizes its scratch for), an unknown path or an N / cp that is no mode / guard pair; behind those checks
 * DVBT_ERR_NO_DEVICE without a GPU.  tests/test_gpu_drift_kernels.py */
enum { DVBT_DEBUG_DRIFT_MAX_CALLS = 65536 };
int dvbt_debug_drift(int N, int cp, int nsym, const int32_t *sw, const double *incA, const double *incB, const float *ph_base, int status, int path,
                     float *delta_host, int32_t *flags, float *ms);

/* the per-symbol kernels of the segment path alone (csrc/k_symbol8k.hpp, csrc/k_symbol2k.hpp: derotation, FFT, pilot engine, equaliser, demapper) through the segment
 * path's own launch routine (launch_symbols of csrc/dvbt_hip.hip, which enqueue calls), on the handle's tables and buffers.  Mode, constellation, hierarchy, guard
 * interval, soft decisions and the tap state are the handle's, the instantiation the one a segment would get.  From the host: nsamples complex64 samples; nsym symbols
 * whose state block says call0; keep_last and avail (samples in memory: reads at or beyond it return zeros) as in FrontParams; per symbol cp_start, sw, ph_base, incA,
 * incB as the acquisition's SymMeta (symbol s reads the N samples from (call0 + s)(N + cp) + cp_start - N + 1 on); grid: workgroups, 0 = as a segment of nsym calls;
 * delta_host: NULL, or float[nsym][N / 32] deviations -- then the drift flag word is 1 and the DRIFT instantiation works.  Every buffer the kernels write is 0xA5 up
 * to its capacity before the launch, the ticket is zero; behind it the ticket and the drift flag words are zero again.  Outputs (each may be NULL), nread symbols each
 * (0: nsym; more than nsym shows what lies behind the last symbol): labels uint8[nread][payload], freq_offset / mod_index int32[nread], tpsval cfloat[nread][n_tps],
 * acq / fft cfloat[nread][N], eq cfloat[nread][payload], csi float[nread][payload] -- a tap the handle does not have (dvbt_rx_enable_taps; csi: soft decisions) leaves
 * its array as it was.  DVBT_ERR_INVALID, nothing allocated or launched, for: a null required pointer; nsym < 1 or beyond the calls the handle's buffers hold; grid
 * outside [0, the handle's workgroup count]; avail outside (0, nsamples]; a non-finite ph_base / incA / incB; a symbol whose window begins before sample 0 (the kernels
 * check the upper bound only); |delta| >= 2e-3 (the kernels' stated precondition); nread outside [nsym, capacity].  Behind the checks that need no handle
 * DVBT_ERR_NO_DEVICE without a GPU.  tests/test_gpu_symbol_kernels.py */
int dvbt_debug_symbols(dvbt_rx *h, const void *iq_host, size_t nsamples, int nsym, int call0, int keep_last, int64_t avail, const int32_t *cp_start,
                       const int32_t *sw, const float *ph_base, const double *incA, const double *incB, int grid, const float *delta_host, int nread,
                       uint8_t *labels, int32_t *freq_offset, int32_t *mod_index, void *tpsval, void *acq, void *fft, void *eq, float *csi);

/* the launches between the symbol kernels and the Viterbi decoder alone (DBPSK vote, TPS / frame bookkeeping in its segment-parallel form with the sequential
 * fallback, the sizes of every later stage, symbol and bit de-interleaver: tps_vote_kernel, tps_fsm_par_kernel, tps_tail_kernel, inner_kernel) through the segment
 * path's own launch routine (launch_frames of csrc/dvbt_hip.hip, which enqueue calls), on the handle's tables and buffers; launched for as many calls as the handle
 * holds, as a segment launches more than it acquires.  From the host: n_symbols (the state block's) and keep_last as in a segment; mod_index int32[n] the scattered
 * pilots' pattern per symbol (the other fields of the per-symbol record are 0xA5); tpsval cfloat[n][n_tps] the equalised TPS carriers; prev0 NULL, or cfloat[n_tps]
 * the TPS carriers in front of symbol 0 -- then the period is a continuation: sequential bookkeeping, the members carried on, the superframe hunt restarted; init
 * NULL, or the pilot engine's members in front of symbol 0 (a fresh period starts from them, d_init taken as 0, as a piece of a stream with known counters does; a continuation
 * carries on from them, and with NULL from what the handle's last period left); labels uint8[n][payload]; sym_off (a multiple of 272) and start_delay_symbols as in
 * dvbt_rx_cut.  Before the launches the flag words and, for a fresh period without init, the pilot engine's state are what the acquisition's reset leaves; the vote,
 * the symbol indices, the parallel pass's edge records, both de-interleaver outputs and the symbol de-interleaver's tap, and what lies behind the n rows of the inputs,
 * are 0xA5 up to capacity.  Outputs: the report (the state block behind the launches, the two flag words, the capacities); maj and sym_index int32[cap_symbols];
 * final_state; bitdeint, bitdeint_lp, symdeint uint8[cap_bytes] (cap_bytes = cap_symbols * payload + 64; the last two may be NULL, and stay as they were where the
 * handle has no such buffer: has_lp, has_tap).  The caller sizes the arrays from the handle's max_samples: cap_symbols = (max_samples - (2 N + cp + 16)) / (N + cp) + 1.
 * DVBT_ERR_INVALID, nothing written, allocated or launched, for: a null required pointer, a negative n_symbols, a sym_off that is negative or no multiple of 272, a
 * start_delay_symbols outside [0, 272), and -- behind DVBT_ERR_NO_DEVICE without a GPU -- a null or soft-decision handle and n_symbols beyond the handle's calls.
 * tests/test_gpu_frames.py */
typedef struct { uint64_t fifo_lo; uint32_t fifo_hi; int32_t symbol_index, symbol_index_known, frame_index, prev_mod, d_init; } dvbt_tps_state;   /* bit i of the FIFO = s_i */
typedef struct {
  int32_t status, call0, cp_start0, n_symbols, first_out, n_out_symbols;
  int32_t descr_base, descr_index, rs_fail, rs_corr, rs_list_n, small_viol, drift_known_off, descr_unclean;
  int64_t n_vit_in, n_vit_steps, n_vit_bytes, n_rs_items, n_ts_bytes, sym_off, n_rs_words, stream_rs_items, ts_first_packet;
  uint64_t tps_bits;                   /* bit 63: a valid frame was seen; bits 17..53 its static fields */
  int32_t first_cand, need_seq;        /* the flag words: the parallel pass's earliest start candidate (0x7fffffff: none), 1 = the sequential bookkeeping ran */
  int32_t cap_symbols, has_lp, has_tap, reserved;
  int64_t cap_bytes;
} dvbt_frames_report;
int dvbt_debug_frames(dvbt_rx *h, int n_symbols, int keep_last, const int32_t *mod_index, const void *tpsval, const void *prev0, const dvbt_tps_state *init,
                      const uint8_t *labels, int64_t sym_off, int start_delay_symbols, dvbt_frames_report *report, int32_t *maj, int32_t *sym_index,
                      dvbt_tps_state *final_state, uint8_t *bitdeint, uint8_t *bitdeint_lp, uint8_t *symdeint);

/* the acquisition kernels of the segment path alone (csrc/k_frontend.hpp: initial search, anchors, centres, tracking metric, the Jacobi placement and its
 * bookkeeping, the light and the float-faithful sequential walk, acq_small_kernel) through the segment path's own launch routine (launch_acquisition of
 * csrc/dvbt_hip.hip, which enqueue calls), as an acquisition-only pass on the handle's buffers.  iq_host: hist + nsamples complex64 samples; the segment begins at
 * sample `hist` of it, the `hist` samples in front are the stream's history (FrontParams.hist); avail as in FrontParams (reads at or beyond it return zeros);
 * init_tries windows for the initial search; use_carry / carry_avg the peak detector's average carried in; path 0 = the general kernels, 1 = acq_small_kernel;
 * force (path 0): 1 = need_seq is set behind acq_finalize_kernel (the light walk runs on a period the placement settled), 2 = need_heavy too (the float-faithful
 * walk).  Every buffer the kernels write -- both metrics, anchors, centres, the placement's peaks and estimates, the SymMeta rows, the 16 flag words, the state
 * block -- is 0xA5 up to its capacity before the launches.  Outputs: the report; meta[nread] (more than n_symbols shows what lies behind the last symbol); and, each
 * NULL or: g_init cfloat / l_init float [min(init_tries, ncalls)][N]; anchor_pos int32[cap_symbols / 256 + 4]; centre int32[nread]; g_trk cfloat / l_trk float
 * [nread][32]; init_flags uint8 [min(init_tries, ncalls)][N]: bit 0 the rise, bit 1 the keep decision of acq_init_fsm_kernel for every sample of every window it
 * examined (0xA5 behind the window that held the peak).  Behind the call the state block and the flag words are zero, as a fresh handle's.  cap_symbols = (max_samples - (2 N + cp + 16)) / (N + cp) + 1.  DVBT_ERR_INVALID, nothing allocated or launched, for: a null required pointer;
 * nsamples outside (0, 2^31]; hist outside [0, 2^20]; avail outside (0, nsamples]; init_tries outside [1, 64]; an unknown path; force outside [0, 2] or non-zero on
 * path 1; a non-finite carried average; a negative nread; and -- behind DVBT_ERR_NO_DEVICE without a GPU -- a null handle, fewer samples than one acquisition
 * window, more calls or a larger nread than the handle's buffers hold, path 1 with more than 768 calls.  tests/test_gpu_acquire.py */
typedef struct { int32_t cp_start, sw; float eps, ph_base; double incA, incB; } dvbt_sym_meta;
typedef struct {
  int32_t status, call0, cp_start0, n_symbols;
  float avg, eps_init, avg_lost;
  int32_t small_viol, drift_known_off;
  int32_t changed[4], need_seq, need_heavy;   /* the flag words behind the launches */
  int32_t ncalls, cap_symbols;
  int32_t small_passes, general_passes;       /* what this call added to the walk counters of dvbt_rx_walk_stats */
  int32_t reserved;
} dvbt_acquire_report;
int dvbt_debug_acquire(dvbt_rx *h, const void *iq_host, size_t nsamples, int64_t hist, int64_t avail, int init_tries, int use_carry, float carry_avg,
                       int path, int force, dvbt_acquire_report *report, dvbt_sym_meta *meta, int nread, void *g_init, float *l_init, int32_t *anchor_pos,
                       int32_t *centre, void *g_trk, float *l_trk, uint8_t *init_flags);

/* the channel-error kernel alone (csrc/k_quality.hpp) on host bytes: in_host = n_in decoder input bytes (m bits each), vit_host = n_vit decoded bytes; counts as
 * dvbt_rx_quality's channel_bits / channel_bit_errors (n_vit < 2: both 0).  Sizes outside [0, 2^30] are refused before the device is asked for. */
int dvbt_debug_quality_channel(int constellation, int code_rate, const uint8_t *in_host, int64_t n_in, const uint8_t *vit_host, int64_t n_vit, int64_t *bits, int64_t *errors);
/* the post-Viterbi kernel alone: n_words RS words of 188 bytes (rs_host) against the words regathered from the n_vit bytes of vit_host */
int dvbt_debug_quality_post(const uint8_t *vit_host, int64_t n_vit, const uint8_t *rs_host, int64_t n_words, int64_t *bits, int64_t *errors);
/* every kernel of dvbt_rx_quality alone on the last finished segment's buffers, `warmup` launches and `iters` timed ones each (HIP events): ms[4][iters] in the order
 * mer, sum, channel, rs; bytes_read[4] what each reads.  tools/quality_bench.py */
int dvbt_debug_quality_time(dvbt_rx *h, int warmup, int iters, float *ms, int64_t *bytes_read);

/* ------------------------------------------------------------------ the channel: echoes, carrier offset, seeded AWGN
 * What stands between a modulator and a receiver in a loopback (the noise source and adder of apps/dvbt_rx_demo*.grc, plus static multipath and a carrier
 * offset), on complex64 baseband, in one kernel and one pass over the samples (csrc/k_channel.hpp).  For the stream's absolute sample index n:
 *   e[n] = x[n] + sum_i a_i x[n - d_i]                  x[k] = 0 in front of the stream's first sample; the direct path is implicit
 *   r[n] = e[n] exp(2 pi j phi(n))                      phi(n) = (inc n mod 2^64) / 2^64, inc = round(cfo / fft_length 2^64) mod 2^64: cfo in subcarrier spacings
 *   y[n] = r[n] + noise_sigma (g_re(n) + j g_im(n))     noise_sigma: standard deviation per component, sqrt(ref_power / 10^(snr_db / 10) / 2) for an SNR
 * The noise of sample n is a function of (seed, n) alone: Philox4x32-10 with key (seed low 32, seed high 32) and counter (n >> 1, 0, 0) split into low and high
 * words; sample n takes output words (0, 1) for even n, (2, 3) for odd n as (w_a, w_b); u1 = ((w_a >> 9) + 0.5) 2^-23, u2 = (w_b >> 8) 2^-24, rho =
 * sqrt(-2 ln u1), g = rho (cos, sin)(2 pi u2).  u1 >= 2^-24, so the Gaussian's tails end at 5.77 sigma.  The phase is an integer product -- exact, wrapping by
 * itself, as good at n = 2^40 as at 0 -- and the phasor is taken from its top 32 bits.  The handle keeps the last DVBT_CHANNEL_MAX_DELAY input samples on the
 * device, so calls of any size (0 and 1 included) continue the stream, and a stream cut into calls gives bit for bit what one call gives.  With no paths, cfo == 0
 * and noise_sigma == 0 the output is the input bit for bit.
 * Buffers: n <= 2^31 complex64 each per call, 8-byte aligned; input and output ranges that overlap are DVBT_ERR_INVALID (the echoes read behind the sample being written).  A
 * failed call leaves the stream position and the history as they were.  dvbt_channel_run_device only enqueues on `stream`; calls on different streams are ordered
 * by the handle (an event).  One thread per handle.  Every parameter is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a
 * good one DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU path. */
enum { DVBT_CHANNEL_MAX_PATHS = 8, DVBT_CHANNEL_MAX_DELAY = 8192 };
typedef struct {
  int n_paths; int delay[8]; float amp_re[8], amp_im[8];
  double cfo; int fft_length;          /* fft_length > 0 whenever cfo != 0 */
  float noise_sigma; uint64_t seed;    /* noise_sigma >= 0, finite */
  int64_t first_sample;                /* >= 0: absolute index of the stream's first sample (a piece of a cut stream) */
  int device;
} dvbt_channel_params;
typedef struct dvbt_channel dvbt_channel;
int  dvbt_channel_create(const dvbt_channel_params *p, dvbt_channel **out);
int  dvbt_channel_run(dvbt_channel *h, const void *iq_host, size_t n, void *out_host);
int  dvbt_channel_run_device(dvbt_channel *h, const void *iq_device, size_t n, void *out_device, void *stream);
/* mean of |x|^2 over n > 0 samples of a device buffer (the ref_power of noise_sigma): partial sums in double, added in a fixed order without atomics -- two calls
 * on the same data return the same bits.  Ordered on `stream`; synchronises. */
int  dvbt_channel_power(dvbt_channel *h, const void *iq_device, size_t n, void *stream, double *mean_power);   /* synchronises */
int  dvbt_channel_reset(dvbt_channel *h);   /* back to first_sample, history cleared */
void dvbt_channel_destroy(dvbt_channel *h);

/* ------------------------------------------------------------------ the sample-clock offset: windowed-sinc resampling by ppm
 * The stream as a receiver whose sample clock is off by `ppm` sees it (oracle/pyoracle.py::clock_offset on the device, csrc/k_clock.hpp), on complex64
 * baseband, as a block of its own in front of or behind the channel: the sample count changes, which the channel's in = out contract does not allow.
 * Positions are integers.  With H = taps / 2, S = 2^64 + rint(ppm 1e-6 2^64) (ties to even) and P0 = trunc(start 2^64), output m of the stream samples the
 * input at P(m) = P0 + m S in units of 2^-64 input samples (a 128-bit integer): base = P >> 64, f = P mod 2^64, and
 *   y[m] = sum_{k = -(H-1)}^{H} h(k - f / 2^64) x[base + k]      h(a) = sinc(a) (0.54 + 0.46 cos(pi a / (H + 1)))      x[i] = 0 for i < first_in
 * m and the x index are absolute: the stream's first input sample is x[first_in], its first output y[first_out].  f == 0 gives x[base] bit for bit.  The sum
 * runs in a fixed order (k ascending) in float, so an output's bits depend on m and its taps inputs alone: a stream cut into calls of any size (0 and 1
 * included) gives bit for bit what one call gives, and a handle with first_out = M, first_in = base(M) - (H - 1) continues a cut stream at output M.
 * Counts: E(N) = the smallest m >= 0 with base(m) + H >= N.  With N = first_in + the inputs pushed so far, the outputs emitted so far are those in front of
 * E(N), from first_out on; a call emits every output it can complete, max(E(N_after), first_out) - max(E(N_before), first_out), a number the host computes in
 * integer arithmetic (dvbt_clock_outputs_for, dvbt_clock_outputs) without waiting for the device.  Every input sample is consumed; the handle keeps the last
 * 64 on the device.  There is no flush: the outputs whose support reaches behind the last input are never emitted.
 * Parameters: |ppm| <= 1000; 0 <= start < 2^31 (input samples; taps / 2 is the oracle's alignment); taps 16, 32 or 64 (0: 16); first_out, first_in in
 * [0, 2^48]; at most 2^56 input samples per stream.  Buffers: n_in <= 2^31 complex64 per call, 8-byte aligned; input and output ranges that overlap are
 * DVBT_ERR_INVALID; out_cap below the call's count is DVBT_ERR_CAPACITY.  A failed call leaves the stream position and the history as they were.
 * dvbt_clock_run_device only enqueues on `stream`; calls on different streams are ordered by the handle (an event).  One thread per handle.  Every parameter
 * is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU path. */
typedef struct { double ppm, start; int taps; int64_t first_out, first_in; int device; } dvbt_clock_params;
typedef struct dvbt_clock dvbt_clock;
/* outputs emitted once n_in_total (<= 2^56) inputs have been pushed: host arithmetic, needs no device */
int  dvbt_clock_outputs(const dvbt_clock_params *p, int64_t n_in_total, int64_t *n_out_total);
int  dvbt_clock_create(const dvbt_clock_params *p, dvbt_clock **out);
int  dvbt_clock_outputs_for(const dvbt_clock *h, size_t n_in, size_t *n_out);   /* what the NEXT call of n_in samples emits */
int  dvbt_clock_run(dvbt_clock *h, const void *iq_host, size_t n_in, void *out_host, size_t out_cap, size_t *n_out);
int  dvbt_clock_run_device(dvbt_clock *h, const void *iq_device, size_t n_in, void *out_device, size_t out_cap, size_t *n_out, void *stream);
int  dvbt_clock_reset(dvbt_clock *h);   /* back to first_in / first_out, history cleared */
void dvbt_clock_destroy(dvbt_clock *h);

/* ------------------------------------------------------------------ fading: time-varying multipath with a Doppler spectrum
 * What a moving receiver sees: a tapped delay line whose taps fade as sums of sinusoids (Clarke's spectrum, optionally with a fixed part: Rice), on complex64
 * baseband, in one kernel (csrc/k_fading.hpp).  For the stream's absolute sample index n:
 *   y[n] = sum_{i < n_paths} g_i(n) x[n - d_i]          x[k] = 0 in front of the stream's first sample; i ascending, the first path's product starts the sum
 * Sinusoid table (host, double, the same bits everywhere; dvbt_fading_table): for path i and sinusoid m < M = n_sinusoids, w = Philox4x32-10 with key (seed low
 * 32, seed high 32) and counter (m, i, 0, 0x46414445) -- disjoint from the channel's noise counters (P lo, P hi, 0, 0), so the same seed in a dvbt_channel
 * behind this block is independent; u = (w0 + 0.5) 2^-32; angle of arrival alpha = (m + u) / M turns (stratified: one sinusoid per M-th of the circle);
 * f = doppler cos(2 pi alpha), the cosine by quarter-turn reduction and a Taylor polynomial in plain double arithmetic; inc = nearbyint(f 2^64) mod 2^64;
 * ph = (w1 << 32) | w2.
 * Knots (float32, each operation rounded on its own): every DVBT_FADING_KNOT absolute samples, S_i(k) = sum_m cis(top 32 bits of (ph + inc 64 k mod 2^64)),
 * m ascending from 0; G_i(k) = los_i + s_i S_i(k), s_i = (float)(sigma_i / sqrt(M)).
 * Gain: k = n >> 6, t = (n & 63) 2^-6, g_i(n) = G_i(k) + t (G_i(k + 1) - G_i(k)) per component.  The piecewise-linear gain IS the specification; its distance
 * from the sum of sinusoids taken at every sample is at most sigma_i sqrt(M) (2 pi 64 doppler)^2 / 8 (the chord error of a unit phasor, per sinusoid 9.7e-6
 * at 200 Hz and 64/7 Msps, 1.2e-3 at the largest doppler).  Product: (ar x.re - ai x.im, ar x.im + ai x.re).
 * The block adds no noise and no carrier offset (a dvbt_channel without echoes behind it does both) and does not normalise the mean power: sum_i (|los_i|^2 +
 * sigma_i^2) is the caller's.  A path with sigma == 0 is static; one path (0, 1, 0) gives the input as values.
 * The handle keeps the last DVBT_FADING_MAX_DELAY input samples on the device, so calls of any size (0 and 1 included) continue the stream, and a stream cut
 * into calls gives bit for bit what one call gives; a handle with first_sample = s fed the stream from s on gives, from s + DVBT_FADING_MAX_DELAY on, the
 * bits of the handle that began at 0.
 * Buffers: n <= 2^31 complex64 each per call, 8-byte aligned; input and output ranges that overlap are DVBT_ERR_INVALID.  A failed call leaves the stream
 * position and the history as they were.  dvbt_fading_run_device only enqueues on `stream`; calls on different streams are ordered by the handle (an event).
 * One thread per handle.  Every parameter is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one
 * DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU path, except dvbt_fading_table, which is host arithmetic. */
enum { DVBT_FADING_MAX_PATHS = 24, DVBT_FADING_MAX_DELAY = 8192, DVBT_FADING_MAX_SINUSOIDS = 32, DVBT_FADING_KNOT = 64 };
typedef struct {
  int n_paths;                                   /* 1 .. 24 */
  int delay[24];                                 /* 0 .. 8192 samples; equal delays allowed */
  float los_re[24], los_im[24];                  /* the path's fixed part */
  float sigma[24];                               /* rms of its scattered part, >= 0; 0: the path is static */
  double doppler;                                /* largest Doppler shift in cycles per sample, 0 .. 2^-12 (2.2 kHz at 64/7 Msps) */
  int n_sinusoids;                               /* 0 = 16; 1 .. 32 */
  uint64_t seed; int64_t first_sample; int device;
} dvbt_fading_params;
typedef struct dvbt_fading dvbt_fading;
/* the sinusoid table of a valid struct, n_paths x M words each (row i, column m): host arithmetic, needs no device */
int  dvbt_fading_table(const dvbt_fading_params *p, uint64_t *inc, uint64_t *phase);
int  dvbt_fading_create(const dvbt_fading_params *p, dvbt_fading **out);
int  dvbt_fading_run(dvbt_fading *h, const void *iq_host, size_t n, void *out_host);
int  dvbt_fading_run_device(dvbt_fading *h, const void *iq_device, size_t n, void *out_device, void *stream);
int  dvbt_fading_reset(dvbt_fading *h);   /* back to first_sample, history cleared */
void dvbt_fading_destroy(dvbt_fading *h);

/* ------------------------------------------------------------------ rf: the transmitter's amplifier, oscillator phase noise, the tuner's IQ imbalance and DC
 * What the radio hardware on either side of a channel does to complex64 baseband, in one kernel (csrc/k_rf.hpp).  For the stream's absolute sample index n
 * (first_sample + the samples the handle has seen), four stages in this order, each off by default:
 *   1. amplifier, Rapp AM/AM   u = x (1 + (|x|^2 / A^2)^p)^(-1/(2p))       A = sat_amplitude (0: off), p = smoothness in [0.5, 16] (0 = 2).  The phase is
 *      untouched, |u| < A, x = 0 gives 0; right for every finite x (above |x| = A the kernel uses t^(-1/2) (1 + t^(-p))^(-1/(2p)), t = |x|^2 / A^2).
 *   2. phase noise             r = u (cos phi, sin phi)    phi(n) = sum_{m < n_tones} a_m sin(2 pi theta_m(n)), m ascending in float32;  theta_m(n) = the
 *      top 32 bits of (tone_phase[m] + tone_inc[m] n mod 2^64) times 2^-32: an integer product, as exact at n = 2^40 as at 0.  n_tones == 0: off.
 *      a_m = tone_amp[m] >= 0, and their sum must not exceed pi.  Product: (ar x.re - ai x.im, ar x.im + ai x.re).
 *   3. IQ imbalance            v = mu r + nu conj(r)       mu == (0, 0) stands for (1, 0), so a zeroed struct is the identity; off where mu == 1 and nu == 0.
 *   4. DC offset               y = v + dc                  off where dc == 0.
 * With every stage off the output is the input bit for bit.  The block is memoryless: a sample's output bits depend on (the struct, n, x[n]) alone, so calls
 * of any size (0 and 1 included) continue the stream, a stream cut into calls gives bit for bit what one call gives, and a handle with first_sample = s gives
 * the bits of the handle that began at 0 from s on.
 * Tones from a phase-noise mask (dvbt_rf_phase_noise_tones; host arithmetic in double, needs no device): the mask is 2 to 8 points (offset_hz[k], dbc_hz[k]),
 * offsets > 0 and strictly ascending, the last <= sample_rate / 2; L(f) is linear in dB over log f between them.  With rho = f_last / f_0, M = n_tones:
 * edges e_m = f_0 exp(ln rho m / M), e_M = f_last; w = Philox4x32-10 with key (seed low 32, seed high 32) and counter (m, 0, 0, 0x5246504E) -- disjoint from
 * the channel's noise counters and from the fading table's; u = (w0 + 0.5) 2^-32; f_m = f_0 exp(ln rho (m + u) / M) (one tone per M-th of the log axis);
 * inc = nearbyint(f_m / sample_rate 2^64); ph = (w1 << 32) | w2; a_m = (float)(2 sqrt(B_m)), B_m = the integral of L over [e_m, e_m+1] in closed form, so
 * that sum a_m^2 / 2 = 2 integral L df (both sidebands) for every M.  A caller with a measured spur list fills the three arrays itself.
 * Buffers: n <= 2^31 complex64 each per call, 8-byte aligned.  Input and output may be the SAME buffer (in place); ranges that overlap in any other way are
 * DVBT_ERR_INVALID.  A failed call leaves the stream position as it was.  dvbt_rf_run_device only enqueues on `stream`; calls on different streams are ordered
 * by the handle (an event).  One thread per handle.  Every parameter is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a
 * good one DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU path. */
enum { DVBT_RF_MAX_TONES = 32, DVBT_RF_MAX_MASK_POINTS = 8 };
typedef struct {
  float sat_amplitude;                           /* A; 0: no amplifier */
  float smoothness;                              /* p: 0 = 2; 0.5 .. 16 */
  int n_tones;                                   /* 0 .. 32; 0: no phase noise */
  uint64_t tone_inc[32], tone_phase[32];         /* per sample in units of 2^-64 turns; the phase at n = 0 */
  float tone_amp[32];                            /* radians, >= 0, sum <= pi */
  float mu_re, mu_im, nu_re, nu_im;              /* mu == (0, 0): (1, 0) */
  float dc_re, dc_im;
  int64_t first_sample; int device;
} dvbt_rf_params;
typedef struct {
  int n_points;                                  /* 2 .. 8 */
  double offset_hz[8], dbc_hz[8];
  double sample_rate;                            /* Hz */
} dvbt_rf_mask;
typedef struct dvbt_rf dvbt_rf;
/* n_tones (1 .. 32) words each; on refusal nothing is written */
int  dvbt_rf_phase_noise_tones(const dvbt_rf_mask *mask, int n_tones, uint64_t seed, uint64_t *inc, uint64_t *phase, float *amp);
int  dvbt_rf_create(const dvbt_rf_params *p, dvbt_rf **out);
int  dvbt_rf_run(dvbt_rf *h, const void *iq_host, size_t n, void *out_host);
int  dvbt_rf_run_device(dvbt_rf *h, const void *iq_device, size_t n, void *out_device, void *stream);
int  dvbt_rf_reset(dvbt_rf *h);   /* back to first_sample */
void dvbt_rf_destroy(dvbt_rf *h);

/* ------------------------------------------------------------------ spectrum: Welch's averaged periodogram, power sum, peak and a histogram of |x|^2
 * A measurement block (csrc/k_spectrum.hpp): it consumes complex64 baseband as a stream, changes nothing and accumulates on the device, in one pass.
 *   Segments   segment k is the stream's samples [k hop, k hop + N), counted from the first sample pushed since create or reset.  N = fft_size, a power of
 *              two in 64..8192; hop in [N / 8, N], 0 = N / 2.  S = the number of complete segments.
 *   Window     0 rectangular, 1 Hann, 2 four-term Blackman-Harris (0.35875, 0.48829, 0.14128, 0.01168); periodic (the argument is n / N), computed in
 *              double and rounded to a float table w.
 *   PSD        psd[b] = sum_k |X_k[(b - N/2) mod N]|^2 / (S N sum w^2),  X_k = FFT(w x_k): fft-shifted as dvbt_fft, power per bin, so that sum_b psd[b]
 *              is the mean power of a stationary signal.  The equivalent noise bandwidth is N sum w^2 / (sum w)^2 bins: an on-bin tone of amplitude A
 *              reads A^2 / ENBW.  S = 0 reads a zero PSD.
 *   Statistics cover exactly the samples [0, S hop) -- the first hop samples of every complete segment -- once each: sum_power = sum |x|^2 (double),
 *              peak_power = max |x|^2, hist[float_bits(|x|^2) >> 20]++ with |x|^2 = fmaf(re, re, im im) in float and the sign bit (which only a NaN can
 *              carry) dropped: 8 bins per octave over the whole float range, no scale and no clamping.  Bins 2040.. hold inf and NaN (`nonfinite`); a NaN
 *              in the counted range makes sum_power NaN and peak_power a NaN.
 * A stream cut into calls of any sizes (1 and 0 included, shorter than hop, 8-byte aligned only) gives the PSD, sums and histogram of one call, bit for
 * bit, through either entry, on any device: sums are formed in an order fixed by the stream (groups of 32 segments in float, the groups in ascending order in
 * double), never by atomics in floating point.  dvbt_spectrum_read synchronises and does not disturb the accumulation.  dvbt_spectrum_push_device only
 * enqueues on `stream`; calls on different streams are ordered by the handle (an event).  n <= 2^31 per call, 2^56 per stream.  One thread per handle.  Every
 * parameter is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is
 * no CPU path.  A failed call leaves the state as it was. */
enum { DVBT_SPECTRUM_HIST_BINS = 2048 };
typedef struct { int device, fft_size, hop, window; } dvbt_spectrum_params;
typedef struct {
  long long segments, samples_pushed, samples_counted, nonfinite;
  double sum_power;
  float peak_power;
} dvbt_spectrum_result;
typedef struct dvbt_spectrum dvbt_spectrum;
int  dvbt_spectrum_create(const dvbt_spectrum_params *p, dvbt_spectrum **out);
int  dvbt_spectrum_push(dvbt_spectrum *h, const void *iq_host, size_t n);
int  dvbt_spectrum_push_device(dvbt_spectrum *h, const void *iq_device, size_t n, void *stream);
int  dvbt_spectrum_read(dvbt_spectrum *h, dvbt_spectrum_result *result, double *psd /* fft_size, may be NULL */,
                        unsigned long long *hist /* DVBT_SPECTRUM_HIST_BINS, may be NULL */);
int  dvbt_spectrum_reset(dvbt_spectrum *h);   /* back to the state after create */
void dvbt_spectrum_destroy(dvbt_spectrum *h);

/* ------------------------------------------------------------------ sounder: the echo profile and the amplitude response from the scattered pilots
 * A measurement block (csrc/k_sounder.hpp): it consumes demodulated symbols as a stream of fft-shifted rows, changes nothing and accumulates on the device.
 * Every fourth symbol has a scattered pilot on every twelfth carrier, so four consecutive symbols give the channel on every third carrier, and the inverse
 * transform of that comb is the impulse response over Tu / 3.
 *   Mode       2k or 8k, with N, K (1705 / 6817) and zl = zeros_on_left as dvbt_get_dims gives them.  Kp = (K - 1) / 3 + 1 (569 / 2273), M = N / 2
 *              (1024 / 4096), w_k = +-4/3 the pilots' reference values.
 *   Input      per symbol s (the stream position, counted over all calls since create or reset) one row Y_s of N complex64 in fft-shifted order -- the
 *              layout of DVBT_TAP_FFT, of dvbt_fft with shift and of dvbt_tx_read_carriers -- and three int32: symbol_index (0..67), freq_offset (-8..7)
 *              and cp_start.  Each of the three arrays may be NULL: 0, 0 and the index (first_index + s) mod 68, for rows straight from a modulator.
 *   Group      group g is the symbols [4 g, 4 g + 4).  It is USED iff the four indices are consecutive mod 68 (and in 0..67), the four offsets are equal
 *              (and in -8..7) and |d_i| <= 64, d_i = cp_start[4 g + i] - cp_start[4 g].  Any other group is SKIPPED and counted; it adds nothing.
 *   Symbol     of a used group, with l = index mod 4, o = freq_offset, c0 = (K - 1) / 2:
 *                tau_i(k) = cis(-2 pi ((k - c0) d_i mod N) / N)          (an exact N-th root of unity: the FFT's own twiddle table)
 *                c_i      = sum_k Y[zl + k + o] w_k tau_i(k)             over the continual-pilot carriers
 *                r_i      = c_0 conj(c_i) / |c_0 conj(c_i)|              (1 where that is 0 or not finite)
 *                E[k / 3] = Y[zl + k + o] w_k (9/16) tau_i(k) r_i        for k = 3 l + 12 p < K
 *              tau undoes the move of the receiver's FFT window inside the group, r the common phase between its symbols.  Each of the Kp entries is
 *              written exactly once per group.
 *   Profile    per used group x[j] = E[j] win[j] for j < Kp and 0 up to M; win is 0 rectangular or 1 periodic Hann, 0.5 - 0.5 cos(2 pi j / Kp), a float
 *              table computed in double.  h[m] = (sum_j x[j] e^{+2 pi i j m / M}) / sum win, so that a single unit path reads |h|^2 = 1.
 *              pdp[m] += |h[m]|^2 and resp[j] += |E[j]|^2: both are sums over the used groups.
 *   Geometry   bin m is a delay of 2 m / 3 samples; the profile is periodic in N / 3 samples; bins from M / 2 on read as negative delays (pre-echoes).
 * A stream cut into calls of any sizes (0 and 1 included) gives the pdp, resp and counts of one call, bit for bit, through either entry: sums are formed in an
 * order fixed by the stream (runs of 8 groups in float, the runs in ascending order in double), never by atomics in floating point; the symbols of a group
 * that a call leaves open are carried on the device.  dvbt_sounder_read synchronises and does not disturb the accumulation; pdp takes M doubles and resp Kp
 * (cap_*: what the caller's arrays hold; either may be NULL).  dvbt_sounder_push_device takes four device pointers and only enqueues on `stream`; calls on
 * different streams are ordered by the handle (an event).  nsym <= 2^24 per call, 2^56 per stream; rows 8-byte aligned.  One thread per handle.  Every
 * parameter is checked before the device is asked for: a bad struct or pointer is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU --
 * there is no CPU path.  A refused call leaves the stream where it was. */
typedef struct { int device, transmission_mode, window, first_index; } dvbt_sounder_params;
typedef struct {
  long long symbols_pushed, groups_used, groups_skipped;
  int M, Kp;
} dvbt_sounder_result;
typedef struct dvbt_sounder dvbt_sounder;
int  dvbt_sounder_create(const dvbt_sounder_params *p, dvbt_sounder **out);
int  dvbt_sounder_push(dvbt_sounder *h, const void *rows_host, const int *idx_host, const int *off_host, const int *cps_host, size_t nsym);
int  dvbt_sounder_push_device(dvbt_sounder *h, const void *rows_dev, const int *idx_dev, const int *off_dev, const int *cps_dev, size_t nsym, void *stream);
int  dvbt_sounder_read(dvbt_sounder *h, dvbt_sounder_result *result, double *pdp /* M, may be NULL */, size_t cap_pdp,
                       double *resp /* Kp, may be NULL */, size_t cap_resp);
int  dvbt_sounder_reset(dvbt_sounder *h);   /* back to the state after create */
void dvbt_sounder_destroy(dvbt_sounder *h);

/* ------------------------------------------------------------------ constellation: the I/Q density, the error cloud of every point and the MER per carrier
 * A measurement block (csrc/k_constellation.hpp): it consumes equalised data cells as a stream of rows of P = row_length complex64 -- the layout of
 * DVBT_TAP_EQ, P = payload_length there -- changes nothing and accumulates on the device, in one pass.  Every accumulated quantity is an INTEGER: the error
 * vector is quantised once per cell to 2^-12 of the grid unit, in float32 operations that are spelled out below, and everything behind that is integer adds.
 *   Grid       constellation DVBT_QPSK / DVBT_QAM16 / DVBT_QAM64: L = 2, 4, 8 levels per axis, H = L / 2.  hierarchy DVBT_NH, DVBT_ALPHA1, DVBT_ALPHA2,
 *              DVBT_ALPHA4: alpha = 1, 1, 2, 4 (QPSK takes DVBT_NH only).  The ideal levels of a half axis are alpha + 2 j, j = 0 .. H - 1, in units of d,
 *              the `norm` of dvbt_get_dims.  inv_d = the float nearest to sqrt(s): s = 2, 10, 42 for alpha 1; 20, 60 for alpha 2; 52, 108 for alpha 4.
 *   Axis       per cell and per axis, x the float component.  Every operation is ONE float32 operation rounded to nearest, none contracted into an fma:
 *                neg   = the sign bit of x (-0.0 is negative);  a = |x|
 *                the cell is NON-FINITE if either component has an all-ones exponent: it is counted in `nonfinite` and adds nothing else
 *                u     = a * inv_d
 *                t     = (u - (float)(alpha - 1)) * 0.5f
 *                j     = t < 1 ? 0 : t >= H ? H - 1 : (int)t;   level = alpha + 2 j
 *                dl    = u - (float)level
 *                r     = rintf(dl * 4096.0f)
 *                q     = (int)fminf(fmaxf(r, -32767.f), 32767.f);   a cell with |r| > 32767 on either axis is also counted in `clipped` (it still adds)
 *                q     = neg ? -q : q
 *                index = neg ? H - 1 - j : H + j           (the column from the real part, the row from the imaginary part)
 *              point p = row * L + col.
 *   Density    G = DVBT_CONSTELLATION_GRID bins per axis over [-S, S) in units of d, S = the smallest power of two not below alpha + L - 1 (2, 4, 8 for
 *              alpha 1; 8 or 16 otherwise; `span` in the result), so that G / (2 S) is a power of two and the product below exact:
 *                e = neg ? -u : u;   b = (int)fminf(fmaxf(floorf(e * (G / (2 S))), -G / 2), G / 2 - 1) + G / 2    (beyond the span: the edge bins)
 *                hist[b_im * G + b_re]++
 *   Points     per point p (L^2 of them): n and the first and second moments of (q_re, q_im): sum_re, sum_im, sum_re_im (signed), sum_re2, sum_im2.
 *   Carriers   per carrier c = the cell's index within its row (P of them): n, signal += level_re^2 + level_im^2, error += q_re^2 + q_im^2.  The MER of
 *              carrier c is 10 log10(signal 4096^2 / error).
 * All sums are 64-bit integers and integer adds commute: a stream cut into calls of any sizes, through either entry, on any launch geometry, gives the same
 * bits, and a host model (tests/constref.py) reproduces the device exactly.  The quantisation's noise lies about 100 dB below a 64-QAM signal.
 * row_length 1 .. 8192; nrows <= 2^24 per call (0 is accepted and adds nothing); at most 2^33 cells per stream (32767^2 2^33 < 2^63: no sum can wrap), a
 * push beyond that is DVBT_ERR_CAPACITY.  Rows are 8-byte aligned; a null or misaligned pointer with nrows > 0 is DVBT_ERR_INVALID.
 * dvbt_constellation_read synchronises and does not disturb the accumulation; hist takes G G words, points cap_points >= L^2 entries, carriers
 * cap_carriers >= P entries (each may be NULL; a cap that is too small is DVBT_ERR_CAPACITY).  dvbt_constellation_push_device only enqueues on `stream`;
 * calls on different streams are ordered by the handle (an event).  One thread per handle.  Every parameter is checked before the device is asked for: a
 * bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU path.  A refused call leaves the stream
 * where it was. */
enum { DVBT_CONSTELLATION_GRID = 128 };
typedef struct { int device, constellation, hierarchy, row_length; } dvbt_constellation_params;
typedef struct { long long n, sum_re, sum_im, sum_re_im, sum_re2, sum_im2; } dvbt_constellation_point;
typedef struct { long long n, signal, error; } dvbt_constellation_carrier;
typedef struct {
  long long rows_pushed, cells, nonfinite, clipped;
  int points, levels, alpha, span;
} dvbt_constellation_result;
typedef struct dvbt_constellation dvbt_constellation;
int  dvbt_constellation_create(const dvbt_constellation_params *p, dvbt_constellation **out);
int  dvbt_constellation_push(dvbt_constellation *h, const void *rows_host, size_t nrows);
int  dvbt_constellation_push_device(dvbt_constellation *h, const void *rows_dev, size_t nrows, void *stream);
int  dvbt_constellation_read(dvbt_constellation *h, dvbt_constellation_result *result, unsigned long long *hist /* G * G, may be NULL */,
                             dvbt_constellation_point *points /* may be NULL */, size_t cap_points,
                             dvbt_constellation_carrier *carriers /* may be NULL */, size_t cap_carriers);
int  dvbt_constellation_reset(dvbt_constellation *h);   /* back to the state after create */
void dvbt_constellation_destroy(dvbt_constellation *h);

/* ------------------------------------------------------------------ tuner: a recording from an SDR -> complex64 baseband at the elementary rate
 * Raw interleaved I/Q in one of four formats, at the capture's rate and with the channel off-centre, to complex64 at L/M times that rate, in one kernel
 * (csrc/k_tuner.hpp; tests/tunerref.py is this text in numpy).  All indices are absolute: the stream's first input sample is n = first_in, x[n] = 0 in
 * front of it.
 *   Formats    DVBT_IQ_CF32 (8 bytes per sample, float I then float Q), DVBT_IQ_CS16 (4, int16), DVBT_IQ_CS8 (2, int8), DVBT_IQ_CU8 (2, uint8).
 *   1 Convert  swap_iq exchanges I and Q first.  Then per component v = (float)raw * scale; for CU8 v = ((float)raw - 127.5f) * scale (the difference is
 *              exact).  One rounded multiply; CF32 with scale == 1 keeps the bits.  (The usual scales: 1, 1/32768, 1/128, 1/127.5.)
 *   2 Mix      inc = nearbyint(shift 2^64) mod 2^64 (ties to even), shift in cycles per INPUT sample, |shift| <= 0.5.  ph(n) = n inc mod 2^64,
 *              (c, s) = the cosine and sine of the top 32 bits of ph as a fraction of a turn (the channel block's float polynomial, csrc/k_channel.hpp),
 *              z = (v.re c - v.im s, v.re s + v.im c), every product and every sum rounded on its own.  inc == 0: the stage is skipped, z = v bit for bit.
 *   3 Resample by L/M = interpolation / decimation after gcd reduction.  h is a real prototype of ntaps taps at L times the input rate, its branches
 *              br[b][k] = h[b + k L], zero padded to nt = ceil(ntaps / L) taps each.  Output m: n(m) = floor(m M / L), b = m M mod L,
 *                y[m] = sum_{k = nt-1 .. 0} br[b][k] z[n(m) - k]
 *              in that order (ascending input index), re and im apart, every product rounded, then every sum; no fused multiply-add.  The first product
 *              starts the sum: that is a sum from +0 in every bit but one -- a sum whose products are all -0.0 stays -0.0, so L = M = 1 with the one tap
 *              1.0 returns the input's bits, -0.0 included.  A numpy float32 loop over k reproduces an output literally.
 *   Counts     once the inputs in front of Nabs = first_in + N have arrived, every m with n(m) < Nabs has been emitted: ceil(Nabs L / M) -
 *              ceil(first_in L / M) outputs, host integer arithmetic (dvbt_tuner_outputs, dvbt_tuner_outputs_for).  Every input is consumed; no flush.
 *   Streaming  the handle keeps the last 320 values of z on the device (z is a function of the raw sample and n alone).  A stream cut into calls of any
 *              sizes (0, 1 and fewer than nt included; a CS8 or CU8 stream cut at an odd sample is 2-byte aligned) gives bit for bit what one call
 *              gives, and a handle with first_in = n0 fed from n0 on equals the whole stream from output ceil((n0 + nt - 1) L / M) on.  Index
 *              arithmetic is 64-bit: first_in in [0, 2^48], at most 2^48 inputs per stream.
 *   Taps       dvbt_tuner_create takes the caller's prototype (taps, ntaps) or, with taps == NULL, designs one from pass_edge, stop_edge (fractions of
 *              the OUTPUT rate) and atten_db (dB) -- a Kaiser-windowed sinc, computed in double (dvbt_tuner_design is the same rule, needs no device):
 *                L > M: stop = min(stop, M / L - pass) (the images of the capture); refused unless stop > pass
 *                fp = pass / M, fs = stop / M, fc = (fp + fs) / 2
 *                beta = 0.1102 (A - 8.7) for A > 50, else 0.5842 (A - 21)^0.4 + 0.07886 (A - 21)
 *                ntaps = ceil((A - 7.95) / (2.285 2 pi (fs - fp))) + 1, plus one if that is even
 *                h[i] = 2 fc sinc(2 fc (i - c)) Io(beta sqrt(1 - ((i - c) / c)^2)) / Io(beta), c = (ntaps - 1) / 2, Io by its power series
 *                scaled so that sum h = L, then rounded to float.
 *              The group delay is (ntaps - 1) / (2 M) output samples (dvbt_tuner_info: delay_num / delay_den).
 *   Limits     format one of the four; 1 <= L <= 128, 1 <= M <= 1024 after reduction, M / L <= 8; nt <= 320 and L nt <= 8192; scale finite and not 0;
 *              shift finite, |shift| <= 0.5; atten_db in [40, 90]; 0 < pass_edge < stop_edge <= 1 (also where the caller brings the taps); swap_iq 0 or
 *              1; taps finite.  Per call n_in <= 2^31; the input pointer aligned to one raw sample (8 / 4 / 2 / 2 bytes), the output to 8 bytes; input
 *              and output ranges that overlap are DVBT_ERR_INVALID; out_cap below the call's count is DVBT_ERR_CAPACITY.  A failed call leaves the
 *              stream position and the history as they were.
 * dvbt_tuner_run_device only enqueues on `stream`; calls on different streams are ordered by the handle (an event).  One thread per handle.  Every
 * parameter is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is
 * no CPU path, except dvbt_tuner_outputs and dvbt_tuner_design, which are host arithmetic.
 * Deliberately not here: (1) DC blocking and AGC -- sequential filters, not a map over the stream; (2) a level or clip meter -- dvbt_spectrum_* measures
 * the output; (3) ratios that are not rational -- a dvbt_clock_* handle behind the tuner takes the ppm; (4) any change to dvbt_rx_stream_*, which takes
 * the tuner's output through dvbt_rx_stream_push_device; (5) GNU Radio shells around the block. */
enum { DVBT_IQ_CF32 = 0, DVBT_IQ_CS16 = 1, DVBT_IQ_CS8 = 2, DVBT_IQ_CU8 = 3 };
typedef struct {
  int format;                                    /* DVBT_IQ_* */
  int interpolation, decimation;                 /* L / M before reduction */
  int swap_iq;                                   /* 0 or 1 */
  double shift;                                  /* cycles per input sample, -0.5 .. 0.5 */
  float scale;                                   /* finite, not 0 */
  double pass_edge, stop_edge, atten_db;         /* of the designed prototype: fractions of the output rate, dB */
  int64_t first_in; int device;
} dvbt_tuner_params;
typedef struct {
  int interpolation, decimation;                 /* reduced */
  int ntaps, nt;                                 /* of the prototype in use; taps per branch */
  int64_t delay_num, delay_den;                  /* group delay in output samples: (ntaps - 1) / (2 M) */
  uint64_t phase_inc;                            /* inc of the mixer */
} dvbt_tuner_desc;
typedef struct dvbt_tuner dvbt_tuner;
/* the designed prototype of a valid struct: *ntaps = its length; taps (cap floats) may be NULL to ask for the length alone */
int  dvbt_tuner_design(const dvbt_tuner_params *p, float *taps, int cap, int *ntaps);
/* outputs emitted once n_in_total (<= 2^48) inputs have been pushed; ntaps = the caller's prototype length, 0: the designed one (it decides only whether
 * the struct is accepted).  Host arithmetic, needs no device. */
int  dvbt_tuner_outputs(const dvbt_tuner_params *p, int ntaps, int64_t n_in_total, int64_t *n_out_total);
int  dvbt_tuner_create(const dvbt_tuner_params *p, const float *taps /* NULL: designed */, int ntaps, dvbt_tuner **out);
int  dvbt_tuner_get_taps(const dvbt_tuner *h, float *taps /* may be NULL */, int cap, int *ntaps);
int  dvbt_tuner_info(const dvbt_tuner *h, dvbt_tuner_desc *desc);
int  dvbt_tuner_outputs_for(const dvbt_tuner *h, size_t n_in, size_t *n_out);   /* what the NEXT call of n_in samples emits */
int  dvbt_tuner_run(dvbt_tuner *h, const void *raw_host, size_t n_in, void *out_host, size_t out_cap, size_t *n_out);
int  dvbt_tuner_run_device(dvbt_tuner *h, const void *raw_device, size_t n_in, void *out_device, size_t out_cap, size_t *n_out, void *stream);
int  dvbt_tuner_reset(dvbt_tuner *h);   /* back to first_in, history cleared */
void dvbt_tuner_destroy(dvbt_tuner *h);

/* ------------------------------------------------------------------ transport stream: the PIDs, their continuity and the timing of their PCRs
 * A measurement block (csrc/k_ts.hpp; tests/tsref.py is this text in Python): it consumes a stream of 188-byte packets -- the layout of DVBT_TAP_TS --
 * changes nothing and accumulates on the device.  Every accumulated quantity is a 64-bit INTEGER.  The checks are those of ETSI TR 101 290's first two
 * priority tables that need no section parsing.  Packets are numbered i = 0, 1, ... from create / reset, across calls; a packet's bytes are b0 .. b187.
 *   1 Sync        b0 != 0x47: count `sync_errors`.  The packet adds nothing else and belongs to no PID.
 *   2 Header      tei = b1 >> 7, pusi = (b1 >> 6) & 1, pid = ((b1 & 0x1f) << 8) | b2, tsc = b3 >> 6, afc = (b3 >> 4) & 3, cc = b3 & 15, pay = afc & 1,
 *                 af = afc >> 1.
 *   3 Transport   tei set: count `transport_errors` and the PID's `tei`.  The packet adds nothing else and is not a MEMBER (its other fields are unreliable).
 *   4 Members     every other packet is a member of its PID's sequence.  Per PID: `packets`, `pusi`, `scrambled` (tsc != 0), `payload` (pay), `adaptation`
 *                 (af), and `first` / `last`, the smallest and the largest i of a member.
 *   5 Reserved    afc == 0: also count `afc_reserved` (a total).
 *   6 Adaptation  only if af is set.  afl = b4.  afl is BAD if afl > 183 - pay: count `af_length_errors` (a total) and read nothing more of the field.
 *                 Otherwise, if afl >= 1: di = b5 >> 7, rai = (b5 >> 6) & 1, pf = (b5 >> 4) & 1.  di counts `discontinuity`, rai `random_access`.
 *                 pf set and afl < 7: count `af_length_errors` and take no PCR.  pf set and afl >= 7: base = b6 << 25 | b7 << 17 | b8 << 9 | b9 << 1 |
 *                 b10 >> 7, ext = (b10 & 1) << 8 | b11, pcr = 300 base + ext; count the PID's `pcr`.  Without a readable field di = rai = pf = 0.
 *   7 Continuity  not evaluated for PID 0x1FFF.  For a member i, j is the previous member of the same PID and k the one before j.
 *                   same(i) = pay_i && pay_j && cc_i == cc_j && !di_i; 0 without a j.  (same(j) needs k and nothing older.)
 *                   no j, or di_i set:                    nothing
 *                   else cc_i == ((cc_j + pay_i) & 15):   in order
 *                   else same(i) && !same(j):             count `duplicates` (the one repeat the standard allows)
 *                   else:                                 count `cc_errors` (a third copy counts here)
 *   8 PCR pairs   per PID, over its members that carry a PCR: a the previous such member, b the current one (no a: no pair, nothing is counted).
 *                   di_b:                                 count `pcr_discontinuity_signalled`; the pair ends there
 *                   else dt = (pcr_b - pcr_a) mod (2^33 300), dp = i_b - i_a
 *                   dt > 2,700,000 (100 ms):              count `pcr_over_100ms`; the pair adds nothing else (a backwards jump lands here)
 *                   else:                                 count `pcr_pairs`, sum_dt += dt, sum_dp += dp, update min_dt, max_dt, max_dp; dt > 1,080,000
 *                                                         (40 ms): count `pcr_over_40ms`
 *   9 Totals      packets_pushed, sync_errors, transport_errors, afc_reserved, af_length_errors, pids_seen (the PIDs with packets + tei > 0).
 * `first` and `min_dt` are -1 while unset; max_dt and max_dp are 0.  The transport stream's rate follows on the host from a PCR PID's sums:
 * sum_dp 188 8 27e6 / sum_dt bits per second.
 * The continuity rule and the PCR pairs relate a packet to the previous packet of its PID wherever that was -- another tile, batch or call: the handle keeps
 * per PID (cc, pay, same) of its last member and its last PCR with index.  A stream cut into calls of any sizes, through either entry, gives the same bits.
 * The packet pointer may have ANY byte alignment.  A null pointer with npackets > 0 is DVBT_ERR_INVALID; npackets = 0 is accepted and adds nothing.  A call
 * is worked off in batches of min(max_packets, 2^19) packets inside the call; the scratch is sized for one batch, once, at create.  max_packets 1 .. 2^24.
 * More than 2^40 packets per stream is DVBT_ERR_CAPACITY.  dvbt_ts_read synchronises and does not disturb the accumulation: it returns the entries of the
 * PIDs seen, ascending by pid, *n_pids of them (pids may be NULL to ask for the totals and the count alone; a cap below the count is DVBT_ERR_CAPACITY).
 * dvbt_ts_push_device only enqueues on `stream`; calls on different streams are ordered by the handle (an event).  One thread per handle.  Every parameter
 * is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU
 * path.  A refused call leaves the stream where it was.
 * Deliberately not here: (1) section parsing -- PAT, PMT, CRC, the indicators 1.3, 1.5, 2.2; (2) PCR accuracy (jitter against a fit); (3) PTS; (4) whether a
 * duplicate repeats its packet byte for byte; (5) a GNU Radio shell; (6) sync search on the device (the stream starts on a packet). */
enum { DVBT_TS_PACKET = 188, DVBT_TS_PIDS = 8192, DVBT_TS_TILE = 1024 /* packets per workgroup tile: where the device's work is cut */ };
typedef struct { int device; int max_packets; } dvbt_ts_params;
typedef struct {
  long long pid, packets, pusi, scrambled, payload, adaptation, discontinuity, random_access, pcr, tei, duplicates, cc_errors, first, last,
            pcr_pairs, pcr_discontinuity_signalled, pcr_over_100ms, pcr_over_40ms, sum_dt, sum_dp, min_dt, max_dt, max_dp;
} dvbt_ts_pid;
typedef struct { long long packets_pushed, sync_errors, transport_errors, afc_reserved, af_length_errors, pids_seen; } dvbt_ts_result;
typedef struct dvbt_ts dvbt_ts;
int  dvbt_ts_create(const dvbt_ts_params *p, dvbt_ts **out);
int  dvbt_ts_push(dvbt_ts *h, const void *packets_host, size_t npackets);
int  dvbt_ts_push_device(dvbt_ts *h, const void *packets_dev, size_t npackets, void *stream);
int  dvbt_ts_read(dvbt_ts *h, dvbt_ts_result *result, dvbt_ts_pid *pids /* may be NULL */, size_t cap, size_t *n_pids /* may be NULL */);
int  dvbt_ts_reset(dvbt_ts *h);   /* back to the state after create */
void dvbt_ts_destroy(dvbt_ts *h);

/* ------------------------------------------------------------------ cfr: crest-factor reduction by iterative clipping and filtering, per OFDM symbol
 * What a DVB-T exciter does to its baseband before the amplifier: the peaks are clipped, and the clipping error is filtered so that it stays on the occupied
 * carriers and off the ones the receiver leans on.  complex64 in, as many out, whole symbols of G + N samples (N = 2048 or 8192, G = N / 32 .. N / 4), one
 * workgroup per symbol (csrc/k_cfr.hpp); tests/cfrref.py is this text in numpy (complex128).  The receiver needs no change.
 * For one symbol, u its last N samples, A = threshold, os = oversampling, l the symbol's index in the stream (first_symbol + the symbols the handle has seen):
 *   1 Spectrum  X0[k] = sum_n u[n] e^{-2 pi i n k / N}.  Signed index kappa = k for k < N / 2, else k - N.  Bin k is occupied iff |kappa| <= (K - 1) / 2,
 *               K = 1705 (2k) or 6817 (8k); its carrier is c = kappa + (K - 1) / 2.
 *   2 Phases    phase p < os of the current spectrum X: x_p[n] = (1 / N) sum_k X[k] e^{+2 pi i kappa (n + p / os) / N} -- ONE N-point inverse transform of
 *               X[k] r_p[k], r_p[k] = e^{2 pi i kappa p / (os N)} (sine and cosine at full precision of the exactly formed argument; r_0 = 1 is not
 *               multiplied).  The os phases together are the symbol at os times the sample rate; no transform larger than N exists.
 *   3 Clip      c_p[n] = x_p[n] where |x_p[n]|^2 <= A^2 (both sides float32), else x_p[n] g, g = A / sqrt(|x_p[n]|^2), division and root correctly rounded.
 *   4 Back      C[k] = (1 / os) sum_p FFT_N(c_p)[k] conj(r_p[k]), p ascending: on the occupied bins exactly the os N-point spectrum of the clipped
 *               oversampled signal (the aliases cancel).
 *   5 Filter    E = C - X0, then E[k] = 0 on every unoccupied bin; E = 0 on the continual pilots and on the scattered pilots of symbol l (carriers
 *               3 (l mod 4) + 12 j) when keep & DVBT_CFR_KEEP_PILOTS; E = 0 on the TPS carriers when keep & DVBT_CFR_KEEP_TPS.  X = X0 + E: the
 *               kernel takes C[k] itself where the error passes and leaves X0[k], bit for bit, everywhere else.
 *   6 Repeat    2 .. 5 `iterations` times, from X = X0.
 *   7 Output    the useful part (1 / N) sum_k X[k] e^{+2 pi i n k / N}; its last G samples repeated in front as the cyclic prefix.
 * A symbol is passed through bit for bit, prefix included, (a) when any of its G + N samples is not finite -- counted in symbols_nonfinite, nothing else of
 * it is looked at; (b) when iterations == 0; (c) when no |x_p[n]|^2 > A^2 in the first iteration.  Every other symbol runs exactly `iterations` iterations
 * (from the second on many samples sit AT A, and an early exit would be decided by rounding).  What is outside the occupied band in the input stays as it is;
 * the mean power drops by about 1 % at 7 dB and is not made up for.  Samples beyond 1.8e19 in magnitude overflow |x|^2 and are the caller's to avoid.
 * Accumulators on the device, read by dvbt_cfr_read (it synchronises and disturbs nothing): symbols; symbols_clipped (those that ran the iterations);
 * symbols_nonfinite; samples_over, the count of |x_p[n]|^2 > A^2 over all phases of the first iteration; peak_power_in, the largest |x_p[n]|^2 seen in a
 * first iteration (the max of non-negative floats, taken on their bit patterns).  dvbt_cfr_reset zeroes them and goes back to first_symbol.
 * The scattered-pilot phase is all a symbol takes from its position: a stream cut into calls at any symbol boundaries, on any streams, gives the bits of one
 * call, and a handle with first_symbol = s gives the bits of the handle that began at 0 from symbol s on.
 * Buffers: nsamples <= 2^31 complex64 each per call, 8-byte aligned, nsamples a multiple of G + N (0 is accepted and does nothing).  Input and output may be
 * the SAME buffer (in place); ranges that overlap in any other way are DVBT_ERR_INVALID.  A refused call leaves the symbol counter and the accumulators as they
 * were.  dvbt_cfr_run_device only enqueues on `stream`; calls on different streams are ordered by the handle (an event).  One thread per handle.  Every
 * parameter is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is
 * no CPU path.
 * Deliberately not here: (1) a bound on the error per carrier; (2) tone reservation; (3) power renormalisation; (4) calls that cut a symbol; (5) a GNU Radio
 * shell. */
enum { DVBT_CFR_KEEP_PILOTS = 1, DVBT_CFR_KEEP_TPS = 2 };
typedef struct {
  int transmission_mode, guard_interval;         /* dvbt_transmission_mode_t, dvbt_guard_interval_t */
  float threshold;                               /* A: finite, > 0 */
  int iterations;                                /* 0 .. 8; 0: pass-through */
  int oversampling;                              /* 1, 2 or 4 */
  int keep;                                      /* DVBT_CFR_KEEP_* */
  int64_t first_symbol;                          /* >= 0: the stream's first symbol's index in its frame (mod 4 is what matters) */
  int device;
} dvbt_cfr_params;
typedef struct { long long symbols, symbols_clipped, symbols_nonfinite, samples_over; float peak_power_in; } dvbt_cfr_result;
typedef struct dvbt_cfr dvbt_cfr;
int  dvbt_cfr_create(const dvbt_cfr_params *p, dvbt_cfr **out);
int  dvbt_cfr_run(dvbt_cfr *h, const void *iq_host, size_t nsamples, void *out_host);
int  dvbt_cfr_run_device(dvbt_cfr *h, const void *iq_device, size_t nsamples, void *out_device, void *stream);
int  dvbt_cfr_read(dvbt_cfr *h, dvbt_cfr_result *result);
int  dvbt_cfr_reset(dvbt_cfr *h);   /* back to first_symbol, accumulators zeroed */
void dvbt_cfr_destroy(dvbt_cfr *h);

/* ------------------------------------------------------------------ scan: FFT size, guard interval, symbol timing and fractional carrier offset of an unknown signal
 * A measurement block (csrc/k_scan.hpp): it consumes complex64 baseband at the elementary rate as a stream, changes nothing and accumulates on the device, in
 * one pass, the cyclic-prefix correlation at the lags 2048 and 8192 folded at the eight symbol lengths a DVB-T signal can have.  dvbt_rx_stream_* reads
 * constellation, hierarchy and code rate from the TPS word (DVBT_AUTO) but must be given mode and guard: this block finds them.  tests/scanref.py is this
 * text in numpy.
 *   Hypotheses h = 0 .. 7, mode = h >> 2, guard = h & 3: N = 2048 or 8192, G = N / 32, N / 16, N / 8 or N / 4, S = N + G.
 *   Positions  n = 0 is the first sample pushed since create or reset.
 *   Terms      for a = x[n], b = x[n + N], in float32, every product and every sum rounded on its own (no FMA):
 *                p.re = (a.re b.re) + (a.im b.im)      p.im = (a.im b.re) - (a.re b.im)      e = ((a.re a.re) + (a.im a.im)) + ((b.re b.re) + (b.im b.im))
 *   Symbols    symbol j of hypothesis h is the positions [j S, j S + S), its bin m = n - j S.  A symbol is folded once it is complete, i.e. when
 *              (j + 1) S + N <= samples pushed: J_h = (samples - N) / S symbols (0 below N), the same count in every bin of a hypothesis.
 *   Sums       a group is DVBT_SCAN_GROUP = 16 consecutive symbols [16 g, 16 g + 16) of a hypothesis.  Per bin, the terms of a group are added in float32 in
 *              ascending j, starting from +0 (acc = acc + term); closed groups are added to double accumulators in ascending g; the open group is kept
 *              as it stands and dvbt_scan_read / dvbt_scan_accumulators add it, converted to double, last.  This gives A_h[m] (complex) and E_h[m], m < S.
 *   Evaluation in double on the host, per hypothesis, every operation rounded on its own, sums running from 0.0 in ascending index:
 *                mean   = (sum_m A[m]) / S, re and im each;   A'[m] = A[m] - mean.  (What correlates at every lag -- DC, a CW spur, the pilots' comb --
 *                         reads rho ~ 0.9 on all eight hypotheses without this and ~ 0.02 with it.)
 *                C[0]   = sum_{k < G} A'[k];   C[m + 1] = (C[m] - A'[m]) + A'[(m + G) mod S].   Phi[m] likewise from E, the mean not removed.
 *                m*     = the smallest m that maximises q[m] = (C.re C.re) + (C.im C.im)  (found with >, so a NaN never wins)
 *                rho    = sqrt(q[m*]) / (Phi[m*] / 2); 0 when J_h = 0 or Phi[m*] <= 0; NaN when sum_m A[m] or sum_m E[m] is not finite
 *                symbol_start = m*: the stream position, modulo S, of the first sample of a guard interval
 *                cfo    = -atan2(C.im, C.re) / (2 pi) at m*, in carrier spacings, in (-0.5, 0.5]  (-0.5 is returned as 0.5)
 *   Verdict    b = the hypothesis of the largest rho, r = the largest of the others (the smallest h among equals, both).  detected = 1 iff every J_h >= 8
 *              (i.e. samples >= DVBT_SCAN_MIN_SAMPLES), nonfinite == 0 and every rho finite, rho[b] >= rho_min, and rho[b] >= ratio_min rho[r].  mode and
 *              guard are b's when detected, else -1; symbols (J_h), rho, symbol_start and cfo are filled for all eight either way.
 *              rho_min = 0 means 0.1 and ratio_min = 0 means 1.5 (DESIGN.md 4h7 has the figures behind them); otherwise 0 < rho_min <= 1, 1 <= ratio_min <= 1e6.
 * A stream cut into calls of any sizes (1 and 0 included, 8-byte aligned only) gives the accumulators of one call, bit for bit, through either entry, on any
 * device; no atomics in floating point.  Non-finite samples (either part inf or NaN) are counted, each once, by an integer atomic.  The handle carries the up to
 * 10240 + 8192 - 1 newest samples in two buffers written alternately; which symbols a call completes is host arithmetic on the sample count, so a device push
 * never waits.  dvbt_scan_push_device only enqueues on `stream`; calls on different streams are ordered by the handle (an event).  dvbt_scan_read synchronises,
 * evaluates through dvbt_scan_evaluate, and does not disturb the accumulation.  n <= 2^31 per call, 2^56 per stream.  One thread per handle.  Every parameter
 * is checked before the device is asked for: a bad struct is DVBT_ERR_INVALID everywhere, a good one DVBT_ERR_NO_DEVICE without a GPU -- there is no CPU path,
 * except dvbt_scan_evaluate, which is host arithmetic.  A refused call leaves the stream where it was.
 *   dvbt_scan_accumulators  hypothesis hyp's sums as dvbt_scan_read sees them: A as S pairs (re, im), E as S doubles; cap = the bins the buffers hold, >= S.
 *   dvbt_scan_evaluate      the evaluation alone.  symbols[h] = J_h >= 0; A[h] (S pairs) and E[h] (S doubles) may be NULL where symbols[h] = 0.  p->device is
 *                           checked like the rest and not used.
 * Deliberately not here: (1) the integer part of the carrier offset -- the receiver's continual-pilot search finds it; (2) a search over 6 and 7 MHz
 * channels -- the caller's tuner sets the elementary rate; (3) any change to dvbt_rx_stream_*: the detected pair goes into its parameters. */
enum { DVBT_SCAN_HYPOTHESES = 8, DVBT_SCAN_GROUP = 16, DVBT_SCAN_MIN_SAMPLES = 8 * 10240 + 8192 };
typedef struct { int device; double rho_min, ratio_min; } dvbt_scan_params;
typedef struct {
  int detected, mode, guard;                     /* mode: dvbt_transmission_mode_t, guard: dvbt_guard_interval_t, -1 unless detected */
  int symbol_start[8];
  long long samples_pushed, nonfinite;
  long long symbols[8];
  double rho[8], cfo[8];
} dvbt_scan_result;
typedef struct dvbt_scan dvbt_scan;
int  dvbt_scan_create(const dvbt_scan_params *p, dvbt_scan **out);
int  dvbt_scan_push(dvbt_scan *h, const void *iq_host, size_t n);
int  dvbt_scan_push_device(dvbt_scan *h, const void *iq_device, size_t n, void *stream);
int  dvbt_scan_read(dvbt_scan *h, dvbt_scan_result *result);
int  dvbt_scan_accumulators(dvbt_scan *h, int hyp, double *A_re_im /* 2 S */, double *E /* S */, int cap);
int  dvbt_scan_evaluate(const dvbt_scan_params *p, const int64_t symbols[8], const double *const A[8], const double *const E[8], int64_t samples,
                        int64_t nonfinite, dvbt_scan_result *result);
int  dvbt_scan_reset(dvbt_scan *h);   /* back to the state after create */
void dvbt_scan_destroy(dvbt_scan *h);

#ifdef __cplusplus
}
#endif
#endif /* DVBT_HIP_H */
