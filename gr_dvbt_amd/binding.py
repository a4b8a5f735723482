import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_HERE, "lib", "libdvbt_hip.so")
_SRC = os.path.join(_HERE, "csrc", "dvbt_hip.hip")

QPSK, QAM16, QAM64 = 0, 1, 2
AUTO = -1          # RxStream: constellation / hierarchy / code_rate from the stream's TPS word
NH = 0
C1_2, C2_3, C3_4, C5_6, C7_8 = 0, 1, 2, 3, 4
T2k, T8k = 0, 1
G1_32, G1_16, G1_8, G1_4 = 0, 1, 2, 3
(TAP_ACQ, TAP_FFT, TAP_EQ, TAP_DEMAP, TAP_SYMDEINT, TAP_BITDEINT, TAP_VITERBI, TAP_DEINT, TAP_RS,
 TAP_TS, TAP_CP_START, TAP_SYMBOL_INDEX, TAP_FREQ_OFFSET, TAP_BITDEINT_LP, TAP_SOFT, TAP_CSI, TAP_BITDEINT_LOG) = range(17)
ALPHA1, ALPHA2, ALPHA4 = 1, 2, 3


class DvbtError(RuntimeError):
    pass


def hipcc():
    """the ROCm compiler driver (no environment variable is consulted: the package reads none)"""
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def build(force=False):
    """Compile the HIP extension for gfx950 in-tree (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(_ROOT, "include", "dvbt_hip.h"))
    if not force and os.path.exists(_SO) and all(os.path.getmtime(s) <= os.path.getmtime(_SO) for s in srcs):
        return _SO
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
           "-o", _SO, _SRC]
    subprocess.check_call(cmd)
    return _SO


class RxParams(C.Structure):
    _fields_ = [("constellation", C.c_int), ("hierarchy", C.c_int), ("code_rate", C.c_int),
                ("guard_interval", C.c_int), ("transmission_mode", C.c_int), ("include_cell_id", C.c_int),
                ("cell_id", C.c_int), ("snr_db", C.c_float), ("viterbi_bsize", C.c_int),
                ("rs_oracle_compat", C.c_int), ("descramble", C.c_int), ("max_samples", C.c_size_t),
                ("device", C.c_int), ("viterbi_chunk_bytes", C.c_int), ("resample_interp", C.c_int), ("resample_decim", C.c_int),
                ("front_scale", C.c_float), ("soft_decision", C.c_int), ("hier_stream", C.c_int), ("launch_graph", C.c_int), ("front_priority", C.c_int),
                ("viterbi_warm_windows", C.c_int), ("viterbi_verify", C.c_int)]


class RxReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_symbols", C.c_int32), ("first_out_symbol", C.c_int32),
                ("n_out_symbols", C.c_int32), ("cp_start0", C.c_int32), ("first_call", C.c_int32),
                ("n_viterbi_bytes", C.c_int64), ("n_rs_items", C.c_int64), ("n_rs_bytes", C.c_int64),
                ("n_ts_bytes", C.c_int64), ("rs_fail_words", C.c_int32), ("rs_corrected_symbols", C.c_int32),
                ("resume_sample", C.c_int64), ("segment_offset", C.c_int64), ("stream_symbol_offset", C.c_int64),
                ("ts_first_packet", C.c_int64), ("stream_rs_items", C.c_int64), ("tps_bits", C.c_uint64), ("tps_valid", C.c_int32),
                ("tps_length_indicator", C.c_int32), ("tps_constellation", C.c_int32), ("tps_hierarchy", C.c_int32),
                ("tps_code_rate_hp", C.c_int32), ("tps_code_rate_lp", C.c_int32), ("tps_guard_interval", C.c_int32),
                ("tps_transmission_mode", C.c_int32), ("tps_cell_id", C.c_int32), ("tps_mismatch", C.c_int32),
                ("n_lock_periods", C.c_int32), ("total_symbols", C.c_int32)]


class RxQuality(C.Structure):
    """dvbt_rx_quality_report.  The ratios are properties; each is nan where its figure was not measured."""
    _fields_ = [("mer_carriers", C.c_int64), ("mer_signal", C.c_double), ("mer_error", C.c_double),
                ("channel_bits", C.c_int64), ("channel_bit_errors", C.c_int64), ("post_bits", C.c_int64), ("post_bit_errors", C.c_int64),
                ("rs_fail_words", C.c_int32), ("rs_corrected_symbols", C.c_int32), ("n_lock_periods", C.c_int32), ("flags", C.c_int32)]

    @property
    def mer_db(self):
        if self.mer_carriers <= 0 or not self.mer_signal > 0.0:
            return float("nan")
        return float("inf") if self.mer_error <= 0.0 else 10.0 * float(np.log10(self.mer_signal / self.mer_error))

    @property
    def channel_ber(self):
        return self.channel_bit_errors / self.channel_bits if self.channel_bits > 0 else float("nan")

    @property
    def post_viterbi_ber(self):
        return self.post_bit_errors / self.post_bits if self.post_bits > 0 else float("nan")


class LockPeriod(C.Structure):
    _fields_ = [("offset", C.c_int64), ("first_call", C.c_int32), ("cp_start0", C.c_int32), ("n_symbols", C.c_int32),
                ("first_out_symbol", C.c_int32)]


class ViterbiProof(C.Structure):
    _fields_ = [("chunks", C.c_int64), ("decoded_again", C.c_int64), ("sequential", C.c_int64), ("not_proven", C.c_int64)]


class RxCut(C.Structure):
    _fields_ = [("stream_symbol_offset", C.c_int64), ("start_delay_symbols", C.c_int32), ("descr_call_phase", C.c_int32)]


class SymMetaRec(C.Structure):
    """dvbt_sym_meta: what the acquisition leaves per symbol (test hook dvbt_debug_acquire)"""
    _fields_ = [("cp_start", C.c_int32), ("sw", C.c_int32), ("eps", C.c_float), ("ph_base", C.c_float), ("incA", C.c_double), ("incB", C.c_double)]


class AcquireReport(C.Structure):
    """dvbt_acquire_report"""
    _fields_ = [("status", C.c_int32), ("call0", C.c_int32), ("cp_start0", C.c_int32), ("n_symbols", C.c_int32),
                ("avg", C.c_float), ("eps_init", C.c_float), ("avg_lost", C.c_float), ("small_viol", C.c_int32), ("drift_known_off", C.c_int32),
                ("changed", C.c_int32 * 4), ("need_seq", C.c_int32), ("need_heavy", C.c_int32), ("ncalls", C.c_int32), ("cap_symbols", C.c_int32),
                ("small_passes", C.c_int32), ("general_passes", C.c_int32), ("reserved", C.c_int32)]


# dvbt_debug_acquire's arguments (the tests set them on the loaded library: an A/B build of an older commit has no such entry)
ACQUIRE_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                    C.POINTER(AcquireReport), C.c_void_p, C.c_int] + [C.c_void_p] * 7


class Dims(C.Structure):
    _fields_ = [("fft_length", C.c_int), ("cp_length", C.c_int), ("Kmax", C.c_int), ("payload_length", C.c_int),
                ("zeros_on_left", C.c_int), ("m", C.c_int), ("cr_k", C.c_int), ("cr_n", C.c_int),
                ("norm", C.c_float), ("ntraceback", C.c_int), ("info_bits_per_symbol", C.c_int)]


_lib = None


def lib():
    """Load libdvbt_hip.so. Fails loudly when the extension is missing: there is no fallback.

    Note for processes that also use PyTorch: import torch BEFORE the first call of this function, so that
    both share torch's bundled HIP runtime (two HIP runtimes in one process cannot both open the GPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise DvbtError(f"{_SO} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(the product path has no CPU fallback)")
        L = C.CDLL(_SO)
        L.dvbt_last_error.restype = C.c_char_p
        L.dvbt_version.restype = C.c_char_p
        L.dvbt_rx_create.argtypes = [C.POINTER(RxParams), C.POINTER(C.c_void_p)]
        L.dvbt_rx_segment_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RxReport)]
        L.dvbt_rx_segment_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(RxReport)]
        L.dvbt_rx_segment_enqueue_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dvbt_rx_segment_finish.argtypes = [C.c_void_p, C.POINTER(RxReport)]
        L.dvbt_rx_read_tap.restype = C.c_int64
        L.dvbt_rx_read_tap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.dvbt_rx_tap_device_ptr.restype = C.c_void_p
        L.dvbt_rx_tap_device_ptr.argtypes = [C.c_void_p, C.c_int]
        L.dvbt_rx_stage_ms.restype = C.c_double
        L.dvbt_rx_stage_ms.argtypes = [C.c_void_p, C.c_char_p]
        L.dvbt_rx_enable_timing.argtypes = [C.c_void_p, C.c_int]
        L.dvbt_rx_enable_taps.argtypes = [C.c_void_p, C.c_int]
        L.dvbt_rx_set_cut.argtypes = [C.c_void_p, C.POINTER(RxCut)]
        L.dvbt_rx_destroy.argtypes = [C.c_void_p]
        L.dvbt_rx_lock_periods.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.dvbt_get_dims.argtypes = [C.c_int] * 5 + [C.POINTER(Dims)]
        _lib = L
    return _lib


def _chk(r):
    if r < 0:
        raise DvbtError(f"libdvbt_hip error {r}: {lib().dvbt_last_error().decode()}")
    return r


def device_count():
    return lib().dvbt_device_count()


def get_dims(constellation, code_rate, mode, guard=G1_32, hierarchy=NH):
    d = Dims()
    _chk(lib().dvbt_get_dims(constellation, hierarchy, code_rate, guard, mode, C.byref(d)))
    return d


class Rx:
    """Device-resident DVB-T receive chain (segment API of include/dvbt_hip.h)."""

    _TAP_DTYPE = {TAP_ACQ: np.complex64, TAP_FFT: np.complex64, TAP_EQ: np.complex64, TAP_CP_START: np.int32,
                  TAP_SYMBOL_INDEX: np.int32, TAP_FREQ_OFFSET: np.int32, TAP_SOFT: np.int8, TAP_CSI: np.float32}

    def __init__(self, constellation, code_rate, mode, max_samples, guard=G1_32, hierarchy=NH, snr_db=30.0,
                 viterbi_bsize=768, rs_oracle_compat=0, descramble=1, device=0, viterbi_chunk_bytes=0, taps=False,
                 resample=(0, 0), front_scale=0.0, soft_decision=0, hier_stream=0, launch_graph=0, front_priority=0, viterbi_warm_windows=0, viterbi_verify=0, quality=False):
        self.L = lib()
        self.p = RxParams(constellation, hierarchy, code_rate, guard, mode, 0, 0, snr_db, viterbi_bsize,
                          rs_oracle_compat, descramble, max_samples, device, viterbi_chunk_bytes, resample[0], resample[1], front_scale, soft_decision, hier_stream, launch_graph, front_priority,
                          viterbi_warm_windows, viterbi_verify)
        self.h = C.c_void_p()
        _chk(self.L.dvbt_rx_create(C.byref(self.p), C.byref(self.h)))
        self.dims = get_dims(constellation, code_rate, mode, guard, hierarchy)
        if taps:
            _chk(self.L.dvbt_rx_enable_taps(self.h, int(taps)))          # True / 1: the debug taps; 2: plus the per-lock-period log of the decoder's input
        if quality:
            self.enable_quality()
        self.report = None

    def enable_quality(self, on=True):
        """keep the equalised carriers of the segments that follow, so that quality() can measure their MER (dvbt_rx_enable_quality)"""
        self.L.dvbt_rx_enable_quality.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.dvbt_rx_enable_quality(self.h, int(bool(on))))

    def quality(self):
        """RxQuality of the last finished segment (dvbt_rx_quality): MER, channel and post-Viterbi bit errors, measured on the device"""
        q = RxQuality()
        self.L.dvbt_rx_quality.argtypes = [C.c_void_p, C.POINTER(RxQuality)]
        _chk(self.L.dvbt_rx_quality(self.h, C.byref(q)))
        return q

    def run(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        rep = RxReport()
        _chk(self.L.dvbt_rx_segment_run(self.h, iq.ctypes.data_as(C.c_void_p), len(iq), C.byref(rep)))
        self.report = rep
        return rep

    def set_cut(self, stream_symbol_offset):
        """Declare the following segments as the continuation of a cut stream (include/dvbt_hip.h: dvbt_rx_set_cut)."""
        cut = RxCut(int(stream_symbol_offset), 0, 0)
        _chk(self.L.dvbt_rx_set_cut(self.h, C.byref(cut)))

    def run_device(self, dptr, nsamples, stream=None):
        """dvbt_rx_segment_run_device: synchronous, follows every loss of the CP lock inside the segment"""
        rep = RxReport()
        _chk(self.L.dvbt_rx_segment_run_device(self.h, C.c_void_p(dptr), nsamples, C.c_void_p(stream) if stream else None, C.byref(rep)))
        self.report = rep
        return rep

    def enqueue_device(self, dptr, nsamples, stream=None):
        _chk(self.L.dvbt_rx_segment_enqueue_device(self.h, C.c_void_p(dptr), nsamples,
                                                   C.c_void_p(stream) if stream else None))

    def finish(self):
        rep = RxReport()
        _chk(self.L.dvbt_rx_segment_finish(self.h, C.byref(rep)))
        self.report = rep
        return rep

    def tap(self, tap):
        r = self.report
        d = self.dims
        sizes = {TAP_ACQ: r.n_symbols * d.fft_length * 8, TAP_FFT: r.n_symbols * d.fft_length * 8,
                 TAP_EQ: r.n_out_symbols * d.payload_length * 8, TAP_DEMAP: r.n_out_symbols * d.payload_length,
                 TAP_SYMDEINT: r.n_out_symbols * d.payload_length, TAP_BITDEINT: r.n_out_symbols * d.payload_length,
                 TAP_VITERBI: r.n_viterbi_bytes, TAP_DEINT: r.n_rs_bytes // 188 * 204, TAP_RS: r.n_rs_bytes,
                 TAP_TS: r.n_ts_bytes, TAP_CP_START: r.n_symbols * 4, TAP_SYMBOL_INDEX: max(r.n_symbols - 1, 0) * 4,
                 TAP_FREQ_OFFSET: max(r.n_symbols - 1, 0) * 4, TAP_BITDEINT_LP: r.n_out_symbols * d.payload_length,
                 TAP_SOFT: r.n_out_symbols * d.payload_length * d.m, TAP_CSI: r.n_out_symbols * d.payload_length * 4}
        nbytes = max(int(sizes[tap]), 0)
        buf = np.zeros(nbytes, np.uint8)
        if nbytes:
            n = _chk(self.L.dvbt_rx_read_tap(self.h, tap, buf.ctypes.data_as(C.c_void_p), nbytes))
            buf = buf[:n]
        out = buf.view(self._TAP_DTYPE.get(tap, np.uint8))
        if tap in (TAP_ACQ, TAP_FFT):
            out = out.reshape(-1, d.fft_length)
        elif tap in (TAP_EQ, TAP_DEMAP, TAP_SYMDEINT, TAP_BITDEINT, TAP_BITDEINT_LP, TAP_CSI):
            out = out.reshape(-1, d.payload_length)
        elif tap == TAP_SOFT:
            out = out.reshape(-1, d.payload_length * d.m)
        return out

    def lock_periods(self):
        """[(offset, first_call, cp_start0, n_symbols, first_out_symbol)] of the last run() / run_device()"""
        n = _chk(self.L.dvbt_rx_lock_periods(self.h, None, 0))
        buf = (LockPeriod * max(n, 1))()
        _chk(self.L.dvbt_rx_lock_periods(self.h, buf, n))
        return [(b.offset, b.first_call, b.cp_start0, b.n_symbols, b.first_out_symbol) for b in buf[:n]]

    def walk_stats(self):
        """(passes through the one-launch tracker, passes through the general kernels, calls per chunk of the one-launch tracker, its longest window)"""
        class W(C.Structure):
            _fields_ = [("small_passes", C.c_int64), ("general_passes", C.c_int64), ("small_chunk_calls", C.c_int32), ("small_max_calls", C.c_int32)]
        w = W()
        self.L.dvbt_rx_walk_stats.argtypes = [C.c_void_p, C.POINTER(W)]
        _chk(self.L.dvbt_rx_walk_stats(self.h, C.byref(w)))
        return w.small_passes, w.general_passes, w.small_chunk_calls, w.small_max_calls

    def period_taps(self):
        """taps=2: [(decoder input of the lock period (uint8), offset of its decoded bytes in the VITERBI tap, their count)] for every lock period of the
        last run() / run_device() that reached the Viterbi decoder"""
        class P(C.Structure):
            _fields_ = [("bitdeint_offset", C.c_int64), ("bitdeint_bytes", C.c_int64), ("viterbi_offset", C.c_int64), ("viterbi_bytes", C.c_int64)]
        self.L.dvbt_rx_period_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        n = _chk(self.L.dvbt_rx_period_taps(self.h, None, 0))
        buf = (P * max(n, 1))()
        _chk(self.L.dvbt_rx_period_taps(self.h, buf, n))
        total = max([b.bitdeint_offset + b.bitdeint_bytes for b in buf[:n]] + [0])
        log = np.zeros(total, np.uint8)
        if total:
            _chk(self.L.dvbt_rx_read_tap(self.h, TAP_BITDEINT_LOG, log.ctypes.data_as(C.c_void_p), total))
        return [(log[b.bitdeint_offset:b.bitdeint_offset + b.bitdeint_bytes], int(b.viterbi_offset), int(b.viterbi_bytes)) for b in buf[:n]]

    def viterbi_proof(self):
        """what the proof + repair passes of the last launch of the Viterbi decoder did: dict(chunks, decoded_again, sequential, not_proven) -- not_proven is the
        final check's count (viterbi_verify >= 1), -1 when it did not run"""
        p = ViterbiProof()
        self.L.dvbt_rx_viterbi_proof.argtypes = [C.c_void_p, C.POINTER(ViterbiProof)]
        _chk(self.L.dvbt_rx_viterbi_proof(self.h, C.byref(p)))
        return {"chunks": int(p.chunks), "decoded_again": int(p.decoded_again), "sequential": int(p.sequential), "not_proven": int(p.not_proven)}

    def viterbi_proof_total(self):
        """the passes' counters summed over every launch of the handle's decoder since it was created: dict(chunks, decoded_again, sequential, not_proven = -1)"""
        p = ViterbiProof()
        self.L.dvbt_rx_viterbi_proof_total.argtypes = [C.c_void_p, C.POINTER(ViterbiProof)]
        _chk(self.L.dvbt_rx_viterbi_proof_total(self.h, C.byref(p)))
        return {"chunks": int(p.chunks), "decoded_again": int(p.decoded_again), "sequential": int(p.sequential), "not_proven": int(p.not_proven)}

    def set_viterbi_walk(self, always):
        """always: the Viterbi decoder's traceback chains walk every hop instead of taking the shortcut over chained best states (the same bytes)"""
        self.L.dvbt_rx_set_viterbi_walk.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.dvbt_rx_set_viterbi_walk(self.h, int(bool(always))))

    def viterbi_shortcut(self):
        """(shortcut, walked): blocks of 24 windows, per wavefront, whose bytes left by the traceback's shortcut / whose chains walked, since the handle was created"""
        out = (C.c_longlong * 2)()
        self.L.dvbt_rx_viterbi_shortcut.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        _chk(self.L.dvbt_rx_viterbi_shortcut(self.h, out))
        return int(out[0]), int(out[1])

    def viterbi_check(self):
        """viterbi_verify >= 1: (chunks of the last launch of the Viterbi decoder, chunks NOT proven equal to the streaming decoder when the launch ends)"""
        a, b = C.c_int64(), C.c_int64()
        self.L.dvbt_rx_viterbi_check.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        _chk(self.L.dvbt_rx_viterbi_check(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def tap_device_ptr(self, tap):
        return self.L.dvbt_rx_tap_device_ptr(self.h, tap)

    def enable_timing(self, on=True):
        """True / 1: HIP events around every stage; 2: around the decoder only (stage_ms("viterbi")); False / 0: none"""
        _chk(self.L.dvbt_rx_enable_timing(self.h, int(on)))

    def stage_ms(self, name):
        return self.L.dvbt_rx_stage_ms(self.h, name.encode())

    def close(self):
        if self.h:
            self.L.dvbt_rx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamParams(C.Structure):
    _fields_ = [("rx", RxParams), ("segment_superframes", C.c_int), ("rank", C.c_int), ("world", C.c_int), ("ts_ring_bytes", C.c_int64), ("borrow_device_pushes", C.c_int), ("chains", C.c_int)]


class StreamInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("pieces_in_flight", C.c_int32), ("finished", C.c_int32),
                ("samples_pushed", C.c_int64), ("ts_bytes_decoded", C.c_int64), ("ts_bytes_ready", C.c_int64), ("ts_bytes_pulled", C.c_int64),
                ("first_superframe_call", C.c_int64), ("first_ts_packet", C.c_int64),
                ("constellation", C.c_int32), ("hierarchy", C.c_int32), ("code_rate", C.c_int32), ("auto_configured", C.c_int32), ("samples_released", C.c_int64), ("in_walk", C.c_int32)]


class RxStream:
    """dvbt_rx_stream_*: push samples in calls of any size, pull the TS in order; the bytes are those of one chain over the whole stream."""

    def __init__(self, constellation, code_rate, mode, segment_superframes=0, guard=G1_32, hierarchy=NH, snr_db=30.0, viterbi_bsize=768,
                 rs_oracle_compat=0, device=0, rank=0, world=0, soft_decision=0, ts_ring_bytes=0, borrow=0, viterbi_warm_windows=0, viterbi_verify=0, chains=0):
        self.L = lib()
        for fn in ("create", "push", "push_device", "finish", "status"):
            getattr(self.L, f"dvbt_rx_stream_{fn}").restype = C.c_int
        self.L.dvbt_rx_stream_create.argtypes = [C.POINTER(StreamParams), C.POINTER(C.c_void_p)]
        self.L.dvbt_rx_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.L.dvbt_rx_stream_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.L.dvbt_rx_stream_pull.restype = C.c_int64
        self.L.dvbt_rx_stream_pull.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.L.dvbt_rx_stream_finish.argtypes = [C.c_void_p]
        self.L.dvbt_rx_stream_status.argtypes = [C.c_void_p, C.POINTER(StreamInfo)]
        self.L.dvbt_rx_stream_destroy.argtypes = [C.c_void_p]
        rx = RxParams(constellation, hierarchy, code_rate, guard, mode, 0, 0, snr_db, viterbi_bsize, rs_oracle_compat, 1, 0, device, 0, 0, 0, 0.0, soft_decision)
        rx.viterbi_warm_windows = viterbi_warm_windows
        rx.viterbi_verify = viterbi_verify
        self.p = StreamParams(rx, segment_superframes, rank, world, ts_ring_bytes, borrow, chains)
        self.L.dvbt_rx_stream_pull_chunk.restype = C.c_int64
        self.L.dvbt_rx_stream_pull_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64)]
        self.h = C.c_void_p()
        _chk(self.L.dvbt_rx_stream_create(C.byref(self.p), C.byref(self.h)))
        self._out = np.empty(1 << 22, np.uint8)

    def push(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        _chk(self.L.dvbt_rx_stream_push(self.h, iq.ctypes.data_as(C.c_void_p), len(iq)))

    def push_device(self, dptr, nsamples, stream=None):
        _chk(self.L.dvbt_rx_stream_push_device(self.h, C.c_void_p(dptr), nsamples, C.c_void_p(stream) if stream else None))

    def pull(self, max_bytes=None):
        """the TS bytes that are ready (all of them unless max_bytes is given), as a numpy array"""
        chunks = []
        left = max_bytes
        while left is None or left > 0:
            cap = len(self._out) if left is None else min(len(self._out), left)
            n = _chk(self.L.dvbt_rx_stream_pull(self.h, self._out.ctypes.data_as(C.c_void_p), cap))
            if n <= 0:
                break
            chunks.append(self._out[:n].copy())
            if left is not None:
                left -= n
        return np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)

    def pull_chunks(self):
        """[(first packet index in the stream's TS, uint8 array)] of what is ready: this rank's packets of a sharded stream"""
        out = []
        while True:
            fp = C.c_int64()
            n = _chk(self.L.dvbt_rx_stream_pull_chunk(self.h, self._out.ctypes.data_as(C.c_void_p), len(self._out) // 188 * 188, C.byref(fp)))
            if n <= 0:
                break
            out.append((fp.value, self._out[:n].copy()))
        return out

    def finish(self):
        _chk(self.L.dvbt_rx_stream_finish(self.h))

    def trace(self):
        """dvbt_rx_stream_trace: what the stream did (walk windows, epochs, pieces that left their epoch), as text"""
        self.L.dvbt_rx_stream_trace.restype = C.c_int64
        self.L.dvbt_rx_stream_trace.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        buf = C.create_string_buffer(1 << 17)
        self.L.dvbt_rx_stream_trace(self.h, buf, len(buf))
        return buf.value.decode()

    def viterbi_proof(self):
        """the Viterbi stage's proof + repair passes summed over the stream's launches so far: dict(chunks, decoded_again, sequential, not_proven = -1)"""
        p = ViterbiProof()
        self.L.dvbt_rx_stream_viterbi_proof.argtypes = [C.c_void_p, C.POINTER(ViterbiProof)]
        _chk(self.L.dvbt_rx_stream_viterbi_proof(self.h, C.byref(p)))
        return {"chunks": int(p.chunks), "decoded_again": int(p.decoded_again), "sequential": int(p.sequential), "not_proven": int(p.not_proven)}

    def info(self):
        i = StreamInfo()
        _chk(self.L.dvbt_rx_stream_status(self.h, C.byref(i)))
        return i

    def close(self):
        if self.h:
            self.L.dvbt_rx_stream_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _typed_once(set_types):
    """set_types(L) declares a block's argtypes; the decorated name returns the library with them declared, once per load"""
    mark = "_typed" + set_types.__name__

    def get():
        L = lib()
        if not getattr(L, mark, False):
            set_types(L)
            setattr(L, mark, True)
        return L
    return get


class _Handle:
    """What the streaming handles share: the library self.L, the handle self.h (both set by the subclass's __init__) and the C prefix of its entries."""
    _prefix = None

    def _fn(self, name):
        return getattr(self.L, f"{self._prefix}_{name}")

    def reset(self):
        _chk(self._fn("reset")(self.h))

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SampleBlock(_Handle):
    """a handle whose call takes n complex64 and returns n"""

    def run(self, iq):
        """complex64 samples in, as many out; continues the stream"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        out = np.empty_like(iq)
        _chk(self._fn("run")(self.h, iq.ctypes.data_as(C.c_void_p), len(iq), out.ctypes.data_as(C.c_void_p)))
        return out

    def run_device(self, in_ptr, nsamples, out_ptr, stream=None):
        """device pointers (ints) to nsamples complex64 each, not overlapping: enqueues on `stream` (a hipStream_t as int, None: the default stream)"""
        _chk(self._fn("run_device")(self.h, C.c_void_p(in_ptr), nsamples, C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))


TX_SCALE = 0.0022097087      # multiply_const behind the cyclic prefixer in apps/dvbt_tx_demo*.grc


class TxParams(C.Structure):
    _fields_ = [("constellation", C.c_int), ("hierarchy", C.c_int), ("code_rate", C.c_int), ("guard_interval", C.c_int),
                ("transmission_mode", C.c_int), ("include_cell_id", C.c_int), ("cell_id", C.c_int), ("scale", C.c_float),
                ("max_packets", C.c_size_t), ("first_packet", C.c_int64), ("keep_carriers", C.c_int), ("device", C.c_int)]


@_typed_once
def _tx_lib(L):
    L.dvbt_tx_create.argtypes = [C.POINTER(TxParams), C.POINTER(C.c_void_p)]
    L.dvbt_tx_samples_for.restype = C.c_int64
    L.dvbt_tx_samples_for.argtypes = [C.c_void_p, C.c_size_t]
    L.dvbt_tx_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dvbt_tx_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
    L.dvbt_tx_read_carriers.restype = C.c_int64
    L.dvbt_tx_read_carriers.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_tx_reset.argtypes = [C.c_void_p]
    L.dvbt_tx_destroy.argtypes = [C.c_void_p]


class Tx(_Handle):
    """dvbt_tx_*: the modulator of apps/dvbt_tx_demo*.grc on the GPU.  One transport stream, delivered over any number of run() /
    run_device() calls of any number of 188-byte packets; the concatenated outputs are those of one run over the whole stream."""
    _prefix = "dvbt_tx"

    def __init__(self, constellation, code_rate, mode, guard=G1_32, hierarchy=NH, include_cell_id=0, cell_id=0, scale=TX_SCALE,
                 max_packets=1 << 16, first_packet=0, keep_carriers=False, device=0):
        self.L = _tx_lib()
        self.p = TxParams(constellation, hierarchy, code_rate, guard, mode, include_cell_id, cell_id, scale, max_packets, first_packet,
                          int(bool(keep_carriers)), device)
        self.h = C.c_void_p()
        _chk(self.L.dvbt_tx_create(C.byref(self.p), C.byref(self.h)))
        self.dims = get_dims(constellation, code_rate, mode, guard, hierarchy)

    def samples_for(self, npackets):
        """samples the NEXT call with npackets packets will produce"""
        return _chk(self.L.dvbt_tx_samples_for(self.h, npackets))

    def run(self, ts):
        """TS bytes (a whole number of 188-byte packets) -> complex64 baseband of the whole OFDM symbols they complete"""
        ts = np.ascontiguousarray(np.frombuffer(ts, np.uint8) if isinstance(ts, (bytes, bytearray)) else ts, dtype=np.uint8).reshape(-1)
        if len(ts) % 188:
            raise ValueError("the TS must be a whole number of 188-byte packets")
        npk = len(ts) // 188
        out = np.zeros(max(self.samples_for(npk), 0), np.complex64)
        n = C.c_size_t()
        _chk(self.L.dvbt_tx_run(self.h, ts.ctypes.data_as(C.c_void_p), npk, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
        return out[:n.value]

    def run_device(self, ts_ptr, npackets, out_ptr, cap, stream=None):
        """device pointers (ints): enqueues on `stream` (a hipStream_t as int, None: the default stream) and returns the sample count at once"""
        n = C.c_size_t()
        _chk(self.L.dvbt_tx_run_device(self.h, C.c_void_p(ts_ptr), npackets, C.c_void_p(out_ptr), cap, C.c_void_p(stream) if stream else None,
                                       C.byref(n)))
        return n.value

    def carriers(self):
        """keep_carriers: the last call's IFFT input, complex64[nsym, N] (carrier c at column zeros_on_left + c)"""
        nbytes = _chk(self.L.dvbt_tx_read_carriers(self.h, None, 0))
        out = np.zeros(nbytes // 8, np.complex64)
        if nbytes:
            _chk(self.L.dvbt_tx_read_carriers(self.h, out.ctypes.data_as(C.c_void_p), nbytes))
        return out.reshape(-1, self.dims.fft_length)


CHANNEL_MAX_PATHS, CHANNEL_MAX_DELAY = 8, 8192


class ChannelParams(C.Structure):
    _fields_ = [("n_paths", C.c_int), ("delay", C.c_int * 8), ("amp_re", C.c_float * 8), ("amp_im", C.c_float * 8), ("cfo", C.c_double),
                ("fft_length", C.c_int), ("noise_sigma", C.c_float), ("seed", C.c_uint64), ("first_sample", C.c_int64), ("device", C.c_int)]


@_typed_once
def _channel_lib(L):
    L.dvbt_channel_create.argtypes = [C.POINTER(ChannelParams), C.POINTER(C.c_void_p)]
    L.dvbt_channel_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_channel_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.dvbt_channel_power.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_double)]
    L.dvbt_channel_reset.argtypes = [C.c_void_p]
    L.dvbt_channel_destroy.argtypes = [C.c_void_p]


class Channel(_SampleBlock):
    """dvbt_channel_*: static echoes, a carrier offset and seeded AWGN on complex64 baseband, on the GPU.  echoes: ((delay in samples, complex amplitude), ...)
    of the extra paths; cfo in subcarrier spacings of an fft_length-point symbol; noise_sigma per component (Channel.sigma for an SNR).  One stream, delivered
    over any number of run() / run_device() calls of any size; the concatenated outputs are bit for bit those of one call.  The noise of a sample depends on
    (seed, first_sample + its index) alone."""
    _prefix = "dvbt_channel"

    def __init__(self, echoes=(), cfo=0.0, fft_length=0, noise_sigma=0.0, seed=0, first_sample=0, device=0):
        self.L = _channel_lib()
        echoes = tuple(echoes)
        if len(echoes) > CHANNEL_MAX_PATHS:
            raise ValueError(f"at most {CHANNEL_MAX_PATHS} echoes")
        p = ChannelParams()
        p.n_paths = len(echoes)
        for i, (d, a) in enumerate(echoes):
            p.delay[i], p.amp_re[i], p.amp_im[i] = int(d), float(np.real(a)), float(np.imag(a))
        p.cfo, p.fft_length, p.noise_sigma = float(cfo), int(fft_length), float(noise_sigma)
        p.seed, p.first_sample, p.device = int(seed) & 0xffffffffffffffff, int(first_sample), int(device)
        self.p = p
        self.h = C.c_void_p()
        _chk(self.L.dvbt_channel_create(C.byref(p), C.byref(self.h)))

    @staticmethod
    def sigma(snr_db, ref_power):
        """the noise's standard deviation per component for an SNR of snr_db relative to ref_power (power())"""
        return float(np.sqrt(ref_power / 10.0 ** (snr_db / 10.0) / 2.0))

    def power(self, ptr, nsamples, stream=None):
        """mean |x|^2 of nsamples complex64 at the device pointer `ptr`: the ref_power of sigma().  Synchronises `stream`."""
        v = C.c_double()
        _chk(self.L.dvbt_channel_power(self.h, C.c_void_p(ptr), nsamples, C.c_void_p(stream) if stream else None, C.byref(v)))
        return v.value


class ClockParams(C.Structure):
    _fields_ = [("ppm", C.c_double), ("start", C.c_double), ("taps", C.c_int), ("first_out", C.c_int64), ("first_in", C.c_int64), ("device", C.c_int)]


@_typed_once
def _clock_lib(L):
    L.dvbt_clock_outputs.argtypes = [C.POINTER(ClockParams), C.c_int64, C.POINTER(C.c_int64)]
    L.dvbt_clock_create.argtypes = [C.POINTER(ClockParams), C.POINTER(C.c_void_p)]
    L.dvbt_clock_outputs_for.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dvbt_clock_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dvbt_clock_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.dvbt_clock_reset.argtypes = [C.c_void_p]
    L.dvbt_clock_destroy.argtypes = [C.c_void_p]


def clock_outputs(params, n_in_total):
    """dvbt_clock_outputs: the outputs a stream with these ClockParams has emitted once n_in_total inputs have been pushed (host arithmetic, needs no GPU)"""
    n = C.c_int64()
    _chk(_clock_lib().dvbt_clock_outputs(C.byref(params), int(n_in_total), C.byref(n)))
    return n.value


class ClockOffset(_Handle):
    """dvbt_clock_*: complex64 baseband as a receiver whose sample clock is off by `ppm` sees it, y[m] = x(start + m (1 + ppm 1e-6)) by windowed-sinc
    interpolation over `taps` samples, on the GPU.  start=None: taps // 2, the alignment of the test oracle's resampler.  One stream, delivered over any
    number of run() / run_device() calls of any size; the concatenated outputs are bit for bit those of one call.  first_out / first_in: the absolute numbers of
    the stream's first output and input (a piece of a cut stream)."""
    _prefix = "dvbt_clock"

    def __init__(self, ppm, start=None, taps=16, first_out=0, first_in=0, device=0):
        self.L = _clock_lib()
        self.p = ClockParams(float(ppm), float(taps // 2 if start is None else start), int(taps), int(first_out), int(first_in), int(device))
        self.h = C.c_void_p()
        _chk(self.L.dvbt_clock_create(C.byref(self.p), C.byref(self.h)))

    def outputs_for(self, n_in):
        """samples the NEXT call with n_in input samples will emit"""
        n = C.c_size_t()
        _chk(self.L.dvbt_clock_outputs_for(self.h, n_in, C.byref(n)))
        return n.value

    def run(self, iq):
        """complex64 samples in, the outputs they complete out; continues the stream"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        out = np.empty(self.outputs_for(len(iq)), np.complex64)
        n = C.c_size_t()
        _chk(self.L.dvbt_clock_run(self.h, iq.ctypes.data_as(C.c_void_p), len(iq), out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
        return out[:n.value]

    def run_device(self, in_ptr, n_in, out_ptr, out_cap, stream=None):
        """device pointers (ints), not overlapping: enqueues on `stream` (a hipStream_t as int, None: the default stream) and returns the output count at once"""
        n = C.c_size_t()
        _chk(self.L.dvbt_clock_run_device(self.h, C.c_void_p(in_ptr), n_in, C.c_void_p(out_ptr), out_cap, C.byref(n), C.c_void_p(stream) if stream else None))
        return n.value


IQ_CF32, IQ_CS16, IQ_CS8, IQ_CU8 = range(4)
IQ_DTYPES = (np.dtype(np.complex64), np.dtype(np.int16), np.dtype(np.int8), np.dtype(np.uint8))
IQ_BYTES = (8, 4, 2, 2)                                     # per sample
IQ_SCALES = (1.0, 1.0 / 32768, 1.0 / 128, 1.0 / 127.5)      # full scale -> 1
TUNER_PASS_EDGE, TUNER_STOP_EDGE, TUNER_ATTEN_DB = 0.42, 0.58, 70.0


class TunerParams(C.Structure):
    _fields_ = [("format", C.c_int), ("interpolation", C.c_int), ("decimation", C.c_int), ("swap_iq", C.c_int), ("shift", C.c_double), ("scale", C.c_float),
                ("pass_edge", C.c_double), ("stop_edge", C.c_double), ("atten_db", C.c_double), ("first_in", C.c_int64), ("device", C.c_int)]

    @classmethod
    def of(cls, format, interpolation, decimation, shift=0.0, scale=None, pass_edge=0, stop_edge=0, atten_db=0, swap_iq=False, first_in=0, device=0):
        """the struct with the Python layer's defaults filled in: scale None is the format's full scale, an edge or attenuation of 0 the default"""
        if format not in (IQ_CF32, IQ_CS16, IQ_CS8, IQ_CU8):
            raise ValueError("format must be IQ_CF32, IQ_CS16, IQ_CS8 or IQ_CU8")
        return cls(int(format), int(interpolation), int(decimation), int(bool(swap_iq)), float(shift), float(IQ_SCALES[format] if scale is None else scale),
                   float(pass_edge or TUNER_PASS_EDGE), float(stop_edge or TUNER_STOP_EDGE), float(atten_db or TUNER_ATTEN_DB), int(first_in), int(device))


class TunerDesc(C.Structure):
    _fields_ = [("interpolation", C.c_int), ("decimation", C.c_int), ("ntaps", C.c_int), ("nt", C.c_int), ("delay_num", C.c_int64), ("delay_den", C.c_int64),
                ("phase_inc", C.c_uint64)]


@_typed_once
def _tuner_lib(L):
    L.dvbt_tuner_design.argtypes = [C.POINTER(TunerParams), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.dvbt_tuner_outputs.argtypes = [C.POINTER(TunerParams), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    L.dvbt_tuner_create.argtypes = [C.POINTER(TunerParams), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.dvbt_tuner_get_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.dvbt_tuner_info.argtypes = [C.c_void_p, C.POINTER(TunerDesc)]
    L.dvbt_tuner_outputs_for.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dvbt_tuner_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dvbt_tuner_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.dvbt_tuner_reset.argtypes = [C.c_void_p]
    L.dvbt_tuner_destroy.argtypes = [C.c_void_p]
    L.dvbt_device_malloc.restype = C.c_void_p
    L.dvbt_device_malloc.argtypes = [C.c_size_t]
    L.dvbt_device_free.argtypes = [C.c_void_p]
    L.dvbt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_synchronize.argtypes = [C.c_void_p]


def tuner_outputs(params, n_in_total, ntaps=0):
    """dvbt_tuner_outputs: the outputs a stream with these TunerParams has emitted once n_in_total inputs have been pushed; ntaps is the length of the
    caller's prototype, 0 for the designed one (host arithmetic, needs no GPU)"""
    n = C.c_int64()
    _chk(_tuner_lib().dvbt_tuner_outputs(C.byref(params), int(ntaps), int(n_in_total), C.byref(n)))
    return n.value


def tuner_design(params):
    """dvbt_tuner_design: the prototype the library designs for these TunerParams, as float32 (host arithmetic, needs no GPU)"""
    L = _tuner_lib()
    n = C.c_int()
    _chk(L.dvbt_tuner_design(C.byref(params), None, 0, C.byref(n)))
    taps = np.empty(n.value, np.float32)
    _chk(L.dvbt_tuner_design(C.byref(params), taps.ctypes.data_as(C.c_void_p), len(taps), C.byref(n)))
    return taps


class Tuner(_Handle):
    """dvbt_tuner_*: raw interleaved I/Q as an SDR records it (`format`: IQ_CF32, IQ_CS16, IQ_CS8, IQ_CU8) to complex64 baseband at interpolation /
    decimation times the capture's rate, on the GPU: conversion with `scale` (None: full scale -> 1), a mixer of `shift` cycles per input sample, a polyphase
    low-pass with the caller's `taps` or one designed from pass_edge / stop_edge (fractions of the output rate; 0: 0.42 / 0.58) and atten_db (0: 70).  One
    stream, delivered over any number of run() / run_device() calls of any size; the concatenated outputs are bit for bit those of one call."""
    _prefix = "dvbt_tuner"

    def __init__(self, format, interpolation, decimation, shift=0.0, scale=None, taps=None, pass_edge=0, stop_edge=0, atten_db=0, swap_iq=False, first_in=0,
                 device=0):
        self.L = _tuner_lib()
        self.h = C.c_void_p()
        self._bufs = [0, 0, 0, 0]                  # feed(): input pointer, its bytes, output pointer, its samples
        self.p = TunerParams.of(format, interpolation, decimation, shift, scale, pass_edge, stop_edge, atten_db, swap_iq, first_in, device)
        self.format = int(format)
        if taps is not None:
            taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
            _chk(self.L.dvbt_tuner_create(C.byref(self.p), taps.ctypes.data_as(C.c_void_p), len(taps), C.byref(self.h)))
        else:
            _chk(self.L.dvbt_tuner_create(C.byref(self.p), None, 0, C.byref(self.h)))
        self.desc = TunerDesc()
        _chk(self.L.dvbt_tuner_info(self.h, C.byref(self.desc)))

    @classmethod
    def for_capture(cls, sample_rate, format, channel_mhz=8, offset_hz=0.0, **kw):
        """the tuner of a capture at sample_rate (Hz) whose DVB-T channel of channel_mhz lies offset_hz above the capture's centre: the ratio is exactly
        (64/7 MHz * channel_mhz / 8) / sample_rate, the shift -offset_hz / sample_rate.  A ratio outside the block's limits raises."""
        from fractions import Fraction
        ratio = Fraction(64_000_000 * channel_mhz, 56) / Fraction(sample_rate)
        if ratio.numerator > 128 or ratio.denominator > 1024 or ratio.denominator > 8 * ratio.numerator:
            raise ValueError(f"the ratio {ratio} of a {sample_rate} Hz capture is outside the tuner's limits (L <= 128, M <= 1024, M / L <= 8)")
        return cls(format, ratio.numerator, ratio.denominator, shift=-float(offset_hz) / float(sample_rate), **kw)

    @property
    def taps(self):
        """the prototype in use, float32"""
        t = np.empty(self.desc.ntaps, np.float32)
        n = C.c_int()
        _chk(self.L.dvbt_tuner_get_taps(self.h, t.ctypes.data_as(C.c_void_p), len(t), C.byref(n)))
        return t

    @property
    def delay(self):
        """the group delay in output samples"""
        from fractions import Fraction
        return Fraction(self.desc.delay_num, self.desc.delay_den)

    def outputs_for(self, n_in):
        """samples the NEXT call with n_in input samples will emit"""
        n = C.c_size_t()
        _chk(self.L.dvbt_tuner_outputs_for(self.h, n_in, C.byref(n)))
        return n.value

    def _raw(self, raw):
        """the caller's samples as one contiguous array of the format's dtype and their count; flat and interleaved, or shaped (n, 2)"""
        raw = np.asarray(raw)
        want = IQ_DTYPES[self.format]
        if raw.dtype != want:
            raise ValueError(f"this tuner takes {want} samples, not {raw.dtype}")
        raw = np.ascontiguousarray(raw).reshape(-1)
        if self.format != IQ_CF32 and len(raw) % 2:
            raise ValueError("interleaved I/Q has an even number of components")
        return raw, (len(raw) if self.format == IQ_CF32 else len(raw) // 2)

    def run(self, raw):
        """raw samples in (complex64, or int16 / int8 / uint8 interleaved or shaped (n, 2)), the complex64 outputs they complete out; continues the stream"""
        raw, n_in = self._raw(raw)
        out = np.empty(self.outputs_for(n_in), np.complex64)
        n = C.c_size_t()
        _chk(self.L.dvbt_tuner_run(self.h, raw.ctypes.data_as(C.c_void_p), n_in, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
        return out[:n.value]

    def run_device(self, in_ptr, n_in, out_ptr, out_cap, stream=None):
        """device pointers (ints), not overlapping: enqueues on `stream` (a hipStream_t as int, None: the default stream) and returns the output count at once"""
        n = C.c_size_t()
        _chk(self.L.dvbt_tuner_run_device(self.h, C.c_void_p(in_ptr), n_in, C.c_void_p(out_ptr), out_cap, C.byref(n), C.c_void_p(stream) if stream else None))
        return n.value

    def feed(self, stream, raw):
        """raw samples through the tuner on the device and on into an RxStream (push_device); returns the number of samples pushed.  Correct rather than
        fast: the stream object copies the samples on its own HIP stream, so this waits for the device before the next call reuses the buffers
        (INTEGRATION.md 3j has the fast path)."""
        raw, n_in = self._raw(raw)
        n_out = self.outputs_for(n_in)
        b = self._bufs
        if raw.nbytes > b[1]:
            self.L.dvbt_device_free(C.c_void_p(b[0]))
            b[0], b[1] = self.L.dvbt_device_malloc(raw.nbytes), raw.nbytes
        if n_out > b[3]:
            self.L.dvbt_device_free(C.c_void_p(b[2]))
            b[2], b[3] = self.L.dvbt_device_malloc(8 * n_out), n_out
        if n_in and not b[0] or n_out and not b[2]:
            raise DvbtError("device allocation failed")
        if n_in:
            _chk(self.L.dvbt_copy_to_device(C.c_void_p(b[0]), raw.ctypes.data_as(C.c_void_p), raw.nbytes))
        got = self.run_device(b[0], n_in, b[2], b[3])
        _chk(self.L.dvbt_synchronize(None))
        if got:
            stream.push_device(b[2], got)
            _chk(self.L.dvbt_synchronize(None))
        return got

    def close(self):
        if self.h:
            for i in (0, 2):
                if self._bufs[i]:
                    self.L.dvbt_device_free(C.c_void_p(self._bufs[i]))
            self._bufs = [0, 0, 0, 0]
        super().close()


FADING_MAX_PATHS, FADING_MAX_DELAY, FADING_MAX_SINUSOIDS, FADING_KNOT = 24, 8192, 32, 64
TU6_DELAYS_US = (0.0, 0.2, 0.5, 1.6, 2.3, 5.0)          # COST 207 TU6
TU6_POWERS_DB = (-3.0, 0.0, -2.0, -6.0, -8.0, -10.0)


class FadingParams(C.Structure):
    _fields_ = [("n_paths", C.c_int), ("delay", C.c_int * 24), ("los_re", C.c_float * 24), ("los_im", C.c_float * 24), ("sigma", C.c_float * 24),
                ("doppler", C.c_double), ("n_sinusoids", C.c_int), ("seed", C.c_uint64), ("first_sample", C.c_int64), ("device", C.c_int)]

    @classmethod
    def of(cls, paths, doppler=0.0, n_sinusoids=16, seed=0, first_sample=0, device=0):
        """paths: ((delay in samples, fixed part (complex), sigma of the scattered part), ...)"""
        paths = tuple(paths)
        if len(paths) > FADING_MAX_PATHS:
            raise ValueError(f"at most {FADING_MAX_PATHS} paths")
        p = cls()
        p.n_paths = len(paths)
        for i, (d, los, sg) in enumerate(paths):
            p.delay[i], p.los_re[i], p.los_im[i], p.sigma[i] = int(d), float(np.real(los)), float(np.imag(los)), float(sg)
        p.doppler, p.n_sinusoids = float(doppler), int(n_sinusoids)
        p.seed, p.first_sample, p.device = int(seed) & 0xffffffffffffffff, int(first_sample), int(device)
        return p


@_typed_once
def _fading_lib(L):
    L.dvbt_fading_table.argtypes = [C.POINTER(FadingParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.dvbt_fading_create.argtypes = [C.POINTER(FadingParams), C.POINTER(C.c_void_p)]
    L.dvbt_fading_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_fading_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.dvbt_fading_reset.argtypes = [C.c_void_p]
    L.dvbt_fading_destroy.argtypes = [C.c_void_p]


def fading_table(params):
    """dvbt_fading_table: (inc, phase) of these FadingParams, two uint64 arrays [n_paths][M] (host arithmetic, needs no GPU)"""
    np_, M = max(int(params.n_paths), 0), int(params.n_sinusoids) or 16
    n = max(np_ * M, 1) if 0 <= M <= FADING_MAX_SINUSOIDS and np_ <= FADING_MAX_PATHS else 1      # a bad struct is refused before anything is written
    inc, ph = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    _chk(_fading_lib().dvbt_fading_table(C.byref(params), inc.ctypes.data_as(C.POINTER(C.c_uint64)), ph.ctypes.data_as(C.POINTER(C.c_uint64))))
    return inc.reshape(np_, M), ph.reshape(np_, M)


def tu6_paths(doppler_hz, sample_rate=64e6 / 7, rice_k_db=None):
    """COST 207 TU6 as (paths, doppler in cycles per sample): delays rounded to samples, powers normalised to a total of 1.  With rice_k_db (K in dB) the
    scatter is scaled by 1 / (1 + K) in power and a fixed part sqrt(K / (1 + K)) stands on path 0."""
    pw = [10.0 ** (d / 10.0) for d in TU6_POWERS_DB]
    tot = sum(pw)
    K = None if rice_k_db is None else 10.0 ** (rice_k_db / 10.0)
    scat = 1.0 if K is None else 1.0 / (1.0 + K)
    paths = []
    for i, (us, w) in enumerate(zip(TU6_DELAYS_US, pw)):
        los = float(np.sqrt(K / (1.0 + K))) if (K is not None and i == 0) else 0.0
        paths.append((int(round(us * 1e-6 * sample_rate)), complex(los), float(np.sqrt(w / tot * scat))))
    return tuple(paths), float(doppler_hz) / float(sample_rate)


class Fading(_SampleBlock):
    """dvbt_fading_*: time-varying multipath on complex64 baseband, on the GPU.  paths: ((delay in samples, fixed part, sigma), ...): every path's gain is
    its fixed part plus a sum of n_sinusoids sinusoids of rms sigma whose frequencies follow Clarke's spectrum up to `doppler` cycles per sample.  One stream,
    delivered over any number of run() / run_device() calls of any size; the concatenated outputs are bit for bit those of one call.  The gain of a sample
    depends on (paths, doppler, n_sinusoids, seed, first_sample + its index) alone.  No noise, no carrier offset: put a Channel behind it."""
    _prefix = "dvbt_fading"

    def __init__(self, paths=((0, 1.0, 0.0),), doppler=0.0, n_sinusoids=16, seed=0, first_sample=0, device=0):
        self.L = _fading_lib()
        self.p = FadingParams.of(paths, doppler, n_sinusoids, seed, first_sample, device)
        self.h = C.c_void_p()
        _chk(self.L.dvbt_fading_create(C.byref(self.p), C.byref(self.h)))

    @classmethod
    def tu6(cls, doppler_hz, sample_rate=64e6 / 7, rice_k_db=None, **kw):
        """COST 207 TU6 at a largest Doppler shift of doppler_hz; rice_k_db: a Ricean first path (tu6_paths); kw: n_sinusoids, seed, first_sample, device"""
        paths, doppler = tu6_paths(doppler_hz, sample_rate, rice_k_db)
        return cls(paths, doppler, **kw)


RF_MAX_TONES, RF_MAX_MASK_POINTS = 32, 8


class RfParams(C.Structure):
    _fields_ = [("sat_amplitude", C.c_float), ("smoothness", C.c_float), ("n_tones", C.c_int), ("tone_inc", C.c_uint64 * 32),
                ("tone_phase", C.c_uint64 * 32), ("tone_amp", C.c_float * 32), ("mu_re", C.c_float), ("mu_im", C.c_float), ("nu_re", C.c_float),
                ("nu_im", C.c_float), ("dc_re", C.c_float), ("dc_im", C.c_float), ("first_sample", C.c_int64), ("device", C.c_int)]

    @classmethod
    def of(cls, sat_amplitude=0.0, smoothness=2.0, tones=None, mu=1, nu=0, dc=0, first_sample=0, device=0):
        """tones: (inc, phase, amp), three sequences of equal length (phase_noise_tones, or a measured spur list), or None"""
        p = cls()
        p.sat_amplitude, p.smoothness = float(sat_amplitude), float(smoothness)
        if tones is not None:
            inc, ph, amp = tones
            if not len(inc) == len(ph) == len(amp):
                raise ValueError("tones: three sequences of equal length")
            if len(inc) > RF_MAX_TONES:
                raise ValueError(f"at most {RF_MAX_TONES} tones")
            p.n_tones = len(inc)
            for m in range(len(inc)):
                p.tone_inc[m], p.tone_phase[m], p.tone_amp[m] = int(inc[m]) & 0xffffffffffffffff, int(ph[m]) & 0xffffffffffffffff, float(amp[m])
        p.mu_re, p.mu_im, p.nu_re, p.nu_im = float(np.real(mu)), float(np.imag(mu)), float(np.real(nu)), float(np.imag(nu))
        p.dc_re, p.dc_im = float(np.real(dc)), float(np.imag(dc))
        p.first_sample, p.device = int(first_sample), int(device)
        return p


class RfMask(C.Structure):
    _fields_ = [("n_points", C.c_int), ("offset_hz", C.c_double * 8), ("dbc_hz", C.c_double * 8), ("sample_rate", C.c_double)]


@_typed_once
def _rf_lib(L):
    L.dvbt_rf_phase_noise_tones.argtypes = [C.POINTER(RfMask), C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    L.dvbt_rf_create.argtypes = [C.POINTER(RfParams), C.POINTER(C.c_void_p)]
    L.dvbt_rf_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_rf_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.dvbt_rf_reset.argtypes = [C.c_void_p]
    L.dvbt_rf_destroy.argtypes = [C.c_void_p]


def phase_noise_tones(points, n_tones=32, seed=0, sample_rate=64e6 / 7):
    """dvbt_rf_phase_noise_tones: the tone table (inc, phase: uint64 arrays; amp: float32 radians) of a phase-noise mask ((offset in Hz, level in dBc/Hz),
    ...), 2 to 8 points, linear in dB over log f between them: n_tones tones, one drawn per n_tones-th of the log axis, whose powers add up to the mask's
    integral whatever n_tones is.  Host arithmetic, needs no GPU.  The result is RfFrontend's `tones`."""
    points = tuple(points)
    if len(points) > RF_MAX_MASK_POINTS:
        raise ValueError(f"at most {RF_MAX_MASK_POINTS} mask points")
    mk = RfMask()
    mk.n_points, mk.sample_rate = len(points), float(sample_rate)
    for k, (f, d) in enumerate(points):
        mk.offset_hz[k], mk.dbc_hz[k] = float(f), float(d)
    n = min(max(int(n_tones), 1), RF_MAX_TONES)                    # a bad count is refused before anything is written
    inc, ph, amp = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.float32)
    _chk(_rf_lib().dvbt_rf_phase_noise_tones(C.byref(mk), int(n_tones), int(seed) & 0xffffffffffffffff, inc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             ph.ctypes.data_as(C.POINTER(C.c_uint64)), amp.ctypes.data_as(C.POINTER(C.c_float))))
    return inc, ph, amp


class RfFrontend(_SampleBlock):
    """dvbt_rf_*: what the radio hardware does to complex64 baseband, on the GPU, in this order: the transmitter's amplifier (Rapp AM/AM with saturation
    amplitude sat_amplitude and smoothness p; 0: off), oscillator phase noise as a sum of `tones` (phase_noise_tones; None: off), the tuner's IQ imbalance
    v = mu r + nu conj(r) (iq_imbalance) and its DC offset.  One stream, delivered over any number of run() / run_device() calls of any size; the
    concatenated outputs are bit for bit those of one call.  A sample's output depends on (the parameters, first_sample + its index, the sample) alone."""
    _prefix = "dvbt_rf"

    def __init__(self, sat_amplitude=0.0, smoothness=2.0, tones=None, mu=1, nu=0, dc=0, first_sample=0, device=0):
        self.L = _rf_lib()
        self.p = RfParams.of(sat_amplitude, smoothness, tones, mu, nu, dc, first_sample, device)
        self.h = C.c_void_p()
        _chk(self.L.dvbt_rf_create(C.byref(self.p), C.byref(self.h)))

    @staticmethod
    def saturation(ibo_db, ref_power):
        """the sat_amplitude of an input back-off of ibo_db relative to the mean power ref_power (Channel.power)"""
        return float(np.sqrt(ref_power * 10.0 ** (ibo_db / 10.0)))

    @staticmethod
    def iq_imbalance(gain_db, phase_deg):
        """(mu, nu) of a tuner whose arms differ by gain_db in gain and phase_deg in phase: image rejection |mu|^2 / |nu|^2"""
        g, psi = 10.0 ** (gain_db / 20.0), np.deg2rad(phase_deg)
        return complex((1.0 + g * np.exp(-1j * psi)) / 2.0), complex((1.0 - g * np.exp(1j * psi)) / 2.0)

    def run_device(self, in_ptr, nsamples, out_ptr, stream=None):
        """device pointers (ints) to nsamples complex64 each, the same buffer (in place) or not overlapping: enqueues on `stream` (a hipStream_t as int,
        None: the default stream)"""
        super().run_device(in_ptr, nsamples, out_ptr, stream)


SPECTRUM_HIST_BINS = 2048
SPECTRUM_WINDOWS = {"rect": 0, "rectangular": 0, "hann": 1, "blackman-harris": 2, "blackmanharris": 2}


class SpectrumParams(C.Structure):
    _fields_ = [("device", C.c_int), ("fft_size", C.c_int), ("hop", C.c_int), ("window", C.c_int)]


class SpectrumResult(C.Structure):
    _fields_ = [("segments", C.c_longlong), ("samples_pushed", C.c_longlong), ("samples_counted", C.c_longlong), ("nonfinite", C.c_longlong),
                ("sum_power", C.c_double), ("peak_power", C.c_float)]


@_typed_once
def _spectrum_lib(L):
    L.dvbt_spectrum_create.argtypes = [C.POINTER(SpectrumParams), C.POINTER(C.c_void_p)]
    L.dvbt_spectrum_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_spectrum_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_spectrum_read.argtypes = [C.c_void_p, C.POINTER(SpectrumResult), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]
    L.dvbt_spectrum_reset.argtypes = [C.c_void_p]
    L.dvbt_spectrum_destroy.argtypes = [C.c_void_p]


def spectrum_window(fft_size, window):
    """the float32 table of window 0 (rectangular), 1 (Hann) or 2 (4-term Blackman-Harris): periodic, computed in double"""
    t = 2.0 * np.pi * np.arange(fft_size, dtype=np.float64) / fft_size
    if window == 0:
        w = np.ones(fft_size)
    elif window == 1:
        w = 0.5 - 0.5 * np.cos(t)
    elif window == 2:
        w = 0.35875 - 0.48829 * np.cos(t) + 0.14128 * np.cos(2.0 * t) - 0.01168 * np.cos(3.0 * t)
    else:
        raise ValueError("window must be 0, 1 or 2")
    return w.astype(np.float32)


class SpectrumReading:
    """What Spectrum.read() returns: `psd` (fft_size doubles, fft-shifted, power per bin), `hist` (2048 uint64 counts of |x|^2 by float_bits >> 20) and the
    fields of dvbt_spectrum_result.  The helpers are numpy in double on the host and need no GPU; frequencies are in Hz for `sample_rate`."""

    def __init__(self, psd, hist, segments, samples_pushed, samples_counted, nonfinite, sum_power, peak_power, fft_size, hop, window, sample_rate=64e6 / 7):
        self.psd = np.asarray(psd, dtype=np.float64)
        self.hist = np.asarray(hist, dtype=np.uint64)
        self.segments, self.samples_pushed, self.samples_counted, self.nonfinite = int(segments), int(samples_pushed), int(samples_counted), int(nonfinite)
        self.sum_power, self.peak_power = float(sum_power), np.float32(peak_power)
        self.fft_size, self.hop, self.window, self.sample_rate = int(fft_size), int(hop), int(window), float(sample_rate)
        assert self.psd.shape == (self.fft_size,) and self.hist.shape == (SPECTRUM_HIST_BINS,)

    def freqs(self, sample_rate=None):
        fs = self.sample_rate if sample_rate is None else float(sample_rate)
        return (np.arange(self.fft_size, dtype=np.float64) - self.fft_size // 2) * (fs / self.fft_size)

    @property
    def mean_power(self):
        return self.sum_power / self.samples_counted if self.samples_counted else 0.0

    @property
    def enbw(self):
        """equivalent noise bandwidth of the window in bins: an on-bin tone of amplitude A reads A^2 / enbw"""
        w = spectrum_window(self.fft_size, self.window).astype(np.float64)
        return self.fft_size * float((w * w).sum()) / float(w.sum()) ** 2

    def band_power(self, f_lo, f_hi):
        f = self.freqs()
        return float(self.psd[(f >= f_lo) & (f <= f_hi)].sum())

    def occupied_bandwidth(self, fraction=0.99):
        """width in Hz of the narrowest band centred on 0 Hz (2 m + 1 bins) that holds `fraction` of the power"""
        c, total = self.fft_size // 2, float(self.psd.sum())
        for m in range(c + 1):
            if float(self.psd[max(c - m, 0):c + m + 1].sum()) >= fraction * total:
                return (2 * m + 1) * self.sample_rate / self.fft_size
        return self.sample_rate

    def _inband(self, half_bandwidth):
        f = self.freqs()
        return float(self.psd[np.abs(f) <= 0.9 * half_bandwidth].mean())

    def shoulder_db(self, half_bandwidth, lo=300e3, hi=700e3):
        """(lower, upper): 10 log10 of the mean PSD over |f| <= 0.9 half_bandwidth divided by the largest PSD bin whose distance from the band edge on that
        side is in [lo, hi]"""
        if half_bandwidth + hi > self.sample_rate / 2:
            raise ValueError("the shoulder's band lies beyond Nyquist")
        f, inband = self.freqs(), self._inband(half_bandwidth)
        up = self.psd[(f - half_bandwidth >= lo) & (f - half_bandwidth <= hi)]
        dn = self.psd[(-f - half_bandwidth >= lo) & (-f - half_bandwidth <= hi)]
        if not len(up) or not len(dn):
            raise ValueError("no bin in the shoulder's band")
        return 10.0 * np.log10(inband / float(dn.max())), 10.0 * np.log10(inband / float(up.max()))

    def ccdf(self):
        """(levels, prob): the lower edges of histogram bins 1 .. 2039 in dB above the mean power, and the share of the counted samples at or above each"""
        edges = (np.arange(1, 2040, dtype=np.uint32) << np.uint32(20)).view(np.float32).astype(np.float64)
        above = np.cumsum(self.hist[::-1].astype(np.float64))[::-1]
        return 10.0 * np.log10(edges / self.mean_power), above[1:2040] / float(self.samples_counted)

    def papr_db(self, prob=None):
        """peak over mean in dB; with `prob`, the level that a sample exceeds with that probability (linear in dB between the histogram's bin edges)"""
        if prob is None:
            return 10.0 * np.log10(float(self.peak_power) / self.mean_power)
        lev, p = self.ccdf()
        j = int(np.argmax(p <= prob))
        if p[j] > prob:
            raise ValueError("no level is exceeded that rarely")
        if j == 0:
            return float(lev[0])
        return float(lev[j - 1] + (lev[j] - lev[j - 1]) * (p[j - 1] - prob) / (p[j - 1] - p[j]))

    def mask_margin(self, points, half_bandwidth):
        """the smallest of (mask - PSD) in dB over a mask of (offset from the centre in Hz, dB relative to the in-band mean) points, linear in Hz between
        them, applied to both sides; negative where the mask is broken"""
        pts = sorted((float(o), float(d)) for o, d in points)
        off, db = np.array([o for o, _ in pts]), np.array([d for _, d in pts])
        if len(pts) < 2 or off[0] < 0 or off[-1] > self.sample_rate / 2:
            raise ValueError("a mask is two or more points between 0 and Nyquist")
        f = np.abs(self.freqs())
        sel = (f >= off[0]) & (f <= off[-1])
        with np.errstate(divide="ignore"):
            rel = 10.0 * np.log10(self.psd[sel] / self._inband(half_bandwidth))
        return float((np.interp(f[sel], off, db) - rel).min())


class Spectrum(_Handle):
    """dvbt_spectrum_*: a spectrum analyser on the GPU.  It consumes complex64 baseband as one stream over any number of push() / push_device() calls of any
    size and accumulates Welch's averaged periodogram (fft_size a power of two in 64..8192, hop in [fft_size / 8, fft_size], None: fft_size / 2; window
    "rect", "hann" or "blackman-harris") and the statistics of |x|^2 over the first hop samples of every complete segment.  read() synchronises and returns
    a SpectrumReading; it does not disturb the accumulation.  A stream cut into calls gives the bits of one call."""
    _prefix = "dvbt_spectrum"

    def __init__(self, fft_size=2048, hop=None, window="hann", device=0, sample_rate=64e6 / 7):
        self.L = _spectrum_lib()
        if isinstance(window, str):
            if window.lower() not in SPECTRUM_WINDOWS:
                raise DvbtError(f"window must be one of {sorted(SPECTRUM_WINDOWS)}")
            window = SPECTRUM_WINDOWS[window.lower()]
        self.p = SpectrumParams(int(device), int(fft_size), 0 if hop is None else int(hop), int(window))
        self.sample_rate = float(sample_rate)
        self.h = C.c_void_p()
        _chk(self.L.dvbt_spectrum_create(C.byref(self.p), C.byref(self.h)))

    def push(self, iq):
        """complex64 samples from the host; continues the stream"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        _chk(self.L.dvbt_spectrum_push(self.h, iq.ctypes.data_as(C.c_void_p), len(iq)))

    def push_device(self, ptr, nsamples, stream=None):
        """a device pointer (int) to nsamples complex64: enqueues on `stream` (a hipStream_t as int, None: the default stream)"""
        _chk(self.L.dvbt_spectrum_push_device(self.h, C.c_void_p(ptr), nsamples, C.c_void_p(stream) if stream else None))

    def read(self):
        r = SpectrumResult()
        psd, hist = np.zeros(self.p.fft_size, np.float64), np.zeros(SPECTRUM_HIST_BINS, np.uint64)
        _chk(self.L.dvbt_spectrum_read(self.h, C.byref(r), psd.ctypes.data_as(C.POINTER(C.c_double)), hist.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return SpectrumReading(psd, hist, r.segments, r.samples_pushed, r.samples_counted, r.nonfinite, r.sum_power, r.peak_power, self.p.fft_size,
                               self.p.hop or self.p.fft_size // 2, self.p.window, self.sample_rate)


SOUNDER_WINDOWS = {"rect": 0, "rectangular": 0, "hann": 1}


class SounderParams(C.Structure):
    _fields_ = [("device", C.c_int), ("transmission_mode", C.c_int), ("window", C.c_int), ("first_index", C.c_int)]


class SounderResult(C.Structure):
    _fields_ = [("symbols_pushed", C.c_longlong), ("groups_used", C.c_longlong), ("groups_skipped", C.c_longlong), ("M", C.c_int), ("Kp", C.c_int)]


_PI = C.POINTER(C.c_int)


@_typed_once
def _sounder_lib(L):
    L.dvbt_sounder_create.argtypes = [C.POINTER(SounderParams), C.POINTER(C.c_void_p)]
    L.dvbt_sounder_push.argtypes = [C.c_void_p, C.c_void_p, _PI, _PI, _PI, C.c_size_t]
    L.dvbt_sounder_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_sounder_read.argtypes = [C.c_void_p, C.POINTER(SounderResult), C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_double), C.c_size_t]
    L.dvbt_sounder_reset.argtypes = [C.c_void_p]
    L.dvbt_sounder_destroy.argtypes = [C.c_void_p]
    L.dvbt_device_malloc.restype = C.c_void_p
    L.dvbt_device_malloc.argtypes = [C.c_size_t]
    L.dvbt_device_free.argtypes = [C.c_void_p]
    L.dvbt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]


class SounderReading:
    """What Sounder.read() returns: `pdp` (M doubles: the sums of |h|^2 over the used groups, bin m a delay of 2 m / 3 samples), `resp` (Kp doubles: the sums
    of |E|^2, carrier 3 j) and the fields of dvbt_sounder_result.  The helpers are numpy in double on the host and need no GPU."""

    def __init__(self, pdp, resp, symbols_pushed, groups_used, groups_skipped, mode, sample_rate=64e6 / 7):
        self.pdp, self.resp = np.asarray(pdp, np.float64), np.asarray(resp, np.float64)
        self.symbols_pushed, self.groups_used, self.groups_skipped = int(symbols_pushed), int(groups_used), int(groups_skipped)
        self.mode, self.sample_rate = int(mode), float(sample_rate)
        self.M, self.Kp = len(self.pdp), len(self.resp)

    def delays(self, sample_rate=None):
        """the delay of every bin relative to the strongest, signed (bins from M / 2 on behind it read as pre-echoes), in samples, or in seconds for a
        sample rate"""
        m0 = int(np.argmax(self.pdp))
        d = ((np.arange(self.M) - m0 + self.M // 2) % self.M - self.M // 2) * (2.0 / 3.0)
        return d if sample_rate is None else d / float(sample_rate)

    def _five(self, m):
        return float(self.pdp[(m + np.arange(-2, 3)) % self.M].sum())

    def paths(self, threshold_db=-30.0):
        """[(delay in samples, level in dB relative to the strongest)] of the local maxima at or above the threshold, the strongest (0, 0) first, then by
        delay.  A level is the sum of the five bins around the maximum over the same sum around the strongest.  A local maximum is a bin above every other
        within five bins (3.3 samples) of it: the Hann window's main lobe is 7.2 bins wide and its first side lobe stands 4.5 bins from the centre, where the
        five bins would reach back into the main lobe."""
        p, d = self.pdp, self.delays()
        m0 = int(np.argmax(p))
        ref = self._five(m0)
        if not ref > 0.0:
            return []
        out = []
        around = np.max([np.roll(p, k) for k in range(-5, 6) if k], axis=0)
        for m in np.nonzero(p > around)[0]:
            lev = 10.0 * np.log10(self._five(int(m)) / ref) if self._five(int(m)) > 0.0 else -np.inf
            if m != m0 and lev >= threshold_db:
                out.append((float(d[m]), float(lev)))
        return [(0.0, 0.0)] + sorted(out)

    def outside_guard_db(self, cp):
        """10 log10 of the share of the profile's power whose delay relative to the strongest path lies outside [0, cp] samples -- by more than four bins
        (2.7 samples), the half width of the window's main lobe, which a path at 0 or at cp itself spreads over"""
        d, total = self.delays(), float(self.pdp.sum())
        outside = float(self.pdp[(d < -8.0 / 3.0 - 1e-9) | (d > cp + 8.0 / 3.0 + 1e-9)].sum())
        return 10.0 * np.log10(outside / total) if outside > 0.0 and total > 0.0 else -np.inf

    def ripple_db(self):
        """max over min of the amplitude response's power over the Kp carriers, in dB"""
        lo, hi = float(self.resp.min()), float(self.resp.max())
        return 10.0 * np.log10(hi / lo) if lo > 0.0 else np.inf


class Sounder(_Handle):
    """dvbt_sounder_*: a channel sounder on the GPU.  It consumes demodulated symbols -- rows of N complex64 in fft-shifted order, with the symbol index, the
    integer carrier offset and cp_start of each -- as one stream over any number of push() / push_device() calls and accumulates the echo profile and the
    amplitude response from the scattered pilots of every four consecutive symbols (include/dvbt_hip.h has the definitions).  read() synchronises and returns
    a SounderReading; it does not disturb the accumulation.  A stream cut into calls gives the bits of one call."""
    _prefix = "dvbt_sounder"

    def __init__(self, mode, window="hann", first_index=0, device=0, sample_rate=64e6 / 7):
        self.L = _sounder_lib()
        if isinstance(window, str):
            if window.lower() not in SOUNDER_WINDOWS:
                raise DvbtError(f"window must be one of {sorted(SOUNDER_WINDOWS)}")
            window = SOUNDER_WINDOWS[window.lower()]
        self.p = SounderParams(int(device), int(mode), int(window), int(first_index))
        self.sample_rate = float(sample_rate)
        self.h = C.c_void_p()
        self._ints = None
        _chk(self.L.dvbt_sounder_create(C.byref(self.p), C.byref(self.h)))
        self.N = 8192 if int(mode) == T8k else 2048

    def push(self, rows, index=None, offset=None, cp_start=None):
        """rows [n][N] complex64 from the host and up to three int arrays of n (None: index first_index + position, offset 0, cp_start 0); continues the
        stream"""
        rows = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.N)
        ints = [None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (index, offset, cp_start)]
        if any(a is not None and len(a) != len(rows) for a in ints):
            raise DvbtError("index, offset and cp_start take one value per row")
        _chk(self.L.dvbt_sounder_push(self.h, rows.ctypes.data_as(C.c_void_p), *[None if a is None else a.ctypes.data_as(_PI) for a in ints], len(rows)))

    def push_device(self, rows_ptr, nsym, index_ptr=None, offset_ptr=None, cp_start_ptr=None, stream=None):
        """device pointers (ints; the three int arrays may be None): enqueues on `stream` (a hipStream_t as int, None: the default stream)"""
        _chk(self.L.dvbt_sounder_push_device(self.h, C.c_void_p(rows_ptr), *[C.c_void_p(p) if p else None for p in (index_ptr, offset_ptr, cp_start_ptr)],
                                             nsym, C.c_void_p(stream) if stream else None))

    def read(self):
        r = SounderResult()
        M, Kp = self.N // 2, (1705 if self.N == 2048 else 6817) // 3 + 1
        pdp, resp = np.zeros(M, np.float64), np.zeros(Kp, np.float64)
        _chk(self.L.dvbt_sounder_read(self.h, C.byref(r), pdp.ctypes.data_as(C.POINTER(C.c_double)), M, resp.ctypes.data_as(C.POINTER(C.c_double)), Kp))
        assert (r.M, r.Kp) == (M, Kp)
        return SounderReading(pdp, resp, r.symbols_pushed, r.groups_used, r.groups_skipped, self.p.transmission_mode, self.sample_rate)

    def push_rx(self, rx, first_row=0):
        """the last finished segment of an Rx(taps=True): rows first_row .. n_symbols - 2 of its FFT tap straight from the device, with the symbol-index,
        carrier-offset and cp_start taps (4 bytes a symbol each, which the receiver keeps inside per-symbol records: read to the host and put back as three
        arrays)"""
        if rx.report is None:
            raise DvbtError("the receiver has not run a segment")
        n = rx.report.n_symbols - 1 - int(first_row)
        rows = rx.tap_device_ptr(TAP_FFT)
        if first_row < 0 or not rows:
            raise DvbtError("no FFT tap to read")
        if n <= 0:
            return
        ints = np.stack([np.asarray(rx.tap(t)[first_row:first_row + n], np.int32) for t in (TAP_SYMBOL_INDEX, TAP_FREQ_OFFSET, TAP_CP_START)])
        if ints.shape != (3, n):
            raise DvbtError("the receiver's taps are shorter than its report (taps=True is needed)")
        self._free_ints()
        self._ints = self.L.dvbt_device_malloc(ints.nbytes)
        if not self._ints:
            raise DvbtError("no device memory for the int arrays")
        ints = np.ascontiguousarray(ints)
        _chk(self.L.dvbt_copy_to_device(C.c_void_p(self._ints), ints.ctypes.data_as(C.c_void_p), ints.nbytes))
        self.push_device(rows + 8 * self.N * int(first_row), n, self._ints, self._ints + 4 * n, self._ints + 8 * n)
        _chk(self.L.dvbt_synchronize(None))        # the int arrays and the receiver's tap may change once this returns

    @classmethod
    def from_rx(cls, rx, window="hann", first_row=0):
        """a sounder of the receiver's mode and device that has been pushed its last finished segment (push_rx)"""
        s = cls(rx.p.transmission_mode, window, 0, rx.p.device)
        s.push_rx(rx, first_row)
        return s

    def _free_ints(self):
        if getattr(self, "_ints", None):
            self.L.dvbt_device_free(C.c_void_p(self._ints))
            self._ints = None

    def close(self):
        if self.h:
            self._free_ints()
        super().close()


CONSTELLATION_GRID = 128
CONSTELLATION_STEP = 4096.0      # quantisation steps per grid unit d
POINT_DTYPE = np.dtype([(f, np.int64) for f in ("n", "sum_re", "sum_im", "sum_re_im", "sum_re2", "sum_im2")])
CARRIER_DTYPE = np.dtype([(f, np.int64) for f in ("n", "signal", "error")])


class ConstellationParams(C.Structure):
    _fields_ = [("device", C.c_int), ("constellation", C.c_int), ("hierarchy", C.c_int), ("row_length", C.c_int)]


class ConstellationResult(C.Structure):
    _fields_ = [("rows_pushed", C.c_longlong), ("cells", C.c_longlong), ("nonfinite", C.c_longlong), ("clipped", C.c_longlong),
                ("points", C.c_int), ("levels", C.c_int), ("alpha", C.c_int), ("span", C.c_int)]


@_typed_once
def _constellation_lib(L):
    L.dvbt_constellation_create.argtypes = [C.POINTER(ConstellationParams), C.POINTER(C.c_void_p)]
    L.dvbt_constellation_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_constellation_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_constellation_read.argtypes = [C.c_void_p, C.POINTER(ConstellationResult), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.dvbt_constellation_reset.argtypes = [C.c_void_p]
    L.dvbt_constellation_destroy.argtypes = [C.c_void_p]


def constellation_grid(constellation, hierarchy=NH):
    """(levels L, alpha, span S) of a constellation and hierarchy, as dvbt_constellation_result echoes them"""
    if constellation not in (QPSK, QAM16, QAM64) or hierarchy not in (NH, ALPHA1, ALPHA2, ALPHA4) or (constellation == QPSK and hierarchy != NH):
        raise DvbtError("no such constellation / hierarchy")
    L, alpha = (2, 4, 8)[constellation], (1, 1, 2, 4)[hierarchy]
    S = 2
    while S < alpha + L - 1:
        S *= 2
    return L, alpha, S


def _db(num, den):
    """10 log10(num / den) in float64: nan where either is empty, inf where only the denominator is"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(num > 0, np.where(den > 0, 10.0 * np.log10(num / np.where(den > 0, den, 1.0)), np.inf), np.nan)
    return out


class ConstellationReading:
    """What Constellation.read() returns: `hist` ([G][G] uint64: the I/Q density, hist[b_im][b_re] over [-span, span) grid units per axis), `points` (L^2
    records n, sum_re, sum_im, sum_re_im, sum_re2, sum_im2 of the quantised error, point p = row L + col), `carriers` (row_length records n, signal, error)
    and the totals of dvbt_constellation_result.  The figures of TR 101 290's constellation analysis are float64 on the host from these integers, in grid
    units d, and need no GPU; each is nan where its inputs are empty."""

    def __init__(self, hist, points, carriers, rows_pushed, cells, nonfinite, clipped, levels, alpha, span):
        self.hist = np.asarray(hist, dtype=np.uint64).reshape(CONSTELLATION_GRID, CONSTELLATION_GRID)
        self.points = np.asarray(points, dtype=POINT_DTYPE).reshape(-1)
        self.carriers = np.asarray(carriers, dtype=CARRIER_DTYPE).reshape(-1)
        self.rows_pushed, self.cells, self.nonfinite, self.clipped = int(rows_pushed), int(cells), int(nonfinite), int(clipped)
        self.levels, self.alpha, self.span = int(levels), int(alpha), int(span)
        assert len(self.points) == self.levels ** 2

    @property
    def ideal(self):
        """[L^2][2]: (re, im) of every point in grid units, point p = row L + col"""
        H = self.levels // 2
        i = np.arange(self.levels)
        ax = np.where(i >= H, self.alpha + 2.0 * (i - H), -(self.alpha + 2.0 * (H - 1 - i)))
        return np.stack([np.tile(ax, self.levels), np.repeat(ax, self.levels)], axis=1)

    @property
    def mer_db(self):
        return float(_db(float(self.carriers["signal"].sum()) * CONSTELLATION_STEP ** 2, float(self.carriers["error"].sum())))

    @property
    def mer_per_carrier_db(self):
        return _db(self.carriers["signal"].astype(np.float64) * CONSTELLATION_STEP ** 2, self.carriers["error"].astype(np.float64))

    def means(self):
        """(n, [L^2][2] mean error of every point in grid units; nan where the point was never hit)"""
        n = self.points["n"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.stack([self.points["sum_re"], self.points["sum_im"]], axis=1) / (CONSTELLATION_STEP * n[:, None])
        return n, d

    def fit(self):
        """(A, b): the least-squares affine map from ideal point to measured mean, mean_p = A ideal_p + b, A real 2 x 2, weights n_p"""
        n, d = self.means()
        use = n > 0
        if use.sum() < 3:
            return np.full((2, 2), np.nan), np.full(2, np.nan)
        x, w = self.ideal[use], n[use]
        X = np.concatenate([x, np.ones((len(x), 1))], axis=1) * np.sqrt(w)[:, None]
        Y = (x + d[use]) * np.sqrt(w)[:, None]
        sol, _, rank, _ = np.linalg.lstsq(X, Y, rcond=None)
        if rank < 3:
            return np.full((2, 2), np.nan), np.full(2, np.nan)
        return sol[:2].T.copy(), sol[2].copy()

    @property
    def carrier_suppression_db(self):
        _, b = self.fit()
        return float(_db(float((self.ideal ** 2).sum(axis=1).mean()), float(b @ b))) if np.isfinite(b).all() else float("nan")

    @property
    def amplitude_imbalance_pct(self):
        A, _ = self.fit()
        v = np.hypot(A[0], A[1])                   # the lengths of A's columns
        return float((v.max() / v.min() - 1.0) * 100.0) if np.isfinite(v).all() and v.min() > 0 else float("nan")

    @property
    def quadrature_error_deg(self):
        A, _ = self.fit()
        if not np.isfinite(A).all():
            return float("nan")
        c = float(A[:, 0] @ A[:, 1]) / float(np.hypot(*A[:, 0]) * np.hypot(*A[:, 1]))
        return 90.0 - float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))

    def ste(self):
        """(STEM, STED): the mean and the standard deviation over the points hit of |d_p| / S_rms, d_p the mean error of point p and S_rms the rms magnitude
        of the ideal points"""
        n, d = self.means()
        use = n > 0
        if not use.any():
            return float("nan"), float("nan")
        s = np.hypot(d[use, 0], d[use, 1]) / np.sqrt((self.ideal ** 2).sum(axis=1).mean())
        return float(s.mean()), float(s.std())

    @property
    def phase_jitter_deg(self):
        """over the four corner points, from their second moments: sqrt(max(var_tangential - var_radial, 0)) / |corner|, in degrees"""
        L = self.levels
        p = self.points[[0, L - 1, L * (L - 1), L * L - 1]]
        n = p["n"].astype(np.float64)
        if not (n > 0).all():
            return float("nan")
        corners = self.ideal[[0, L - 1, L * (L - 1), L * L - 1]]
        s = CONSTELLATION_STEP
        mx, my = p["sum_re"] / (s * n), p["sum_im"] / (s * n)
        vxx, vyy, vxy = p["sum_re2"] / (s * s * n) - mx * mx, p["sum_im2"] / (s * s * n) - my * my, p["sum_re_im"] / (s * s * n) - mx * my
        rho = np.hypot(corners[:, 0], corners[:, 1])
        ur, ui = corners[:, 0] / rho, corners[:, 1] / rho                      # radial unit vectors; the tangential one is (-ui, ur)
        var_r = ur * ur * vxx + 2.0 * ur * ui * vxy + ui * ui * vyy
        var_t = ui * ui * vxx - 2.0 * ur * ui * vxy + ur * ur * vyy
        w = n / n.sum()
        return float(np.degrees(np.sqrt(max(float((w * (var_t - var_r)).sum()), 0.0)) / float(rho[0])))


class Constellation(_Handle):
    """dvbt_constellation_*: a constellation analyser on the GPU.  It consumes equalised data cells -- rows of row_length complex64, the layout of the
    receiver's TAP_EQ -- as one stream over any number of push() / push_device() calls and accumulates, in integers, the I/Q density, the error cloud of
    every constellation point and the signal and error sums of every carrier (include/dvbt_hip.h has the definitions).  read() synchronises and returns a
    ConstellationReading; it does not disturb the accumulation.  A stream cut into calls gives the same bits."""
    _prefix = "dvbt_constellation"

    def __init__(self, constellation, hierarchy=NH, row_length=1512, device=0):
        self.L = _constellation_lib()
        self.p = ConstellationParams(int(device), int(constellation), int(hierarchy), int(row_length))
        self.h = C.c_void_p()
        _chk(self.L.dvbt_constellation_create(C.byref(self.p), C.byref(self.h)))

    def push(self, rows):
        """rows [n][row_length] complex64 from the host; continues the stream"""
        rows = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.p.row_length)
        _chk(self.L.dvbt_constellation_push(self.h, rows.ctypes.data_as(C.c_void_p), len(rows)))

    def push_device(self, rows_ptr, nrows, stream=None):
        """a device pointer (int) to nrows rows: enqueues on `stream` (a hipStream_t as int, None: the default stream)"""
        _chk(self.L.dvbt_constellation_push_device(self.h, C.c_void_p(rows_ptr), nrows, C.c_void_p(stream) if stream else None))

    def read(self):
        r = ConstellationResult()
        levels = constellation_grid(self.p.constellation, self.p.hierarchy)[0]
        hist = np.zeros((CONSTELLATION_GRID, CONSTELLATION_GRID), np.uint64)
        points, carriers = np.zeros(levels ** 2, POINT_DTYPE), np.zeros(self.p.row_length, CARRIER_DTYPE)
        _chk(self.L.dvbt_constellation_read(self.h, C.byref(r), hist.ctypes.data_as(C.c_void_p), points.ctypes.data_as(C.c_void_p), len(points),
                                            carriers.ctypes.data_as(C.c_void_p), len(carriers)))
        assert r.points == len(points) and r.levels == levels
        return ConstellationReading(hist, points, carriers, r.rows_pushed, r.cells, r.nonfinite, r.clipped, r.levels, r.alpha, r.span)

    def push_rx(self, rx, first_row=0):
        """the last finished segment of an Rx(taps=True) or Rx(quality=True): rows first_row .. n_out_symbols - 1 of its EQ tap (the rows from
        first_out_symbol on) straight from the device"""
        if rx.report is None:
            raise DvbtError("the receiver has not run a segment")
        if rx.dims.payload_length != self.p.row_length or (rx.p.constellation, rx.p.hierarchy) != (self.p.constellation, self.p.hierarchy):
            raise DvbtError("the receiver's constellation, hierarchy or payload length is not the analyser's")
        base = rx.tap_device_ptr(TAP_EQ)
        if not base:
            raise DvbtError("the receiver keeps no equalised cells: create it with taps=True or quality=True")
        n = rx.report.n_out_symbols - int(first_row)
        if first_row < 0:
            raise DvbtError("first_row must not be negative")
        if n <= 0:
            return
        self.push_device(base + 8 * self.p.row_length * (max(rx.report.first_out_symbol, 0) + int(first_row)), n)
        _chk(self.L.dvbt_synchronize(None))        # the receiver's tap may change once this returns

    @classmethod
    def from_rx(cls, rx, first_row=0):
        """an analyser of the receiver's constellation, hierarchy, payload length and device that has been pushed its last finished segment (push_rx)"""
        if rx.report is None:
            raise DvbtError("the receiver has not run a segment")
        c = cls(rx.p.constellation, rx.p.hierarchy, rx.dims.payload_length, rx.p.device)
        try:
            c.push_rx(rx, first_row)
        except Exception:
            c.close()
            raise
        return c


TS_PACKET, TS_PIDS, TS_TILE = 188, 8192, 1024
TS_NULL_PID = 0x1FFF
TS_PCR_HZ = 27e6
TS_PID_FIELDS = ("pid", "packets", "pusi", "scrambled", "payload", "adaptation", "discontinuity", "random_access", "pcr", "tei", "duplicates", "cc_errors",
                 "first", "last", "pcr_pairs", "pcr_discontinuity_signalled", "pcr_over_100ms", "pcr_over_40ms", "sum_dt", "sum_dp", "min_dt", "max_dt",
                 "max_dp")
TS_PID_DTYPE = np.dtype([(f, np.int64) for f in TS_PID_FIELDS])
TS_TOTALS = ("packets_pushed", "sync_errors", "transport_errors", "afc_reserved", "af_length_errors", "pids_seen")


class TsParams(C.Structure):
    _fields_ = [("device", C.c_int), ("max_packets", C.c_int)]


class TsResult(C.Structure):
    _fields_ = [(f, C.c_longlong) for f in TS_TOTALS]


@_typed_once
def _ts_lib(L):
    L.dvbt_ts_create.argtypes = [C.POINTER(TsParams), C.POINTER(C.c_void_p)]
    L.dvbt_ts_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_ts_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_ts_read.argtypes = [C.c_void_p, C.POINTER(TsResult), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dvbt_ts_reset.argtypes = [C.c_void_p]
    L.dvbt_ts_destroy.argtypes = [C.c_void_p]


def ts_align(data):
    """the first offset at which five consecutive packets start with 0x47 (a file from elsewhere need not start on a packet); raises if there is none"""
    d = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    n = len(d) - 4 * TS_PACKET
    if n > 0:
        ok = d[:n] == 0x47
        for k in range(1, 5):
            ok &= d[k * TS_PACKET:k * TS_PACKET + n] == 0x47
        hit = np.flatnonzero(ok)
        if len(hit):
            return int(hit[0])
    raise DvbtError("no five consecutive packets that start with 0x47")


class TsReading:
    """What TsAnalyser.read() returns: the totals of dvbt_ts_result and `pids`, the entries (TS_PID_DTYPE) of the PIDs seen, ascending.  The figures are
    float64 on the host from these integers and need no GPU; each is nan where its inputs are empty."""

    def __init__(self, totals, pids):
        for f in TS_TOTALS:
            setattr(self, f, int(totals[f] if isinstance(totals, dict) else getattr(totals, f)))
        self.pids = np.asarray(pids, dtype=TS_PID_DTYPE).reshape(-1)

    def entry(self, pid):
        """the entry of one PID (all zero, first = min_dt = -1, where it was never seen)"""
        hit = np.flatnonzero(self.pids["pid"] == pid)
        if len(hit):
            return self.pids[hit[0]]
        e = np.zeros((), TS_PID_DTYPE)
        e["pid"], e["first"], e["min_dt"] = pid, -1, -1
        return e

    @property
    def members(self):
        return int(self.pids["packets"].sum())

    def share(self, pid):
        """the PID's members over all members"""
        return float(self.entry(pid)["packets"]) / self.members if self.members else float("nan")

    @property
    def null_share(self):
        return self.share(TS_NULL_PID)

    def ts_bitrate(self, pid):
        """bits per second of the whole stream by the PCRs of `pid`: sum_dp 188 8 27e6 / sum_dt"""
        e = self.entry(pid)
        return float(e["sum_dp"]) * (TS_PACKET * 8) * TS_PCR_HZ / float(e["sum_dt"]) if e["sum_dt"] > 0 else float("nan")

    def pid_bitrate(self, pid, ts_bitrate):
        """bits per second of one PID, given the stream's (ts_bitrate(pcr_pid)): its share of all packets pushed"""
        return float(self.entry(pid)["packets"]) / self.packets_pushed * float(ts_bitrate) if self.packets_pushed else float("nan")

    def pcr_interval_ms(self, pid):
        """(min, mean, max) of the PID's PCR intervals that entered pcr_pairs"""
        e = self.entry(pid)
        if e["pcr_pairs"] <= 0:
            return float("nan"), float("nan"), float("nan")
        ms = 1e3 / TS_PCR_HZ
        return float(e["min_dt"]) * ms, float(e["sum_dt"]) / float(e["pcr_pairs"]) * ms, float(e["max_dt"]) * ms

    def tr101290(self):
        """the first- and second-priority indicators of TR 101 290 that this block can state, as event counts"""
        return {"sync_byte_error": self.sync_errors, "continuity_count_error": int(self.pids["cc_errors"].sum()), "transport_error": self.transport_errors,
                "PCR_repetition_error": int(self.pids["pcr_over_40ms"].sum() + self.pids["pcr_over_100ms"].sum()),
                "PCR_discontinuity_indicator_error": int(self.pids["pcr_over_100ms"].sum())}


class TsAnalyser(_Handle):
    """dvbt_ts_*: a transport-stream analyser on the GPU.  It consumes 188-byte packets -- the layout of the receiver's TAP_TS -- as one stream over any
    number of push() / push_device() calls and accumulates, in 64-bit integers, the packets, flags and continuity errors of every PID and the timing of its
    PCRs (include/dvbt_hip.h has the specification).  read() synchronises and returns a TsReading; it does not disturb the accumulation.  A stream cut
    into calls gives the same bits."""
    _prefix = "dvbt_ts"

    def __init__(self, max_packets=1 << 19, device=0):
        self.L = _ts_lib()
        self.p = TsParams(int(device), int(max_packets))
        self.h = C.c_void_p()
        _chk(self.L.dvbt_ts_create(C.byref(self.p), C.byref(self.h)))

    def push(self, packets):
        """whole packets from the host (bytes or a uint8 array of any shape); continues the stream"""
        d = np.frombuffer(packets, np.uint8) if isinstance(packets, (bytes, bytearray, memoryview)) else np.ascontiguousarray(packets, dtype=np.uint8).reshape(-1)
        if len(d) % TS_PACKET:
            raise DvbtError("whole packets of 188 bytes only")
        _chk(self.L.dvbt_ts_push(self.h, C.c_void_p(d.ctypes.data) if len(d) else None, len(d) // TS_PACKET))

    def push_device(self, packets_ptr, npackets, stream=None):
        """a device pointer (int, any byte alignment) to npackets packets: enqueues on `stream` (a hipStream_t as int, None: the default stream)"""
        _chk(self.L.dvbt_ts_push_device(self.h, C.c_void_p(packets_ptr), npackets, C.c_void_p(stream) if stream else None))

    def read(self):
        r, n = TsResult(), C.c_size_t()
        pids = np.zeros(TS_PIDS, TS_PID_DTYPE)
        _chk(self.L.dvbt_ts_read(self.h, C.byref(r), pids.ctypes.data_as(C.c_void_p), len(pids), C.byref(n)))
        assert n.value == r.pids_seen
        return TsReading(r, pids[:n.value].copy())

    def push_rx(self, rx):
        """the last finished segment of an Rx: the whole packets of its TS tap (the receiver's output buffer) straight from the device"""
        if rx.report is None:
            raise DvbtError("the receiver has not run a segment")
        base = rx.tap_device_ptr(TAP_TS)
        if not base:
            raise DvbtError("the receiver keeps no transport-stream tap")
        n = max(int(rx.report.n_ts_bytes), 0) // TS_PACKET
        if n <= 0:
            return
        self.push_device(base, n)
        _chk(self.L.dvbt_synchronize(None))        # the receiver's tap may change once this returns

    @classmethod
    def from_rx(cls, rx, max_packets=1 << 19):
        """an analyser on the receiver's device that has been pushed its last finished segment (push_rx)"""
        if rx.report is None:
            raise DvbtError("the receiver has not run a segment")
        a = cls(max_packets, rx.p.device)
        try:
            a.push_rx(rx)
        except Exception:
            a.close()
            raise
        return a


KEEP_PILOTS, KEEP_TPS = 1, 2      # CfrParams.keep: DVBT_CFR_KEEP_*
CFR_MAX_ITERATIONS = 8
CFR_FIELDS = ("symbols", "symbols_clipped", "symbols_nonfinite", "samples_over", "peak_power_in")


class CfrParams(C.Structure):
    _fields_ = [("transmission_mode", C.c_int), ("guard_interval", C.c_int), ("threshold", C.c_float), ("iterations", C.c_int),
                ("oversampling", C.c_int), ("keep", C.c_int), ("first_symbol", C.c_int64), ("device", C.c_int)]


class CfrResult(C.Structure):
    _fields_ = [(f, C.c_longlong) for f in CFR_FIELDS[:4]] + [("peak_power_in", C.c_float)]


@_typed_once
def _cfr_lib(L):
    L.dvbt_cfr_create.argtypes = [C.POINTER(CfrParams), C.POINTER(C.c_void_p)]
    L.dvbt_cfr_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_cfr_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.dvbt_cfr_read.argtypes = [C.c_void_p, C.POINTER(CfrResult)]
    L.dvbt_cfr_reset.argtypes = [C.c_void_p]
    L.dvbt_cfr_destroy.argtypes = [C.c_void_p]


class CfrReading:
    """What Cfr.read() returns: dvbt_cfr_result's four counters as ints and peak_power_in as a float.  Two readings compare equal field by field."""

    def __init__(self, r):
        for f in CFR_FIELDS[:4]:
            setattr(self, f, int(r[f] if isinstance(r, dict) else getattr(r, f)))
        self.peak_power_in = float(r["peak_power_in"] if isinstance(r, dict) else r.peak_power_in)

    def as_tuple(self):
        return tuple(getattr(self, f) for f in CFR_FIELDS)

    def __eq__(self, other):
        return isinstance(other, CfrReading) and self.as_tuple() == other.as_tuple()

    def __repr__(self):
        return "CfrReading(" + ", ".join(f"{f}={getattr(self, f)!r}" for f in CFR_FIELDS) + ")"

    def peak_db(self, ref_power):
        """the highest peak seen in a first iteration, in dB over the mean power ref_power (Channel.power)"""
        return float(_db(self.peak_power_in, ref_power))


class Cfr(_SampleBlock):
    """dvbt_cfr_*: crest-factor reduction of DVB-T baseband on the GPU by iterative clipping and filtering, one OFDM symbol at a time (include/dvbt_hip.h has
    the specification, tests/cfrref.py is it in numpy).  Samples above `threshold` in magnitude -- looked for at `oversampling` times the sample rate -- are
    clipped, and the clipping error is kept to the occupied carriers and, by default, off the pilots and the TPS carriers; `iterations` times.  The stream is
    whole symbols of guard + useful part, starting at the frame's symbol `first_symbol` (what matters is the scattered-pilot phase, first_symbol mod 4), over
    any number of run() / run_device() calls; the concatenated outputs are bit for bit those of one call.  read() synchronises and returns a CfrReading.
    The mean power drops by about 1 % at 7 dB; the block does not make up for it."""
    _prefix = "dvbt_cfr"

    def __init__(self, mode, guard, threshold, iterations=4, oversampling=2, keep=KEEP_PILOTS | KEEP_TPS, first_symbol=0, device=0):
        self.L = _cfr_lib()
        self.p = CfrParams(int(mode), int(guard), float(threshold), int(iterations), int(oversampling), int(keep), int(first_symbol), int(device))
        self.h = C.c_void_p()
        _chk(self.L.dvbt_cfr_create(C.byref(self.p), C.byref(self.h)))

    @staticmethod
    def threshold_for(papr_db, ref_power):
        """the threshold that stands papr_db above the mean power ref_power (Channel.power)"""
        return float(np.sqrt(ref_power * 10.0 ** (papr_db / 10.0)))

    def run_device(self, in_ptr, nsamples, out_ptr, stream=None):
        """device pointers (ints) to nsamples complex64 each (whole symbols), the same buffer (in place) or not overlapping: enqueues on `stream` (a
        hipStream_t as int, None: the default stream)"""
        super().run_device(in_ptr, nsamples, out_ptr, stream)

    def read(self):
        r = CfrResult()
        _chk(self.L.dvbt_cfr_read(self.h, C.byref(r)))
        return CfrReading(r)


SCAN_HYPOTHESES = 8
SCAN_GROUP = 16
SCAN_MIN_SAMPLES = 8 * 10240 + 8192


class ScanParams(C.Structure):
    _fields_ = [("device", C.c_int), ("rho_min", C.c_double), ("ratio_min", C.c_double)]


class ScanResult(C.Structure):
    _fields_ = [("detected", C.c_int), ("mode", C.c_int), ("guard", C.c_int), ("symbol_start", C.c_int * 8),
                ("samples_pushed", C.c_longlong), ("nonfinite", C.c_longlong), ("symbols", C.c_longlong * 8),
                ("rho", C.c_double * 8), ("cfo", C.c_double * 8)]


_PD = C.POINTER(C.c_double)


@_typed_once
def _scan_lib(L):
    L.dvbt_scan_create.argtypes = [C.POINTER(ScanParams), C.POINTER(C.c_void_p)]
    L.dvbt_scan_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dvbt_scan_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.dvbt_scan_read.argtypes = [C.c_void_p, C.POINTER(ScanResult)]
    L.dvbt_scan_accumulators.argtypes = [C.c_void_p, C.c_int, _PD, _PD, C.c_int]
    L.dvbt_scan_evaluate.argtypes = [C.POINTER(ScanParams), C.POINTER(C.c_int64), C.POINTER(_PD), C.POINTER(_PD), C.c_int64, C.c_int64, C.POINTER(ScanResult)]
    L.dvbt_scan_reset.argtypes = [C.c_void_p]
    L.dvbt_scan_destroy.argtypes = [C.c_void_p]


def scan_dims(h):
    """(N, G, S) of hypothesis h = 4 mode + guard: the useful part, the guard interval and the symbol, in samples"""
    N = 8192 if h >> 2 else 2048
    G = N >> (5 - (h & 3))
    return N, G, N + G


class ScanReading:
    """What Scanner.read() and scan_evaluate() return: the fields of dvbt_scan_result.  `detected` says whether `mode` and `guard` (T2k / T8k, G1_32 ..
    G1_4; -1 otherwise) are to be believed; rho, symbol_start, cfo and symbols hold all eight hypotheses (h = 4 mode + guard) either way."""

    def __init__(self, r, device=0):
        self.detected, self.mode, self.guard = bool(r.detected), int(r.mode), int(r.guard)
        self.samples_pushed, self.nonfinite = int(r.samples_pushed), int(r.nonfinite)
        self.symbols = [int(v) for v in r.symbols]
        self.symbol_start = [int(v) for v in r.symbol_start]
        self.rho, self.cfo = [float(v) for v in r.rho], [float(v) for v in r.cfo]
        self.device = int(device)

    @property
    def hypothesis(self):
        """4 mode + guard of the detected signal, None if nothing was detected"""
        return 4 * self.mode + self.guard if self.detected else None

    def rx_stream(self, **kw):
        """an RxStream for the detected mode and guard; constellation, hierarchy and code rate come from the stream's TPS word (AUTO) unless given"""
        if not self.detected:
            raise DvbtError("the scanner detected no DVB-T signal: there is no mode and guard to build a receiver from")
        kw.setdefault("device", self.device)
        return RxStream(kw.pop("constellation", AUTO), kw.pop("code_rate", AUTO), self.mode, guard=self.guard, hierarchy=kw.pop("hierarchy", AUTO), **kw)

    def __repr__(self):
        return (f"ScanReading(detected={self.detected}, mode={self.mode}, guard={self.guard}, samples_pushed={self.samples_pushed}, "
                f"nonfinite={self.nonfinite}, rho={[round(v, 4) for v in self.rho]})")


def scan_evaluate(symbols, A, E, samples, nonfinite=0, rho_min=0, ratio_min=0):
    """dvbt_scan_evaluate: the scanner's verdict from its sums, on the host (needs no GPU).  symbols[8]; A[8] complex and E[8] real, S bins each (None
    where symbols[h] is 0)."""
    L = _scan_lib()
    keep, Ap, Ep = [], (_PD * 8)(), (_PD * 8)()
    for h in range(SCAN_HYPOTHESES):
        if A[h] is None or E[h] is None:
            continue
        S = scan_dims(h)[2]
        a, e = np.ascontiguousarray(A[h], dtype=np.complex128).reshape(-1), np.ascontiguousarray(E[h], dtype=np.float64).reshape(-1)
        if len(a) != S or len(e) != S:
            raise DvbtError(f"hypothesis {h} has {S} bins")
        keep += [a, e]
        Ap[h], Ep[h] = a.ctypes.data_as(_PD), e.ctypes.data_as(_PD)
    r = ScanResult()
    _chk(L.dvbt_scan_evaluate(C.byref(ScanParams(0, float(rho_min), float(ratio_min))), (C.c_int64 * 8)(*[int(v) for v in symbols]), Ap, Ep,
                              int(samples), int(nonfinite), C.byref(r)))
    return ScanReading(r)


class Scanner(_Handle):
    """dvbt_scan_*: what an unknown DVB-T capture is -- FFT size, guard interval, where a symbol starts and the fractional carrier offset -- from the
    cyclic-prefix correlation at the lags 2048 and 8192, folded at the eight candidate symbol lengths on the GPU (include/dvbt_hip.h has the specification,
    tests/scanref.py is it in numpy).  It consumes complex64 baseband at the elementary rate as one stream over any number of push() / push_device() calls of
    any size and changes nothing; read() synchronises, evaluates on the host and does not disturb the accumulation.  SCAN_MIN_SAMPLES is the least a verdict
    takes; rho_min and ratio_min (0: the defaults 0.1 and 1.5) are the floor of the winner's correlation and of its lead over the runner-up."""
    _prefix = "dvbt_scan"

    def __init__(self, rho_min=0, ratio_min=0, device=0):
        self.L = _scan_lib()
        self.p = ScanParams(int(device), float(rho_min), float(ratio_min))
        self.h = C.c_void_p()
        _chk(self.L.dvbt_scan_create(C.byref(self.p), C.byref(self.h)))

    def push(self, iq):
        """complex64 samples from the host; continues the stream"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        _chk(self.L.dvbt_scan_push(self.h, iq.ctypes.data_as(C.c_void_p), len(iq)))

    def push_device(self, ptr, nsamples, stream=None):
        """a device pointer (int) to nsamples complex64: enqueues on `stream` (a hipStream_t as int, None: the default stream)"""
        _chk(self.L.dvbt_scan_push_device(self.h, C.c_void_p(ptr), nsamples, C.c_void_p(stream) if stream else None))

    def read(self):
        r = ScanResult()
        _chk(self.L.dvbt_scan_read(self.h, C.byref(r)))
        return ScanReading(r, self.p.device)

    def accumulators(self, h):
        """(A complex128 [S], E float64 [S]) of hypothesis h as they stand: the folded sums read() evaluates"""
        S = scan_dims(h)[2] if 0 <= h < SCAN_HYPOTHESES else 1
        a, e = np.zeros(S, np.complex128), np.zeros(S, np.float64)
        _chk(self.L.dvbt_scan_accumulators(self.h, int(h), a.ctypes.data_as(_PD), e.ctypes.data_as(_PD), S))
        return a, e

    @classmethod
    def detect(cls, iq, **kw):
        """one push and one read of a whole capture"""
        s = cls(**kw)
        try:
            s.push(iq)
            return s.read()
        finally:
            s.close()


# ------------------------------------------------------------------ per-block C ABI (one triple per reference block)
TAG_SYNC_START, TAG_SUPERFRAME_START, TAG_SYMBOL_INDEX = 1, 2, 3


class Tag(C.Structure):
    _fields_ = [("rel_offset", C.c_int64), ("key", C.c_int32), ("value", C.c_int32)]


class Sideband(C.Structure):
    _fields_ = [("in_tags", C.POINTER(Tag)), ("n_in_tags", C.c_int), ("out_tags", C.POINTER(Tag)), ("out_cap", C.c_int),
                ("n_out_tags", C.c_int), ("n_consumed", C.c_int)]


def _params(fields):
    return type("P", (C.Structure,), {"_fields_": fields})


_I = C.c_int
BLOCK_PARAMS = {
    "ofdm_sym_acquisition": _params([("blocks", _I), ("fft_length", _I), ("occupied_tones", _I), ("cp_length", _I), ("snr", C.c_float)]),
    "fft": _params([("fft_size", _I), ("forward", _I), ("shift", _I)]),
    "demod_reference_signals": _params([(n, _I) for n in ("itemsize", "ninput", "noutput", "constellation", "hierarchy", "code_rate_hp",
                                                          "code_rate_lp", "guard_interval", "transmission_mode", "include_cell_id", "cell_id")]),
    "demap": _params([("nsize", _I), ("constellation", _I), ("hierarchy", _I), ("transmission_mode", _I), ("gain", C.c_float)]),
    "symbol_inner_interleaver": _params([("nsize", _I), ("transmission_mode", _I), ("direction", _I)]),
    "bit_inner_deinterleaver": _params([("nsize", _I), ("constellation", _I), ("hierarchy", _I), ("transmission_mode", _I)]),
    "viterbi_decoder": _params([("constellation", _I), ("hierarchy", _I), ("code_rate", _I), ("bsize", _I), ("S0", _I), ("SK", _I)]),
    "convolutional_deinterleaver": _params([("blocks", _I), ("I", _I), ("M", _I)]),
    "reed_solomon_dec": _params([(n, _I) for n in ("p", "m", "gfpoly", "n", "k", "t", "s", "blocks", "oracle_compat")]),
    "energy_descramble": _params([("nblocks", _I)]),
    "resampler": _params([("interpolation", _I), ("decimation", _I), ("scale", C.c_float)]),
    # the transmit blocks (dvbt_txblocks.inc)
    "energy_dispersal": _params([("nblocks", _I)]),
    "reed_solomon_enc": _params([(n, _I) for n in ("p", "m", "gfpoly", "n", "k", "t", "s", "blocks")]),
    "convolutional_interleaver": _params([("blocks", _I), ("I", _I), ("M", _I)]),
    "inner_coder": _params([(n, _I) for n in ("ninput", "noutput", "constellation", "hierarchy", "code_rate")]),
    "bit_inner_interleaver": _params([("nsize", _I), ("constellation", _I), ("hierarchy", _I), ("transmission_mode", _I)]),
    "map": _params([("nsize", _I), ("constellation", _I), ("hierarchy", _I), ("transmission_mode", _I), ("gain", C.c_float)]),
    "reference_signals": _params([(n, _I) for n in ("itemsize", "ninput", "noutput", "constellation", "hierarchy", "code_rate_hp",
                                                    "code_rate_lp", "guard_interval", "transmission_mode", "include_cell_id", "cell_id")]),
}
TX_BLOCKS = ("energy_dispersal", "reed_solomon_enc", "convolutional_interleaver", "inner_coder", "bit_inner_interleaver", "map", "reference_signals")


class Block:
    """Generic driver of dvbt_<name>_{create,forecast,work,destroy}; mirrors gr::dvbt::<name>::make(...)."""

    def __init__(self, name, *args):
        self.L = lib()
        self.name = name
        self.params = BLOCK_PARAMS[name](*args)
        self.h = C.c_void_p()
        _chk(getattr(self.L, f"dvbt_{name}_create")(C.byref(self.params), C.byref(self.h)))
        self._work = getattr(self.L, f"dvbt_{name}_work")
        self._work.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Sideband)]
        self._work_device = getattr(self.L, f"dvbt_{name}_work_device", None)
        if self._work_device is not None:
            self._work_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Sideband), C.c_void_p]
        self._tout = (Tag * 4096)()

    def forecast(self, noutput_items):
        n = C.c_int()
        _chk(getattr(self.L, f"dvbt_{self.name}_forecast")(self.h, noutput_items, C.byref(n)))
        return n.value

    def work(self, noutput_items, ninput_items, inp, out, tags=()):
        """returns (items produced, items consumed, [(rel_offset, key, value)] attached to the output)"""
        tin = (Tag * max(len(tags), 1))(*[Tag(*t) for t in tags])
        tout = (Tag * 4096)()
        sb = Sideband(tin, len(tags), tout, 4096, 0, 0)
        r = _chk(self._work(self.h, noutput_items, ninput_items, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(sb)))
        return r, sb.n_consumed, [(tout[i].rel_offset, tout[i].key, tout[i].value) for i in range(min(sb.n_out_tags, 4096))]

    def work_device(self, noutput_items, ninput_items, in_ptr, out_ptr, tags=(), stream=None):
        """dvbt_<name>_work_device: device pointers (ints) in and out, the caller's HIP stream; same return as work()"""
        tin = (Tag * max(len(tags), 1))(*[Tag(*t) for t in tags])
        tout = self._tout
        sb = Sideband(tin, len(tags), tout, 4096, 0, 0)
        r = _chk(self._work_device(self.h, noutput_items, ninput_items, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.byref(sb),
                                   C.c_void_p(stream) if stream else None))
        return r, sb.n_consumed, [(tout[i].rel_offset, tout[i].key, tout[i].value) for i in range(min(sb.n_out_tags, 4096))]

    def viterbi_proof(self):
        """viterbi_decoder only: the proof + repair passes' counters summed over the calls since the last reset"""
        p = ViterbiProof()
        self.L.dvbt_viterbi_decoder_proof.argtypes = [C.c_void_p, C.POINTER(ViterbiProof)]
        _chk(self.L.dvbt_viterbi_decoder_proof(self.h, C.byref(p)))
        return {"chunks": int(p.chunks), "decoded_again": int(p.decoded_again), "sequential": int(p.sequential), "not_proven": int(p.not_proven)}

    def set_viterbi_walk(self, always):
        """viterbi_decoder only: the traceback chains of the following calls walk every hop instead of taking the shortcut over chained best states"""
        self.L.dvbt_viterbi_decoder_set_walk.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.dvbt_viterbi_decoder_set_walk(self.h, int(bool(always))))

    def set_viterbi_chunk_bytes(self, nbytes):
        """viterbi_decoder only, a test hook: chunks of nbytes (0 = the default 264, else a multiple of 24 in [24, 264]) from the next stream reset on"""
        self.L.dvbt_viterbi_decoder_set_chunk_bytes.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.dvbt_viterbi_decoder_set_chunk_bytes(self.h, int(nbytes)))

    def set_viterbi_warm_windows(self, windows):
        """viterbi_decoder only: the chunk decoders' warm-up (0 = the default 72, else a multiple of 24 in [48, 576])"""
        self.L.dvbt_viterbi_decoder_set_warm_windows.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.dvbt_viterbi_decoder_set_warm_windows(self.h, int(windows)))

    def set_viterbi_verify(self, mode):
        """viterbi_decoder only, a test hook: RxParams.viterbi_verify (-1 .. 4) from the next stream reset on"""
        self.L.dvbt_viterbi_decoder_set_verify.argtypes = [C.c_void_p, C.c_int]
        _chk(self.L.dvbt_viterbi_decoder_set_verify(self.h, int(mode)))

    def viterbi_last_ctl(self):
        """viterbi_decoder only, a test hook: the 16 header words of the last launch's control block (k_viterbi3.hpp, V3_CTL_*)"""
        out = (C.c_int * 16)()
        self.L.dvbt_viterbi_decoder_last_ctl.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        _chk(self.L.dvbt_viterbi_decoder_last_ctl(self.h, out))
        return [int(x) for x in out]

    def viterbi_shortcut(self):
        """viterbi_decoder only: (shortcut, walked) blocks of 24 windows, per wavefront, since the block was created"""
        out = (C.c_longlong * 2)()
        self.L.dvbt_viterbi_decoder_shortcut.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        _chk(self.L.dvbt_viterbi_decoder_shortcut(self.h, out))
        return int(out[0]), int(out[1])

    def close(self):
        if self.h:
            fn = getattr(self.L, f"dvbt_{self.name}_destroy")
            fn.argtypes = [C.c_void_p]
            fn(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
