"""gr_dvbt_amd -- host-side Python binding of libdvbt_hip.so (the MI355X DVB-T RX hot path, the modulator, the channel block, the sample-clock offset block, the fading block, the RF front-end block, the spectrum analyser, the channel sounder, the constellation analyser, the tuner, the transport-stream analyser, the crest-factor reduction block and the signal scanner).

Thin ctypes layer over the C ABI declared in include/dvbt_hip.h.  There is no CPU
fallback: importing works anywhere, but every compute entry point raises unless the HIP
library is built in-tree (gr_dvbt_amd/lib/libdvbt_hip.so) and a GPU is visible.
"""
from .binding import (  # noqa: F401
    lib, build, DvbtError, RxParams, RxReport, RxQuality, Rx, RxStream, TxParams, Tx, TX_SCALE, ChannelParams, Channel, CHANNEL_MAX_PATHS, CHANNEL_MAX_DELAY, ClockParams, ClockOffset, clock_outputs, FadingParams, Fading, fading_table, tu6_paths,
    FADING_MAX_PATHS, FADING_MAX_DELAY, FADING_MAX_SINUSOIDS, FADING_KNOT, RfParams, RfMask, RfFrontend, phase_noise_tones, RF_MAX_TONES, RF_MAX_MASK_POINTS, SpectrumParams, SpectrumResult, SpectrumReading, Spectrum,
    SounderParams, SounderResult, SounderReading, Sounder,
    TunerParams, TunerDesc, Tuner, tuner_outputs, tuner_design, IQ_CF32, IQ_CS16, IQ_CS8, IQ_CU8, IQ_DTYPES, IQ_BYTES, IQ_SCALES,
    TUNER_PASS_EDGE, TUNER_STOP_EDGE, TUNER_ATTEN_DB,
    ConstellationParams, ConstellationResult, ConstellationReading, Constellation, constellation_grid, CONSTELLATION_GRID, CONSTELLATION_STEP, POINT_DTYPE, CARRIER_DTYPE,
    TsParams, TsResult, TsReading, TsAnalyser, ts_align, TS_PID_DTYPE, TS_PID_FIELDS, TS_PACKET, TS_PIDS, TS_TILE, TS_NULL_PID,
    CfrParams, CfrResult, CfrReading, Cfr, KEEP_PILOTS, KEEP_TPS, CFR_MAX_ITERATIONS, CFR_FIELDS,
    ScanParams, ScanResult, ScanReading, Scanner, scan_evaluate, scan_dims, SCAN_GROUP, SCAN_MIN_SAMPLES, SCAN_HYPOTHESES,
    spectrum_window, SPECTRUM_HIST_BINS, get_dims, device_count, Block, Tag, Sideband, BLOCK_PARAMS, TX_BLOCKS,
    TAG_SYNC_START, TAG_SUPERFRAME_START, TAG_SYMBOL_INDEX,
    QPSK, QAM16, QAM64, NH, C1_2, C2_3, C3_4, C5_6, C7_8, T2k, T8k, G1_32, G1_16, G1_8, G1_4,
    TAP_ACQ, TAP_FFT, TAP_EQ, TAP_DEMAP, TAP_SYMDEINT, TAP_BITDEINT, TAP_VITERBI, TAP_DEINT,
    TAP_RS, TAP_TS, TAP_CP_START, TAP_SYMBOL_INDEX, TAP_FREQ_OFFSET, TAP_BITDEINT_LP, TAP_SOFT, TAP_CSI, TAP_BITDEINT_LOG, ALPHA1, ALPHA2, ALPHA4, AUTO,
)
