"""The loopback cases of the signal-quality tests (tests/test_quality_model.py, tests/test_gpu_quality.py, tests/golden/make_quality_golden.py):
seeded stream, seeded noise; the receiver is told the same SNR."""
import numpy as np

# (name, constellation, code rate, mode, superframes, SNR dB or None)
CASES = [
    ("2k_qam16_1_2_4sf_clean", 1, 0, 0, 4, None),
    ("2k_qam16_1_2_4sf_12dB", 1, 0, 0, 4, 12.0),
    ("2k_qam64_7_8_4sf_24dB", 2, 4, 0, 4, 24.0),
    ("8k_qam64_3_4_1sf_19dB", 2, 2, 1, 1, 19.0),
    ("2k_qam16_1_2_4sf_9dB", 1, 0, 0, 4, 9.0),
]
ONE_PERIOD = [c[0] for c in CASES[:4]]
STREAM_SEED = 9
NOISE_SEED = 5
CLEAN_RX_SNR = 30.0          # what the receiver is told where no noise is added (its default)


def case(name):
    return next(c for c in CASES if c[0] == name)


def rx_snr(c):
    return CLEAN_RX_SNR if c[5] is None else c[5]


def make_iq(po, c):
    """(oracle configuration, complex64 baseband) of a case"""
    cfg = po.cfg(c[1], c[2], c[3])
    iq = po.stream_slice(cfg, c[4], STREAM_SEED)
    if c[5] is not None:
        iq = po.channel(iq, cfg.N, snr_db=c[5], seed=NOISE_SEED)
    return cfg, np.ascontiguousarray(iq, dtype=np.complex64)
