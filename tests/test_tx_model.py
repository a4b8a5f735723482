"""CPU model of the GPU modulator's decomposition (csrc/k_tx.hpp, csrc/dvbt_tx.inc), pinned against the oracle's generator.

The GPU builds every OFDM symbol on its own: its info bits are a window of the byte-interleaved stream, gathered straight from the
RS-coded bytes (byte i = rs[i - 204 (i mod 12)]), the encoder's state is the 6 bits in front of the window, and the pilots / TPS
come from per-class carrier tables and a 4 x 68 TPS sign table.  Between calls only the packet and symbol counts and the last
`hist` RS bytes are carried.  This restates that decomposition in numpy -- same windows, same tables, same carried state -- and
checks that it gives the oracle's frequency-domain frames (o_tx_generate_from's freq_taps) bit for bit, in one call and split at
arbitrary packet counts.  The GPU kernels are checked against the same frames in tests/test_gpu_tx.py.
"""
import ctypes as C

import numpy as np
import pytest

OFF = (0, 63, 105, 42, 21, 84)           # bit interleaver H_e(w) = (w + OFF[e]) mod 126
PUNCT = {0: (1, 1), 1: (1, 1, 0, 1), 2: (1, 1, 0, 1, 1, 0), 3: (1, 1, 0, 1, 1, 0, 0, 1, 1, 0),
         4: (1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0)}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- outer coder
def _gf():
    exp, log = np.zeros(512, np.int64), np.zeros(256, np.int64)
    reg = 1
    for i in range(255):
        exp[i] = exp[i + 255] = reg
        log[reg] = i
        reg <<= 1
        if reg & 0x100:
            reg ^= 0x11d
    return exp, log


def _enc_table():
    exp, log = _gf()

    def mul(a, b):
        return 0 if a == 0 or b == 0 else int(exp[log[a] + log[b]])
    g = [1] + [0] * 16
    for i in range(16):
        root = int(exp[i])
        for k in range(16, 0, -1):
            g[k] = g[k - 1] ^ mul(g[k], root)
        g[0] = mul(g[0], root)
    return np.array([[mul(b, g[15 - i]) for i in range(16)] for b in range(256)], np.uint8)


def _prbs():
    seq, reg = np.zeros(1504, np.uint8), 0xa9
    c = 0
    for p in range(8):
        c += 1
        for k in range(188):
            v = 0
            for _ in range(8):
                fb = ((reg >> 13) ^ (reg >> 14)) & 1
                reg = ((reg << 1) | fb) & 0x7fff
                v = (v << 1) | fb
            if k < 187:
                seq[c] = v
                c += 1
    return seq


ENC, PRBS = _enc_table(), _prbs()


def outer(ts, pk0):
    """packets -> RS-coded packets (dispersal phase from the packet's index pk0 + p in the whole TS), all packets at once"""
    pk = ts.reshape(-1, 188).copy()
    g = (pk0 + np.arange(len(pk))) % 8
    pk ^= PRBS.reshape(8, 188)[g]
    pk[:, 0] = np.where(g == 0, 0xB8, 0x47)
    reg = np.zeros((len(pk), 16), np.uint8)
    for k in range(188):
        fb = pk[:, k] ^ reg[:, 0]
        reg = np.concatenate([reg[:, 1:], np.zeros((len(pk), 1), np.uint8)], axis=1) ^ ENC[fb]
    return np.concatenate([pk, reg], axis=1).reshape(-1)


# ---------------------------------------------------------------- per-configuration tables
class Model:
    def __init__(self, po, c, first_packet=0):
        self.c, self.first_packet = c, first_packet
        L = po.lib()
        self.ibits = c.payload * c.m * c.k // c.n
        self.hist = (2244 + self.ibits // 8 + 3 + 15) & ~15
        K = c.Kmax + 1
        wk = np.zeros(K, np.int8)
        L.o_prbs_wk(C.byref(c), _p(wk))
        self.pref = (4 * 2 * (0.5 - wk.astype(np.float64)) / 3).astype(np.float32)
        self.tps = np.array([c.tps[i] for i in range(c.n_tps)])
        cpl = [c.cpilot[i] for i in range(c.n_cpilot)]
        # carrier classes from the generator's own walk (sp wraps at n_spilot + 1 on symbol_index 0, at n_spilot otherwise)
        self.pay, self.pil = [], []
        for cls in range(5):
            si = 0 if cls == 4 else (4 if cls == 0 else cls)
            sp = cpi = tpi = 0
            size = c.n_spilot + (1 if si == 0 else 0)
            pay, pil = [], []
            for k in range(K):
                is_pay, is_pil = True, False
                if k == 3 * (si % 4) + 12 * sp:
                    sp = (sp + 1) % size; is_pil = True; is_pay = False
                if k == cpl[cpi]:
                    cpi = (cpi + 1) % len(cpl); is_pil = True; is_pay = False
                if k == self.tps[tpi]:
                    tpi = (tpi + 1) % len(self.tps); is_pil = False; is_pay = False
                (pil if is_pil else pay if is_pay else []).append(k)
            assert len(pay) == c.payload
            self.pay.append(np.array(pay)); self.pil.append(np.array(pil))
        # TPS sign table: symbol s of frame f carries (-1)^(t_f[1] + ... + t_f[s]) times 2 (0.5 - w_k)
        self.sign = np.zeros((4, 68), np.float32)
        for f in range(4):
            t = np.zeros(68, np.uint8)
            L.o_tps_format(C.byref(c), f, _p(wk), _p(t))
            self.sign[f] = np.where(np.cumsum(np.r_[0, t[1:]]) % 2, -1.0, 1.0)
        self.tps_base = (2 * (0.5 - wk[self.tps].astype(np.float64))).astype(np.float32)
        H = np.zeros(c.payload, np.int32)
        L.o_sym_H(C.byref(c), _p(H))
        self.H, self.Hinv = H, np.argsort(H)
        pts = np.zeros(c.csize, np.complex64)
        L.o_constellation(C.byref(c), C.c_float(1.0), _p(pts))
        self.points = pts
        # coded bit o of a puncture period: (info bit of the period, 0 = x / 1 = y)
        P = PUNCT[c.code_rate]
        self.cmap = [(j, xy) for j in range(c.k) for xy in (0, 1) if P[2 * j + xy]]
        assert len(self.cmap) == c.n
        v = c.m
        self.kinv = [0] * v
        for kk in range(v):
            self.kinv[kk // (v // 2) + 2 * (kk % (v // 2))] = kk
        # which info bit / output each coded bit of a symbol is, and which coded bits every output word of the bit interleaver takes
        cb = np.arange(c.payload * v)
        self.cb_t = (cb // c.n) * c.k + np.array([self.cmap[o][0] for o in range(c.n)])[cb % c.n]
        self.cb_y = np.array([self.cmap[o][1] for o in range(c.n)])[cb % c.n]
        q = np.arange(c.payload)
        blk, wq = q // 126, q % 126
        self.word_cb = np.stack([v * (blk * 126 + (wq + OFF[e]) % 126) + self.kinv[e] for e in range(v)], axis=1)

    def symbol(self, buf, base, sg):
        """frequency-domain frame of stream symbol sg from the RS bytes buf (buf[0] = RS byte `base` of the stream)"""
        c = self.c
        Bg = sg * self.ibits
        gb0 = (Bg >> 3) - 1
        nA = ((Bg + self.ibits - 1) >> 3) - gb0 + 1
        gi = gb0 + np.arange(nA, dtype=np.int64)
        j = gi - 204 * (gi % 12)
        assert (j[(gi >= 0) & (j >= 0)] - base >= 0).all(), "the carried history is too short"
        il = np.where((gi >= 0) & (j >= 0), buf[np.clip(j - base, 0, len(buf) - 1)], 0).astype(np.uint8)
        bits = np.unpackbits(il).astype(np.int64)
        o = (Bg & 7) + 8                                           # index of info bit 0 in bits[]
        t = np.arange(self.ibits)
        b = [bits[o + t - d] for d in range(7)]                    # b[d] = info bit t - d (the encoder's history for t < 6)
        x = b[0] ^ b[1] ^ b[2] ^ b[3] ^ b[6]                       # G1 = 171 (octal)
        y = b[0] ^ b[2] ^ b[3] ^ b[5] ^ b[6]                       # G2 = 133
        coded = np.where(self.cb_y == 1, y[self.cb_t], x[self.cb_t])
        words = np.zeros(c.payload, np.int64)
        for e in range(c.m):
            words = (words << 1) | coded[self.word_cb[:, e]]
        si, fi = sg % 68, (sg // 68) % 4
        lab = np.zeros(c.payload, np.int64)
        lab[self.Hinv if si % 2 else self.H] = words
        cls = 4 if si == 0 else si % 4
        f = np.zeros(c.N, np.complex64)
        f[c.zeros_left + self.pay[cls]] = self.points[lab]
        f[c.zeros_left + self.pil[cls]] = self.pref[self.pil[cls]]
        f[c.zeros_left + self.tps] = self.sign[fi, si] * self.tps_base
        return f

    def run(self, ts, splits):
        """the stream in calls of splits[i] packets: every call's frames, the carried state being (packets, symbols, last hist RS bytes)"""
        hist = np.zeros(self.hist, np.uint8)
        P0 = S0 = 0
        calls = []
        for npk in splits:
            buf = np.concatenate([hist, outer(ts[P0 * 188:(P0 + npk) * 188], self.first_packet + P0)])
            base = P0 * 204 - self.hist
            S1 = (P0 + npk) * 1632 // self.ibits
            calls.append(np.array([self.symbol(buf, base, s) for s in range(S0, S1)]).reshape(-1, self.c.N))
            hist = buf[len(buf) - self.hist:]
            P0, S0 = P0 + npk, S1
        return calls


def _oracle(po, c, ts, first_packet=0):
    _, freq = po.tx(c, ts, scale=1.0, want_freq=True, packet0=first_packet)
    return freq


def test_outer_coder_matches_the_oracle_rs_encoder(po):
    """dispersal + the table-driven RS register == o_energy_dispersal_from + o_rs_encode"""
    L = po.lib()
    ts = po.make_ts(19, 3)
    disp = np.zeros(19 * 188, np.uint8)
    L.o_energy_dispersal_from(_p(ts), _p(disp), C.c_size_t(19), C.c_size_t(5))
    rs = po.RS()
    L.o_rs_init(C.byref(rs))
    want = []
    for p in range(19):
        w = np.zeros(255, np.uint8)
        w[51:239] = disp[p * 188:(p + 1) * 188]
        L.o_rs_encode(C.byref(rs), _p(w), _p(w[239:]))
        want.append(w[51:])
    assert (outer(ts, 5) == np.concatenate(want)).all()


@pytest.mark.parametrize("const,cr,mode,nsf", [
    (0, 2, 0, 2),      # 2k QPSK 3/4: 2268 info bits = 283.5 bytes per symbol
    (1, 0, 0, 2),      # 2k QAM16 1/2
    (2, 4, 1, 2),      # 8k QAM64 7/8
])
def test_per_symbol_model_is_the_generator(po, const, cr, mode, nsf):
    c = po.cfg(const, cr, mode)
    npk = po.packets_per_superframe(c) * nsf + 3
    ts = po.make_ts(npk, 11)
    ref = _oracle(po, c, ts)
    assert len(ref) >= 68 * 4 * nsf // 4
    got = Model(po, c).run(ts, [npk])[0]
    assert got.shape == ref.shape and (got == ref).all()


@pytest.mark.parametrize("const,cr,mode,splits", [
    (0, 2, 0, [1, 7, 13, 200, 1, 90, 300]),
    (2, 4, 1, [1, 7, 500, 2, 750]),
])
def test_carry_across_splits(po, const, cr, mode, splits):
    c = po.cfg(const, cr, mode)
    ts = po.make_ts(sum(splits), 4)
    ref = _oracle(po, c, ts)
    m = Model(po, c)
    calls = m.run(ts, splits)
    S = 0
    for npk, got in zip(np.cumsum(splits), calls):
        assert len(got) == npk * 1632 // m.ibits - S
        S += len(got)
    assert (np.concatenate(calls) == ref).all()


def test_first_packet_and_cell_id(po):
    c = po.cfg(1, 3, 0, guard=po.G1_4, hierarchy=2, include_cell_id=1, cell_id=0x5a)
    npk = po.packets_per_superframe(c) + 50
    ts = po.make_ts(npk, 9)
    ref = _oracle(po, c, ts, first_packet=13)
    calls = Model(po, c, first_packet=13).run(ts, [40, 1, npk - 41])
    assert (np.concatenate(calls) == ref).all()


def test_tps_sign_table_is_dbpsk_of_the_tps_word(po):
    """the 4 x 68 sign table against the generator's running DBPSK value on the TPS carriers"""
    c = po.cfg(2, 4, 1, include_cell_id=1, cell_id=0x3c)
    m = Model(po, c)
    npk = po.packets_per_superframe(c)
    ref = _oracle(po, c, po.make_ts(npk, 1))
    assert len(ref) == 4 * 68
    tps = ref[:, c.zeros_left + m.tps].real
    assert (tps == m.sign.reshape(-1, 1) * m.tps_base).all()
