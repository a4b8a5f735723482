"""One copy of the comparisons with the REFERENCE's recordings (tests/golden/ref_blocks.json / .npz, cases of oracle/ref_cases.py), for the two things that are held
to them: the per-block C-ABI entries (gr_dvbt_amd.Block; tests/test_gpu_ref_blocks.py) and the GNU Radio block shells on top of them (oracle/_ref/libdvbt_shells_hip.so;
tests/test_gpu_gr_shells.py).  A case function takes a factory mk(name, *args) -- the arguments of gr_dvbt_amd.Block -- whose blocks offer
    forecast(noutput) -> [items required per input]
    work(noutput, nvisible, x, outs, tags) -> (returned, consumed, [(rel_offset, key id, value)]);  x: the visible input bytes, outs: one uint8 array per output
    hints(noutputs), close()
drives the block in the recorded calls with the recorded input tags, asserts the recorded result -- integer outputs by SHA-256, items produced and consumed per call and
the output tags exactly; the demodulator's equalised carriers within the EQ-tap contract |d| <= 1e-3 * 2 * d_norm per component, the mapper's points and
reference_signals' cells within 1e-5 of the peak (no tolerance is new) -- and returns the output bytes.

The hierarchical 64-QAM LP bytes that the reference reads from behind its matrix are excluded (ref_cases.lp_undefined_mask).  Reed-Solomon: the reference as compiled
is the decoder's oracle_compat = 1 (SURVEY B-1); a factory with rs_compat = 1 builds that decoder and must give the recorded bytes.  A shell's make() has no such
argument and builds the correct decoder: its words are held to the recording through what B-1 states and DESIGN 7 (2) measured -- in a word that is corrected, the
as-compiled reference leaves the byte at the lowest error location as received, and nothing else differs (rs_as_compiled)."""
import ctypes as C

import numpy as np

from oracle import ref_cases as rc
from oracle import refblocks as rb

KEYS = {"sync_start": 1, "superframe_start": 2, "symbol_index": 3}
NAMES = {v: k for k, v in KEYS.items()}
SHELL_NAMES = {"demap": "dvbt_demap", "map": "dvbt_map", "fft": "fft_hip"}                # C-ABI stem -> class name, where they differ


class AbiBlock:
    """gr_dvbt_amd.Block"""

    def __init__(self, g, name, *args):
        self.g, self.name, self.b = g, name, g.Block(name, *args)

    def forecast(self, n):
        return [self.b.forecast(n)]

    def work(self, n, vis, x, outs, tags=()):
        if len(outs) == 1:
            return self.b.work(n, vis, x, outs[0], tags)
        assert self.name == "bit_inner_deinterleaver" and not tags                      # the one block with a second output
        L = self.g.lib()
        L.dvbt_bit_inner_deinterleaver_work_hier.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(self.g.Sideband)]
        tout = (self.g.Tag * 16)()
        sb = self.g.Sideband(None, 0, tout, 16, 0, 0)
        r = L.dvbt_bit_inner_deinterleaver_work_hier(self.b.h, n, vis, x.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data, C.byref(sb))
        assert r >= 0 and sb.n_out_tags == 0, (r, L.dvbt_last_error())
        return r, sb.n_consumed, []

    def close(self):
        self.b.close()


def abi_factory(g, rs_compat=1):
    def mk(name, *args):
        if name == "reed_solomon_dec":
            args = tuple(args) + (rs_compat,)
        return AbiBlock(g, name, *args)
    mk.rs_compat = rs_compat
    return mk


class ShellBlock:
    """a GNU Radio block shell in oracle/_ref/libdvbt_shells_hip.so, made through its make(): input tags go in as gr::tag_t at absolute offsets, output tags come back
    from add_item_tag, consumed from consume_each; the driver advances nitems_read / nitems_written as a scheduler would"""

    def __init__(self, name, *args):
        args, gain = list(args), 0.0
        if args and isinstance(args[-1], float):
            gain = args.pop()
        self.b = rb.Block(SHELL_NAMES.get(name, name), args, gain, nin=1, nout=2, which="hip")
        self.max_out = self.b.nout                                                     # the outputs the shell declares
        self.given, self.ntags = set(), 0

    def forecast(self, n):
        return self.b.forecast(n)

    def hints(self, noutputs):
        return self.b.hints(noutputs)

    def work(self, n, vis, x, outs, tags=()):
        b = self.b
        assert len(outs) <= self.max_out
        b.nout = len(outs)
        r0, w0 = b.nitems_read(), b.L.refblk_nitems_written(b.h, 0)
        for off, key, val in tags:                                                     # a tag that two overlapping windows show is still one gr::tag_t
            t = (r0 + off, key, val)
            if t not in self.given:
                self.given.add(t)
                b.tag(r0 + off, NAMES[key], val)
        x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        r, cons, o = b.work(n, [x if len(x) else np.zeros(8, np.uint8)], vis)
        for dst, src in zip(outs, o):
            assert len(src) <= len(dst)
            dst[:len(src)] = src
        new = b.out_tags()[self.ntags:]
        self.ntags += len(new)
        assert all(port == 0 for port, _, _, _ in new)
        return r, cons[0], [(off - w0, KEYS[key], val) for _, off, key, val in new]

    def close(self):
        self.b.close()


def shell_factory():
    def mk(name, *args):
        return ShellBlock(name, *args)
    mk.rs_compat = 0                                                                    # reed_solomon_dec::make has no such argument: the correct decoder
    return mk


# ------------------------------------------------------------------------------------------------------------------------------------------
def drive(b, x, in_item, out_item, calls, in_tags=(), visible=None, nout=1):
    """the recorded calls [noutput, returned, consumed] on the block: every call sees `visible(noutput)` input items (default: what its forecast asks for) from where
    the last one stopped and the input tags that fall among them; returns ([output bytes per port], [[noutput, returned, consumed]], [[0, absolute offset, key, value]])"""
    x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    total = len(x) // in_item
    pos, written, outs, log, tags = 0, 0, [[] for _ in range(nout)], [], []
    for n, _, _ in calls:
        vis = min(visible(n) if visible else max(b.forecast(n)), total - pos)
        tin = [(t - pos, KEYS[k], v) for t, k, v in in_tags if pos <= t < pos + vis]
        out = [np.full(n * out_item, 0xee if j else 0, np.uint8) for j in range(nout)]
        r, cons, tout = b.work(n, vis, x[pos * in_item:(pos + vis) * in_item], out, tin)
        log.append([n, r, cons])
        tags += [[0, written + off, NAMES[key], val] for off, key, val in tout]
        for j in range(nout):
            outs[j].append(out[j][:r * out_item])
        pos += cons
        written += r
    b.close()
    return [np.concatenate(o) if o else np.zeros(0, np.uint8) for o in outs], log, tags


def check(want, outs, log, tags):
    assert log == rc.unrle(want["log"])
    assert tags == rc.unrle(want["tags"])
    for port, out in enumerate(outs):
        assert len(out) == want["nbytes"][port] and rc.sha(out) == want["sha256"][port], "output %d" % port


def rs_as_compiled(out, inp):
    """the correct decoder's words as the as-compiled reference leaves them (SURVEY B-1): in a word with 1 .. 8 symbol errors, the lowest of them among
    the 188 data bytes, that byte stays as received.  Asserts on the way that every such word was corrected to what was sent and every other one passed through."""
    w = out.reshape(-1, 188).copy()
    recv = inp["in"][0].reshape(-1, 204)
    for i, pos in enumerate(inp["errpos"][:len(w)]):
        if len(pos) <= 8:
            assert (w[i] == inp["sent"][i, :188]).all(), "word %d with %d errors not corrected" % (i, len(pos))
            if pos and pos[0] < 188:
                w[i, pos[0]] = recv[i, pos[0]]
        else:
            assert (w[i] == recv[i, :188]).all(), "word %d beyond the code not passed through" % i
    return w.reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# one function per kind of case: (po, mk, golden, name) -> [output bytes per port]
# ------------------------------------------------------------------------------------------------------------------------------------------
def _setup(po, golden, name):
    case, want = rc.CASES[name], golden[0]["cases"][name]
    return case, want, rc.make_input(po, case), rc.unrle(want["log"])


def case_sym(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    P = rc.P8K if case["mode"] else rc.P2K
    b = mk("symbol_inner_interleaver", P, case["mode"], case["direction"])
    tags = [(i, "symbol_index", s) for i, s in enumerate(case["indices"])]
    r = drive(b, inp["in"][0], P, P, calls, tags)
    check(want, *r)
    return r[0]


def case_bit(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    if case["kind"] == "bitint" or case["hier"] == 0:
        b = mk("bit_inner_interleaver" if case["kind"] == "bitint" else "bit_inner_deinterleaver", rc.P2K, case["const"], 0, 0)
        r = drive(b, inp["in"][0], rc.P2K, rc.P2K, calls)
        check(want, *r)
        return r[0]
    b = mk("bit_inner_deinterleaver", rc.P2K, case["const"], case["hier"], 0)
    outs, log, tags = drive(b, inp["in"][0], rc.P2K, rc.P2K, calls, nout=2)              # both outputs, in the recorded calls
    outs[1] = rc._mask_lp(case, outs[1])
    check(want, outs, log, tags)
    return outs


def case_vit(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    b = mk("viterbi_decoder", case["const"], 0, case["rate"], 768, 0, -1)
    tags = [(t, "superframe_start", 0xaa) for t in inp["tags"]]
    r = drive(b, inp["in"][0], 1, 1, calls, tags)
    check(want, *r)
    return r[0]


def case_conv(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    if case["kind"] == "convint":
        r = drive(mk("convolutional_interleaver", 136, 12, 17), inp["in"][0], 1632, 1, calls)
    else:
        tags = [(t, "superframe_start", 1) for t in case["tags"]]
        r = drive(mk("convolutional_deinterleaver", 136, 12, 17), inp["in"][0], 1, 1632, calls, tags)
    check(want, *r)
    return r[0]


def case_rs(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    if name == "rs_enc":
        r = drive(mk("reed_solomon_enc", *rc.RS_ARGS), inp["in"][0], 8 * 188, 8 * 204, calls)
        check(want, *r)
        return r[0]
    outs, log, tags = drive(mk("reed_solomon_dec", *rc.RS_ARGS), inp["in"][0], 8 * 204, 8 * 188, calls)
    if mk.rs_compat:                                                                    # the decoder as the reference is compiled
        check(want, outs, log, tags)
    else:
        check(want, [rs_as_compiled(outs[0], inp)], log, tags)
    return outs


def case_disp_coder(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    if case["kind"] == "disp":
        # every byte that is left is visible: behind a sync byte at offset i the reference reads i + 1504 bytes whatever ninput_items says (its forecast
        # promises 1512), the GPU block takes an item only when it has been given all of it
        r = drive(mk("energy_dispersal", 1), inp["in"][0], 1, 1504, calls, visible=lambda n: 1 << 30)
    else:
        r = drive(mk("inner_coder", 1, rc.P2K, case["const"], case["hier"], case["rate"]), inp["in"][0], 1, rc.P2K, calls)
    check(want, *r)
    return r[0]


def case_descr(po, mk, golden, name):
    """in the recorded regime: the smallest call, 4 items visible (output 0 of the recording; output 1 is the reference in larger calls)"""
    case, want, inp, calls = _setup(po, golden, name)
    r = drive(mk("energy_descramble", 8), inp["in"][0], 1504, 1, calls, visible=lambda n: 4)
    check(want, *r)
    return r[0]


def case_map_demap(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    if case["kind"] == "demap":
        r = drive(mk("demap", rc.P2K, case["const"], case["hier"], 0, 1.0), inp["in"][0], 8 * rc.P2K, rc.P2K, calls)
        check(want, *r)
        return r[0]
    (out,), log, tags = drive(mk("map", rc.P2K, case["const"], case["hier"], 0, 1.0), inp["in"][0], rc.P2K, 8 * rc.P2K, calls)
    assert log == calls and tags == [] and len(out) == want["nbytes"][0]
    got = out.view(np.complex64)
    ref = rc.run_oracle(po, case, inp)["out"][0]
    assert rc.sha(ref) == want["sha256"][0]                                            # the oracle's points are the reference's, bit for bit
    for key, (off, nbytes) in want["kept"].items():
        kept = golden[1][key]
        assert (ref[off:off + nbytes].view(np.complex64) == kept).all()
        assert np.abs(got[off // 8:(off + nbytes) // 8] - kept).max() <= 1e-5 * np.abs(kept).max()
    ref = ref.view(np.complex64)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    return [out]


def demod_args(case, c):
    return (8, c.N, c.payload, case["const"], 0, case["rate"], case["rate"], 0, case["mode"], 0, 0)


def case_demod(po, mk, golden, name):
    case, want, inp, calls = _setup(po, golden, name)
    c = inp["cfg"]
    tags = [(t, "sync_start", 1) for t in case["sync"]]
    (out,), log, otags = drive(mk("demod_reference_signals", *demod_args(case, c)), inp["in"][0], 8 * c.N, 8 * c.payload, calls, tags, visible=lambda n: 2 * n)
    assert log == calls
    assert otags == rc.unrle(want["tags"])
    assert len(out) == want["nbytes"][0] > 0
    got = out.view(np.complex64)
    tol = 1e-3 * 2 * c.norm                                                            # the EQ-tap contract, DESIGN 7
    for key, (off, nbytes) in want.get("kept", {}).items():                            # the reference's recorded values
        d = got[off // 8:(off + nbytes) // 8] - golden[1][key]
        assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= tol
    ref = rc.run_oracle(po, case, inp)["out"][0]
    assert rc.sha(ref) == want["sha256"][0]                                            # the reference's bits, all items
    d = got - ref.view(np.complex64)
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= tol
    return [out]


def refsig_args(case, c):
    cell = case.get("cell", (0, 0))
    return (8, c.payload, c.N, case["const"], 0, case["rate"], case["rate"], 0, case["mode"], cell[0], cell[1])


def case_refsig(po, mk, golden, name):
    """reference_signals over the payload the reference block was given: the generator's payload cells in the generator's order (the reference put them where
    the generator had them: the recording is the generator's symbols, bit for bit)"""
    case, want, inp, calls = _setup(po, golden, name)
    c = inp["cfg"]
    F = inp["F"]
    assert rc.sha(np.ascontiguousarray(F[:want["nbytes"][0] // (8 * c.N)]).reshape(-1).view(np.uint8)) == want["sha256"][0]
    # payload cells of a symbol: every carrier that is no pilot and no TPS cell, in rising order -- read off a run of the block itself over numbered cells
    args = refsig_args(case, c)
    n = inp["nitems"]
    mark = np.zeros((n, c.payload), np.complex64)
    mark.real = 1000 + np.arange(c.payload)
    mark.imag = 7
    (numbered,), _, _ = drive(mk("reference_signals", *args), mark, 8 * c.payload, 8 * c.N, [[n, n, n]])
    numbered = numbered.view(np.complex64).reshape(n, c.N)
    pos = np.stack([np.flatnonzero(numbered[s].imag == 7) for s in range(n)])
    assert pos.shape == (n, c.payload)
    pay = np.take_along_axis(F, pos, axis=1)
    (out,), log, tags = drive(mk("reference_signals", *args), pay, 8 * c.payload, 8 * c.N, calls)
    assert log == calls and tags == [] and len(out) == want["nbytes"][0]
    got = out.view(np.complex64)
    ref = np.ascontiguousarray(F[:len(got) // c.N]).reshape(-1)
    peak = np.abs(ref).max()
    for key, (off, nbytes) in want.get("kept", {}).items():
        assert np.abs(got[off // 8:(off + nbytes) // 8] - golden[1][key]).max() <= 1e-5 * peak
    assert np.abs(got - ref).max() <= 1e-5 * peak
    return [out]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the chain cases: the receive blocks from demod_reference_signals to energy_descramble, each in its smallest calls, tags handed on by hand (ref_cases.run_ref)
# ------------------------------------------------------------------------------------------------------------------------------------------
def stream(b, x, in_item, out_item, nitems, calls, in_tags=(), visible=None, pad_items=4):
    """refblocks.Block.stream on a factory's block: call after call with noutput_items from `calls` (the last entry repeats), each exposing what the block's
    forecast asks for (or `visible` items), until the input left is less than that.  returns (output bytes, [[noutput, returned, consumed]], [[0, offset, key, value]])"""
    x = np.concatenate([np.ascontiguousarray(x).view(np.uint8).reshape(-1), np.zeros(pad_items * in_item, np.uint8)])
    pos, written, outs, log, tags, ci = 0, 0, [], [], [], 0
    while True:
        n = calls[min(ci, len(calls) - 1)]
        need = max(b.forecast(n)) if visible is None else visible
        if pos + need > nitems:
            break
        tin = [(t - pos, KEYS[k], v) for t, k, v in in_tags if pos <= t < pos + need]
        out = np.zeros(n * out_item, np.uint8)
        r, cons, tout = b.work(n, need, x[pos * in_item:(pos + need) * in_item], [out], tin)
        log.append([n, r, cons])
        tags += [[0, written + off, NAMES[key], val] for off, key, val in tout]
        outs.append(out[:max(r, 0) * out_item])
        pos += cons
        written += max(r, 0)
        ci += 1
        if r <= 0 and cons == 0:
            break
    b.close()
    return (np.concatenate(outs) if outs else np.zeros(0, np.uint8)), log, tags


def case_chain(po, mk, golden, name):
    """every integer tap by SHA-256 and the tags exactly; the equalised carriers (a float tap) within the EQ-tap contract of the oracle's, whose bits are the recorded ones"""
    case, want = rc.CASES[name], golden[0]["cases"][name]
    inp = rc.make_input(po, case)
    c, o = inp["cfg"], inp["rx"]
    P, m = c.payload, case["mode"]
    sync = [(int(j), "sync_start", 1) for j in np.flatnonzero(o["sync_flag"])]
    eq, _, eqt = stream(mk("demod_reference_signals", 8, c.N, P, case["const"], 0, case["rate"], case["rate"], 0, m, 0, 0), o["fft"], 8 * c.N, 8 * P, inp["nitems"], [1], sync)
    n = len(eq) // (8 * P)
    demap, _, _ = stream(mk("demap", P, case["const"], 0, m, 1.0), eq, 8 * P, P, n, [1])
    symd, _, _ = stream(mk("symbol_inner_interleaver", P, m, 0), demap, P, P, n, [1], [(off, key, val) for _, off, key, val in eqt if key == "symbol_index"])
    bitd, _, _ = stream(mk("bit_inner_deinterleaver", P, case["const"], 0, m), symd, P, P, n, [1])
    # the superframe_start tag travels with its item through the three 1:1 blocks
    vit, _, vitt = stream(mk("viterbi_decoder", case["const"], 0, case["rate"], 768, 0, 0), bitd, 1, 1, n * P, [768 * c.k // 8],
                          [(off * P, key, val) for _, off, key, val in eqt if key == "superframe_start"])
    dei, deil, _ = stream(mk("convolutional_deinterleaver", 136, 12, 17), vit, 1, 1632, len(vit), [2], [(off, key, val) for _, off, key, val in vitt])
    rs, _, _ = stream(mk("reed_solomon_dec", *rc.RS_ARGS), dei, 8 * 204, 8 * 188, len(dei) // 1632, [1])
    ts, _, _ = stream(mk("energy_descramble", 1), rs, 1504, 1, len(rs) // 1504, [4 * 1504], visible=4)
    outs = [eq, demap, symd, bitd, vit, dei, rs, ts]
    pos, kept = 0, []                                                                   # the Viterbi tap without the bytes the byte de-interleaver drops in front of a tag
    for _, r, cons in deil:
        if r > 0:
            kept.append(vit[pos:pos + cons])
        pos += cons
    outs[4] = np.concatenate(kept + [vit[pos:]])
    assert eqt[:1] + vitt == rc.unrle(want["tags"])
    ref = np.ascontiguousarray(o["eq"]).reshape(-1).view(np.uint8)
    assert rc.sha(ref) == want["sha256"][0]                                            # the oracle's equalised carriers are the reference's, bit for bit
    assert len(eq) == want["nbytes"][0] > 0
    d = eq.view(np.complex64) - ref.view(np.complex64)
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= 1e-3 * 2 * c.norm         # the EQ-tap contract, DESIGN 7
    for j in range(1, 8):
        assert len(outs[j]) == want["nbytes"][j] > 0 and rc.sha(outs[j]) == want["sha256"][j], rc.CHAIN_TAPS[j]
    return outs


CASE_FN = {"sym": case_sym, "bitdeint": case_bit, "bitint": case_bit, "vit": case_vit, "convint": case_conv, "convdeint": case_conv, "rsenc": case_rs, "rsdec": case_rs,
           "disp": case_disp_coder, "coder": case_disp_coder, "descr": case_descr, "demap": case_map_demap, "map": case_map_demap, "demod": case_demod,
           "refsig": case_refsig, "chain": case_chain}


def run_case(po, mk, golden, name):
    return CASE_FN[rc.CASES[name]["kind"]](po, mk, golden, name)
