"""Model of the constellation analyser (numpy only): the specification of dvbt_constellation_* as include/dvbt_hip.h states it.  Every step of the per-axis
arithmetic is one float32 operation (numpy rounds each to nearest), everything behind the quantisation is int64: the device must give these very integers.

analyse(cells, constellation, hierarchy) takes rows [n][P] complex64 and returns a gr_dvbt_amd.ConstellationReading built from plain arrays.
contract=True is the variant the definition forbids: the product a inv_d fused into the subtraction that follows it, fma(a, inv_d, -c) in step 5 and
fma(a, inv_d, -level) in step 8, i.e. the difference formed from the unrounded product (exact in float64: 24 x 24 bits) and rounded once.
"""
import numpy as np

G = 128
STEP = 4096.0
S_OF = {(0, 1): 2, (1, 1): 10, (2, 1): 42, (1, 2): 20, (2, 2): 60, (1, 4): 52, (2, 4): 108}
GRIDS = [(0, 0), (1, 0), (2, 0), (1, 2), (2, 2), (1, 3), (2, 3)]          # (constellation, hierarchy): the seven grids (hierarchy 1 is alpha 1 again)
ALPHA = (1, 1, 2, 4)

f32 = np.float32


def grid(constellation, hierarchy=0):
    """(L, H, alpha, S, inv_d)"""
    L = (2, 4, 8)[constellation]
    alpha = ALPHA[hierarchy]
    assert constellation or hierarchy == 0
    S = 2
    while S < alpha + L - 1:
        S *= 2
    return L, L // 2, alpha, S, f32(np.sqrt(np.float64(S_OF[(constellation, alpha)])))


def ideal_cells(constellation, hierarchy=0):
    """the L^2 ideal points as complex64 cells (level * d in float32, d = 1 / inv_d rounded as the tables' norm), point p = row L + col"""
    L, H, alpha, S, inv_d = grid(constellation, hierarchy)
    d = f32(1.0 / np.sqrt(np.float64(S_OF[(constellation, alpha)])))
    i = np.arange(L)
    ax = np.where(i >= H, alpha + 2 * (i - H), -(alpha + 2 * (H - 1 - i))).astype(np.float32) * d
    return (np.tile(ax, L) + 1j * np.repeat(ax, L)).astype(np.complex64)


def axis(x, constellation, hierarchy=0, contract=False):
    """one component: (neg, nonfinite, u, j, level, q before the sign, clipped, q, index, bin)"""
    L, H, alpha, S, inv_d = grid(constellation, hierarchy)
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32)
    neg = (bits >> np.uint32(31)) != 0
    nonfinite = (bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (bits & np.uint32(0x7fffffff)).view(np.float32)
        u = a * inv_d
        if contract:
            prod = a.astype(np.float64) * np.float64(inv_d)                  # the product a fused operation keeps unrounded
            t = (prod - (alpha - 1)).astype(np.float32) * f32(0.5)
        else:
            t = (u - f32(alpha - 1)) * f32(0.5)
        tj = np.where(nonfinite, f32(0), t)
        j = np.where(tj < 1, 0, np.where(tj >= H, H - 1, np.minimum(tj, f32(H)).astype(np.int64))).astype(np.int64)
        level = alpha + 2 * j
        if contract:
            r = np.rint((prod - level).astype(np.float32) * f32(4096.0))
        else:
            dl = u - level.astype(np.float32)
            r = np.rint(dl * f32(4096.0))
        r = np.where(nonfinite, f32(0), r)
        clipped = np.abs(r) > f32(32767.0)
        q0 = np.minimum(np.maximum(r, f32(-32767.0)), f32(32767.0)).astype(np.int64)
        q = np.where(neg, -q0, q0)
        idx = np.where(neg, H - 1 - j, H + j)
        e = np.where(neg, -u, u)
        e = np.where(nonfinite, f32(0), e)
        b = np.minimum(np.maximum(np.floor(e * f32(G // (2 * S))), f32(-G // 2)), f32(G // 2 - 1)).astype(np.int64) + G // 2
    return dict(neg=neg, nonfinite=nonfinite, u=u, j=j, level=level, clipped=clipped, q=q, idx=idx, bin=b)


def sums(cells, constellation, hierarchy=0, contract=False):
    """(hist [G][G] uint64, points, carriers, totals dict) of rows [n][P]"""
    import gr_dvbt_amd as g
    cells = np.ascontiguousarray(cells, dtype=np.complex64)
    assert cells.ndim == 2
    n, P = cells.shape
    L = grid(constellation, hierarchy)[0]
    x = axis(cells.real.reshape(-1), constellation, hierarchy, contract)
    y = axis(cells.imag.reshape(-1), constellation, hierarchy, contract)
    ok = ~(x["nonfinite"] | y["nonfinite"])
    col = np.tile(np.arange(P), n)[ok]
    qx, qy, lx, ly = x["q"][ok], y["q"][ok], x["level"][ok], y["level"][ok]
    p = y["idx"][ok] * L + x["idx"][ok]
    hist = np.bincount(y["bin"][ok] * G + x["bin"][ok], minlength=G * G).astype(np.uint64).reshape(G, G)
    points = np.zeros(L * L, g.POINT_DTYPE)
    carriers = np.zeros(P, g.CARRIER_DTYPE)

    def isum(index, values, size):
        out = np.zeros(size, np.int64)
        np.add.at(out, index, values)
        return out
    points["n"] = np.bincount(p, minlength=L * L)
    for name, v in (("sum_re", qx), ("sum_im", qy), ("sum_re_im", qx * qy), ("sum_re2", qx * qx), ("sum_im2", qy * qy)):
        points[name] = isum(p, v, L * L)
    carriers["n"] = np.bincount(col, minlength=P)
    carriers["signal"] = isum(col, lx * lx + ly * ly, P)
    carriers["error"] = isum(col, qx * qx + qy * qy, P)
    totals = dict(rows_pushed=n, cells=n * P, nonfinite=int((~ok).sum()), clipped=int(((x["clipped"] | y["clipped"]) & ok).sum()))
    return hist, points, carriers, totals


def analyse(cells, constellation, hierarchy=0, contract=False):
    import gr_dvbt_amd as g
    L, H, alpha, S, _ = grid(constellation, hierarchy)
    hist, points, carriers, t = sums(cells, constellation, hierarchy, contract)
    return g.ConstellationReading(hist, points, carriers, t["rows_pushed"], t["cells"], t["nonfinite"], t["clipped"], L, alpha, S)


def bits_of(r):
    """everything a reading holds, as comparable bytes and integers"""
    return (r.hist.tobytes(), r.points.tobytes(), r.carriers.tobytes(), r.rows_pushed, r.cells, r.nonfinite, r.clipped, r.levels, r.alpha, r.span)


def special_cells(constellation, hierarchy=0):
    """cells on every decision boundary, on histogram bin edges, at +-0.0, denormals, 1e30 and the non-finite values, each on either axis, as complex64"""
    L, H, alpha, S, inv_d = grid(constellation, hierarchy)
    d = np.float64(1.0) / np.float64(inv_d)
    vals = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan, 9.0 / float(inv_d), -9.0 / float(inv_d)]
    for j in range(1, H):                                                  # the boundary between levels j - 1 and j: u = alpha - 1 + 2 j
        b = f32((alpha - 1 + 2 * j) * d)
        vals += [b, np.nextafter(b, f32(0)), np.nextafter(b, f32(100)), -b, -np.nextafter(b, f32(0))]
    for k in (-G // 2, -1, 1, 3, G // 2 - 1, G // 2):                       # bin edges: u = k 2 S / G
        b = f32(k * 2.0 * S / G * d)
        vals += [b, np.nextafter(b, f32(0)), np.nextafter(b, f32(100) * np.sign(b))]
    v = np.array(vals, np.float32)
    re, im = np.meshgrid(v, v)
    out = np.empty(re.size, np.complex64)
    out.real, out.imag = re.reshape(-1), im.reshape(-1)
    return out


_streams = {}


def stream(constellation, hierarchy, nrows, P, seed=1, snr_db=15.0, specials=True):
    """rows [nrows][P] complex64: random points plus Gaussian error at snr_db (relative to the constellation's unit mean power) in float32, with the special
    cells mixed in at fixed places.  Computed once per key and left unchanged."""
    key = (constellation, hierarchy, nrows, P, seed, snr_db, specials)
    if key not in _streams:
        rng = np.random.RandomState(1000 * seed + 10 * constellation + hierarchy)
        pts = ideal_cells(constellation, hierarchy)
        n = nrows * P
        sigma = np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
        cells = pts[rng.randint(0, len(pts), n)] + (sigma * (rng.randn(n) + 1j * rng.randn(n))).astype(np.complex64)
        cells = cells.astype(np.complex64)
        if specials and n:
            sp = special_cells(constellation, hierarchy)
            at = rng.permutation(n)[:min(len(sp), n)]
            cells[at] = sp[:len(at)]
        cells = cells.reshape(nrows, P)
        cells.setflags(write=False)
        _streams[key] = cells
    return _streams[key]
