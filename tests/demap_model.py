"""The definition of include/psk_soft_hip.h, "frames as soft bits", restated in numpy: float32 throughout, every operation rounded
once (numpy rounds each elementwise operation; nothing here can fuse), the first-minimum rule as a loop over k, rint and the
clamp, the one NaN of the float32 form, the piece / lane / tree / wave / piece summation order in float64, the splice of the
symbols in front of a row.  The tests hold psk_soft_demap_host and the device to it byte for byte."""
import numpy as np

F32 = np.float32
RECORD_BYTES, IN_BYTES = 64, 64
PIECE, THREADS, WAVE = 1024, 256, 64
FRONT_SYMBOLS = 127
I8, FRONT = 1, 2
DATA, REC_I8, PLANNED = 1, 2, 128
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(F32)[0]

RECORD_DTYPE = np.dtype([("n_symbols", "<u8"), ("n_finite", "<u8"), ("n_clip", "<u8"), ("n_nan", "<u8"), ("sum_e", "<f8"),
                         ("sum_err", "<f8"), ("bits", "<u4"), ("flags", "<u4"), ("pad", "<u4", (2,))])
assert RECORD_DTYPE.itemsize == RECORD_BYTES


def bits_of(M):
    return {2: 1, 4: 2, 8: 3}[M]


def segment_symbols(soft, pos, count, front=None):
    """the (count, 2) float32 symbols pos .. pos + count - 1 of the row; positions below 0 come from `front` (254 floats: the 127
    symbols in front of the row), zeros if it is None"""
    x = np.ascontiguousarray(soft, F32).reshape(-1, 2)
    assert pos >= -FRONT_SYMBOLS and pos + count <= len(x)
    fr = np.zeros((FRONT_SYMBOLS, 2), F32) if front is None else np.ascontiguousarray(front, F32).reshape(FRONT_SYMBOLS, 2)
    full = np.concatenate([fr, x])  # full[127 + g] = x[g]
    return full[FRONT_SYMBOLS + pos: FRONT_SYMBOLS + pos + count]


def first_min(ds):
    """the FIRST minimum of the arrays ds, in their order: a later one must compare less (a NaN in the first stays)"""
    m = ds[0].copy()
    for d in ds[1:]:
        m = np.where(d < m, d, m)
    return m


def symbol_terms(points, labels, x, gain, scale):
    """(e, dmin, v (count, B), finite) of the symbols x (count, 2), all float32"""
    p = np.ascontiguousarray(points, F32).reshape(-1, 2)
    M, B = len(p), bits_of(len(p))
    gr, gi, s = F32(gain[0]), F32(gain[1]), F32(scale)
    xr, xi = x[:, 0], x[:, 1]
    with np.errstate(all="ignore"):
        yr = xr * gr - xi * gi
        yi = xr * gi + xi * gr
        e = yr * yr + yi * yi
        d = []
        for k in range(M):
            dr, di = yr - p[k, 0], yi - p[k, 1]
            d.append(dr * dr + di * di)
        dmin = first_min(d)
        v = np.empty((len(x), B), F32)
        for j in range(B):
            one = [d[k] for k in range(M) if (int(labels[k]) >> (B - 1 - j)) & 1]
            zero = [d[k] for k in range(M) if not (int(labels[k]) >> (B - 1 - j)) & 1]
            v[:, j] = (first_min(one) - first_min(zero)) * s
    assert all(a.dtype == F32 for a in (yr, yi, e, dmin, v))
    finite = np.isfinite(yr) & np.isfinite(yi) & np.isfinite(e) & np.isfinite(dmin)
    return e, dmin, v, finite


def to_i8(v):
    """(the int8 values, how many the clamp changed): rint (ties to even), clamped to -127 .. 127, a NaN as 0"""
    with np.errstate(all="ignore"):
        r = np.rint(v)
    nan = np.isnan(r)
    clipped = ~nan & ((r > 127) | (r < -127))
    r = np.where(nan, F32(0), np.clip(r, -127, 127))
    return r.astype(np.int8), int(clipped.sum())


def ordered_sum(terms, finite):
    """the float64 sum of the float32 terms of the finite symbols in the record's order: pieces of 1024; lane t of 256 its symbols
    t, t + 256, t + 512, t + 768 from 0.0; a xor tree across each wave, offsets 32 .. 1; the four waves in order from wave 0's
    value; the pieces in ascending order from piece 0's"""
    t = np.where(finite, terms, F32(0)).astype(np.float64)
    lanes_of = np.arange(WAVE)
    total = None
    for lo in range(0, len(t), PIECE):
        piece = np.zeros(PIECE)
        piece[: min(PIECE, len(t) - lo)] = t[lo: lo + PIECE]
        lanes = np.zeros(THREADS)
        for turn in range(PIECE // THREADS):
            lanes = lanes + piece[turn * THREADS: (turn + 1) * THREADS]
        w = lanes.reshape(THREADS // WAVE, WAVE)
        off = WAVE // 2
        while off >= 1:
            w = w + w[:, lanes_of ^ off]
            off //= 2
        s = w[0, 0]
        for k in range(1, THREADS // WAVE):
            s = s + w[k, 0]
        total = s if total is None else total + s
    return 0.0 if total is None else total


def model_segment(points, labels, soft, pos, count, gain, scale, flags=0, front=None):
    """(the count * B values -- int8 with I8, float32 without --, the record as a numpy scalar of RECORD_DTYPE)"""
    rec = np.zeros((), RECORD_DTYPE)
    i8 = bool(flags & I8)
    if count == 0:
        return np.zeros(0, np.int8 if i8 else F32), rec
    assert pos >= 0 or flags & FRONT
    x = segment_symbols(soft, pos, count, front)
    e, dmin, v, finite = symbol_terms(points, labels, x, gain, scale)
    flat = v.reshape(-1)
    rec["n_symbols"], rec["n_finite"], rec["n_nan"] = count, int(finite.sum()), int(np.isnan(flat).sum())
    rec["sum_e"], rec["sum_err"] = ordered_sum(e, finite), ordered_sum(dmin, finite)
    rec["bits"], rec["flags"] = v.shape[1], DATA | (REC_I8 if i8 else 0)
    if i8:
        out, rec["n_clip"] = to_i8(flat)
    else:
        out = np.where(np.isnan(flat), QUIET_NAN, flat)  # (sign and payload of a NaN differ between machines: one NaN is written)
    return out, rec


def as_np(rec):
    """a ctypes DemapRecord (or an array of them) as numpy of RECORD_DTYPE"""
    return np.frombuffer(bytes(rec), RECORD_DTYPE)


def assert_same(rec, model, ctx):
    """byte for byte; on a miss, name the first member that differs"""
    got = as_np(rec)[0]
    if got.tobytes() == model.tobytes():
        return
    for name in RECORD_DTYPE.names:
        assert got[name].tobytes() == model[name].tobytes(), "%s: %s differs: %r != %r" % (ctx, name, got[name], model[name])
    raise AssertionError(ctx)


# ---- maps and rows the tests share -----------------------------------------------------------------------------------------------

def gray_labels(M):
    return np.array([k ^ (k >> 1) for k in range(M)], np.uint8)


def odd_map(M, seed=5):
    """M points off the unit circle with labels that are not Gray: the general distance, no unit-modulus shortcut"""
    rng = np.random.default_rng(seed + M)
    z = np.exp(2j * np.pi * (np.arange(M) + 0.3) / M) * rng.uniform(0.6, 1.4, M) + 0.05 * (rng.standard_normal(M) + 1j * rng.standard_normal(M))
    p = np.empty(2 * M, F32)
    p[0::2], p[1::2] = z.real, z.imag
    labels = {2: [1, 0], 4: [2, 0, 3, 1], 8: [5, 0, 6, 3, 1, 7, 2, 4]}[M]
    return p, np.array(labels, np.uint8)


def noisy_row(M, n, seed, sigma=0.15, gain=0.9 + 0.5j):
    """n symbols of odd_map(M) turned back by 1 / gain, with noise, interleaved float32"""
    rng = np.random.default_rng(seed)
    p, _ = odd_map(M)
    z = (p[0::2] + 1j * p[1::2])[rng.integers(0, M, n)] / gain
    z = z + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.empty(2 * n, F32)
    x[0::2], x[1::2] = z.real, z.imag
    return x
