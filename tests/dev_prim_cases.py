"""Case sets, layouts and the reference side for the device primitives (tests/support/dev_prims.hip).

Everything here is pure: a case set is drawn from a generator seeded by its own name (section 4.2's rule), its sha256 is pinned in
tests/golden/dev_prim_cases.json.  The reference side is the oracle's exported primitives (array forms, oracle/psk_soft_oracle.h),
this machine's glibc through them, IEEE division, and numpy models of pure data movement, of the DPP step order that
psk_wave.h documents and of what psk_tile_any.h's reductions are to compute (the maximum and the minimum over 64 values, the
merge's three lines) -- never the code under test.  The one exception the design asks for: lm_slice8_fast's `near` flag is held
to the host build of the same header (tests/support/libm_host.cpp), which tests/test_dev_prim_cases.py pins on the CPU.

A `kind` is an input domain; several operations and forms share the cases of a kind (tests/test_gpu_dev_prims.py: FORMS)."""
import atexit
import ctypes
import hashlib
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32, u32, i64, u64 = np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64
N_RANDOM = 1 << 20
PI4 = np.pi / 4


def _rng(name):
    d = hashlib.sha256(name.encode()).digest()
    return np.random.default_rng(int.from_bytes(d[:16], "little"))


def _f(bits):
    return np.asarray(bits, dtype=u32).view(f32)


def _bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(u32)


def _signs(x):
    """x and -x"""
    x = np.asarray(x, f32)
    return np.concatenate([x, -x])


def _near(x, span):
    """the floats within `span` ulps of each positive float of x (bit patterns clipped to [+0, +inf]): shape (x.size, 2 span + 1)"""
    b = _bits(np.abs(np.asarray(x, f32))).astype(i64)[:, None] + np.arange(-span, span + 1, dtype=i64)[None, :]
    return _f(np.clip(b, 0, 0x7F800000).astype(u32))


def _random_f32(rng, n):
    return _f(rng.integers(0, 1 << 32, n, dtype=u64).astype(u32))


def _random_f64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=u64).view(f64)


# ---- the specials: F (58 values), G (24 of them) ----
_ULP1 = _f([0x3F800001])[0]
_POW_K = (12, 25, 29, 31, 60, 61, 63, 64, 100, 126)
F = _signs(np.concatenate([
    _f([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F800001, 0x7F7FFFFF, 0x7F800000, 0x7FC00000]),
    np.array([2.0 ** k for k in _POW_K] + [2.0 ** -k for k in _POW_K], f32)]))
G = _signs(np.concatenate([
    _f([0x00000000, 0x00000001, 0x3F800000, 0x3F800001, 0x7F7FFFFF, 0x7F800000, 0x7FC00000]),
    np.array([2.0 ** 63, 2.0 ** 64, 2.0 ** -64, 2.0 ** 100, 2.0 ** -100], f32)]))
assert F.size == 58 and G.size == 24


def _grid(*axes):
    return tuple(np.ascontiguousarray(m.ravel()) for m in np.meshgrid(*axes, indexing="ij"))


class CaseSet:
    def __init__(self, kind, name, inputs, unit=1):
        self.kind, self.name, self.unit = kind, name, unit
        self.inputs = tuple(np.ascontiguousarray(a) for a in inputs)
        self.n = self.inputs[0].size // unit  # cases; `unit` elements of every input make one
        assert all(a.size == self.n * unit for a in self.inputs), name

    def digest(self):
        h = hashlib.sha256()
        for a in self.inputs:
            h.update(str(a.dtype).encode())
            h.update(a.tobytes())
        return h.hexdigest()


# =====================================================================================================================
# case sets by kind
# =====================================================================================================================
ATAN_BOUNDS = (7 / 16, 11 / 16, 19 / 16, 39 / 16, 2.0 ** -29, 2.0 ** 25)
WRAP_VALUES = np.array([12.566371, 25.132741, 50.265482], f32)  # 4 pi, 8 pi, 16 pi: wrapValue of constelationSize 2, 4, 8


def _atan2_sets():
    out = []
    y, x = _grid(F, F)
    out.append(("specials", (y, x)))
    # |y/x| within 8 ulps of every range bound, x in every binade from the denormals to 2^120 (a power of two and a drawn
    # significand each), all four sign pairs
    rng = _rng("atan2/bounds")
    e = np.arange(-149, 121)
    xs = np.concatenate([np.ldexp(1.0, e), np.ldexp(1.0 + rng.random(e.size), e)]).astype(f32)
    ys, xx = [], []
    for B in ATAN_BOUNDS:
        with np.errstate(over="ignore"):
            y0 = (xs.astype(f64) * B).astype(f32)
        yn = _near(y0, 8)
        ys.append(yn.ravel())
        xx.append(np.repeat(xs, yn.shape[1]))
    y, x = np.concatenate(ys), np.concatenate(xx)
    out.append(("bounds", (np.concatenate([y, y, -y, -y]), np.concatenate([x, -x, x, -x]))))
    # exponent differences of +-59 .. +-62 (e_atan2f.c's shortcuts sit at 60), all sign pairs
    rng = _rng("atan2/expdiff")
    ys, xx = [], []
    for d in (59, 60, 61, 62):
        for lo in range(-149, 127 - d, 7):
            m = 1.0 + rng.random(4)
            for a, b in ((lo + d, lo), (lo, lo + d)):
                ys.append(np.ldexp(m, a))
                xx.append(np.ldexp(m[::-1], b))
    y, x = np.concatenate(ys).astype(f32), np.concatenate(xx).astype(f32)
    out.append(("expdiff", (np.concatenate([y, y, -y, -y]), np.concatenate([x, -x, x, -x]))))
    # zeros against everything
    rng = _rng("atan2/zeros")
    other = np.concatenate([F, _random_f32(rng, 1024)])
    z = _f([0, 0x80000000])
    a, b = _grid(z, other)
    out.append(("zeros", (np.concatenate([a, b]), np.concatenate([b, a]))))
    rng = _rng("atan2/random")
    out.append(("random", (_random_f32(rng, N_RANDOM), _random_f32(rng, N_RANDOM))))
    return out


def _sincos_sets():
    out = []
    # (k = 1 .. 256, then 64 more spread up to 2^31: a power of two with a multiplicative-hash offset, no library function)
    far = [(1 << (8 + j * 23 // 64)) + (j * 2654435761) % (1 << (8 + j * 23 // 64)) for j in range(64)]
    ks = np.concatenate([np.arange(1, 257), np.array(far + [(1 << 31) - 1, 1 << 31])]).astype(f64)
    out.append(("kpi4", (_signs(_near((ks * PI4).astype(f32), 64).ravel()),)))
    out.append(("edges", (_signs(_near(np.array([2.0 ** -12, 120.0, PI4], f32), 64).ravel()),)))
    rng = _rng("sincos/exponents")
    e = np.repeat(np.arange(7, 128), 1000)
    b = ((e + 127).astype(u32) << 23) | rng.integers(0, 1 << 23, e.size, dtype=u64).astype(u32) | (rng.integers(0, 2, e.size, dtype=u64).astype(u32) << 31)
    out.append(("exponents", (_f(b),)))
    rng = _rng("sincos/specials")
    den = _f(np.concatenate([np.arange(1, 65), np.arange(0x7FFFC0, 0x800040), rng.integers(1, 0x800000, 256)]).astype(u32))
    out.append(("specials", (np.concatenate([_signs(den), F]),)))
    out.append(("stride", (_f(np.arange(0, 1 << 32, 1 << 11, dtype=u64).astype(u32)),)))
    out.append(("random", (_random_f32(_rng("sincos/random"), N_RANDOM),)))
    return out


T1, T3 = math.sqrt(2.0) - 1.0, math.sqrt(2.0) + 1.0  # tan(pi/8), tan(3 pi/8)
SLICE_FAR = (32, 64, 128, 256, 512, 1024, 2048, 4096)  # ulps: lm_slice8_fast's band of 4e-5 is about 335 wide


def _slice8_sets():
    out = []
    m = np.ldexp(1.0, np.arange(-149, 128, 4)).astype(f32)
    res, ims = [], []
    for T in (T1, T3):
        with np.errstate(over="ignore"):
            c = (m.astype(f64) * T).astype(f32)
        nb = _near(c, 16)
        res.append(np.repeat(m, nb.shape[1]))
        ims.append(nb.ravel())
    re, im = np.concatenate(res), np.concatenate(ims)
    re, im = np.concatenate([re, -re, re, -re]), np.concatenate([im, im, -im, -im])
    out.append(("rays", (np.concatenate([re, im]), np.concatenate([im, re]))))
    # the same rays from further off, out to where `near` is false again: +-32 .. +-4096 ulps at normal magnitudes
    m = np.ldexp(1.0, np.arange(-120, 121, 16)).astype(f32)
    off = np.array([s * o for o in SLICE_FAR for s in (-1, 1)], i64)
    res, ims = [], []
    for T in (T1, T3):
        c = (m.astype(f64) * T).astype(f32)
        nb = _f((_bits(c).astype(i64)[:, None] + off[None, :]).astype(u32))
        res.append(np.repeat(m, off.size))
        ims.append(nb.ravel())
    re, im = np.concatenate(res), np.concatenate(ims)
    re, im = np.concatenate([re, -re, re, -re]), np.concatenate([im, im, -im, -im])
    out.append(("rays_far", (np.concatenate([re, im]), np.concatenate([im, re]))))
    rng = _rng("slice8/axes")
    v = np.concatenate([F, _random_f32(rng, 512)])
    z = _f([0, 0x80000000])
    a, b = _grid(z, v)
    out.append(("axes", (np.concatenate([a, b]), np.concatenate([b, a]))))
    out.append(("specials", _grid(F, F)))
    rng = _rng("slice8/random")
    out.append(("random", (_random_f32(rng, N_RANDOM), _random_f32(rng, N_RANDOM))))
    return out


def _pair_sets(kind):
    rng = _rng(kind + "/random")
    return [("specials", _grid(F, F)), ("random", (_random_f32(rng, N_RANDOM), _random_f32(rng, N_RANDOM)))]


def _moderate_complex(rng, n, emax):
    """n complex floats, every quadrant and a spread of angles, each part below 2^(emax + 1) in magnitude and the larger one at
    least 2^-emax (drawn as sign, significand and exponent: no library function takes part, the draw is the same everywhere)"""
    e = rng.integers(-emax, emax + 1, n)
    d = rng.integers(0, 4, (2, n)) * rng.integers(0, 2, n)[None, :] * np.array([[1], [0]])  # one part up to 2^-3 of the other
    d = np.where(rng.integers(0, 2, n)[None, :] == 1, d, d[::-1])
    parts = [np.ldexp((1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n), (e - d[k]).astype(np.int32)).astype(f32) for k in range(2)]
    return parts[0], parts[1]


def _cmul_sets():
    rng = _rng("cmul/random")
    out = [("specials", _grid(G, G, G, G)), ("random", tuple(_random_f32(rng, N_RANDOM) for _ in range(4)))]
    rng = _rng("cmul/moderate")
    out.append(("moderate", _moderate_complex(rng, 1 << 18, 30) + _moderate_complex(rng, 1 << 18, 30)))
    return out


def _cdiv_sets():
    out = [("specials", _grid(G, G, G, G))]
    # last = (0, 0): the first symbol of every differentially decoded stream, every sign of the zeros
    rng = _rng("cdiv/last0")
    v = np.concatenate([F, _random_f32(rng, 256)])
    a, b = _grid(v, v)
    z = _f([0, 0x80000000])
    out.append(("last0", (np.tile(a, 4), np.tile(b, 4), np.repeat(z[[0, 1, 0, 1]], a.size), np.repeat(z[[0, 0, 1, 1]], a.size))))
    rng = _rng("cdiv/random")
    out.append(("random", tuple(_random_f32(rng, N_RANDOM) for _ in range(4))))
    rng = _rng("cdiv/moderate")
    out.append(("moderate", _moderate_complex(rng, 1 << 18, 30) + _moderate_complex(rng, 1 << 18, 30)))
    return out


CPOW_M = (1, 2, 3, 4, 5, 8, 16, 64)
N_RANDOM_CPOW = 1 << 18  # per exponent; with the moderate set (drawn for the exponent) the finite share stays above a half


def _cpow_sets(M):
    rng = _rng("cpow/random")  # (the same operands for every exponent)
    out = [("specials", _grid(G, G)), ("random", (_random_f32(rng, N_RANDOM_CPOW), _random_f32(rng, N_RANDOM_CPOW)))]
    out.append(("moderate", _moderate_complex(_rng("cpow/moderate/%d" % M), N_RANDOM_CPOW + (N_RANDOM_CPOW >> 2), int(126.0 / M - 1.5))))
    return out


def _div_known_sets():
    out = []

    def numer(rng, n):
        a = np.ldexp(rng.random(n) - 0.5, rng.integers(-40, 40, n).astype(np.int32))
        half = n // 2  # half of them next to a multiple of the divisor: quotients next to integers and half-integers
        return a, half

    rng = _rng("div_known/two_pi")
    n = 1 << 18
    a, half = numer(rng, n)
    b = np.full(n, 2 * np.pi)
    a[:half] = np.nextafter(rng.integers(-1 << 22, 1 << 22, half) * 0.5 * b[:half], rng.choice([-np.inf, np.inf], half))
    out.append(("two_pi", (a, b, 1.0 / b)))
    rng = _rng("div_known/float")
    a, half = numer(rng, n)
    b = (rng.random(n) * 1e3 + 1e-6).astype(f32).astype(f64)
    with np.errstate(invalid="ignore"):
        b[::3] = np.abs(_random_f32(rng, b[::3].size)).astype(f64)
    b[~np.isfinite(b) | (b == 0)] = 1.5
    out.append(("float", (a, b, 1.0 / b)))
    rng = _rng("div_known/integer")
    b = np.repeat(np.arange(1, 65536, dtype=f64), 8)
    a, half = numer(rng, b.size)
    a[::2] = rng.integers(-1 << 40, 1 << 40, a[::2].size).astype(f64)
    out.append(("integer", (a, b, 1.0 / b)))
    # numerators where the three-step quotient is not the division by itself: zeros of both signs, infinities, NaN,
    # denormal and barely normal quotients, quotients that overflow -- against each kind of divisor
    rng = _rng("div_known/numerators")
    bs = np.concatenate([[2 * np.pi, 1.0, 2.0, 3.0, 7.0, 50.0, 65535.0],
                         np.array([2.5e-9, 0.01, 1000.0, 3.0e-38, 1.0e-45, 3.0e38], f32).astype(f64),
                         (rng.random(32) * 1e3 + 1e-6).astype(f32).astype(f64), rng.integers(1, 65536, 32).astype(f64)])
    tiny = np.ldexp(1.0 + rng.random(48), np.repeat(np.arange(-1074, -1010, 4), 3).astype(np.int32))
    edge = np.ldexp(1.0 + rng.random(48), np.repeat(np.arange(-520, -488, 2), 3).astype(np.int32))  # around 2^-500
    huge = np.ldexp(1.0 + rng.random(48), np.repeat(np.arange(488, 520, 2), 3).astype(np.int32))    # around 2^500
    top = np.ldexp(1.0 + rng.random(48), np.repeat(np.arange(960, 1024, 4), 3).astype(np.int32))
    sp = np.concatenate([[0.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308], tiny, edge, huge, top])
    a, b = _grid(np.concatenate([sp, -sp]), bs)
    with np.errstate(all="ignore"):
        out.append(("numerators", (a, b, 1.0 / b)))
    # 2^20 random bit patterns for the numerator, the product's divisors in rotation
    rng = _rng("div_known/random")
    a = _random_f64(rng, N_RANDOM)
    fl = np.abs(_random_f32(rng, N_RANDOM))
    fl[~np.isfinite(fl) | (fl == 0)] = 1.5
    b = np.where(np.arange(N_RANDOM) % 3 == 0, 2 * np.pi, np.where(np.arange(N_RANDOM) % 3 == 1, fl.astype(f64),
                 rng.integers(1, 65536, N_RANDOM).astype(f64)))
    with np.errstate(all="ignore"):
        out.append(("random", (a, b, 1.0 / b)))
    return out


def _to_long_sets():
    v = [F.astype(f64)]
    for c in (2.0 ** 31, 2.0 ** 63, 2.0 ** 32, 2.0 ** 53):
        near = c + np.arange(-4, 4.5, 0.5)
        steps = [c]
        for _ in range(4):
            steps.append(np.nextafter(steps[-1], np.inf))
        lo = [c]
        for _ in range(4):
            lo.append(np.nextafter(lo[-1], -np.inf))
        v.append(np.concatenate([near, steps, lo]))
    for w in WRAP_VALUES.astype(f64):
        v.append(np.concatenate([np.floor(w) + np.arange(-2, 2.5, 0.5), [w, np.nextafter(w, 0), np.nextafter(w, 100)]]))
    v = np.concatenate(v)
    v = np.concatenate([v, -v, [np.nan, -np.nan, np.inf, -np.inf, 0.5, -0.5, 0.49999999999999994, 1e300, -1e300, 5e-324]])
    return [("directed", (v,)), ("random", (_random_f64(_rng("to_long/random"), N_RANDOM),))]


def _wrap_test_sets():
    p = [F]
    for c in (2.0 ** 31, 2.0 ** 63, 2.0 ** 24):
        p.append(_near(np.array([c], f32), 8).ravel())
        p.append((c + np.arange(-4, 4.5, 0.5)).astype(f32))
    for w in WRAP_VALUES:
        p.append(_near(np.array([w, np.floor(w), np.floor(w) + 1, np.floor(w) + 2], f32), 4).ravel())
        p.append((np.floor(w) + np.arange(-2, 2.5, 0.5)).astype(f32))
    p = _signs(np.concatenate(p))
    w = np.concatenate([WRAP_VALUES, F])
    a, b = _grid(p, w)
    rng = _rng("wrap_test/random")
    pr = _random_f32(rng, N_RANDOM)
    pr[::2] = (80.0 * (rng.random(pr[::2].size) - 0.5)).astype(f32)
    wr = WRAP_VALUES[rng.integers(0, 3, N_RANDOM)]
    wr[::4] = _random_f32(rng, wr[::4].size)
    return [("directed", (a, b)), ("random", (pr, wr))]


def _unwrap_sets():
    rng = _rng("unwrap/half")
    th = np.concatenate([np.array([np.pi, -np.pi, 0.0, 0.5, -0.5, np.pi / 2, -np.pi / 2], f32),
                         rng.uniform(-np.pi, np.pi, 9).astype(f32)]).astype(f64)
    ks = [0.0, -1.0]
    for j in range(0, 21):
        ks += [2.0 ** j, -(2.0 ** j), 2.0 ** j + 1, -(2.0 ** j) - 1]
    for c in (2.0 ** 31, 2.0 ** 52, 2.0 ** 62, 2.0 ** 63):
        ks += [c - 2 ** 8, c, c + 2 ** 8, -c - 2 ** 8, -c, -c + 2 ** 8, c * (1 - 2.0 ** -23), c * (1 + 2.0 ** -22), -c * (1 - 2.0 ** -23)]
    ks = np.array(ks)
    t, k = _grid(th, ks)
    c = (t + 2 * np.pi * (k + 0.5)).astype(f32)
    pe = _f((_bits(c).astype(i64)[:, None] + np.arange(-2, 3, dtype=i64)[None, :]).astype(u32)).ravel()
    out = [("half", (pe, np.repeat(t, 5)))]
    sp = np.concatenate([F, WRAP_VALUES])
    ths = np.concatenate([th, [np.nan, np.inf, -np.inf]])
    a, b = _grid(sp, ths)
    out.append(("specials", (a, b)))
    rng = _rng("unwrap/random")
    pe = _random_f32(rng, N_RANDOM)
    pe[::2] = (5000.0 * (rng.random(pe[::2].size) - 0.5)).astype(f32)
    tr = rng.uniform(-np.pi, np.pi, N_RANDOM).astype(f32).astype(f64)
    with np.errstate(invalid="ignore"):
        tr[::8] = _random_f32(rng, tr[::8].size).astype(f64)
    out.append(("random", (pe, tr)))
    return out


FIT_XDELTA = np.array([2.5e-9, 0.01, 1.0, 1000.0], f32)
FIT_PTS = np.arange(2, 65536, dtype=u32)


# (ySum, xySum) that are not finite or where a quotient is a zero, a denormal or overflows: the last lanes of every group
_BIG = 2400.0 * 65535
FIT_SPECIAL_SUMS = np.array([(np.nan, _BIG), (np.inf, -np.inf), (-np.inf, np.inf), (_BIG, np.nan), (np.inf, np.inf), (-np.inf, -np.inf),
                             (np.inf, 1.0), (1.0, -np.inf), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (5e-324, -5e-324),
                             (-3e-310, 2e-309), (1e300, -1e300), (-1.7e308, 1.7e308), (1e-320, 1e305)])
N_FIT_SPECIAL = len(FIT_SPECIAL_SUMS)


def _fit_random(name, n_groups, lanes):
    """random bit patterns for both sums, a drawn (xdelta, pts) per group of `lanes` cases"""
    rng = _rng(name)
    x = np.repeat(FIT_XDELTA[rng.integers(0, FIT_XDELTA.size, n_groups)], lanes)
    p = np.repeat(rng.integers(2, 65536, n_groups).astype(u32), lanes)
    return (_random_f64(rng, n_groups * lanes), _random_f64(rng, n_groups * lanes), x, p)


def _fit_sums(rng, xd, pts, lanes):
    """`lanes` (ySum, xySum) pairs for every (xdelta, pts): the mean phase sweeps from zero through 2400 rad (and its sums over
    65535 points) up to where the float results overflow; the last lanes hold non-finite sums.  Shape (pts.size, lanes)."""
    n = pts.size
    p = pts.astype(f64)[:, None]
    x = xd.astype(f64)[:, None]
    L = lanes - N_FIT_SPECIAL
    # one row of mean phases (sign, significand and exponent per lane) times a factor per (xdelta, pts): every element gets a
    # significand of its own from the product, at a few array operations in all
    e = np.round(np.linspace(-40.0, 132.0, L)).astype(np.int32)
    mean = np.ldexp(1.0 + rng.random(L), e) * rng.choice([-1.0, 1.0], L)
    mean[0] = 0.0
    tilt = rng.uniform(-2.0, 2.0, L) * mean
    with np.errstate(over="ignore", invalid="ignore"):
        ysum = mean[None, :] * (p * rng.uniform(0.5, 2.0, (n, 1)))
        xysum = ysum * (x * (p - 1) / 2)
        xysum += tilt[None, :] * (rng.uniform(0.5, 2.0, (n, 1)) * x * (p * p / 12.0))
    ys = np.concatenate([ysum, np.broadcast_to(FIT_SPECIAL_SUMS[None, :, 0], (n, N_FIT_SPECIAL))], axis=1)
    xys = np.concatenate([xysum, np.broadcast_to(FIT_SPECIAL_SUMS[None, :, 1], (n, N_FIT_SPECIAL))], axis=1)
    return ys, xys


def _fit_den_sets():
    x, p = _grid(FIT_XDELTA, FIT_PTS)
    return [("all", (x, p))]


def _fit_value_sets():
    x, p = _grid(FIT_XDELTA, FIT_PTS)
    ys, xys = _fit_sums(_rng("fit_value/all"), x, p, 24)
    return [("all", (ys.ravel(), xys.ravel(), np.repeat(x, 24), np.repeat(p, 24))), ("random", _fit_random("fit_value/random", N_RANDOM, 1))]


def _fit_known_sets():
    """a wave per (xdelta, pts): fit_known's members are wave-uniform (v_readfirstlane)"""
    x, p = _grid(FIT_XDELTA, FIT_PTS)
    ys, xys = _fit_sums(_rng("fit_known/all"), x, p, 64)
    return [("all", (ys.ravel(), xys.ravel(), np.repeat(x, 64), np.repeat(p, 64))), ("random", _fit_random("fit_known/random", N_RANDOM // 64, 64))]


# ---- wave primitives: a case is a wave of 64 values ----
N_SCAN_WAVES = 1024


def _scan_waves(rng, dt, n_mixed):
    """mixed-sign addends over 2^+-40 (the order of additions shows in the bits), then all-equal, single-lane and
    exact-cancellation waves: (waves, 64)"""
    mant = 1.0 + rng.random((n_mixed, 64))
    mixed = (np.ldexp(mant, rng.integers(-40, 41, (n_mixed, 64)).astype(np.int32)) * rng.choice([-1.0, 1.0], (n_mixed, 64))).astype(dt)
    vals = np.array([0.1, 1.0, -3.0, 2.0 ** -140, 1.0 + 2.0 ** -20, 16777216.0, 0.0, -0.0], f64).astype(dt)
    equal = np.repeat(vals[:, None], 64, axis=1)
    single = np.zeros((64, 64), dt)
    single[np.arange(64), np.arange(64)] = (1.0 + rng.random(64)).astype(dt)
    canc = np.zeros((64, 64), dt)
    for w in range(64):
        big = np.ldexp(1.0 + rng.random(32), rng.integers(20, 41, 32).astype(np.int32)).astype(dt)
        small = (1.0 + rng.random(64)).astype(dt)
        row = small.copy()
        pos = rng.permutation(64)
        row[pos[:32]] = big
        row[pos[32:]] = -big  # every big addend has its negative somewhere in the wave
        canc[w] = row if w % 2 else np.concatenate([big, -big])[rng.permutation(64)]
    return np.concatenate([mixed, equal, single, canc]), n_mixed


def _scan_sets(kind):
    rng = _rng(kind + "/waves")
    if kind == "scan_f64":
        w, _ = _scan_waves(rng, f64, N_SCAN_WAVES)
        return [("waves", (w.ravel(),), 64)]
    if kind == "scan_i32":
        w = rng.integers(-1 << 31, 1 << 31, (N_SCAN_WAVES, 64)).astype(i32)
        w[::4] = rng.integers(-1000, 1000, w[::4].shape)
        return [("waves", (w.ravel(),), 64)]
    N = int(kind.split("/")[1])  # scan_f32_multi/N: each of the N interleaved scans has data of its own
    per = [_scan_waves(_rng("%s/%d" % (kind, k)), f32, 128)[0] for k in range(N)]
    return [("waves", (np.stack(per, axis=2).ravel(),), 64 * N)]


def _max_f32_sets():
    rng = _rng("max_f32/waves")
    w = _f(rng.integers(0, 0x7F800001, (512, 64), dtype=u64).astype(u32)).copy()
    w[0:8] = 0.0  # +0 everywhere
    w[8:72] = _f(rng.integers(0, 0x800000, (64, 64), dtype=u64).astype(u32))  # zeros and denormals only
    w[72:136] = 0.0
    w[72 + np.arange(64), np.arange(64)] = _f(rng.integers(1, 0x7F800000, 64, dtype=u64).astype(u32))  # one lane, each in turn
    w[136 + np.arange(64), rng.permutation(64)] = np.inf  # +inf somewhere
    w[200 + np.arange(64), np.arange(64)] = _f([1])[0]  # the smallest denormal among zeros
    w[200:264][w[200:264] != _f([1])[0]] = 0.0
    return [("waves", (w.ravel(),), 64)]


def _u32_sets():
    rng = _rng("u32/waves")
    w = rng.integers(0, 1 << 32, (512, 64), dtype=u64).astype(u32)
    w[0:4] = np.array([0, 0xFFFFFFFF, 0x80000000, 7], u32)[:, None]
    w[4 + np.arange(64), np.arange(64)] = 0xFFFFFFFF
    w[68:132] = rng.integers(1, 1 << 31, (64, 64), dtype=u64).astype(u32)
    w[68 + np.arange(64), np.arange(64)] = 0
    return [("waves", (w.ravel(),), 64)]


_WT = {"i32": i32, "f32": f32, "f64": f64}


def _raw(rng, t, shape):
    if t == "f64":
        return rng.integers(0, 1 << 64, shape, dtype=u64).view(f64)
    return rng.integers(0, 1 << 32, shape, dtype=u64).astype(u32).view(_WT[t])


def _up1_sets(kind):
    rng = _rng(kind + "/waves")
    t = kind.split("/")[1]
    return [("waves", (_raw(rng, t, (256, 64)).ravel(), _raw(rng, t, (256, 64)).ravel()), 64)]


def _read_lane_sets(kind):
    rng = _rng(kind + "/waves")
    t = kind.split("/")[1]
    lane = rng.integers(0, 64, (256, 64)).astype(i32)
    lane[:, 0] = np.arange(256) % 64  # the wave's first lane names the lane read: every lane in turn
    return [("waves", (_raw(rng, t, (256, 64)).ravel(), lane.ravel()), 64)]


def _med3_sets():
    s = np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1, 5, -5], i64).astype(i32)
    rng = _rng("med3/random")
    r = [rng.integers(-1 << 31, 1 << 31, N_RANDOM).astype(i32) for _ in range(3)]
    r[1][::3] = r[0][::3]  # ties
    r[2][::5] = r[1][::5]
    return [("specials", _grid(s, s, s)), ("random", tuple(r))]


# ---- the first-maximum reductions of psk_tile_any.h: a case is a wave of 64 values (times U for the level-by-level forms) ----
ANY_PAIR_LANES = (0, 15, 16, 31, 32, 47, 48, 63)  # the first and last lane of every DPP row: both sides of each cross-row step
ANY_PAIRS = tuple((a, b) for i, a in enumerate(ANY_PAIR_LANES) for b in ANY_PAIR_LANES[i + 1:])
ANY_U = 8  # the width psk_tile_front_any_kernel<1> instantiates
N_ANY_RANDOM = 512


def _any_finite(rng, shape):
    """doubles of both signs over 2^+-40"""
    return np.ldexp(1.0 + rng.random(shape), rng.integers(-40, 41, shape).astype(np.int32)) * rng.choice([-1.0, 1.0], shape)


def _any_f64_waves(rng):
    """Named runs of waves for the maximum: the extremum in each lane in turn (far above the others; one ulp above 64 equal
    values), equal extrema in two lanes for every pair of ANY_PAIR_LANES, all lanes equal, -inf in every lane but one, finite
    values next to NaN (some lanes; every lane but one), random bit patterns (a NaN among them made the quiet one: what an
    addition leaves behind)."""
    ar = np.arange(64)
    far = _any_finite(rng, (64, 64))
    far[ar, ar] = np.ldexp(1.0 + rng.random(64), 41)
    base = _any_finite(rng, 64)
    ulp = np.repeat(base[:, None], 64, axis=1)
    ulp[ar, ar] = np.nextafter(base, np.inf)
    pairs = _any_finite(rng, (len(ANY_PAIRS), 64))
    for w, (a, b) in enumerate(ANY_PAIRS):
        pairs[w, a] = pairs[w, b] = np.ldexp(1.0 + rng.random(), 41)
    vals = np.array([0.1, 1.0, -3.0, 2.0 ** -1040, 0.0, -0.0, -np.inf, np.inf, 1e300, -1e300], f64)
    equal = np.repeat(vals[:, None], 64, axis=1)
    zeros = np.where(rng.random((8, 64)) < 0.5, 0.0, -0.0)  # zeros of both signs, some above negative values only
    zeros[4:][rng.random((4, 64)) < 0.5] = -1.5
    one = np.full((64, 64), -np.inf)
    one[ar, ar] = _any_finite(rng, 64)
    some_nan = _any_finite(rng, (64, 64))
    some_nan[rng.random((64, 64)) < rng.random((64, 1))] = np.nan
    lane = rng.permutation(64)
    some_nan[ar, lane] = np.nan
    some_nan[ar, (lane + rng.integers(1, 64, 64)) % 64] = _any_finite(rng, 64)  # (a NaN and a finite value in every wave)
    but_one = np.full((64, 64), np.nan)
    but_one[ar, ar] = _any_finite(rng, 64)
    rnd = _random_f64(rng, N_ANY_RANDOM * 64).reshape(-1, 64).copy()
    rnd[np.isnan(rnd)] = np.nan
    return [("each_lane", np.concatenate([far, ulp])), ("pairs", pairs), ("equal", np.concatenate([equal, zeros])), ("inf_but_one", one),
            ("nan", np.concatenate([some_nan, but_one])), ("random", rnd)]


def _any_u32_waves(rng):
    """The same for the unsigned minimum: the extremum in each lane in turn (far below; one below 64 equal values), equal
    minima in two lanes for every pair, all lanes equal, 0xFFFFFFFF in every lane but one, random (values on both sides of
    2^31 in every wave: a signed comparison shows)."""
    ar = np.arange(64)
    far = rng.integers(1 << 16, 1 << 32, (64, 64), dtype=u64).astype(u32)
    far[ar, ar] = rng.integers(0, 1 << 16, 64, dtype=u64).astype(u32)
    base = rng.integers(1, 1 << 32, 64, dtype=u64).astype(u32)
    base[::4] = 0x80000000  # (one below: the largest positive int)
    one_below = np.repeat(base[:, None], 64, axis=1)
    one_below[ar, ar] = base - u32(1)
    pairs = rng.integers(1 << 16, 1 << 32, (len(ANY_PAIRS), 64), dtype=u64).astype(u32)
    for w, (a, b) in enumerate(ANY_PAIRS):
        pairs[w, a] = pairs[w, b] = u32(rng.integers(0, 1 << 16))
    equal = np.repeat(np.array([0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 7], u32)[:, None], 64, axis=1)
    one = np.full((64, 64), 0xFFFFFFFF, u32)
    one[ar, ar] = rng.integers(0, 1 << 32, 64, dtype=u64).astype(u32)
    one[ar[::8], ar[::8]] = u32(0xFFFFFFFE)
    rnd = rng.integers(0, 1 << 32, (N_ANY_RANDOM, 64), dtype=u64).astype(u32)
    return [("each_lane", np.concatenate([far, one_below])), ("pairs", pairs), ("equal", equal), ("max_but_one", one), ("random", rnd)]


ANY_MERGE_VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 2.5, 1e300, np.inf, np.nan], f64)
ANY_MERGE_K = np.array([0, 1, 15, 16, 63, 64, 1023, 0x7FFFFFFF], i32)  # (0x7fffffff: the sentinel the front stage starts from)


def _any_merge_sets():
    """(a.best, a.second, b.best, b.second, a.k, b.k).  `best_k`: every pair of values with every pair of phases, both seconds
    -inf as the front stage builds its operands -- equal `best` with the lower phase on either side, and equal `k`;
    `seconds`: every combination of the four doubles with the phases in either order; `random`: all six drawn from the pools,
    so that a tie is common."""
    V, K = ANY_MERGE_VALUES, ANY_MERGE_K
    ab, bb, ak, bk = _grid(V, V, K, K)
    ninf = np.full(ab.size, -np.inf)
    out = [("best_k", (ab, ninf, bb, ninf.copy(), ak, bk))]
    ab, as_, bb, bs, flip = _grid(V, V, V, V, np.array([0, 1], i32))
    out.append(("seconds", (ab, as_, bb, bs, np.where(flip, 5, 3).astype(i32), np.where(flip, 3, 5).astype(i32))))
    rng = _rng("any_merge/random")
    n = 1 << 16
    out.append(("random", tuple(V[rng.integers(0, V.size, n)] for _ in range(4)) + tuple(K[rng.integers(0, K.size, n)] for _ in range(2))))
    return out


def _any_sets(kind):
    base = kind.split("/")[0]
    waves = _any_f64_waves if "f64" in base else _any_u32_waves
    if "/" not in kind:
        return [(name, (w.ravel(),), 64) for name, w in waves(_rng(kind + "/waves"))]
    U = int(kind.split("/")[1])  # each of the U interleaved reductions has data of its own
    per = [waves(_rng("%s/%d" % (kind, k))) for k in range(U)]
    return [(name, (np.stack([p[j][1] for p in per], axis=2).ravel(),), 64 * U) for j, (name, _) in enumerate(per[0])]


ANY_KINDS = ("any_f64", "any_u32", "any_f64_multi/%d" % ANY_U, "any_u32_multi/%d" % ANY_U)
WAVE_KINDS = (("scan_f64", "scan_i32") + tuple("scan_f32_multi/%d" % n for n in range(1, 33)) + ("max_f32", "u32")
              + tuple("up1/" + t for t in ("i32", "f32", "f64")) + tuple("read_lane/" + t for t in ("f32", "f64")) + ANY_KINDS)
POINT_KINDS = (("atan2", "sincos", "slice8", "norm", "qpsk", "cmul", "cdiv") + tuple("cpow/%d" % m for m in CPOW_M)
               + ("div_known", "to_long", "wrap_test", "unwrap", "fit_den", "fit_value", "med3", "any_merge"))
KINDS = POINT_KINDS + ("fit_known",) + WAVE_KINDS


def case_sets(kind):
    """the case sets of a kind, in a fixed order"""
    base = kind.split("/")[0]
    if kind in ("scan_f64", "scan_i32") or base == "scan_f32_multi":
        raw = _scan_sets(kind)
    elif base == "up1":
        raw = _up1_sets(kind)
    elif base == "read_lane":
        raw = _read_lane_sets(kind)
    elif base == "cpow":
        raw = _cpow_sets(int(kind.split("/")[1]))
    elif kind in ("norm", "qpsk"):
        raw = _pair_sets(kind)
    elif kind in ANY_KINDS:
        raw = _any_sets(kind)
    elif kind == "any_merge":
        raw = _any_merge_sets()
    else:
        raw = {"atan2": _atan2_sets, "sincos": _sincos_sets, "slice8": _slice8_sets, "cmul": _cmul_sets, "cdiv": _cdiv_sets,
               "div_known": _div_known_sets, "to_long": _to_long_sets, "wrap_test": _wrap_test_sets, "unwrap": _unwrap_sets,
               "fit_den": _fit_den_sets, "fit_value": _fit_value_sets, "fit_known": _fit_known_sets, "max_f32": _max_f32_sets,
               "u32": _u32_sets, "med3": _med3_sets}[kind]()
    return [CaseSet(kind, "%s/%s" % (kind, r[0]), r[1], r[2] if len(r) > 2 else 1) for r in raw]


def unit_of(kind):
    """elements of an input per case: 64 for a wave (times N for the interleaved scans), 64 for fit_known's uniform waves"""
    if kind in WAVE_KINDS:
        return 64 * (int(kind.split("/")[1]) if "_multi/" in kind else 1)
    return 64 if kind == "fit_known" else 1


class Cases:
    """all case sets of a kind as one run of cases: inputs, the set of every case, its class"""

    def __init__(self, kind, digests=False):
        sets = case_sets(kind)
        self.kind, self.sets = kind, [s.name for s in sets]
        self.unit = unit_of(kind)
        self.inputs = tuple(np.concatenate([s.inputs[k] for s in sets]) for k in range(len(sets[0].inputs)))
        per = [s.inputs[0].size // self.unit for s in sets]
        self.n = sum(per)  # units: cases, or waves
        self.set_of = np.repeat(np.arange(len(sets)), per)
        self.digests = {s.name: s.digest() for s in sets} if digests else None
        self.counts = {s.name: m for s, m in zip(sets, per)}


# =====================================================================================================================
# classes: conditions on the inputs, evaluated with numpy alone (and the host build for `near`)
# =====================================================================================================================
ATAN2_CLASSES = ("ordinary", "rare", "special")
SINCOS_CLASSES = ("ordinary", "tiny", "big", "nonfinite")


def atan2_ratio(y, x):
    with np.errstate(all="ignore"):
        return np.abs(y / x)


def atan_range(a):
    """index of s_atanf.c's range for a >= 0: 0 below 7/16, 1 below 11/16, 2 below 19/16, 3 below 39/16, 4 above"""
    ia = _bits(a).astype(i64)
    return (ia > 0x3EDFFFFF).astype(int) + (ia > 0x3F2FFFFF) + (ia > 0x3F97FFFF) + (ia > 0x401BFFFF)


def classes(kind, inputs):
    """(class of every case, class names), or (None, None) for a kind with one class"""
    base = kind.split("/")[0]
    if base == "atan2":
        y, x = inputs
        iy, ix = _bits(y) & 0x7FFFFFFF, _bits(x) & 0x7FFFFFFF
        ia = _bits(atan2_ratio(y, x))
        special = (ix > 0x7F7FFFFF) | (iy > 0x7F7FFFFF)
        rare = (ix == 0) | (iy == 0) | (ia >= 0x4C000000)
        return np.where(special, 2, np.where(rare, 1, 0)), ATAN2_CLASSES
    if base == "sincos":
        top = (_bits(inputs[0]) >> 20) & 0x7FF
        return np.where(top >= 0x7F8, 3, np.where(top >= (0x42F00000 >> 20), 2, np.where(top < (0x39800000 >> 20), 1, 0))), SINCOS_CLASSES
    if base == "slice8":
        return host_slice8_fast(*inputs)[1].astype(int), ("far", "near")
    if base == "cmul":
        return cmul_branch(*inputs).clip(0, 1), ("plain", "both parts NaN")
    if base == "cdiv":
        return cdiv_branch(*inputs).clip(0, 1), ("plain", "both parts NaN")
    if base == "cpow":
        r = reference("cpow", inputs, int(kind.split("/")[1]))
        return (~(np.isfinite(r[0]) & np.isfinite(r[1]))).astype(int), ("finite", "not finite")
    return None, None


def cmul_branch(a, b, c, d):
    """0: no recovery; else which of __mulsc3's recoveries runs: 1 an infinite left factor, 2 an infinite right factor, 3 both,
    4 an overflowed product, 5 both parts NaN and nothing to recover"""
    with np.errstate(all="ignore"):
        ac, bd, ad, bc = a * c, b * d, a * d, b * c
        both = np.isnan(ac - bd) & np.isnan(ad + bc)
    l, r = np.isinf(a) | np.isinf(b), np.isinf(c) | np.isinf(d)
    ovf = np.isinf(ac) | np.isinf(bd) | np.isinf(ad) | np.isinf(bc)
    br = np.where(l & r, 3, np.where(l, 1, np.where(r, 2, np.where(ovf, 4, 5))))
    return np.where(both, br, 0)


def cdiv_branch(a, b, c, d):
    """0: no recovery; else __divsc3's: 1 a zero divisor, 2 an infinite numerator, 3 an infinite divisor, 4 none applies"""
    with np.errstate(all="ignore"):
        aa, bb, cc, dd = (v.astype(f64) for v in (a, b, c, d))
        den = cc * cc + dd * dd
        x, y = ((aa * cc + bb * dd) / den).astype(f32), ((bb * cc - aa * dd) / den).astype(f32)
    both = np.isnan(x) & np.isnan(y)
    z = (c == 0) & (d == 0) & (~np.isnan(a) | ~np.isnan(b))
    n = (np.isinf(a) | np.isinf(b)) & np.isfinite(c) & np.isfinite(d)
    dv = (np.isinf(c) | np.isinf(d)) & np.isfinite(a) & np.isfinite(b)
    return np.where(both, np.where(z, 1, np.where(n, 2, np.where(dv, 3, 4))), 0)


# =====================================================================================================================
# layouts
# =====================================================================================================================
def layouts(kind, n, klass):
    """index arrays over the n cases (waves for a wave kind), each a multiple of 64 long for the point kinds:
    grouped -- by class, every class padded to whole waves with its own cases: whole waves ordinary, whole waves rare;
    shuffled -- a fixed permutation: rare and ordinary cases share waves"""
    per_wave = 1 if unit_of(kind) > 1 else 64

    def pad(ix):
        short = (-ix.size) % per_wave
        return np.concatenate([ix, ix[:1].repeat(short)]) if short else ix

    if klass is None:
        grouped = pad(np.arange(n))
    else:
        order = np.argsort(klass, kind="stable")
        k = klass[order]
        grouped = np.concatenate([pad(order[k == c]) for c in np.unique(k)])
    shuffled = pad(_rng(kind + "/shuffle").permutation(n))
    return {"grouped": grouped, "shuffled": shuffled}


def take(inputs, ix, unit):
    """the inputs in the order of a layout"""
    if unit == 1:
        return tuple(a[ix] for a in inputs)
    return tuple(np.ascontiguousarray(a.reshape(-1, unit)[ix]).ravel() for a in inputs)


# =====================================================================================================================
# the reference side
# =====================================================================================================================
_ORC_OPS = {name: k for k, name in enumerate(
    ("atan2f", "sincosf", "polar1", "norm", "cmul", "cdiv", "cpow", "wrap_test", "to_long", "unwrap", "slice8", "qpsk",
     "denominator", "calc_fit"))}
_orc = None


def oracle_array(op, inputs, out_types, param=0):
    """n cases through psk_oracle_prim_array (oracle/psk_soft_oracle.h)"""
    global _orc
    if _orc is None:
        from oracle import pyoracle

        pyoracle.build()
        L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libpsk_soft_oracle.so"))
        L.psk_oracle_prim_array.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        L.psk_oracle_prim_array.restype = ctypes.c_int
        _orc = L
    arrs = [np.ascontiguousarray(a) for a in inputs]
    n = arrs[0].size
    assert all(a.size == n for a in arrs)
    res = [np.empty(n, t) for t in out_types]
    pin = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    pout = (ctypes.c_void_p * len(res))(*[r.ctypes.data for r in res])
    assert _orc.psk_oracle_prim_array(_ORC_OPS[op], param, pin, pout, n) == 0, op
    return tuple(res)


_host = None


def host_libm():
    """psk_libm.h compiled for the host (tests/support/libm_host.cpp), with the flags of tests/test_libm_pin.py"""
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="psk_libm_host_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libm_host.so")
        subprocess.run(["g++", "-O2", "-std=gnu++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "psk_soft_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "support", "libm_host.cpp")],
                       check=True)
        _host = ctypes.CDLL(so)
    return _host


def _host_call(fn, inputs, out_types):
    arrs = [np.ascontiguousarray(a) for a in inputs]
    res = [np.empty(arrs[0].size, t) for t in out_types]
    f = getattr(host_libm(), fn)
    f.restype = None
    f(*[ctypes.c_void_p(a.ctypes.data) for a in arrs + res], ctypes.c_long(arrs[0].size))
    return tuple(res)


def host_slice8_fast(re, im):
    """(sector, near) of the host build of lm_slice8_fast"""
    return _host_call("lmh_slice8_fast", (re, im), (i32, i32))


def scan_model(v, op=np.add, masked_rows_add_zero=False):
    """the DPP step order psk_wave.h documents, on (waves, 64) of one type: row_shr 1, 2, 4, 8 inside rows of 16 with zero
    fill, then lane 15 into rows 1 and 3, then lane 31 into rows 2 and 3; one rounded operation a step.  In the two cross-row
    steps the rows masked off keep their value in the float forms (one DPP instruction a step); in the forms written with the
    builtins (wave_scan_f64, wave_scan_i32: dpp_zero) they receive 0 and add it, which turns a -0.0 into +0.0."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = v.reshape(-1, 4, 16).copy()
        zero = np.zeros_like(r[:, 0, :])
        for s in (1, 2, 4, 8):
            sh = np.zeros_like(r)
            sh[:, :, s:] = r[:, :, :-s]
            r = op(r, sh)
        l15, l47 = r[:, 0, 15:16].copy(), r[:, 2, 15:16].copy()
        r[:, 1, :] = op(r[:, 1, :], l15)
        r[:, 3, :] = op(r[:, 3, :], l47)
        if masked_rows_add_zero:
            r[:, 0, :] = op(r[:, 0, :], zero)
            r[:, 2, :] = op(r[:, 2, :], zero)
        l31 = r[:, 1, 15:16].copy()
        r[:, 2, :] = op(r[:, 2, :], l31)
        r[:, 3, :] = op(r[:, 3, :], l31)
        if masked_rows_add_zero:
            r[:, 0, :] = op(r[:, 0, :], zero)
            r[:, 1, :] = op(r[:, 1, :], zero)
    return r.reshape(-1, 64)


def reference(op, inputs, param=0):
    """the outputs of an operation (tests/dev_prims_lib.py: OPS) by the reference side"""
    if op == "atan2":
        return oracle_array("atan2f", inputs, (f32,))
    if op == "sincos":
        return oracle_array("sincosf", inputs, (f32, f32))
    if op in ("slice8", "slice8_atan"):
        return (oracle_array("slice8", inputs, (i32,))[0].astype(u32),)
    if op == "slice8_fast":  # the oracle's index (compared where near is false), the host build's flag
        return (oracle_array("slice8", inputs, (i32,))[0].astype(u32), host_slice8_fast(*inputs)[1].astype(u32))
    if op == "div_known":
        with np.errstate(all="ignore"):
            return (inputs[0] / inputs[1],)
    if op == "norm":
        return oracle_array("norm", inputs, (f32,))
    if op in ("cmul", "cdiv"):
        return oracle_array(op, inputs, (f32, f32))
    if op == "cpow":
        return oracle_array("cpow", inputs, (f32, f32), param & 0xFF)
    if op == "to_long":
        return oracle_array("to_long", inputs, (i64,))
    if op == "unwrap":
        return oracle_array("unwrap", inputs, (i64,))
    if op == "fit_den":
        return oracle_array("denominator", inputs, (f32, f32))
    if op == "fit_value":
        return oracle_array("calc_fit", inputs, (f32, f32, f32))
    if op == "fit_known":
        return oracle_array("calc_fit", inputs, (f32, f32, f32))[:2]
    if op == "qpsk":
        if param == 0:
            return oracle_array("qpsk", inputs, (i32, i32))
        # PSK_SOFT_OPT_QPSK_SIGN_BITMAP, a product option the oracle does not have: the signs, by the diagram the option cites
        r, m = (inputs[0] > 0).astype(i32), (inputs[1] > 0).astype(i32)
        return (r ^ m, m ^ 1)
    if op == "wrap_test":
        return (oracle_array("wrap_test", inputs, (i32,))[0].astype(u32),)
    if op == "med3":
        return (np.sort(np.stack(inputs), axis=0)[1],)
    # ---- wave primitives: numpy models on (waves, 64) ----
    v = inputs[0]
    if op in ("scan_f64", "scan_i32"):
        return (scan_model(v.reshape(-1, 64), masked_rows_add_zero=True).ravel(),)
    if op == "sum_f64":
        return (np.repeat(scan_model(v.reshape(-1, 64), masked_rows_add_zero=True)[:, 63], 64),)
    if op == "scan_f32_multi":
        w = v.reshape(-1, 64, param)
        return (np.stack([scan_model(np.ascontiguousarray(w[:, :, k])) for k in range(param)], axis=2).ravel(),)
    if op == "max_f32":
        return (np.repeat(scan_model(v.reshape(-1, 64), np.maximum)[:, 63], 64),)
    if op in ("max_u32", "min_u32"):
        w = v.reshape(-1, 64)
        return (np.repeat(w.max(axis=1) if op == "max_u32" else w.min(axis=1), 64),)
    if op in ("up1", "up1_zero"):
        w = v.reshape(-1, 64)
        r = np.empty_like(w)
        r[:, 1:] = w[:, :-1]
        r[:, 0] = inputs[1].reshape(-1, 64)[:, 0] if op == "up1" else 0
        return (r.ravel(),)
    if op == "read_lane":
        w = v.reshape(-1, 64)
        lane = inputs[1].reshape(-1, 64)[:, 0] & 63
        return (np.repeat(w[np.arange(w.shape[0]), lane], 64),)
    # ---- psk_tile_any.h: "the maximum over 64 values" (fmax: a NaN next to a number drops out), "the minimum over 64 values",
    # and the three lines of the merge -- every lane holds the result
    if op in ("any_max_f64", "any_min_u32"):
        w = v.reshape(-1, 64)
        return (np.repeat(np.fmax.reduce(w, axis=1) if op == "any_max_f64" else w.min(axis=1), 64),)
    if op in ("any_max_f64_multi", "any_min_u32_multi"):
        w = v.reshape(-1, 64, param)
        r = np.fmax.reduce(w, axis=1) if op == "any_max_f64_multi" else w.min(axis=1)
        return (np.ascontiguousarray(np.broadcast_to(r[:, None, :], w.shape)).ravel(),)
    if op == "any_merge":
        ab, as_, bb, bs, ak, bk = inputs
        with np.errstate(invalid="ignore"):
            b_wins = (bb > ab) | ((bb == ab) & (bk < ak))  # the larger sum, the lower phase on a tie
            loser = np.where(b_wins, ab, bb)
            s2 = np.where(as_ > bs, as_, bs)
            return (np.where(b_wins, bb, ab), np.where(loser > s2, loser, s2), np.where(b_wins, bk, ak))
    raise KeyError(op)


# =====================================================================================================================
# the comparison rule: the suite's own (tests/test_gpu_parity.py: assert_parity), per element
# =====================================================================================================================
def differs(got, ref, raw=False, zeros=False):
    """True where got is not ref: every finite value by its bit pattern (signed zeros included), infinities by position and
    sign, NaN by position only; integers equal.  raw: bit patterns throughout (pure data movement).  zeros: a zero of either
    sign equals a zero of the other (psk_tile_any.h: the callers only test the results with ==)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    if got.dtype.kind != "f":
        return got != ref
    ut = u32 if got.dtype == f32 else u64
    d = got.view(ut) != ref.view(ut)
    if raw:
        return d
    if zeros:
        d &= ~((got == 0) & (ref == 0))
    return d & ~(np.isnan(got) & np.isnan(ref))


def hexes(inputs, i):
    """element i of every operand array as a hex pattern"""
    out = []
    for a in inputs:
        w = np.asarray(a[i])
        out.append("0x%0*x" % (w.itemsize * 2, int(w.view({4: u32, 8: u64}[w.itemsize]))))
    return "(" + ", ".join(out) + ")"


# =====================================================================================================================
# the table: every operation in every form the kernels call, the kind whose cases it runs, how it is compared
# =====================================================================================================================
class Form:
    """label; op and param of tests/dev_prims_lib.py; kind; n_in: the leading inputs of the kind the op takes;
    divergent: run once more inside a lane-divergent branch; rule: "all", "finite" (the screened tier: wherever the oracle's
    result is finite in both parts), "slice8_fast" (sector wherever near is false, near everywhere), "raw" (bit patterns),
    "zeros" (as "all", zeros of either sign equal)"""

    def __init__(self, family, label, op, kind, param=0, divergent=False, rule="all", n_in=None):
        self.family, self.label, self.op, self.kind, self.param = family, label, op, kind, param
        self.divergent, self.rule, self.n_in = divergent, rule, n_in


def _forms():
    T = []
    add = lambda *a, **k: T.append(Form(*a, **k))
    add("libm", "atan2f_wave<AtanTabDev>", "atan2", "atan2", 0)
    add("libm", "atan2f_wave<AtanTabWave>", "atan2", "atan2", 1, divergent=True)
    add("libm", "sincosf_wave(dep=0)", "sincos", "sincos", 0, divergent=True)
    add("libm", "sincosf_wave(dep varying)", "sincos", "sincos", 1)
    add("libm", "lm_div_known(rb given)", "div_known", "div_known", 0)
    add("libm", "lm_div_known(rb = 1.0 / b on the device)", "div_known", "div_known", 1)
    add("slicing", "lm_slice8_fast", "slice8_fast", "slice8", rule="slice8_fast")
    add("slicing", "slice_8psk<AtanTabDev>", "slice8", "slice8", 0)
    add("slicing", "slice_8psk<AtanTabWave>", "slice8", "slice8", 1, divergent=True)
    add("slicing", "slice_8psk_atan<AtanTabDev>", "slice8_atan", "slice8", 0)
    add("slicing", "slice_8psk_atan<AtanTabWave>", "slice8_atan", "slice8", 1, divergent=True)
    add("slicing", "qpsk_bits(reference map)", "qpsk", "qpsk", 0)
    add("slicing", "qpsk_bits(sign map)", "qpsk", "qpsk", 1)
    add("complex", "norm_f", "norm", "norm")
    add("complex", "cmul<true>", "cmul", "cmul", 1, divergent=True)
    add("complex", "cmul<false>", "cmul", "cmul", 0, rule="finite")
    add("complex", "cdiv<true>", "cdiv", "cdiv", divergent=True)
    for M in CPOW_M:
        add("cpow", "cpow_uint<true>(M=%d)" % M, "cpow", "cpow/%d" % M, M | 0x100, divergent=True)
        add("cpow", "cpow_uint<false>(M=%d)" % M, "cpow", "cpow/%d" % M, M, rule="finite")
    add("unwrap_fit", "to_long_x86(dep=0)", "to_long", "to_long", 0)
    add("unwrap_fit", "to_long_x86(dep varying)", "to_long", "to_long", 1)
    add("unwrap_fit", "unwrap_count(dep=0)", "unwrap", "unwrap", 0)
    add("unwrap_fit", "unwrap_count(dep varying)", "unwrap", "unwrap", 1)
    add("unwrap_fit", "wrap_test", "wrap_test", "wrap_test")
    add("unwrap_fit", "fit_denominator", "fit_den", "fit_den")
    add("unwrap_fit", "fit_value", "fit_value", "fit_value")
    add("fit_known", "fit_known + fit_value_known", "fit_known", "fit_known")
    add("wave", "wave_scan_f64", "scan_f64", "scan_f64")
    add("wave", "wave_sum_f64", "sum_f64", "scan_f64")
    add("wave", "wave_scan_i32", "scan_i32", "scan_i32")
    for N in range(1, 33):
        add("wave", "wave_scan_f32_multi<%d>" % N, "scan_f32_multi", "scan_f32_multi/%d" % N, N)
    add("wave", "wave_max_f32", "max_f32", "max_f32")
    add("wave", "wave_max_u32", "max_u32", "u32")
    add("wave", "wave_min_u32", "min_u32", "u32")
    for p, t in enumerate(("i32", "f32", "f64")):
        add("wave", "wave_up1(%s)" % t, "up1", "up1/" + t, p, rule="raw")
        add("wave", "wave_up1_zero(%s)" % t, "up1_zero", "up1/" + t, p, rule="raw", n_in=1)
    add("wave", "read_lane(f32)", "read_lane", "read_lane/f32", 1, rule="raw")
    add("wave", "read_lane(f64)", "read_lane", "read_lane/f64", 2, rule="raw")
    add("wave", "med3_i32", "med3", "med3")
    add("any", "any_merge", "any_merge", "any_merge", rule="zeros")
    add("any", "any_max_f64", "any_max_f64", "any_f64", rule="zeros")
    add("any", "any_min_u32", "any_min_u32", "any_u32")
    add("any", "any_max_f64_multi<%d>" % ANY_U, "any_max_f64_multi", "any_f64_multi/%d" % ANY_U, ANY_U, rule="zeros")
    add("any", "any_min_u32_multi<%d>" % ANY_U, "any_min_u32_multi", "any_u32_multi/%d" % ANY_U, ANY_U)
    return T


FORMS = _forms()
FAMILIES = ("libm", "slicing", "complex", "cpow", "unwrap_fit", "fit_known", "wave", "any")
assert {f.family for f in FORMS} == set(FAMILIES) and {f.kind for f in FORMS} == set(KINDS)


def form_reference(form, inputs):
    """the reference outputs of a form over the inputs of its kind (any order of cases)"""
    return reference(form.op, inputs if form.n_in is None else inputs[:form.n_in], form.param)


def compare_mask(form, ref):
    """per output: None (compare everywhere) or the cases that count, from the reference alone"""
    if form.rule == "finite":
        fin = np.isfinite(ref[0]) & np.isfinite(ref[1])
        return [fin, fin]
    if form.rule == "slice8_fast":
        return [ref[1] == 0, None]
    return [None] * len(ref)

