"""The inputs of tests/test_gpu_prepass_probe.py, built without a GPU: tests/test_prepass_probe.py asserts what each of them
has to reach (nothing about them is left to chance), the GPU tests launch them.  Every builder is cached: a case is built,
and its models run, once a session."""
import functools

import numpy as np

from tests import fir_model as fm
from tests import prepass_probe as pp
from tests import resample_model as rm  # noqa: F401  (the tests reach the model through this module)
from tests import tune_model as tm

F32 = np.float32
ONE = 1 << 32
STEP_837 = int(8.37 / 8 * 2.0 ** 32)
DRAWN_STEPS = (0x9E3779B9, 0x1B504F333, 0xC90FDAA2)  # (0.618, 1.707 and 0.785 input samples an output)
STEPS = (1 << 31, ONE, 1 << 33, STEP_837) + DRAWN_STEPS
FRACTIONS = (0, 255, 256, 0xFFFFFFFF)  # (255: mu is 0 though the fraction is not)
POS_MAX = 1 << 33
NEG = (1 << 63) + 12345
TUNE_STEPS = (tm.step_word(0.003), tm.step_word(-0.01), 1, NEG)


@functools.lru_cache(maxsize=None)
def piece():
    """kResamplePiece, from the header the kernel is built with"""
    return pp.constant("resample_piece")


def samples(rng, fmt, n, scale=None):
    """n complex samples in the format's dtype: int8-range values for the integer and half formats, floats with every mantissa
    bit in use for float32; with `scale` (a power of two; float32 only) floats within +-4 times it"""
    if fmt == pp.FORMAT_CF32:
        if scale is None:
            return (rng.standard_normal(2 * n) * 40.0).astype(F32)
        return (np.clip(rng.standard_normal(2 * n), -4.0, 4.0).astype(F32) * F32(scale)).astype(F32)
    assert scale is None
    return rng.integers(-127, 128, 2 * n).astype(pp.DTYPE_OF[fmt])


def _history(rng, k):
    """every third packet starts from the handle's zeros, the others from a history preset in the arena"""
    return None if k % 3 == 0 else (rng.standard_normal(6) * 30.0).astype(F32)


def _packet(rng, k, n, pos, rstep, fmt=None, stride=None, tuned=None, restart=None, scale=None):
    fmt = pp.FORMATS[k % 4] if fmt is None else fmt
    stride = (1, 7)[(k // 4 + k) % 2] if stride is None else stride
    tuned = (k // 2) % 3 != 1 if tuned is None else tuned
    restart = k % 5 == 2 if restart is None else restart
    hist = _history(rng, k)
    if hist is not None and scale is not None:
        hist = (np.clip(hist / F32(30.0), -4.0, 4.0).astype(F32) * F32(scale)).astype(F32)
    tune = ((0x9E3779B97F4A7C15 * (k + 1)) % (1 << 64), TUNE_STEPS[(k // 3) % 4]) if tuned else None
    return dict(fmt=fmt, stride=stride, iq=samples(rng, fmt, n, scale), tune=tune, pos=pos, rstep=rstep, restart=restart, hist=hist)


# ---- resample: launch shapes -----------------------------------------------------------------------------------------------------

def _long_outputs(P):
    """packets, longest n_out and the n_out of the long packets of each launch shape"""
    return {
        1: (1, 3 * P + 1, [3 * P + 1]),
        700: (700, 7 * P + 1, [7 * P + 1, 6 * P, 5 * P + 2, 4 * P - 1, 3 * P + 1, 2 * P, P + 1, P, P - 1, 7 * P]),
        1100: (1100, 6 * P - 1, [2 * P + 1, 3 * P, 4 * P + 2, 5 * P + 3, 6 * P - 1, 5 * P + 3, 4 * P + 2, 3 * P, 2 * P + 1, P + 7]),
        2100: (2100, 4 * P, [4 * P, 4 * P - 1, 3 * P + 1, 2 * P + 2, P + 1, 3 * P, 2 * P, P, 4 * P - 3, P + 513]),
    }


SHAPES = (1, 700, 1100, 2100)


@functools.lru_cache(maxsize=None)
def resample_shape(packets, variant=0):
    """A launch of `packets` packets (a key of _long_outputs).  About ten are long, spread over the launch; the others have 1 ..
    40 samples, n = 1, 2 and 3 and the packets without output whose history still moves (pos 2^33, n 1 or 2) among them.
    variant: the one-packet shape in another format, stride, tune and history."""
    P = piece()
    n_pk, longest, longs = _long_outputs(P)[packets]
    rng = np.random.default_rng(7000 + packets + variant)
    at = {(j * n_pk) // len(longs) + (3 if n_pk > 3 else 0): j for j in range(len(longs))}
    out = []
    for i in range(n_pk):
        k = i + variant
        if i in at:
            j = at[i]
            step = STEPS[(j + variant) % len(STEPS)]
            n, pos = pp.length_for(longs[j], step)
            out.append(_packet(rng, j + variant, n, pos, step))
            continue
        step = STEPS[k % len(STEPS)]
        if k % 50 == 10:  # no output, but the history moves
            out.append(_packet(rng, k, 1 + (k // 50) % 2, POS_MAX, step))
        else:
            n = (1, 2, 3)[k % 3] if k % 20 == 1 else 1 + (k * 13) % 40
            pos = (FRACTIONS[k % 4] + ONE * (k % 2)) if k % 7 == 0 else int(rng.integers(0, step))
            out.append(_packet(rng, k, n, pos, step))
    case = pp.ResampleCase(out)
    assert case.max_n_out == longest
    return case


# ---- resample: arithmetic edges ----------------------------------------------------------------------------------------------------

TINY, HUGE = 2.0 ** -130, 2.0 ** 125


@functools.lru_cache(maxsize=None)
def resample_edges():
    """(the case, {name: descriptors of that kind}).  Every step with every pos fraction, at an integer part of 0 and of 1; pos
    2^33; float32 samples scaled by 2^-130 (every product w * s is subnormal) and up to 2^125 (y stays finite); packets of zeros
    of both signs at step 2^32, pos 0."""
    rng = np.random.default_rng(7100)
    out, kinds = [], {}

    def add(kind, p):
        kinds.setdefault(kind, []).append(len(out))
        out.append(p)

    k = 0
    for step in STEPS:
        for frac in FRACTIONS:
            pos = frac + ONE * (k % 2)
            if pos < POS_MAX:
                add("grid", _packet(rng, k, 290 + 17 * (k % 9), pos, step))
            k += 1
        add("pos_max", _packet(rng, k, 300 + k % 5, POS_MAX, step))
        k += 1
    for j, step in enumerate((STEP_837, 1 << 31, 1 << 33, DRAWN_STEPS[0])):
        add("tiny", _packet(rng, k + j, 700 + j, (j * 0x3243F6A9) % step, step, fmt=pp.FORMAT_CF32, stride=(1, 7)[j % 2], tuned=j >= 2,
                            restart=j == 1, scale=TINY))
    k += 4
    for j, step in enumerate((STEP_837, 1 << 31, 1 << 33, DRAWN_STEPS[1])):
        p = _packet(rng, k + j, 600 + j, (j * 0x9E3779B1) % step, step, fmt=pp.FORMAT_CF32, stride=1, tuned=j >= 2, restart=True)
        # (uniform in (-2^125, 2^125); a tuned sample grows by sqrt(2) at the most, an output by the weights' 1.25)
        p["iq"] = (rng.uniform(-1.0, 1.0, p["iq"].size) * HUGE * (0.5 if j >= 2 else 1.0)).astype(F32)
        p["iq"][:4] = F32(HUGE * (0.5 if j >= 2 else 1.0)) * np.array([1, -1, -1, 1], F32)
        add("huge", p)
    k += 4
    for j, fmt in enumerate((pp.FORMAT_CF32, pp.FORMAT_CF16, pp.FORMAT_CF32, pp.FORMAT_CF16)):
        p = _packet(rng, k + j, 257 + j, 0, ONE, fmt=fmt, stride=(1, 7)[j % 2], tuned=False, restart=j < 2)
        z = np.where(rng.integers(0, 2, p["iq"].size) == 1, -0.0, 0.0)
        if j >= 2:  # zeros of both signs between samples that are not zero
            z = np.where(rng.integers(0, 3, z.size) == 0, rng.integers(-9, 10, z.size).astype(np.float64), z)
        p["iq"] = z.astype(pp.DTYPE_OF[fmt])
        if p["hist"] is not None:
            p["hist"] = np.array([0.0, -0.0, -0.0, 0.0, 1.0, -0.0], F32)
        add("zeros", p)
    return pp.ResampleCase(out), kinds


# ---- tune ------------------------------------------------------------------------------------------------------------------------------

TUNE_LENGTHS = (1, 2, 511, 512, 513, 8191, 8192, 8193, 70001)  # the edges of kTuneMinPiece and of the 512-sample unit
TUNE_COUNTS = (1, 200, 300, 2100)
# (phase, step): step 0 with a phase, the least step, half a turn a sample, one below a whole turn, and two ordinary ones
TUNE_WORDS = ((0x6A09E667F3BCC908, 0), (0x123456789ABCDEF0, 1), (0xBB67AE8584CAA73B, 1 << 63), (5, (1 << 64) - 1),
              (0x9E3779B97F4A7C15, TUNE_STEPS[0]), (0x3C6EF372FE94F82B, NEG))


def tune_grid(n_desc, max_n):
    """(workgroups per packet, samples of a piece), as psk::launch_tune (psk_tune.hip) shapes its grid: kTuneMinPiece 8192,
    about 2048 workgroups in all, a piece a multiple of 2 * kTuneThreads = 512.  The numbers are that file's literals."""
    per = max(1, min(-(-max_n // 8192), -(-2048 // n_desc), 65535))
    return per, -(-(-(-max_n // per)) // 512) * 512


@functools.lru_cache(maxsize=None)
def tune_case(count):
    """`count` packets.  The first ones walk TUNE_LENGTHS in the four formats at stride 1 and stride 5 (72 packets, as far as
    `count` lets them; the one-packet launch is the longest length), the rest have 1 .. 600 samples.  One float32 packet is
    scaled by 2^-130."""
    rng = np.random.default_rng(7200 + count)
    out = []
    grid = [(n, fmt, stride) for n in reversed(TUNE_LENGTHS) for fmt in pp.FORMATS for stride in (1, 5)]
    for i in range(count):
        if i < len(grid):
            n, fmt, stride = grid[i]
            if n == 70001 and stride > 1 and fmt != pp.FORMAT_CS8:
                n = 20001  # (the long strided matrix once, in the narrowest format: the arena stays small)
        else:
            n, fmt, stride = 1 + (i * 37) % 600, pp.FORMATS[i % 4], (1, 5)[(i // 4) % 2]
        phase, step = TUNE_WORDS[i % len(TUNE_WORDS)]
        scale = TINY if fmt == pp.FORMAT_CF32 and i % 24 in (8, 17) and n > 1 else None  # (8193 at stride 1, 8192 at stride 5, ..)
        out.append(dict(fmt=fmt, stride=stride, iq=samples(rng, fmt, n, scale), phase=phase, step=step, tiny=scale is not None))
    return pp.TuneCase(out)


# ---- gathers ---------------------------------------------------------------------------------------------------------------------------

SINGLES_COUNTS = (1, 300, 2100)
SINGLES_LENGTHS = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)


def singles_grid(n_desc, max_n):
    """workgroups per packet, as psk::launch_gather_singles (psk_gather.hip) shapes its grid (its literals)"""
    return max(1, min(-(-max_n // 1024), -(-2048 // n_desc), 65535))


@functools.lru_cache(maxsize=None)
def singles_case(sample_bytes, count):
    """`count` packets of 1 .. 4097 samples (one packet: 4097): SINGLES_LENGTHS first, then lengths spread over 1 .. 400;
    strides 1, 3 and 11"""
    pk = []
    for i in range(count):
        n = 4097 if count == 1 else SINGLES_LENGTHS[-1 - i] if i < len(SINGLES_LENGTHS) else 1 + (i * 29) % 400
        pk.append((n, (3, 11, 1)[i % 3]))
    return pp.SinglesCase(sample_bytes, pk, 7300 + 10 * count + sample_bytes)


TILE_WIDTHS = (8, 9, 63, 64, 65, 130)
TILE_LENGTHS = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def tiles_widths_case(sample_bytes):
    """one group of each width of TILE_WIDTHS, the columns' lengths walking TILE_LENGTHS from another start in each group"""
    groups = [([TILE_LENGTHS[(j + k) % len(TILE_LENGTHS)] for j in range(g)], k % 3, (k + 1) % 2) for k, g in enumerate(TILE_WIDTHS)]
    return pp.TilesCase(sample_bytes, groups, 7400 + sample_bytes)


TILE_MANY = 2100


@functools.lru_cache(maxsize=None)
def tiles_many_case(sample_bytes):
    """2100 groups of 8 columns by 10 frames: 2100 tiles on a grid of 2048 workgroups, so `tl += gridDim.x` takes a second trip"""
    return pp.TilesCase(sample_bytes, [([10] * 8, k % 2, 1) for k in range(TILE_MANY)], 7500 + sample_bytes)


# ---- fir -------------------------------------------------------------------------------------------------------------------------------

FIR_DS = tuple(range(1, fm.MAX_DECIM + 1))


def fir_taps(rng, T):
    return (rng.standard_normal(T) / np.sqrt(T)).astype(F32)


def fir_length(n_out, D, pos, extra=0):
    """a packet length with exactly n_out >= 1 outputs at (D, pos): the last output's newest input, and up to D - 1 more"""
    n = pos + (n_out - 1) * D + 1 + extra % D
    assert fm.count(pos, D, n) == n_out
    return n


def _fir_packet(rng, k, D, pos, n, T, fmt=None, stride=None, tuned=None, restart=None):
    """packet k of a launch: format, stride, tune, restart and the kind of history follow from k as in _packet"""
    fmt = pp.FORMATS[k % 4] if fmt is None else fmt
    stride = (1, 7)[(k // 4 + k) % 2] if stride is None else stride
    tuned = (k // 2) % 3 != 1 if tuned is None else tuned
    restart = k % 5 == 2 if restart is None else restart
    hist = None if k % 3 == 0 else (rng.standard_normal(2 * fm.HIST) * 30.0).astype(F32)
    tune = ((0x9E3779B97F4A7C15 * (k + 1)) % (1 << 64), TUNE_STEPS[(k // 3) % 4]) if tuned else None
    return dict(fmt=fmt, stride=stride, iq=samples(rng, fmt, n), tune=tune, taps=fir_taps(rng, T), D=D, pos=pos, restart=restart, hist=hist)


def fir_grid_taps(D):
    """the tap counts of the grid at D: 1, 2, the three around the lead of the lane's first output, 64, 127, 128"""
    lead = pp.fir_split(D, 1)[0]
    return sorted({min(max(t, 1), fm.MAX_TAPS) for t in (1, 2, lead, lead + 1, lead + 2, 64, 127, 128)})


def fir_grid_outputs(D):
    P = pp.fir_piece(D)
    return (1, 2, 3, 4, 5, P - 1, P, P + 1, 2 * P + 1)


@functools.lru_cache(maxsize=None)
def fir_grid(D):
    """One launch at the decimation D: fir_grid_taps(D) x fir_grid_outputs(D), pos walking every value below D"""
    rng = np.random.default_rng(7600 + D)
    out = []
    for T in fir_grid_taps(D):
        for n_out in fir_grid_outputs(D):
            k = len(out)
            pos = k % D
            out.append(_fir_packet(rng, k, D, pos, fir_length(n_out, D, pos, k), T))
    return pp.FirCase(out)


FIR_SHAPES = (700, 1100, 2100)
# the ten long packets of a shape: a D of each lane class and of both LDS layouts, and tap counts of every part of the walk
FIR_LONG_DS = (1, 4, 9, 16, 3, 7, 15, 8, 2, 12)
FIR_LONG_TAPS = (128, 2, 64, 127, 10, 1, 33, 128, 5, 64)
FIR_JOIN_LENGTHS = (1, 2, 126, 127, 128)  # the join of the old history and a packet shorter than it


@functools.lru_cache(maxsize=None)
def fir_shape(packets):
    """A launch of `packets` packets, D mixed by index over 1 .. 16.  Ten are long, spread over the launch: their outputs are
    _long_outputs(P)[packets] at the P of their own D.  The others have 1 .. 40 samples, or one of FIR_JOIN_LENGTHS; every 50th
    has pos >= n: no output, and a history that still moves."""
    rng = np.random.default_rng(7700 + packets)
    at = {(j * packets) // 10 + 3: j for j in range(10)}
    out = []
    for k in range(packets):
        if k in at:
            j = at[k]
            D = FIR_LONG_DS[j]
            pos = (j * 5) % D
            n_out = _long_outputs(pp.fir_piece(D))[packets][2][j]
            out.append(_fir_packet(rng, j, D, pos, fir_length(n_out, D, pos, j), FIR_LONG_TAPS[j]))
            continue
        T = 1 + (k * 29) % fm.MAX_TAPS
        if k % 50 == 10:  # no output, but the history moves
            D = 2 + (k // 50) % 15
            pos = D - 1
            out.append(_fir_packet(rng, k, D, pos, 1 + (k // 50) % pos, T))
        else:
            D = 1 + (k * 7 + k // 16) % 16
            n = FIR_JOIN_LENGTHS[(k // 20) % 5] if k % 20 == 1 else 1 + (k * 13) % 40
            out.append(_fir_packet(rng, k, D, (k * 3 + k // 16) % D, n, T))
    return pp.FirCase(out)


FIR_EDGE_DS = (3, 5, 9)  # one D of each lane class: R = 4, 2 and 1
FIR_SUBNORMAL = np.uint32(0x00000011).view(F32)
# (None: an ordinary tap)
FIR_SPECIAL_TAPS = (FIR_SUBNORMAL, F32(0.0), F32(-0.0), None, -FIR_SUBNORMAL)


@functools.lru_cache(maxsize=None)
def fir_edges():
    """(the case, {name: descriptors of that kind}), every kind at each D of FIR_EDGE_DS with T = 1 among its tap counts.
    tiny: float32 samples (and history) scaled by 2^-130 under taps of 0.5 .. 1.5 in magnitude: every product is subnormal.
    subtaps: taps that are subnormal (0x00000011, either sign), +0 and -0 between ordinary ones, each of them as tap 0.
    zeros: samples that are zeros of both signs (alone, and between small integers) under negative taps.
    huge: samples up to 2^125 / T under taps of at most 1 in magnitude: no sum overflows."""
    rng = np.random.default_rng(7800)
    out, kinds = [], {}

    def add(kind, p):
        kinds.setdefault(kind, []).append(len(out))
        out.append(p)

    for a, D in enumerate(FIR_EDGE_DS):
        for b, T in enumerate((1, 7, 40)):
            k = len(out)
            p = _fir_packet(rng, k, D, k % D, 150 + 7 * k, T, fmt=pp.FORMAT_CF32, stride=(1, 7)[(a + b) % 2], tuned=(a + b) % 3 == 2, restart=b == 1 and a != 1)
            p["iq"] = samples(rng, pp.FORMAT_CF32, 150 + 7 * k, TINY)
            p["hist"] = samples(rng, pp.FORMAT_CF32, fm.HIST, TINY)
            p["taps"] = (rng.uniform(0.5, 1.5, T) * rng.choice((-1.0, 1.0), T)).astype(F32)
            add("tiny", p)
        for v in range(3):  # (tap 0 is the subnormal, +0, -0)
            k = len(out)
            T = (1, 6, 19)[(a + v) % 3]
            p = _fir_packet(rng, k, D, k % D, 90 + 11 * k, T, tuned=v == 1)
            for i in range(T):
                if FIR_SPECIAL_TAPS[(i + v) % 5] is not None:
                    p["taps"][i] = FIR_SPECIAL_TAPS[(i + v) % 5]
            add("subtaps", p)
        for b, T in enumerate((1, 3)):
            k = len(out)
            fmt = (pp.FORMAT_CF32, pp.FORMAT_CF16)[(a + b) % 2]
            p = _fir_packet(rng, k, D, k % D, 120 + 5 * k, T, fmt=fmt, stride=(1, 7)[b], tuned=False, restart=b == 0)
            z = np.where(rng.integers(0, 2, p["iq"].size) == 1, -0.0, 0.0)
            if (a + b) % 2:  # zeros of both signs between samples that are not zero
                z = np.where(rng.integers(0, 3, z.size) == 0, rng.integers(-9, 10, z.size).astype(np.float64), z)
            p["iq"] = z.astype(pp.DTYPE_OF[fmt])
            p["hist"] = np.where(rng.integers(0, 2, 2 * fm.HIST) == 1, -0.0, 0.0).astype(F32)
            p["taps"] = (-rng.uniform(0.25, 1.0, T)).astype(F32)
            add("zeros", p)
        for b, T in enumerate((1, 16, 128)):
            k = len(out)
            tuned = (a + b) % 3 == 0
            top = HUGE / T * (0.5 if tuned else 1.0)  # (a tuned sample grows by sqrt(2) at the most)
            p = _fir_packet(rng, k, D, k % D, 300 + 9 * k, T, fmt=pp.FORMAT_CF32, stride=1, tuned=tuned, restart=True)
            p["iq"] = (rng.uniform(-1.0, 1.0, p["iq"].size) * top).astype(F32)
            p["iq"][:4] = F32(top) * np.array([1, -1, -1, 1], F32)
            p["taps"] = rng.uniform(-1.0, 1.0, T).astype(F32)
            p["taps"][0] = 1.0
            add("huge", p)
    return pp.FirCase(out), kinds
