"""The inputs of tests/test_gpu_prepass_probe.py, built without a GPU: tests/test_prepass_probe.py asserts what each of them
has to reach (nothing about them is left to chance), the GPU tests launch them.  Every builder is cached: a case is built,
and its models run, once a session."""
import functools

import numpy as np

from tests import acquire_model as am
from tests import fir_model as fm
from tests import prepass_probe as pp
from tests import resample_model as rm  # noqa: F401  (the tests reach the model through this module)
from tests import symrate_model as sm
from tests import sync_model as ym
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


# ---- the two looks (psk_symrate.hip, psk_acquire.hip): fold and join ---------------------------------------------------------------

SR_WIDTHS = (1, 2, 4, 8, 16, 32, 64)
SR_CLASS_S = {1: (4, 5, 8), 2: (9, 16), 4: (17, 24, 32), 8: (33, 64), 16: (65, 100, 128), 32: (129, 200, 256), 64: (257, 511, 1000, 1024)}
NONFINITE = (np.nan, np.inf, -np.inf)
BIG_PACKET_BYTES = 1 << 20  # a source matrix above this is laid out contiguous, in a narrow format: the arenas stay below 64 MiB
LOOP_DESCRIPTORS, LOOP_PAIRS = 70000, 70000 - pp.LOOK_GRID_MAX  # 4465 descriptors have a partner on the second trip


def sr_block_counts(W):
    """the block counts of a width's launch, G = 64 / W blocks a wave at a time: either side of one wave, of the four waves of a
    workgroup, of a turn of stage 2 (256), of a piece (512), of the halo behind it (128) and of two pieces; without 1025 at the two
    widest classes"""
    G = 64 // W
    c = {2, 3, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 255, 256, 257, 511, 512, 513, 512 + 127, 512 + 128, 512 + 129, 1025}
    return sorted(b for b in c if b >= 2 and not (W >= 32 and b == 1025))


def sr_signal(S, n, seed):
    """interleaved float32: noisy QPSK at 1.04 S samples a symbol with a shaped pulse (the signal of tests/test_symrate_control.py)"""
    rng = np.random.default_rng(seed)
    u = np.arange(n) / (1.04 * S)
    sym = rng.integers(0, 4, int(u[-1]) + 2)[np.floor(u).astype(int)]
    z = (0.2 + 0.8 * np.sin(np.pi * (u - np.floor(u)))) * np.exp(2j * np.pi * (sym / 4 + 0.002 * np.arange(n)))
    x = np.empty(2 * n, F32)
    x[0::2] = z.real + 0.05 * rng.standard_normal(n)
    x[1::2] = z.imag + 0.05 * rng.standard_normal(n)
    return x


def _as_format(x, fmt):
    """float32 samples of about unit size in the format's dtype (the integer and half formats: scaled by 40, int8's range)"""
    return x if fmt == pp.FORMAT_CF32 else np.clip(np.round(40.0 * x), -127, 127).astype(pp.DTYPE_OF[fmt])


def _look_mix(k, n):
    """format, stride, skew and tune of packet k of a look launch, mixed by index as _packet mixes them; a packet whose matrix
    would be large is contiguous, and CS8 if it still is"""
    fmt, stride = pp.FORMATS[k % 4], (1, 7)[(k // 4 + k) % 2]
    if n * pp.SAMPLE_BYTES[fmt] * stride > BIG_PACKET_BYTES:
        stride = 1
        if n * pp.SAMPLE_BYTES[fmt] > BIG_PACKET_BYTES:
            fmt = (pp.FORMAT_CS8, pp.FORMAT_CS16, pp.FORMAT_CF16)[k % 3] if n * 4 <= BIG_PACKET_BYTES else pp.FORMAT_CS8
    tune = ((0x9E3779B97F4A7C15 * (k + 1)) % (1 << 64), TUNE_STEPS[(k // 3) % 4]) if (k // 2) % 3 != 1 else None
    return dict(fmt=fmt, stride=stride, skew=pp.SAMPLE_BYTES[fmt] if k % 2 else 0, tune=tune)


@functools.lru_cache(maxsize=None)
def symrate_width(W):
    """One launch of every S of a width class x sr_block_counts(W): a ragged tail of 0, S - 1 or 3 samples; the four formats,
    strides 1 and 7, tuned and not, mixed by index"""
    protos = []
    for S in SR_CLASS_S[W]:
        assert sm.width(S) == W
        for b in sr_block_counts(W):
            k = len(protos)
            n = b * S + (0, S - 1, 3)[k % 3]
            p = _look_mix(k, n)
            p.update(S=S, blocks=b, iq=_as_format(sr_signal(S, n, 8000 + 64 * S + k), p["fmt"]))
            protos.append(p)
    return pp.LookCase("symrate", protos, [(k, True) for k in range(len(protos))])


SR_VALIDITY_S = {1: 5, 2: 9, 4: 17, 8: 33, 16: 100, 32: 200, 64: 257}  # an S of each width whose last turn is ragged (W > 1)


def sr_bad_positions(S):
    """positions of a block a bad sample goes to: 0, W - 1, W (lane 0's second turn), the first position of the last turn --
    ragged: `p < S` is false for part of the wave --, S - 1"""
    W = sm.width(S)
    return sorted({0, W - 1, min(W, S - 1), (S - 1) // W * W, S - 1})


def sr_wave_slot(b, G):
    """(turn-and-wave index, sub) of block b in stage 1's walk of its own piece: `base = start + wave * G + turn * 4 G`, start a
    multiple of 64 -- the blocks of one index share a wave's ballot"""
    lo = b // sm.PIECE * sm.PIECE
    start = lo - sm.HALO if lo else 0
    return (b - start) // G, (b - start) % G


def sr_bad_blocks(nb, G):
    """blocks a bad sample goes to: one that is sub 0 of its wave, one that is sub G - 1, the packet's last block; with two
    pieces, in the second piece's own blocks"""
    at = 512 + 2 * G if nb > 512 + 3 * G else (17 // G) * G
    return sorted({at, min(at + G - 1, nb - 2), nb - 1})


@functools.lru_cache(maxsize=None)
def symrate_validity(W):
    """One launch at S = SR_VALIDITY_S[W]: packets of 40, 41 and 642 blocks, one non-finite value each (NaN, +inf, -inf in turn,
    real or imaginary part) at every sr_bad_positions x sr_bad_blocks; the last sample of block 511 (it takes blocks 511 and 512
    out, in piece 1's own blocks and in its halo) and of block 383 (in piece 1's halo only).  p["bad"]: the blocks the
    definition invalidates."""
    S, G = SR_VALIDITY_S[W], 64 // W
    assert sm.width(S) == W
    base = {nb: sr_signal(S, nb * S + 3, 8500 + S + nb) for nb in (40, 41, 642)}
    spots = [(nb, b, pos) for nb in (40, 41, 642) for b in sr_bad_blocks(nb, G) for pos in sr_bad_positions(S)]
    spots += [(642, 511, S - 1), (642, 383, S - 1)]
    protos = []
    for nb, b, pos in spots:
        k = len(protos)
        p = _look_mix(k, nb * S + 3)
        # (a non-finite value needs a float format; half the packets are CF16)
        p["fmt"] = (pp.FORMAT_CF32, pp.FORMAT_CF16)[k % 2] if (nb * S + 3) * 8 * p["stride"] <= BIG_PACKET_BYTES else pp.FORMAT_CF16
        p["skew"] = pp.SAMPLE_BYTES[p["fmt"]] if k % 2 else 0
        x = base[nb].copy() if p["fmt"] == pp.FORMAT_CF32 else (40.0 * base[nb]).astype(np.float16)
        x[2 * (b * S + pos) + (k // 3) % 2] = NONFINITE[k % 3]
        bad = {b, b + 1} if pos == S - 1 and b + 1 < nb else {b}
        p.update(S=S, blocks=nb, iq=x, bad=bad, spot=(nb, b, pos))
        protos.append(p)
    return pp.LookCase("symrate", protos, [(k, True) for k in range(len(protos))])


@functools.lru_cache(maxsize=None)
def symrate_edges():
    """(the case, {name: descriptors of that kind}), at an S of four widths.  tiny: float32 samples scaled by 2^-130 (every e and g
    is zero or subnormal: a flush anywhere would show); huge: 3e19 -- every e overflows, no block is valid; zeros: zeros of both
    signs, alone and between small integers"""
    rng = np.random.default_rng(8700)
    protos, kinds = [], {}
    for j, S in enumerate((8, 24, 200, 257)):
        for kind in ("tiny", "huge", "zeros"):
            k = len(protos)
            n = (40, 530, 700)[(j + k) % 3] * S + 3
            p = _look_mix(k, n)
            p["fmt"] = pp.FORMAT_CF32 if kind != "zeros" or k % 2 else pp.FORMAT_CF16
            p["skew"] = pp.SAMPLE_BYTES[p["fmt"]] if k % 2 else 0
            if n * pp.SAMPLE_BYTES[p["fmt"]] * p["stride"] > BIG_PACKET_BYTES:
                p["stride"] = 1
            x = sr_signal(S, n, 8700 + k)
            if kind == "tiny":
                x = (x * F32(TINY)).astype(F32)
            elif kind == "huge":
                x = (x * F32(3e19)).astype(F32)
            else:
                z = np.where(rng.integers(0, 2, x.size) == 1, -0.0, 0.0)
                if j % 2:
                    z = np.where(rng.integers(0, 3, z.size) == 0, rng.integers(-9, 10, z.size).astype(np.float64), z)
                x = z.astype(pp.DTYPE_OF[p["fmt"]])
            p.update(S=S, iq=x)
            kinds.setdefault(kind, []).append(k)
            protos.append(p)
    return pp.LookCase("symrate", protos, [(k, True) for k in range(len(protos))]), kinds


# ---- the packet loop: more descriptors than a grid has workgroups ------------------------------------------------------------------

LOOP_KINDS = ("two pieces, then a first piece of three", "a first piece of three, then two pieces", "data, then none", "invalid, then valid")


def loop_uses(n_small):
    """the (proto, data) of the 70000 descriptors over protos 0 two pieces, every unit valid; 1 a first piece of three units; 2
    two pieces with invalid units; 3 one short valid piece; 4 .. 4 + n_small - 1 short packets.  Descriptor c < 4465 and its
    partner c + 65535, which the same workgroups take on their second trip, are of LOOP_KINDS[c % 4]; of the others every
    seventh has no data."""
    first = ((0, True), (1, True), (0, True), (2, True))
    second = ((1, True), (0, True), (4, False), (3, True))
    uses = []
    for c in range(LOOP_DESCRIPTORS):
        if c < LOOP_PAIRS:
            uses.append(first[c % 4] if c % 4 != 2 or c % 8 == 2 else (4 + c % n_small, True))
        elif c >= pp.LOOK_GRID_MAX:
            uses.append(second[(c - pp.LOOK_GRID_MAX) % 4])
        else:
            uses.append((4 + (c * 7) % n_small, c % 7 != 0))
    return uses


@functools.lru_cache(maxsize=None)
def symrate_loop():
    """70000 descriptors, max_piece 2, 24 distinct packets: loop_uses over two pieces of S = 4 (600 blocks), three blocks of S =
    5, 600 blocks of S = 4 with NaNs in blocks 100, 511 and 599, five blocks of S = 8, and 2 .. 5 blocks of S = 4 .. 8"""
    protos = []

    def add(S, blocks, tail, bad=()):
        k = len(protos)
        n = blocks * S + tail
        p = _look_mix(k, n)
        if bad:
            p["fmt"] = pp.FORMAT_CF32
        x = _as_format(sr_signal(S, n, 8800 + k), p["fmt"])
        for b in bad:
            x[2 * (b * S + 1)] = np.nan
        p.update(S=S, blocks=blocks, iq=x, bad=set(bad))
        protos.append(p)

    add(4, 600, 3)
    add(5, 3, 4)
    add(4, 600, 0, bad=(100, 511, 599))
    add(8, 5, 7)
    for S in (4, 5, 6, 7, 8):
        for blocks in (2, 3, 4, 5):
            add(S, blocks, (0, S - 1, 3)[len(protos) % 3])
    return pp.LookCase("symrate", protos, loop_uses(20), spare_every=97)


# ---- acquire -----------------------------------------------------------------------------------------------------------------------

def acquire_lengths():
    """EDGE_LENGTHS of tests/test_gpu_acquire.py, and the three at which the join takes a second trip over the partials"""
    P = am.PIECE
    return (1, 2, 127, 128, 129, P - 1, P, P + 1, P + 127, P + 129, 2 * P + 5, 3 * P + 1, 64 * P, 64 * P + 1, 65 * P + 131)


def carrier(seed, M, n):
    """a noisy M-PSK carrier at 0.007 cycles per sample, 4 samples per symbol, interleaved float32"""
    rng = np.random.default_rng(seed)
    z = np.exp(2j * np.pi * (np.repeat(rng.integers(0, M, n // 4 + 1), 4)[:n] / M + 0.007 * np.arange(n))) * rng.uniform(0.8, 1.25)
    x = np.empty(2 * n, F32)
    x[0::2] = z.real + 0.08 * rng.standard_normal(n)
    x[1::2] = z.imag + 0.08 * rng.standard_normal(n)
    return x


PLACEMENTS = ("aligned", "skewed", "strided")


def _acquire_packet(k, n, M, fmt, place, tuned):
    """packet k: across the piece boundaries an inf, a NaN (float formats), a run of 200 zeros and a run of samples too small
    to be valid (float32: a = e, q or q * q lies below FLT_MIN), as the lengths allow"""
    P = am.PIECE
    x = carrier(9000 + 13 * k + M, M, n)
    floats = fmt in (pp.FORMAT_CF32, pp.FORMAT_CF16)
    x = _as_format(x, fmt) if fmt != pp.FORMAT_CF16 else (40.0 * x).astype(np.float16)
    marks = set()
    if n > P and k % 2 == 1 and floats:
        x[2 * (P - 1)], x[2 * P + 1] = np.inf, np.nan  # the last sample of piece 0, the first of piece 1
        marks.add("nonfinite")
    if n >= P + 127 and k % 3 == 0:
        x[2 * (P - 100) : 2 * min(n, P + 100)] = 0
        marks.add("zeros")
    if n >= 2 * P + 5 and floats:
        x[2 * (2 * P - 64) + 1] = -np.inf  # reaches over the next boundary through the longer lags
        marks.add("nonfinite")
    if n >= 129 and fmt == pp.FORMAT_CF32 and k % 2 == 0:
        lo = min(n, P) - 60 if n > 200 else 40
        x[2 * lo : 2 * min(n, lo + 90)] *= F32(1e-20)  # (e about 1e-40: below FLT_MIN)
        marks.add("underflow")
    tune = ((0x9E3779B97F4A7C15 * (k + 1)) % (1 << 64), TUNE_STEPS[(k // 3) % 4]) if tuned else None
    return dict(fmt=fmt, stride=7 if place == "strided" else 1, skew=pp.SAMPLE_BYTES[fmt] if place == "skewed" else 0, tune=tune, M=M, iq=x,
                place=place, marks=marks)


ACQUIRE_LONG = {False: ((pp.FORMAT_CF32, "aligned", 4), (pp.FORMAT_CS16, "skewed", 8), (pp.FORMAT_CS8, "strided", 2)),
                True: ((pp.FORMAT_CF16, "skewed", 2), (pp.FORMAT_CS8, "strided", 4), (pp.FORMAT_CF32, "aligned", 8))}


@functools.lru_cache(maxsize=None)
def acquire_lengths_case(mixed):
    """One launch.  Every (format, placement) takes every third of the twelve short lengths, so that each length meets four of
    them, M turning over 2, 4, 8; the three long lengths once each (ACQUIRE_LONG).  mixed False: no packet is tuned, the fold gets
    no tables; True: two packets in three are tuned."""
    lens = acquire_lengths()
    protos = []
    for q, (fmt, place) in enumerate((f, pl_) for f in pp.FORMATS for pl_ in PLACEMENTS):
        for i, n in enumerate(lens[:12]):
            if (i + q) % 3 == 0:
                k = len(protos)
                protos.append(_acquire_packet(k, n, (2, 4, 8)[(i // 3 + q) % 3], fmt, place, mixed and k % 3 != 1))
    for n, (fmt, place, M) in zip(lens[12:], ACQUIRE_LONG[mixed]):
        k = len(protos)
        protos.append(_acquire_packet(k, n, M, fmt, place, mixed and k % 3 != 1))
    return pp.LookCase("acquire", protos, [(k, True) for k in range(len(protos))], tables=mixed)


@functools.lru_cache(maxsize=None)
def acquire_loop():
    """70000 descriptors, max_piece 2, 24 distinct packets: loop_uses over P + 200 valid samples, three samples, P + 200 samples
    with invalid ones, five samples, and 2 .. 40 samples; tuned and untuned mixed"""
    P = am.PIECE
    protos = []

    def add(n, M, bad=False):
        k = len(protos)
        p = _look_mix(k, n)
        if bad:
            p["fmt"] = pp.FORMAT_CF32
        x = _as_format(carrier(9500 + k, M, n), p["fmt"])
        if bad:
            x[2 * 77], x[2 * (P - 1) + 1], x[2 * (n - 1)] = np.nan, np.inf, 0.0
        p.update(M=M, iq=x, bad=bad)
        protos.append(p)

    add(P + 200, 4)
    add(3, 2)
    add(P + 200, 8, bad=True)
    add(5, 4)
    for i in range(20):
        add(2 + (i * 7) % 39, (2, 4, 8)[i % 3])
    return pp.LookCase("acquire", protos, loop_uses(20), spare_every=97)


# ---- the word search (psk_sync.hip) --------------------------------------------------------------------------------------------------
#
# Rows of two kinds.  A COMB row is one repeated symbol under the word of two points a quarter turn apart: the window at a planted
# word has m = 1, the one in front of it 1/2, the one behind it 0 -- hits exactly where a case puts them, two windows apart if
# need be, and all of them equal bests.  A WORD row is noisy QPSK with a random QPSK word of length L written at given positions.
# Places are given as WINDOW INDICES (window k lies at position p0 + k; piece k // 1024) or as positions relative to x[0].

SY_P = ym.PIECE
SY_SYMBOL = 0.8 - 0.3j
COMB = np.array([1, 0, 0, 1], F32)
COMB_THR = 0.999


def _iq(z):
    x = np.empty(2 * len(z), F32)
    x[0::2], x[1::2] = z.real, z.imag
    return x


@functools.lru_cache(maxsize=None)
def _sync_word_z(L):
    rng = np.random.default_rng(500 + L)
    return ym.psk_points(4, rng.integers(0, 4, L))


def sync_word(L):
    """the word of length L: unit QPSK points, interleaved float32"""
    return _iq(_sync_word_z(L))


def comb_proto(n_windows, hits, restart, zero=(), skew=0):
    """a comb row of n_windows windows with a hit at each window index of `hits` (at least two apart); zero: (lo, hi) ranges of
    window indices whose symbols are all zeros -- none of those windows is valid"""
    hits = sorted(hits)
    assert all(b - a >= 2 for a, b in zip(hits, hits[1:])) and (not hits or 0 <= hits[0] and hits[-1] < n_windows)
    n, p0 = (n_windows + 1, 0) if restart else (n_windows, -1)
    z = np.full(ym.HIST + n, SY_SYMBOL)
    z[ym.HIST + p0 + np.asarray(hits, np.int64) + 1] *= 1j
    for lo, hi in zero:
        assert not any(lo - 1 <= h <= hi for h in hits)
        z[ym.HIST + p0 + lo: ym.HIST + p0 + hi + 1] = 0
    return dict(word=COMB, thr=COMB_THR, x=_iq(z[ym.HIST:]), restart=restart, hist=None if restart else _iq(z[:ym.HIST]), skew=skew, hits=hits,
                kind="comb")


def word_proto(L, n, restart, at, seed, sigma=0.05, thr=0.9, skew=0, clean=(), nan_at=None):
    """a noisy QPSK row of n symbols behind 127 symbols of history with the word of length L written at the positions `at`
    (relative to x[0]; cut at either end) in front of the noise and at the positions `clean` behind it; nan_at: a NaN symbol"""
    rng = np.random.default_rng(seed)
    wz = _sync_word_z(L) * SY_SYMBOL
    z = ym.psk_points(4, rng.integers(0, 4, ym.HIST + n)) * SY_SYMBOL
    noise = sigma * (rng.standard_normal(len(z)) + 1j * rng.standard_normal(len(z)))
    for places, late in ((at, False), (clean, True)):
        if late:
            z = z + noise
        for p in places:
            lo, hi = max(p + ym.HIST, 0), min(p + ym.HIST + L, len(z))
            if hi > lo:
                z[lo:hi] = wz[lo - p - ym.HIST: hi - p - ym.HIST]
    x = _iq(z[ym.HIST:])
    if nan_at is not None:
        x[2 * nan_at + 1] = np.nan
    return dict(word=sync_word(L), thr=thr, x=x, restart=restart, hist=None if restart else _iq(z[:ym.HIST]), skew=skew, kind="word")


def windows_proto(L, n_windows, restart, at, seed, **kw):
    """word_proto by its number of windows"""
    return word_proto(L, n_windows + (L - 1 if restart else 0), restart, at, seed, **kw)


# A. every word length

SYNC_LENGTH_WINDOWS = SY_P + 65  # two pieces, the second with one full turn of wave 0 and one lane of its second
SYNC_LENGTH_IDLE = 1900


@functools.lru_cache(maxsize=None)
def sync_lengths(spread):
    """L = 1 .. 128, each with a continued row (a word across the row's start, through hist_in) and a restarted one, P + 65
    windows each: 256 descriptors.  spread: the same 256 among 1900 descriptors without data -- one workgroup a channel, which
    walks both pieces."""
    protos = []
    for L in range(1, ym.MAX_WORD + 1):
        for restart in (False, True):
            n = SYNC_LENGTH_WINDOWS + (L - 1 if restart else 0)
            at = (3 if restart else -(L // 2), 200, SY_P - L // 2, n - L)
            protos.append(word_proto(L, n, restart, at, 11000 + 2 * L + restart, skew=8 if L % 2 else 0))
    if not spread:
        return pp.SyncCase(protos, [(k, True) for k in range(len(protos))])
    uses = [(0, False)] * (len(protos) + SYNC_LENGTH_IDLE)
    for k in range(len(protos)):
        uses[3 + 8 * k] = (k, True)
    return pp.SyncCase(protos, uses)


# B. workgroups that walk several pieces

SYNC_WALK_SHAPES = (700, 1100, 2100)
SYNC_WALK_LONG, SYNC_WALK_SHORT = (0, 1, 2, 3, 5, 10, 11), (6, 7, 8, 9, 4)
SYNC_WALK_CROWD, SYNC_WALK_ZEROS = (3, 400, 20), 2  # (piece, first window, hits) of proto 0's crowd; proto 1's piece without a valid window


def sync_walk_protos():
    P = SY_P
    pr = []
    # 0: comb, 7 pieces, restarted: three hits in every piece and 20 more in piece 3
    cp, c0, cn = SYNC_WALK_CROWD
    pr.append(comb_proto(6 * P + 950, [p * P + o for p in range(7) for o in (5, 300, 900)] + [cp * P + c0 + 4 * i for i in range(cn)], True))
    # 1: comb, 5 pieces, continued: a hit at position -1, piece 2 all zeros between pieces with valid windows
    pr.append(comb_proto(4 * P + 100, [0, 40, P + 7, P + 900, 3 * P + 1, 3 * P + 500, 4 * P + 2, 4 * P + 77], False,
                         zero=[(SYNC_WALK_ZEROS * P, (SYNC_WALK_ZEROS + 1) * P)], skew=8))
    # 2: L = 31, restarted, four whole pieces of one period of P symbols: the same best, bit for bit, in every piece
    seg = word_proto(31, P, True, (4,), 12001, sigma=0.1)["x"]
    pr.append(dict(word=sync_word(31), thr=0.7, x=np.concatenate([seg] * 4 + [seg[:60]]), restart=True, hist=None, skew=0, kind="periodic"))
    # 3 .. 5: L = 128 continued (a word across the row's start and one across a piece edge) and restarted, L = 31 continued
    pr.append(windows_proto(128, 2 * P + 300, False, (-64, 500, P - 64 - 127, 2 * P + 10), 12003, skew=8))
    pr.append(windows_proto(128, P + 1, True, (30, 700), 12004))
    pr.append(windows_proto(31, 3 * P + 77, False, (-15, 600, P + 3, 2 * P + 500, 3 * P + 10), 12005))
    # 6 .. 9: one and two pieces
    pr.append(comb_proto(39, [3, 20], True, skew=8))
    pr.append(comb_proto(P + 1, [0, P - 2, P], False))
    pr.append(windows_proto(31, 170, True, (50,), 12008, skew=8))
    pr.append(word_proto(128, 100, False, (-100,), 12009))
    # 10: comb, 3 pieces, restarted: 18 hits in each of pieces 1 and 2
    pr.append(comb_proto(2 * P + 500, [9, 700] + [P + 100 + 6 * i for i in range(18)] + [2 * P + 11 + 2 * i for i in range(18)], True))
    # 11: L = 31, 5 pieces, restarted, a NaN symbol at a piece edge
    pr.append(windows_proto(31, 4 * P + 9, True, (100, P + 100, 2 * P + 200, 3 * P + 5, 4 * P - 20), 12011, nan_at=2 * P))
    return pr


@functools.lru_cache(maxsize=None)
def sync_walk(n_desc):
    """700, 1100 and 2100 descriptors -- 3, 2 and 1 workgroups a channel -- over the twelve rows of sync_walk_protos: every 25th
    a row of 3 .. 7 pieces, every ninth without data, the rest rows of 1 and 2 pieces"""
    uses = []
    for i in range(n_desc):
        if i % 9 == 4:
            uses.append((6, False))
        elif i % 25 == 0:
            uses.append((SYNC_WALK_LONG[(i // 25) % len(SYNC_WALK_LONG)], True))
        else:
            uses.append((SYNC_WALK_SHORT[i % len(SYNC_WALK_SHORT)], True))
    return pp.SyncCase(sync_walk_protos(), uses)


# C. the join's chunks of 64 partials

SYNC_CHUNK_PIECES = (1, 63, 64, 65, 127, 128, 129, 130, 66, 66)


def _w(piece, k=0):
    return piece * SY_P + 10 + 4 * k


def sync_chunk_protos():
    """ten rows, comb but one, of SYNC_CHUNK_PIECES pieces.  2: ten hits in pieces 0 .. 54 and ten in piece 63 -- the cap is met in
    lane 63; 3: ten in pieces 3 .. 57 and ten in piece 64 -- the 16th stored hit lies in chunk 1; 4: hits in chunk 1 only; 5: 20
    hits in piece 5, then hits in chunk 1 that are counted and not stored; 6: five, five, and ten in piece 128 -- the cap is met
    in the third chunk; 7: ten either side of piece 64; 8: L = 31 under noise of 0.3 with one noiseless word in piece 64; 9: one
    hit in piece 10 and one in piece 65 -- equal bests in two chunks"""
    P = SY_P
    pr = [comb_proto(P - 7, [3, 500], True),
          comb_proto(62 * P + 300, [_w(0), _w(30), _w(62)], False, skew=8),
          comb_proto(63 * P + 1000, [_w(p) for p in range(0, 60, 6)] + [_w(63, k) for k in range(10)], True),
          comb_proto(64 * P + 65, [_w(p) for p in range(3, 63, 6)] + [_w(64, k) for k in range(10)], False),
          comb_proto(126 * P + 50, [_w(64), _w(64, 1), _w(90), _w(126)], True, skew=8),
          comb_proto(128 * P, [_w(5, k) for k in range(20)] + [_w(64), _w(100), _w(127, 3)], False),
          comb_proto(128 * P + 100, [_w(p) for p in (1, 9, 17, 25, 33, 64, 70, 80, 90, 127)] + [_w(128, k) for k in range(10)], True),
          comb_proto(129 * P + 50, [_w(p) for p in range(0, 64, 7)] + [_w(p) for p in (64, 65, 70, 77, 90, 100, 111, 127, 128, 129)], False, skew=8),
          windows_proto(31, 65 * P + 40, True, (1000, 20000), 13008, sigma=0.3, thr=0.7, clean=(64 * P + 300,)),
          comb_proto(65 * P + 40, [_w(10), _w(65)], True)]
    return pr


@functools.lru_cache(maxsize=None)
def sync_chunks():
    """the ten rows of sync_chunk_protos and two descriptors without data, one launch of fold and join"""
    pr = sync_chunk_protos()
    uses = [(k, True) for k in range(len(pr))]
    uses[4:4] = [(0, False)]
    uses.append((0, False))
    return pp.SyncCase(pr, uses)


SYNC_HIT_COUNTS = (0, 1, 15, 16, 17, 1024)


def synthetic_partial(piece, n_valid, n_hits, m_best):
    """a partial as a fold could have left it for piece `piece`: positions inside the piece, ascending; arbitrary sums"""
    k = np.arange(min(n_hits, ym.HITS))
    hits = np.zeros(len(k), ym.HIT_DTYPE)
    hits["pos"], hits["cr"], hits["ci"], hits["e"], hits["m"] = piece * SY_P + 3 * k, piece + k / 16.0, -1.0 - k, 2.0 + k, 0.9 + k / 256.0
    best = None
    if n_valid:
        best = np.zeros((), ym.HIT_DTYPE)
        best["pos"], best["cr"], best["ci"], best["e"], best["m"] = piece * SY_P + 517, piece, 0.5, 3.0, m_best
    return dict(n_valid=n_valid, n_hits=n_hits, best=best, hits=hits)


def synthetic_proto(name, counts):
    """a row of len(counts) pieces by its partials alone: piece p has counts[p] hits; as many valid windows, but at least 7 --
    and none in every fifth piece without a hit, whose best is poison; the bests are drawn from eleven values, so that equal
    maxima lie in several pieces and chunks"""
    parts = []
    for p, h in enumerate(counts):
        v = 0 if h == 0 and p % 5 == 2 else max(h, 7)
        parts.append(synthetic_partial(p, v, h, 0.25 + ((p * 37 + 5) % 11) / 16.0))
    nw = len(counts) * SY_P
    return dict(parts=parts, n=nw + 4, n_windows=nw, L=5, name=name, counts=tuple(counts))


def _cycle(n, first=0):
    return [SYNC_HIT_COUNTS[(p + first) % len(SYNC_HIT_COUNTS)] for p in range(n)]


@functools.lru_cache(maxsize=None)
def sync_join_alone():
    """the join alone on partials written by numpy: 1, 64, 65 and 200 pieces of 1024 hits each; then 130 pieces with 0, 1, 15, 16,
    17 and 1024 hits mixed: the cap met in lane 0, in lane 63, by the first partial of the second chunk, and in the second chunk
    alone; one descriptor without data"""
    pr = [synthetic_proto("full %d" % k, [1024] * k) for k in (1, 64, 65, 200)]
    pr.append(synthetic_proto("cycle", _cycle(130)))
    pr.append(synthetic_proto("lane 0", [17] + _cycle(129, 1)))
    pr.append(synthetic_proto("lane 63", [0] * 63 + [1024] + _cycle(66)))
    pr.append(synthetic_proto("chunk edge", [0] * 7 + [15] + [0] * 56 + [1, 17] + _cycle(64)))
    pr.append(synthetic_proto("second chunk", [0] * 64 + [1024] + _cycle(65)))
    uses = [(k, True) for k in range(len(pr))]
    uses[2:2] = [(0, False)]
    return pp.SyncCase(pr, uses, which=2)


# D. the channel loop's second trip

SYNC_LOOP_DESCRIPTORS = pp.LOOK_GRID_MAX + 600
SYNC_LOOP_PAIRS = 40
SYNC_LOOP_KINDS = ("L 128, one piece, then L 3, five pieces", "L 3, five pieces, then L 128, one piece", "data, then none", "none, then data")


def sync_loop_first(k):
    """the first descriptor of pair k; its partner is 65535 further"""
    return 7 + 13 * k


@functools.lru_cache(maxsize=None)
def sync_loop():
    """65535 + 600 descriptors, all without data but 40 pairs (i, i + 65535), which share a workgroup of the fold and one of the
    join: SYNC_LOOP_KINDS in turn.  Protos 0, 1: L = 128, 300 symbols, continued and restarted; 2, 3: L = 3, five pieces"""
    P = SY_P
    pr = [word_proto(128, 300, False, (-64, 100), 14000), word_proto(128, 300, True, (10,), 14001, skew=8),
          windows_proto(3, 4 * P + 50, False, (-1, 2 * P), 14002, skew=8), windows_proto(3, 4 * P + 50, True, (5,), 14003)]
    uses = [(0, False)] * SYNC_LOOP_DESCRIPTORS
    for k in range(SYNC_LOOP_PAIRS):
        i, alt = sync_loop_first(k), (k // 4) % 2
        one, five = (alt, True), (2 + alt, True)
        uses[i], uses[i + pp.LOOK_GRID_MAX] = ((one, five), (five, one), ((one, five)[alt], (0, False)), ((0, False), (five, one)[alt]))[k % 4]
    return pp.SyncCase(pr, uses, spare_every=7)


# E. alignment and the history

SYNC_SHORT_L = (1, 64, 128)


def sync_short_lengths(L):
    return sorted({1, L - 1, 126, 127, 128, 300} - {0})


@functools.lru_cache(maxsize=None)
def sync_short_rows():
    """rows of 1, L - 1, 126, 127, 128 and 300 symbols at L = 1, 64 and 128, continued (a word across the row's start) and
    restarted, rows 8 bytes past a line for every second: the history shifts by fewer than 127 symbols, or is the row's end"""
    pr = []
    for L in SYNC_SHORT_L:
        for n in sync_short_lengths(L):
            for restart in (False, True):
                pr.append(word_proto(L, n, restart, (-(L // 2), n // 3), 15000 + 1000 * L + 2 * n + restart, skew=8 if len(pr) % 4 < 2 else 0))
    return pp.SyncCase(pr, [(k, True) for k in range(len(pr))], spare_every=2)


SYNC_CASES = {"lengths": lambda: sync_lengths(False), "lengths spread": lambda: sync_lengths(True), "walk 700": lambda: sync_walk(700),
              "walk 1100": lambda: sync_walk(1100), "walk 2100": lambda: sync_walk(2100), "chunks": sync_chunks, "join alone": sync_join_alone,
              "loop": sync_loop, "short rows": sync_short_rows}
