"""Randomised GPU-vs-oracle comparison (diagnostic; the fixed-seed cases that came out of it live in
tests/test_gpu_parity.py, the named configurations below run in tests/test_gpu_randomised.py).  Every round draws a batch of
channels with random properties, signal shapes and packetisations, random property changes / resets between calls, runs it
through the C ABI and through the oracle, and reports every channel whose four output streams do not match
(bits / sampleIndex exactly; soft / phase exactly too -- PSK_FUZZ_STRICT=0 relaxes that to 1e-5 relative).

usage (GPU box): python tools/fuzz_gpu.py [--config NAME] [rounds] [channels] [seed] [only]

The draw of a round (draw_round), the calls it makes of it (ticks), the expected values (reference) and the run on the GPU
(run_round) are separate functions; the configuration is a value (Config) that main() alone makes from the command line and the
PSK_FUZZ_* variables.  The draws of a seed stay what they were: every draw added later comes from a generator of its own
(tests/test_fuzz_draws.py pins the default draws of the cited seeds)."""
import dataclasses
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from psk_soft_amd import lib as pl  # noqa: E402

DEFAULT_S = tuple([2, 4, 5, 8, 8, 8, 10, 10, 16, 3, 7, 1, 6, 9, 11, 12, 13, 14, 15, 33] + list(range(17, 33)))
DEFAULT_A = (1, 2, 3, 17, 25, 64, 100, 100, 127, 128, 129, 200, 256, 257, 400, 512, 520, 513, 1024)
DEFAULT_N = (1, 2, 3, 10, 50, 50, 128, 200, 384, 385, 400, 900, 1920, 1921)  # phaseAvg
FAR_N = [32641, 32768, 40000, 65535]
WIDTHS = (2, 3, 7, 8, 9, 20, 33, 64, 65)  # of a frame-major matrix, in complex samples
TOL = 1e-5
KEYS = ("soft", "bits", "phase", "index")
F32, F16 = np.dtype(np.float32), np.dtype(np.float16)
I16, I8 = np.dtype(np.int16), np.dtype(np.int8)
FORMAT_NAMES = {F32: "cf32", I16: "cs16", I8: "cs8", F16: "cf16"}


@dataclasses.dataclass(frozen=True)
class Config:
    """What a round draws and how it is run.  The first block is the PSK_FUZZ_* variables (the defaults are the tool's default
    draw); the second block has no variable: a named configuration (--config) sets it."""
    nonfinite: float = 0.0  # PSK_FUZZ_NONFINITE=p: with probability p a stream gets a few NaN / +-inf components
    extreme: float = 0.0    # PSK_FUZZ_EXTREME=p: energies that overflow or vanish in float
    # PSK_FUZZ_M: constellation sizes to draw from (others -- 1, 3, 16 -- produce no bits, cpp/psk_soft.cpp:384-390)
    m_choices: tuple = (2, 4, 4, 8)
    # PSK_FUZZ_XD: SRI.xdelta values, one per channel (default 0.01 for all: LinearFit::xdelta = (float)(1 / sampleRate))
    xd_choices: tuple = (0.01,)
    # PSK_FUZZ_MORE=1: two more kinds of events in the scripts -- samplesPerBaud changed between two calls, and a new SRI (another
    # xdelta, sriChanged set) in the middle of a stream
    more: bool = False
    # PSK_FUZZ_CS16=p: with probability p a channel's stream is complex int16 (PSK_SOFT_FORMAT_CS16; the oracle gets its float cast):
    # half of those send every packet as int16 ("all"), the other half alternate int16 / float32 packets call by call ("alt").  Its
    # signal is the same draw, scaled so that its peak lands between 1 and 32767 LSB (ties of small integers included) and rounded;
    # the non-finite and extreme draws stay with the float and half channels.
    cs16: float = 0.0
    # PSK_FUZZ_CS8=p: with probability p a channel that is not CS16 is complex int8 (PSK_SOFT_FORMAT_CS8): half of those send every
    # packet as int8 ("cs8"), the other half rotate CS8 / CS16 / CF32 packets of the same values call by call ("rot").  The signal
    # is scaled so that its peak lands between 1 and 127 LSB and rounded.
    cs8: float = 0.0
    # PSK_FUZZ_CF16=p: with probability p a channel that is neither is complex float16 (PSK_SOFT_FORMAT_CF16).  Half of those send
    # every packet as half ("cf16"): the signal is scaled so that its peak lands log-uniformly between the smallest subnormal half
    # and 65504 and cast to float16, NaNs and infinities of the non-finite draw included.  The other half rotate CF16 / CS8 / CS16 /
    # CF32 packets of the same values call by call ("rot4"): values every format holds, so scaled and rounded as for CS8.
    cf16: float = 0.0
    # PSK_FUZZ_QUALITY=1: PSK_SOFT_OPT_QUALITY is on, and after every call the record of every channel that had a packet is
    # compared with the model (tests/quality_model.py) applied to the rows the call returned: counts, copied values, snapshot and
    # flags equal, the sums within the bound of n doubles added in any order.  The streams themselves are compared as always.
    quality: bool = False
    # PSK_FUZZ_FAR_FIT=p: PSK_SOFT_OPT_FAR_FIT is on, and with probability p a channel's phaseAvg is drawn above 32640 (the fit
    # window in device memory, psk_farfit.hip; symbols enough that the window fills now and then)
    far_fit: float = 0.0
    strict: bool = True  # PSK_FUZZ_STRICT: every float of soft / phase must equal the oracle's
    # PSK_FUZZ_S / PSK_FUZZ_A / PSK_FUZZ_N: lists that replace the default draws (to aim a run at some instantiations);
    # PSK_FUZZ_WINDOW / PSK_FUZZ_PACKET: the handle's max_window_samples (samplesPerBaud * numAvg; the scripts set numAvg up to 300)
    # and max_packet_complex (a stream is up to 12000 symbols long, 150 for samplesPerBaud > 1024), for samplesPerBaud beyond 64
    s_choices: tuple = DEFAULT_S
    a_choices: tuple = DEFAULT_A
    n_choices: tuple = DEFAULT_N
    window: int = 33 * 1024 + 64
    packet: int = 1 << 20
    dump: object = None  # PSK_FUZZ_DUMP=c, with a single-round replay: keep channel c's case
    # ---- no variable ----
    # the entry a round goes through, one batched call per tick: "host" (psk_soft_process_host), "strided"
    # (psk_soft_process_device_strided) or "tuned" (psk_soft_process_device_tuned, a tune drawn per channel)
    entry: str = "host"
    layout: bool = False    # device entries: a layout per channel -- contiguous, one of a run of adjacent columns, a lone column
    deferred: bool = False  # PSK_SOFT_OPT_DEFERRED_JOIN: calls without an event between them go back to back, results read after join()
    looks: float = 0.0      # with this probability psk_soft_acquire_device runs over some channels in front of a tick
    real: float = 0.0       # with this probability a packet is real data (sri_mode 0), half of those with inputQueueFlushed too
    piece: int = 4096       # samples of a piece of the acquire fold (psk_soft_acquire_piece): the looks' lengths lie around it
    crowded: int = 0        # 2 / 3: the crowded round -- that many window classes of 70 channels, a first call the library cuts


def config_from_env(env, base=Config()):
    """`base` with every PSK_FUZZ_* variable that `env` holds applied"""
    ints = lambda v: tuple(int(x) for x in v.split(","))  # noqa: E731
    on = lambda v: v != "0"  # noqa: E731
    table = [("PSK_FUZZ_NONFINITE", "nonfinite", float), ("PSK_FUZZ_EXTREME", "extreme", float), ("PSK_FUZZ_M", "m_choices", ints),
             ("PSK_FUZZ_XD", "xd_choices", lambda v: tuple(float(x) for x in v.split(","))), ("PSK_FUZZ_MORE", "more", on),
             ("PSK_FUZZ_CS16", "cs16", float), ("PSK_FUZZ_CS8", "cs8", float), ("PSK_FUZZ_CF16", "cf16", float),
             ("PSK_FUZZ_QUALITY", "quality", on), ("PSK_FUZZ_FAR_FIT", "far_fit", float), ("PSK_FUZZ_STRICT", "strict", on),
             ("PSK_FUZZ_S", "s_choices", ints), ("PSK_FUZZ_A", "a_choices", ints), ("PSK_FUZZ_N", "n_choices", ints),
             ("PSK_FUZZ_WINDOW", "window", int), ("PSK_FUZZ_PACKET", "packet", int), ("PSK_FUZZ_DUMP", "dump", int)]
    return dataclasses.replace(base, **{field: conv(env[var]) for var, field, conv in table if env.get(var)})


# The named configurations (tests/test_gpu_randomised.py runs them; tests/test_fuzz_draws.py rehearses their draws without a GPU):
# name -> (Config, channels, [(seed, round)]).  `python tools/fuzz_gpu.py --config NAME rounds C seed only` replays one round.
_WIDE = dict(extreme=0.05, nonfinite=0.05, more=True, s_choices=DEFAULT_S + tuple(range(33, 101)), window=100 * 1024 + 64,
             packet=100 * 12000 + 64, real=0.05)
_FORMATS = dict(cs16=0.25, cs8=0.25, cf16=0.25)
CONFIGS = {
    "wide": (Config(**_WIDE), 64, [(11, 0)]),
    "formats": (Config(nonfinite=0.3, **_FORMATS), 128, [(12, 0)]),
    "quality_far_fit": (Config(quality=True, far_fit=0.3, nonfinite=0.05), 48, [(13, 0)]),
    "strided": (Config(entry="strided", layout=True, real=0.05, **_FORMATS), 128, [(14, 0)]),
    "tuned": (Config(entry="tuned", layout=True, **_FORMATS), 96, [(15, 0)]),
    "looks": (Config(entry="tuned", layout=True, looks=0.7, cf16=0.25, cs16=0.25), 64, [(16, 0)]),
    "crowded": (Config(entry="strided", crowded=2), 140, [(19, 0)]),
    "crowded_deferred": (Config(entry="strided", crowded=2, deferred=True), 140, [(20, 0)]),
    "everything": (Config(entry="tuned", layout=True, looks=0.5, deferred=True, quality=True, far_fit=0.1,
                          **dict(_WIDE, **_FORMATS)), 96, [(31, 0)]),
}


@dataclasses.dataclass
class Round:
    """What draw_round() drew.  Per channel: props (the properties at the start), sigs (the whole stream, interleaved I/Q in the
    dtype of its format), scripts (the events: ("set", key, value) and ("packet", from, to, inputQueueFlushed, new xdelta or
    None)), formats (None: float32, or the send mode: "all" / "alt" / "cs8" / "rot" / "cf16" / "rot4"), layout (None: contiguous,
    or (matrix, column); widths[matrix] complex samples wide), tunes (None, or (phase, step) per packet of the script), modes
    (sri_mode per packet).  options: the handle's options; looks: {tick: the acquire call in front of that tick}."""
    seed: int
    rnd: int
    C: int
    cfg: Config
    props: list
    sigs: list
    scripts: list
    formats: list
    layout: list
    widths: dict
    tunes: list
    modes: list
    options: dict
    looks: dict
    limits: dict


def make_signal(rng, nrng, M, S, n, cfg=Config()):
    n_sym = n // S + 2
    k = nrng.integers(0, M, n_sym)
    kind = rng.choice(["shaped", "shaped", "rect", "tri"])
    j = np.arange(S)
    if kind == "shaped":
        pulse = 0.2 + 0.8 * np.sin(np.pi * (j + rng.uniform(0.1, 1.5)) / (S + rng.uniform(0.5, 2.0)))
    elif kind == "rect":
        pulse = np.ones(S)
    else:
        pulse = 1.0 - np.abs(j - rng.uniform(0, S - 1)) / S
    amp = 10.0 ** rng.uniform(-3.5, 2.5)
    if cfg.extreme and rng.random() < cfg.extreme:
        amp = 10.0 ** rng.choice([rng.uniform(17.0, 19.5), rng.uniform(-24.0, -18.0), rng.uniform(9.0, 17.0)])
    cfo = rng.choice([0.0, 1e-3, 1e-2, 0.2]) * rng.uniform(-1, 1) / M
    ph = 2 * np.pi * k / M + rng.uniform(0, 2 * np.pi)
    x = np.repeat(np.exp(1j * ph), S) * np.tile(pulse, n_sym)
    x = x[:n] * np.exp(1j * cfo * np.arange(n) / S) * amp
    sigma = rng.choice([0.0, 0.003, 0.03, 0.3]) * amp
    x = x + sigma * (nrng.standard_normal(n) + 1j * nrng.standard_normal(n))
    if rng.random() < 0.05:  # a silent stretch
        a = rng.randrange(0, n)
        x[a : a + rng.randrange(1, 4000)] = 0
    out = np.empty(2 * n, np.float32)
    out[0::2] = x.real
    out[1::2] = x.imag
    if cfg.nonfinite and rng.random() < cfg.nonfinite:
        for _ in range(rng.randrange(1, 5)):
            out[rng.randrange(0, 2 * n)] = rng.choice([np.float32("nan"), np.float32("inf"), -np.float32("inf")])
    return out


def _draw_layout(lrng, n):
    """a layout for n adjacent channels: (place, widths, leader).  place[c]: None or (matrix, column); a run of 1 .. 12 adjacent
    channels takes adjacent columns of a matrix of its own (both sides of the 8 columns from which the tile gather takes a run),
    a lone channel one column of a matrix of its own; leader[c]: the first channel of c's run (the channels of a matrix share a
    format within a call)."""
    place, widths, leader = [None] * n, {}, list(range(n))
    c = m = 0
    while c < n:
        kind = lrng.choice(["contig", "run", "run", "lone"])
        if kind == "contig":
            c += 1
            continue
        L = 1 if kind == "lone" else min(lrng.randint(1, 12), n - c)
        W = lrng.choice([w for w in WIDTHS if w >= L])
        col = lrng.randint(0, W - L)
        for j in range(L):
            place[c + j], leader[c + j] = (m, col + j), c
        widths[m] = W
        m += 1
        c += L
    return place, widths, leader


MATRIX_BYTES = 16 << 20  # what a matrix of float32 samples may take: a long packet gets a narrower matrix


def _fit_widths(lrng, place, widths, scripts):
    """narrows the matrices whose longest packet would make them larger than MATRIX_BYTES (to a width that still holds the run)"""
    runs = {}
    for c, pl_c in enumerate(place):
        if pl_c is not None:
            runs.setdefault(pl_c[0], []).append(c)
    for m, chans in runs.items():
        longest = max(e[2] - e[1] for c in chans for e in scripts[c] if e[0] == "packet")
        if 8 * longest * widths[m] <= MATRIX_BYTES:
            continue
        fit = [w for w in WIDTHS if w >= len(chans) and 8 * longest * w <= MATRIX_BYTES]
        widths[m] = max(fit) if fit else min(w for w in WIDTHS if w >= len(chans))
        col = lrng.randint(0, widths[m] - len(chans))
        for j, c in enumerate(chans):
            place[c] = (m, col + j)


def _draw_tune(trng, S):
    """a channel's tune: None (never tuned), or (phase word of its first packet, step word)"""
    from tests import tune_model as tm

    kind = trng.choice(["none", "zero", "step", "step", "step", "one", "neg"])
    if kind == "none":
        return None
    if kind == "zero":
        return (0, 0)
    top = 0.2 / S
    f = 10.0 ** trng.uniform(-4.0, np.log10(top)) if top > 1e-4 else trng.uniform(0.0, top)
    step = {"step": tm.step_word(trng.choice([-1, 1]) * f), "one": 1, "neg": (1 << 63) + trng.randrange(1, 1 << 20)}[kind]
    return (trng.getrandbits(64), step)


def _draw_look(krng, knp, C, cap, P):
    """one psk_soft_acquire_device call: (ch0, items, place, widths, tunes) as tests.test_gpu_acquire.look takes them.  The
    packets are drawn for the purpose: 8-PSK at 0.004 cycles per sample in int8 values (every format holds them), lengths around
    one and two pieces of the fold, and a few short ones."""
    from tests import tune_model as tm

    n = krng.randint(1, min(16, C))
    ch0 = krng.randint(0, C - n)
    place, widths, leader = _draw_layout(krng, n)
    items, dts = [], []
    for i in range(n):
        dts.append(dts[leader[i]] if leader[i] != i else krng.choice([F32, I16, I8, F16]))
        if krng.random() < 0.15:
            items.append(None)
            continue
        L = min(krng.choice([krng.randint(1, 300), P + krng.randint(-130, 130), P + krng.randint(-130, 130), 2 * P + krng.randint(-130, 130)]), cap)
        k = np.arange(L)
        z = 40.0 * np.exp(2j * np.pi * (np.repeat(knp.integers(0, 8, L // 4 + 1), 4)[:L] / 8.0 + 0.004 * k)) + 4.0 * (
            knp.standard_normal(L) + 1j * knp.standard_normal(L))
        x = np.empty(2 * L)
        x[0::2], x[1::2] = z.real, z.imag
        items.append(np.clip(np.rint(x), -128, 127).astype(dts[i]))
    tunes = None
    if krng.random() < 0.7:
        tunes = [krng.choice([(0, 0), (krng.getrandbits(64), tm.step_word(krng.uniform(-0.02, 0.02))), (krng.getrandbits(64), 1),
                              (krng.getrandbits(64), (1 << 63) + krng.randrange(1, 1 << 20))]) for _ in range(n)]
    return (ch0, items, place, widths, tunes)


def _options(cfg):
    return dict(far_fit=bool(cfg.far_fit), quality=cfg.quality, deferred=cfg.deferred)


def _draw_crowded(seed, rnd, C, cfg):
    """The crowded round, the shape that reaches the default wave-scan path and the cut in time: cfg.crowded window classes of
    C / cfg.crowded channels each (more than the 64 up to which a class is time-tiled) -- numAvg up to 128, numAvg 129 .. 256,
    numAvg up to 128 again; the packets of a class of up to 128 are float32 or an integer or half format read in place --, samplesPerBaud 2 .. 16 per class, every channel with a
    packet in each of three calls: the first of 128 blocks of 128 symbols and a little more (and fewer than the 192 blocks from
    which a class of this size is time-tiled), then two short ones.  Ten signals a class, every channel at its own delay."""
    g = random.Random(seed * 1000 + rnd + 0xC0DE)
    nrng = np.random.default_rng(seed * 1000 + rnd + 0xC0DE)
    per = C // cfg.crowded
    assert per * cfg.crowded == C and per >= 65
    props, sigs, scripts, formats = [], [], [], []
    for k in range(cfg.crowded):
        S = g.randint(2, 16)
        A = (g.randint(2, 128), g.randint(129, 256), g.randint(2, 128))[k]
        # (in place: numAvg up to 128 only; not CS16, whose calls the schedule neither cuts nor defers where a pre-pass converts them)
        fmt = g.choice([None, "cs8", "cf16"]) if k != 1 else None
        first = S * (128 * 128 + A + 8)
        base = []
        for _ in range(10):
            M = g.choice(cfg.m_choices)
            base.append((M, make_signal(g, nrng, M, S, first + S * 7000 + per, cfg)))
        for j in range(per):
            M, x = base[j % 10]
            a = first + g.randint(0, S * 900)
            b = a + g.randint(S * 200, S * 3000)
            N = b + g.randint(S * 200, S * 3000)
            sig = x[2 * (j // 10) : 2 * (j // 10 + N)]
            if fmt is not None:
                peak = float(np.abs(sig).max())
                top = {"all": 32767.0, "cs8": 127.0, "cf16": 2048.0}[fmt]  # (half: integers up to 2048 are exact)
                scale = 10.0 ** g.uniform(0.5, np.log10(top)) / peak if peak > 0 else 1.0
                sig = np.rint(sig.astype(np.float64) * scale).astype({"all": I16, "cs8": I8, "cf16": F16}[fmt])
            props.append(dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=g.choice([1, 10, 50, 128, 200, 400, 900, 1920]),
                              differentialDecoding=int(g.random() < 0.25)))
            sigs.append(sig)
            scripts.append([("packet", 0, a, False, None), ("packet", a, b, False, None), ("packet", b, N, False, None)])
            formats.append(fmt)
    return Round(seed, rnd, C, cfg, props, sigs, scripts, formats, [None] * C, {}, [None] * C, [[1, 1, 1] for _ in range(C)], _options(cfg), {},
                 dict(max_window_samples=cfg.window, max_phase_avg=2048, max_packet_complex=cfg.packet))


def draw_round(seed, rnd, C, cfg):
    """Everything round `rnd` of `seed` draws for C channels under `cfg`.  Pure: nothing but the arguments goes in.  rng / nrng
    carry the draws the tool has always made; every later kind of draw has a generator of its own, so that turning it on or off
    leaves the others as they were."""
    if cfg.crowded:
        return _draw_crowded(seed, rnd, C, cfg)
    base = seed * 1000 + rnd
    rng = random.Random(base)
    nrng = np.random.default_rng(base)
    crng = random.Random(base + 0x5C16)
    crng8 = random.Random(base + 0x5C08)
    crngf = random.Random(base + 0xFA12)
    crng16 = random.Random(base + 0xCF16)
    lrng = random.Random(base + 0x1A70)   # layouts
    trng = random.Random(base + 0x70E)    # tunes
    erng = random.Random(base + 0x4EA1)   # real-data packets
    krng = random.Random(base + 0x100C)   # looks
    knp = np.random.default_rng(base + 0x100C)
    device = cfg.entry != "host"
    place, widths, leader = _draw_layout(lrng, C) if (device and cfg.layout) else ([None] * C, {}, list(range(C)))
    props, sigs, scripts, formats, tunes, modes = [], [], [], [], [], []
    for c in range(C):
        S = rng.choice(cfg.s_choices)
        A = rng.choice(cfg.a_choices)
        M = rng.choice(cfg.m_choices)
        n = rng.choice(cfg.n_choices)
        far = bool(cfg.far_fit) and crngf.random() < cfg.far_fit
        if far:
            n = crngf.choice(FAR_N)
        p = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n, differentialDecoding=int(rng.random() < 0.25))
        # (wide symbols, samplesPerBaud > 1024: a few dozen to a few hundred symbols -- at 65535 that is already ~10^7 samples)
        N = max(S * rng.choice([50, 300, 1200, 3000, 12000] if S <= 1024 else [20, 60, 150]), 64)
        if far and S <= 32:
            N = min(S * crngf.choice([12000, 50000, 90000]), cfg.packet)
        sig = make_signal(rng, nrng, M, max(S, 1), N, cfg)
        # script: a list of events; cuts with occasional tiny / empty packets, property changes, resets
        n_calls = rng.choice([1, 2, 3, 5])
        cuts = sorted(rng.sample(range(1, N), min(n_calls - 1, N - 1))) if n_calls > 1 else []
        ev, prev, mode = [], 0, []
        for cut in cuts + [N]:
            if rng.random() < 0.15:
                key = rng.choice(["phaseAvg", "numAvg", "constelationSize", "resetState", "differentialDecoding"])
                val = {"phaseAvg": rng.choice([5, 50, 300]), "numAvg": rng.choice([10, 100, 300] if S <= 1024 else [1, 2, 5]),
                       "constelationSize": rng.choice([2, 4, 8]), "resetState": 1,
                       "differentialDecoding": rng.choice([0, 1])}[key]
                ev.append(("set", key, val))
            new_xd = None
            if cfg.more:
                if rng.random() < 0.08:
                    ev.append(("set", "samplesPerBaud", rng.choice([v for v in cfg.s_choices if v * 300 <= 33 * 1024] or cfg.s_choices)))
                if rng.random() < 0.1:
                    new_xd = rng.choice([0.01, 0.02, 1e-3, 0.5, 2.5e-7])
            flushed = rng.random() < 0.05
            real = bool(cfg.real) and erng.random() < cfg.real
            if real and erng.random() < 0.5:
                flushed = True
            mode.append(0 if real else 1)
            ev.append(("packet", prev, cut, flushed, new_xd))
            prev = cut
        if leader[c] != c:
            fmt = formats[leader[c]]  # (a column of a matrix: the format of the run's first channel)
        elif cfg.cs16 and crng.random() < cfg.cs16:
            fmt = crng.choice(["all", "alt"])
        elif cfg.cs8 and crng8.random() < cfg.cs8:
            fmt = crng8.choice(["cs8", "rot"])
        elif cfg.cf16 and crng16.random() < cfg.cf16:
            fmt = crng16.choice(["cf16", "rot4"])
        else:
            fmt = None
        if fmt is not None:
            peak = float(np.abs(sig[np.isfinite(sig)]).max()) if np.isfinite(sig).any() else 0.0
        if fmt in ("all", "alt"):
            scale = 10.0 ** crng.uniform(0.0, np.log10(32767.0)) / peak if peak > 0 else 1.0
            sig = np.clip(np.rint(np.nan_to_num(sig.astype(np.float64) * scale)), -32768, 32767).astype(np.int16)
        elif fmt in ("cs8", "rot"):
            scale = 10.0 ** crng8.uniform(0.0, np.log10(127.0)) / peak if peak > 0 else 1.0
            sig = np.clip(np.rint(np.nan_to_num(sig.astype(np.float64) * scale)), -128, 127).astype(np.int8)
        elif fmt == "rot4":
            scale = 10.0 ** crng16.uniform(0.0, np.log10(127.0)) / peak if peak > 0 else 1.0
            sig = (np.clip(np.rint(np.nan_to_num(sig.astype(np.float64) * scale)), -128, 127) + 0.0).astype(np.float16)  # (no -0: int8 has none)
        elif fmt == "cf16":
            scale = 10.0 ** crng16.uniform(np.log10(2.0 ** -24), np.log10(65504.0)) / peak if peak > 0 else 1.0
            with np.errstate(over="ignore", invalid="ignore"):  # (the finite peak is 65504 at most; NaN and inf stay what they are)
                sig = (sig.astype(np.float64) * scale).astype(np.float16)
        t = None
        if cfg.entry == "tuned":
            t0 = _draw_tune(trng, max(S, 1))
            if t0 is not None:
                from tests import tune_model as tm

                t, ph = [], t0[0]
                for e in ev:
                    if e[0] != "packet":
                        continue
                    if t0 != (0, 0) and trng.random() < 0.1:
                        ph = trng.getrandbits(64)  # (redrawn mid-stream: a retune)
                    t.append((ph, t0[1]))
                    ph = tm.advance(ph, t0[1], e[2] - e[1])
        formats.append(fmt)
        props.append(p)
        sigs.append(sig)
        scripts.append(ev)
        tunes.append(t)
        modes.append(mode)
    _fit_widths(lrng, place, widths, scripts)
    looks = {}
    if cfg.looks:
        n_ticks = max(sum(e[0] == "packet" for e in ev) for ev in scripts)
        for tick in range(1, n_ticks):
            if krng.random() < cfg.looks:
                looks[tick] = _draw_look(krng, knp, C, cfg.packet, cfg.piece)
    limits = dict(max_window_samples=cfg.window, max_phase_avg=max(2048, max(cfg.n_choices), max(FAR_N) if cfg.far_fit else 0),
                  max_packet_complex=cfg.packet)
    return Round(seed, rnd, C, cfg, props, sigs, scripts, formats, place, widths, tunes, modes, _options(cfg), looks, limits)


def _send(fmt, data, turn):
    """the packet as it is sent in turn `turn` of a channel of send mode `fmt` (the values are the same in every format)"""
    if fmt in (None, "all", "cs8", "cf16"):
        return data
    if fmt == "alt":
        return data if turn % 2 == 0 else data.astype(np.float32)
    if fmt == "rot":
        return (data, data.astype(np.int16), data.astype(np.float32))[turn % 3]
    return (data, data.astype(np.int8), data.astype(np.int16), data.astype(np.float32))[turn % 4]  # "rot4"


def ticks(rd):
    """The calls of a round: the scripts walked in lock step, one batched call per tick.  Returns [dict(sets=[(channel, key,
    value)] applied in front of the call, props=[the properties of each channel in this call], look=the acquire call in front of
    it or None, packets=[None or dict(data=the packet as sent, model=the float32 packet the oracle gets -- the exact cast, tuned by
    tests/tune_model.py where the call tunes it --, xdelta, sriChanged, inputQueueFlushed, mode, tune=(phase, step))])]."""
    from tests import tune_model as tm

    C = rd.C
    pos, first, nth = [0] * C, [True] * C, [0] * C
    cur = [dict(p) for p in rd.props]
    xds = [rd.cfg.xd_choices[(rd.rnd * 7 + c) % len(rd.cfg.xd_choices)] for c in range(C)]
    out = []
    while any(pos[c] < len(rd.scripts[c]) for c in range(C)):
        t = len(out)
        sets, pk = [], []
        for c in range(C):
            if pos[c] >= len(rd.scripts[c]):
                pk.append(None)
                continue
            ev = rd.scripts[c][pos[c]]
            while ev[0] == "set":
                sets.append((c, ev[1], ev[2]))
                cur[c][ev[1]] = ev[2]
                pos[c] += 1
                ev = rd.scripts[c][pos[c]]
            a, b, flushed = ev[1], ev[2], ev[3]
            data = rd.sigs[c][2 * a : 2 * b]
            sri = first[c]
            if len(ev) > 4 and ev[4] is not None:  # (a new SRI in front of this packet)
                xds[c] = ev[4]
                sri = True
            # (the channels of a matrix change format together, by the tick; the others by their own events, as they always have)
            send = _send(rd.formats[c], data, t if rd.layout[c] is not None else pos[c])
            mode = rd.modes[c][nth[c]]
            tune = rd.tunes[c][nth[c]] if rd.tunes[c] is not None else (0, 0)
            model = send.astype(np.float32)  # (exact for every format)
            if tune != (0, 0) and mode == 1 and data.size >= 2:  # (a real-data packet is dropped untuned)
                model = tm.apply(tune[0], tune[1], send)
            pk.append(dict(data=send, model=model, xdelta=xds[c], sriChanged=sri, inputQueueFlushed=flushed, mode=mode, tune=tune))
            first[c] = False
            pos[c] += 1
            nth[c] += 1
        out.append(dict(sets=sets, props=[dict(p) for p in cur], look=rd.looks.get(t), packets=pk))
    return out


def draw_facts(rd, tk):
    """What the draw alone says a run will reach: dict(sent={format: packets}, tuned=[packets tuned, per tick], tiles=[runs of at
    least 8 adjacent columns with a packet, per tick], singles=[untuned strided packets outside such runs, per tick], looked=packets of
    the looks on channels of constelationSize 2 / 4 / 8).  A real-data packet is neither gathered nor tuned."""
    sent, tuned, tiles, singles, looked = {}, [], [], [], 0
    for tick in tk:
        pk = tick["packets"]
        for p in pk:
            if p is not None:
                sent[FORMAT_NAMES[p["data"].dtype]] = sent.get(FORMAT_NAMES[p["data"].dtype], 0) + 1
        tuned.append(sum(p is not None and p["tune"] != (0, 0) and p["mode"] == 1 and p["data"].size >= 2 for p in pk))
        strided = [p is not None and rd.layout[c] is not None and rd.widths[rd.layout[c][0]] != 1 and p["mode"] == 1 and p["data"].size >= 2
                   for c, p in enumerate(pk)]
        n_t = n_s = 0
        c = 0
        while c < rd.C:
            if not strided[c]:
                c += 1
                continue
            e = c + 1
            while e < rd.C and strided[e] and rd.layout[e][0] == rd.layout[c][0] and pk[e]["data"].dtype == pk[c]["data"].dtype:
                e += 1
            if e - c >= 8:
                n_t += 1
            else:  # (a tuned packet outside such a run is read where it lies: no gather)
                n_s += sum(pk[i]["tune"] == (0, 0) for i in range(c, e))
            c = e
        tiles.append(n_t)
        singles.append(n_s)
        if tick["look"] is not None:
            ch0, items, _, _, _ = tick["look"]
            looked += sum(x is not None and tick["props"][ch0 + i]["constelationSize"] in (2, 4, 8) for i, x in enumerate(items))
    return dict(sent=sent, tuned=tuned, tiles=tiles, singles=singles, looked=looked)


def reference(rd, tk):
    """The expected values of a round: ([per channel: [the oracle's dict(soft, bits, phase, index) per tick, None without a
    packet]], {tick: [the model record of each packet of the look]})."""
    from tests import acquire_model as am

    ref = []
    for c in range(rd.C):
        o = po.OracleComponent()
        for k, v in rd.props[c].items():
            setattr(o, k, v)
        rows = []
        for tick in tk:
            for cc, key, val in tick["sets"]:
                if cc == c:
                    setattr(o, key, val)
            p = tick["packets"][c]
            if p is None:
                rows.append(None)
                continue
            r = o.service(p["model"], p["xdelta"], mode=p["mode"], sriChanged=p["sriChanged"], inputQueueFlushed=p["inputQueueFlushed"])
            rows.append(dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index))
        ref.append(rows)
    looks = {}
    for t, tick in enumerate(tk):
        if tick["look"] is not None:
            ch0, items, _, _, tunes = tick["look"]
            looks[t] = [am.model_record(x, tick["props"][ch0 + i]["constelationSize"], tunes[i] if tunes else None) for i, x in enumerate(items)]
    return ref, looks


class _Call:
    """a Handle whose process_device_strided makes the k-th call through it the call of tick ticks[k]: the packets' SRI, flags and
    mode as drawn (tests.test_gpu_strided.strided_run lays them out), through the entry of the configuration"""

    def __init__(self, h, entry, tk):
        from tests.test_gpu_tune import Tuned

        tunes = [[(0, 0) if p is None else p["tune"] for p in t["packets"]] for t in tk]
        self._h, self._tk, self._k = h, tk, 0
        self._to = Tuned(h, [t if any(x != (0, 0) for x in t) else None for t in tunes]) if entry == "tuned" else h

    def __getattr__(self, name):
        return getattr(self._h, name)

    def process_device_strided(self, ch0, pk, strides, outs, stream=None):
        for c, p in enumerate(self._tk[self._k]["packets"]):
            if p is not None:
                pk[c].sri_xdelta, pk[c].sri_mode = p["xdelta"], p["mode"]
                pk[c].sriChanged, pk[c].inputQueueFlushed = int(p["sriChanged"]), int(p["inputQueueFlushed"])
        self._k += 1
        self._to.process_device_strided(ch0, pk, strides, outs, stream)


def replay_line(rd, name=None):
    return "python tools/fuzz_gpu.py %s%d %d %d %d" % ("--config %s " % name if name else "", rd.rnd + 1, rd.C, rd.seed, rd.rnd)


def close(a, b, strict=True):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    if a.size != b.size:
        return False, "size %d vs %d" % (a.size, b.size)
    fin = np.isfinite(b)
    if not np.array_equal(np.isfinite(a), fin):
        return False, "non-finite pattern"
    if fin.any():
        err = np.abs(a[fin] - b[fin]).max() / max(np.abs(b[fin]).max(), 1e-30)
        if err > TOL:
            return False, "rel err %g" % err
        if strict and not np.array_equal(a[fin], b[fin]):  # (float32 values widened: equal doubles = equal floats, +-0 aside)
            return False, "bits differ in %d values (rel err %g)" % (int((a[fin] != b[fin]).sum()), err)
    return True, ""


def _dump(cfg, rd):
    """PSK_FUZZ_DUMP=c, with a single-round replay: keeps channel c's case where it always was kept"""
    if cfg.dump is not None:
        for c, (p, ev, sig) in enumerate(zip(rd.props, rd.scripts, rd.sigs)):
            if cfg.dump == c:
                np.save(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "fuzz_case_sig.npy"), sig)
                print("DUMPED channel %d: props=%s script=%s" % (c, p, ev))


def _compare(rd, got, ref, replay):
    """the findings of the four streams: one record per channel that differs"""
    out = []
    for c in range(rd.C):
        g = {k: np.concatenate([r[k] for r in got[c] if r is not None] or [np.zeros(0)]) for k in KEYS}
        r = {k: np.concatenate([x[k] for x in ref[c] if x is not None] or [np.zeros(0)]) for k in KEYS}
        why = stream = None
        if not np.array_equal(g["index"], r["index"]):
            stream, why = "index", "sampleIndex"
        elif not np.array_equal(g["bits"], r["bits"]):
            stream = "bits"
            why = "bits (%d differ)" % int((g["bits"] != r["bits"]).sum()) if g["bits"].size == r["bits"].size else "bits size"
        else:
            for k in ("soft", "phase"):
                ok, msg = close(g[k], r[k], rd.cfg.strict)
                if not ok:
                    stream, why = k, k + " " + msg
                    break
        if not why:
            continue
        detail = []
        if g["phase"].size == r["phase"].size and g["soft"].size == r["soft"].size and g["phase"].size:
            # where, and what the phase estimate is there: one ulp of a large estimate is the known case
            dp = np.nonzero(g["phase"] != r["phase"])[0]
            ds = np.nonzero(g["soft"] != r["soft"])[0]
            fin = r["phase"][np.isfinite(r["phase"])]
            detail.append("   phase: %d of %d values differ%s; soft: %d floats differ; max |phase| %.1f"
                          % (dp.size, g["phase"].size,
                             "" if not dp.size else " (first at %d: %.9g vs %.9g, %d ulp)" % (
                                 dp[0], g["phase"][dp[0]], r["phase"][dp[0]],
                                 abs(int(g["phase"][dp[0]:dp[0] + 1].view(np.int32)[0]) - int(r["phase"][dp[0]:dp[0] + 1].view(np.int32)[0]))),
                             ds.size, float(np.abs(fin).max()) if fin.size else 0.0))
            if ds.size:
                sym = np.unique(ds // 2)
                detail.append("   soft differs at symbols %s ... (%d symbols); got %s ref %s" % (
                    sym[:16].tolist(), sym.size, g["soft"][2 * sym[0] : 2 * sym[0] + 2], r["soft"][2 * sym[0] : 2 * sym[0] + 2]))
        out.append(dict(round=rd.rnd, channel=c, stream=stream, what=why, format=rd.formats[c], layout=rd.layout[c], props=rd.props[c],
                        script=rd.scripts[c], detail=detail, replay=replay))
    return out


def run_round(rd, tk=None, ref=None, capfd=None, name=None):
    """One round on the GPU against its expected values.  Returns (findings, info).  findings: a list of records dict(round,
    channel, stream, what, props, script, replay, ...), one per channel whose streams differ from the oracle's, per quality or
    acquire record that its model refuses, and one if a source buffer changed.  info: dict(stats=[h.stats() behind each group of
    calls], channel_stats, traces=[the launch lines of each tick's call, with `capfd`], look_traces, sent={format: packets},
    tuned=[packets the draw tuned, per tick], quality_seen, looks_seen).  capfd: pytest's, on a handle created with
    PSK_SOFT_TRACE_LAUNCHES=2."""
    from tests import acquire_model as am
    from tests import quality_model as qm
    from tests.test_gpu_cs16_schedules import parse_trace

    tk = ticks(rd) if tk is None else tk
    ref, look_models = reference(rd, tk) if ref is None else ref
    cfg, C = rd.cfg, rd.C
    replay = replay_line(rd, name)
    findings = []
    facts = draw_facts(rd, tk)
    info = dict(stats=[], traces=[], look_traces=[], sent=facts["sent"], tuned=facts["tuned"], quality_seen=0, looks_seen=0)
    h = pl.Handle(C, device=0, **rd.limits)
    try:
        h.configure(0, rd.props)
        if rd.options["far_fit"]:
            h.set_option(pl.Handle.OPT_FAR_FIT, 1)
        if rd.options["quality"]:
            h.set_option(pl.Handle.OPT_QUALITY, 1)
        if rd.options["deferred"]:
            h.set_option(pl.Handle.OPT_DEFERRED_JOIN, 1)
        got = [[] for _ in range(C)]
        # groups of ticks that go back to back: with the deferred join, the ticks without an event, a look or a record to read
        # in front of them; otherwise every tick by itself
        groups = []
        for t, tick in enumerate(tk):
            if t and cfg.deferred and cfg.entry != "host" and not cfg.quality and not tick["sets"] and tick["look"] is None:
                groups[-1].append(t)
            else:
                groups.append([t])
        for grp in groups:
            t0 = grp[0]
            for c, key, val in tk[t0]["sets"]:
                h.configure(c, [{key: val}])
            if tk[t0]["look"] is not None:
                from tests.test_gpu_acquire import look

                ch0, items, place, widths, tunes = tk[t0]["look"]
                try:
                    _, recs, lines = look(h, items, ch0=ch0, place=place, widths=widths, tunes=tunes, capfd=capfd)
                    info["look_traces"].append(lines)
                    for i, model in enumerate(look_models[t0]):
                        info["looks_seen"] += 1
                        am.assert_record(recs[i], model, "look in front of tick %d, channel %d" % (t0, ch0 + i))
                except AssertionError as e:
                    findings.append(dict(round=rd.rnd, channel=ch0, stream="acquire", what=str(e), props=None, script=None, replay=replay))
            if cfg.entry == "host":
                pk = [None if p is None else dict(data=p["data"], xdelta=p["xdelta"], mode=p["mode"], sriChanged=p["sriChanged"],
                                                  inputQueueFlushed=p["inputQueueFlushed"]) for p in tk[t0]["packets"]]
                if capfd:
                    capfd.readouterr()
                res = h.process_host(0, pk)
                if capfd:
                    info["traces"].append(parse_trace(capfd.readouterr().err))
                rows = {c: [None if pk[c] is None else {k: res[c][k] for k in KEYS}] for c in range(C)}
            else:
                from tests.test_gpu_strided import strided_run

                calls = [[None if p is None else p["data"] for p in tk[t]["packets"]] for t in grp]
                try:
                    rows, traces, _ = strided_run(_Call(h, cfg.entry, [tk[t] for t in grp]), calls, rd.layout, rd.widths, capfd,
                                                  sync_each=not cfg.deferred, k0=t0)
                except AssertionError as e:  # (the source buffer is not what was uploaded)
                    findings.append(dict(round=rd.rnd, channel=-1, stream="source", what="tick %d: %s" % (t0, e), props=None, script=None,
                                         replay=replay))
                    break
                info["traces"].extend(traces)
            for c in range(C):
                got[c].extend(rows[c])
            info["stats"].append(h.stats())
            if cfg.quality:
                recs = h.quality_records()
                for c in range(C):
                    g = rows[c][-1]
                    if g is None:
                        continue
                    info["quality_seen"] += 1
                    cur = tk[grp[-1]]["props"][c]
                    try:
                        qm.assert_record(recs[c], qm.model_record(g["soft"], g["phase"], g["index"], cur["constelationSize"], cur["samplesPerBaud"],
                                                                  cur["differentialDecoding"]), "channel %d" % c)
                    except AssertionError as e:
                        findings.append(dict(round=rd.rnd, channel=c, stream="quality", what=str(e), props=cur, script=rd.scripts[c], replay=replay))
        info["channel_stats"] = h.channel_stats()
    finally:
        h.close()
    if not any(f["stream"] == "source" for f in findings):
        findings.extend(_compare(rd, got, ref, replay))
    return findings, info


def main():
    argv = sys.argv[1:]
    name = None
    if argv and argv[0] == "--config":
        name, argv = argv[1], argv[2:]
    cfg = config_from_env(os.environ, CONFIGS[name][0] if name else Config())
    rounds = int(argv[0]) if len(argv) > 0 else 4
    C = int(argv[1]) if len(argv) > 1 else 192
    seed = int(argv[2]) if len(argv) > 2 else 1
    only = int(argv[3]) if len(argv) > 3 else None  # replay one round (each round draws from its own generator)
    bad_total = 0
    for rnd in range(rounds):
        if only is not None and rnd != only:
            continue
        rd = draw_round(seed, rnd, C, cfg)
        _dump(cfg, rd)
        findings, info = run_round(rd, name=name)
        bad = q_bad = 0
        for f in findings:
            if f["stream"] == "quality":
                q_bad += 1
                print("QUALITY MISMATCH round %d %s  props=%s" % (rnd, f["what"], f["props"]))
            elif f["stream"] in ("acquire", "source"):
                bad += 1
                print("%s MISMATCH round %d %s" % (f["stream"].upper(), rnd, f["what"]))
            else:
                bad += 1
                print("MISMATCH round %d channel %d%s: %s  props=%s script=%s" % (rnd, f["channel"], " (int %s)" % f["format"] if f["format"] else "",
                                                                              f["what"], f["props"], f["script"]))
                for line in f["detail"]:
                    print(line)
        bad_total += bad
        if cfg.quality:
            bad_total += q_bad
            print("round %d: %d quality records compared with the model, %d mismatches" % (rnd, info["quality_seen"], q_bad))
        if rd.looks:
            print("round %d: %d acquire records compared with the model" % (rnd, info["looks_seen"]))
        print("round %d: %d channels (%d CS16 / CS8), %d mismatches, last-call stats %s" % (rnd, C, sum(f is not None for f in rd.formats), bad,
                                                                                         info["stats"][-1] if info["stats"] else None))
    print("TOTAL mismatches:", bad_total)
    return 1 if bad_total else 0


if __name__ == "__main__":
    sys.exit(main())
