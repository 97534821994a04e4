"""The census of the wave-scan family's compiled units: one row per (unit, path), each with a stimulus that drives a call of
its own through that unit.  A plain module: tests/test_instantiation_census.py checks the table and
its stimulus conditions without a GPU, tests/test_gpu_instantiations.py runs the rows on one.

The units come from psk_soft_amd/csrc/Makefile -- its variables, read as text and expanded the way its foreach lists expand
them.  A unit the classification below does not know raises; the totals are asserted at import.

Every row draws from a generator of its own, seeded by the row's name, so adding rows never changes another row's stimulus
(section 4.2's rule).  The H8_E0 rows -- the screened tier with eight blocks of history in registers, selected by
PSK_SOFT_REREAD=0 -- are the H0 rows over again: the same channels, in a process started with that variable.

Paths and drivers:
  settle_in_place     E0 float units: a near-tie signal, default options; the screened kernel settles every block itself
  settle_in_place_h8  H8_E0: the H0 rows with PSK_SOFT_REREAD=0
  exact_tier          E1 float units with H 2/4/8: the near-tie signal with PSK_SOFT_TIES_IN_PLACE=0
  exact_tier_h1       E1 float units with H 1: a shaped pulse; one symbol of the third call scaled so that the M-th power of
                      the picked sample overflows and its energy does not (the whole stream at 1e3 / 1e8)
  format_settle       packet-format E0 units: integer-valued rectangular pulses with exact and near ties, sent in the format
  format_exact        packet-format E1 units: call 0 a CF32 packet with one NaN sample (the fit's feedback never recovers),
                      then two calls of integer-valued ties in the format
  tile_front          psk_tile_S*_H1: the near-tie signal with PSK_SOFT_OPT_TIME_TILED = 2
"""
import functools
import hashlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "psk_soft_amd", "csrc", "Makefile")

KB = 128  # symbols of a block: one wave, two a lane
TIE_GAP = 2.0 ** -22  # relative top-two gap every unit's screening refuses: thr >= (4 << IB) 2^-24 wmax, IB >= 1 (psk_fast_loop.h)
PATHS = ("settle_in_place", "settle_in_place_h8", "exact_tier", "exact_tier_h1", "format_settle", "format_exact", "tile_front")
TIE_PATHS = ("settle_in_place", "settle_in_place_h8", "exact_tier", "tile_front")
TOTALS = dict(float=231, format=90, tile=15)
PATH_COUNTS = dict(settle_in_place=108, settle_in_place_h8=15, exact_tier=77, exact_tier_h1=31, format_settle=45, format_exact=45,
                   tile_front=15)
FORMAT_CLASS = dict(cs16=3, cs8=5, cf16=6)  # psk_ctl.h: kPktFormats[].cls, the H of the launch lines
FORMAT_DTYPE = dict(cs16=np.int16, cs8=np.int8, cf16=np.float16)
# amplitude of the integer-valued pulses: exact in every format (binary16 holds integers up to 2048)
FORMAT_AMPLITUDE = dict(cs16=4000, cs8=40, cf16=200)
NOISE_LADDER = (1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7)  # ref_stimulus.gen_psk's level first
FLIP_LADDER = (0.05, 0.02, 0.01, 0.004, 0.002, 0.001, 0.0005)  # share of samples whose real part is one LSB up
SEED_TRIES = 16


# ---- the units ----------------------------------------------------------------------------------------------------------

def makefile_variables(path=MAKEFILE):
    """NAME := words of the Makefile's list variables (text parse; make is not run)"""
    out = {}
    with open(path) as f:
        for line in f:
            m = re.match(r"^(FAST_S|FAST_S_LONG|FAST_S_WIDE|FAST_H|FAST_E|PKT_FORMATS|PKT_S)\s*:=\s*(.*?)\s*$", line)
            if m:
                assert m[1] not in out, "%s is assigned twice" % m[1]
                out[m[1]] = m[2].split()
    missing = {"FAST_S", "FAST_S_LONG", "FAST_S_WIDE", "FAST_H", "FAST_E", "PKT_FORMATS", "PKT_S"} - out.keys()
    assert not missing, "Makefile variables not found: %s" % sorted(missing)
    return out


def makefile_units(path=MAKEFILE):
    """the unit names of FAST_OBJS, PKT_OBJS (the psk_fast_* ones) and TILE_OBJS (the psk_tile_S* ones), in the Makefile's order"""
    v = makefile_variables(path)
    fl = ["psk_fast_S%s_H%s_E%s" % (s, h, e) for s in v["FAST_S"] for h in v["FAST_H"] for e in v["FAST_E"]]
    fl += ["psk_fast_S%s_H%s_E%s" % (s, h, e) for s in v["FAST_S_WIDE"] for h in ("1", "2", "4") for e in v["FAST_E"]]
    fl += ["psk_fast_S%s_H8_E%s" % (s, e) for s in v["FAST_S_LONG"] for e in v["FAST_E"]]
    fl += ["psk_fast_S%s_H0_E0" % s for s in v["FAST_S_LONG"]]
    fm = ["psk_fast_%s_S%s_H1_E%s" % (f, s, e) for f in v["PKT_FORMATS"] for s in v["PKT_S"] for e in ("0", "1")]
    tl = ["psk_tile_S%s_H1" % s for s in v["FAST_S"]]
    for names in (fl, fm, tl):
        assert len(set(names)) == len(names), "a unit is listed twice"
    return dict(float=fl, format=fm, tile=tl)


_UNIT = re.compile(r"^psk_(?P<kind>fast|tile)_(?:(?P<fmt>cs16|cs8|cf16)_)?S(?P<S>\d+)_H(?P<H>\d+)(?:_E(?P<E>[01]))?$")


def path_of(unit):
    """(path, S, H, E, format or None) of a unit; raises for one no path drives"""
    m = _UNIT.match(unit)
    if not m:
        raise ValueError("no census path for unit %r" % unit)
    S, H, E, fmt = int(m["S"]), int(m["H"]), None if m["E"] is None else int(m["E"]), m["fmt"]
    if m["kind"] == "tile":
        ok, path = (H == 1 and E is None and fmt is None and 2 <= S <= 16), "tile_front"
    elif fmt:
        ok, path = (H == 1 and 2 <= S <= 16), ("format_settle", "format_exact")[E]
    elif E == 0:
        ok = (H in (1, 2, 4) and 2 <= S <= 32) or (H in (0, 8) and 2 <= S <= 16)
        path = "settle_in_place_h8" if H == 8 else "settle_in_place"
    else:
        ok = (H in (1, 2, 4) and 2 <= S <= 32) or (H == 8 and 2 <= S <= 16)
        path = "exact_tier_h1" if H == 1 else "exact_tier"
    if not ok:
        raise ValueError("no census path for unit %r" % unit)
    return path, S, H, E, fmt


def _rng(name, attempt=0):
    d = hashlib.sha256(("%s#%d" % (name, attempt)).encode()).digest()
    return np.random.default_rng(int.from_bytes(d[:16], "little"))


# ---- shapes -------------------------------------------------------------------------------------------------------------

def _num_avg(S, H):
    """the edges of the history class, alternating over samplesPerBaud: upper (128, 256, 512, 1024), lower (129, 257, 513)"""
    upper, lower = {1: (128, 128), 2: (256, 129), 4: (512, 257), 8: (1024, 513)}[H]
    return upper if S % 2 == 0 else lower


def _props(rng, S, Hc, Ms=(2, 4, 8)):
    """Hc: history blocks of the window class (1, 2, 4, 8).  constelationSize cycles over the rows of a class, differential
    decoding is on for every fifth -- both by samplesPerBaud and class, not by position, so that a new row moves no other"""
    return dict(samplesPerBaud=S, constelationSize=Ms[(S + Hc.bit_length()) % len(Ms)], numAvg=_num_avg(S, Hc),
                phaseAvg=int(rng.choice((1, 2, 50, 385))), differentialDecoding=int((S + 2 * Hc.bit_length()) % 5 == 0))


def _layout(rng, S, A, Hc):
    """symbols emitted by the three calls and the packet lengths (complex samples) that give them: a cold start of Hc + 2 full
    blocks (the register history wraps) and a tail of 1 .. 3 symbols; a block and 60 .. 100; two blocks and 127.  Every packet
    leaves a different part of a symbol behind, so none is a multiple of samplesPerBaud."""
    emit = [(Hc + 2) * KB + int(rng.integers(1, 4)), KB + int(rng.integers(60, 101)), 2 * KB + 127]
    rem, lens = 0, []
    for k, n in enumerate(emit):
        new = int(rng.choice([r for r in range(S) if r != rem]))
        lens.append((n + (A - 1 if k == 0 else 0)) * S + new - rem)
        rem = new
    assert all(n % S for n in lens)
    return emit, lens


def emitted(props, lens):
    """symbols each call emits from a cold start (psk_ctl.h: plan_call, regular window mode)"""
    S, A, ring, out = props["samplesPerBaud"], props["numAvg"], 0, []
    for n in lens:
        total = ring + n
        n_out = max(total // S - (A - 1), 0)
        ring = total - n_out * S
        out.append(n_out)
    return out


def _interleave(re_, im_, dtype=np.float32):
    out = np.empty(2 * re_.size, dtype)
    out[0::2] = re_
    out[1::2] = im_
    return out


def _cut(iq, lens):
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [iq[2 * a : 2 * b] for a, b in zip(cuts[:-1], cuts[1:])]


def near_tie_blocks(iq, props, emit):
    """A float64 model of the window sums over the whole stream (all calls, float32-valued samples): for every call, one flag
    per block of 128 emitted symbols -- does the block hold a position whose two largest sums are within TIE_GAP of each
    other, relative to the larger?"""
    S, A = props["samplesPerBaud"], props["numAvg"]
    x = np.asarray(iq, np.float64)
    e = x[0::2] ** 2 + x[1::2] ** 2
    n_sym = e.size // S
    cs = np.concatenate([np.zeros((1, S)), np.cumsum(e[: n_sym * S].reshape(n_sym, S), axis=0)])
    W = cs[A:] - cs[:-A]  # W[i]: the window of output symbol i, symbols i .. i + A - 1
    assert W.shape[0] == sum(emit), (W.shape, emit)
    top = np.partition(W, S - 2, axis=1)[:, S - 2 :]
    tie = (top[:, 1] - top[:, 0]) < TIE_GAP * top[:, 1]
    out, pos = [], 0
    for n in emit:
        out.append([bool(tie[pos + b : min(pos + b + KB, pos + n)].any()) for b in range(0, n, KB)])
        pos += n
    return out


# ---- stimuli ------------------------------------------------------------------------------------------------------------

def _points(M):
    return np.exp(2j * np.pi * np.arange(M) / M)


def _near_tie_float(name, S, Hc):
    """rectangular pulses on ideal constellation points, uniform noise on the real part only (ref_stimulus.gen_psk's shape,
    vectorised); the noise level and the draw are the first of the ladder that put a sure near-tie into every block"""
    for noise in NOISE_LADDER:
        for attempt in range(SEED_TRIES):
            rng = _rng(name, attempt)
            props = _props(rng, S, Hc)
            emit, lens = _layout(rng, S, props["numAvg"], Hc)
            n = sum(lens)
            M = props["constelationSize"]
            sym = _points(M)[rng.integers(0, M, n // S + 1)]
            x = np.repeat(sym, S)[:n]
            iq = _interleave(x.real + noise * rng.random(n), x.imag)
            if all(all(b) for b in near_tie_blocks(iq, props, emit)):
                return props, _cut(iq, lens), emit, dict(noise=noise, attempt=attempt)
    raise AssertionError("%s: no draw of the ladder ties in every block" % name)


def _integer_ties(name, S, fmt, first_float):
    """rectangular pulses of FORMAT_AMPLITUDE on integer points, the real part of a share of the samples one LSB up: window
    sums of integers, exactly tied or one small step apart"""
    a = FORMAT_AMPLITUDE[fmt]
    for flip in FLIP_LADDER:
        for attempt in range(SEED_TRIES):
            rng = _rng(name, attempt)
            props = _props(rng, S, 1)
            emit, lens = _layout(rng, S, props["numAvg"], 1)
            n = sum(lens)
            M = props["constelationSize"]
            # (the constellation turned by a part of its step: a carrier sitting at exactly zero phase is the one signal whose
            # feedback unwrap the screened tier's speculation may give up on -- psk_fast_loop.h: kMaxUnwrapPasses --, a refusal
            # of the fit stage that has nothing to do with the timing.  All samples of a symbol stay the same integer point, so
            # the sums of the timing phases tie as before.)
            turn = np.exp(1j * rng.uniform(0.2, 0.8) * 2 * np.pi / M)
            sym = np.rint(a * turn * _points(M))[rng.integers(0, M, n // S + 1)]
            sym = sym.real.round() + 1j * sym.imag.round()
            x = np.repeat(sym, S)[:n]
            iq = _interleave(x.real + (rng.random(n) < flip), x.imag, np.float64)
            assert np.array_equal(iq, iq.astype(FORMAT_DTYPE[fmt]).astype(np.float64))
            if all(all(b) for b in near_tie_blocks(iq, props, emit)):
                pk = [p.astype(FORMAT_DTYPE[fmt]) for p in _cut(iq, lens)]
                if first_float:
                    # call 0 as CF32 with one NaN sample: from here on the fit's feedback is not finite, and every later call of
                    # the channel is refused by the screened tier's fit stage (tests/test_gpu_parity.py: the poisoned channel)
                    pk[0] = pk[0].astype(np.float32)
                    # (at the first timing phase: the reference's first-maximum search starts there, keeps a NaN sum it starts
                    # with, and so picks the sample itself when its symbol is emitted; at another phase the sum only drops out; a
                    # symbol the first call emits, so that no window of the later calls holds it)
                    pk[0][2 * S * int(rng.integers(props["numAvg"], emit[0] - 1))] = np.float32("nan")
                return props, pk, emit, dict(flip=flip, attempt=attempt)
    raise AssertionError("%s: no draw of the ladder ties in every block" % name)


# the picked sample's magnitude after scaling: its M-th power overflows binary32 (2e5^8 = 2.6e42, 1e10^4 = 1e40), its energy
# (4e10, 1e20) does not, nor does a window sum of it
OVERFLOW_MAGNITUDE = {8: 2e5, 4: 1e10}


def _overflowing_power(name, S):
    """a shaped pulse (psk_soft_amd.stimulus.synth_channel: no near-ties, so the amplitude spread cannot trip the exactness
    guard); all samples of one symbol of the third call scaled.  The symbol is emitted within the last three of the call:
    the estimate is not finite from there on, so is every later value."""
    from psk_soft_amd.stimulus import synth_channel

    rng = _rng(name)
    props = _props(rng, S, 1, Ms=(4, 8))  # (constelationSize 2: power and energy overflow together)
    emit, lens = _layout(rng, S, props["numAvg"], 1)
    n, M = sum(lens), props["constelationSize"]
    iq = synth_channel(int(rng.integers(1 << 20, 1 << 30)), M, S, n).copy()
    g = sum(emit) - 1 - int(rng.integers(0, 3))  # output symbol g is input symbol g (it leaves the window as it is emitted)
    assert g * S >= lens[0] + lens[1], "the symbol arrives with the third call"
    seg = iq[2 * g * S : 2 * (g + 1) * S]
    peak = float(np.sqrt((seg.astype(np.float64)[0::2] ** 2 + seg.astype(np.float64)[1::2] ** 2).max()))
    # The exactness guard (psk_fast_kernel.h) hands a call to the reference-order kernel when a pick is closer than the rounding
    # bound of the call's largest window sum AND the energies spread over more than 2^20.  Next to the scaled symbol's energy
    # (4e10, 1e20) the bound is 0.07 or 2e8: every pick of a stream of ordinary size is that close at constelationSize 4, and at
    # 8 a weak channel's are where the pulse is flat at its peak (samplesPerBaud 32).  So the whole stream is large: its picks
    # stay 1e5 (1e16) apart, and the M-th power of an ordinary sample, 2e3^8 = 3e26 (2e8^4 = 2e33), is still finite.
    base = {8: 1e3, 4: 1e8}[M]
    iq *= np.float32(base)
    peak *= base
    seg *= np.float32(OVERFLOW_MAGNITUDE[M] / peak)
    return props, _cut(iq, lens), emit, dict(symbol=g)


# ---- the table ----------------------------------------------------------------------------------------------------------

class Row:
    """unit, path, name; props; packets (one array per call, its dtype the format); emit (symbols per call); env / options the
    handle needs; draw (what the ladder settled on)"""

    def __init__(self, unit, path, S, H, fmt, seed_name):
        self.unit, self.path, self.S, self.H, self.fmt = unit, path, S, H, fmt
        self.name = "%s/%s" % (unit, path)
        self.seed_name = seed_name
        self.env = {"settle_in_place_h8": {"PSK_SOFT_REREAD": "0"}, "exact_tier": {"PSK_SOFT_TIES_IN_PLACE": "0"}}.get(path, {})
        self.time_tiled = 2 if path == "tile_front" else None
        Hc = 8 if H == 0 else H
        if path in TIE_PATHS:
            self.props, self.packets, self.emit, self.draw = _near_tie_float(seed_name, S, Hc)
        elif path == "exact_tier_h1":
            self.props, self.packets, self.emit, self.draw = _overflowing_power(seed_name, S)
        else:
            self.props, self.packets, self.emit, self.draw = _integer_ties(seed_name, S, fmt, path == "format_exact")
        # the class of the launch lines (PSK_SOFT_TRACE_LAUNCHES=2): history blocks, or the format's class
        self.trace_H = FORMAT_CLASS[fmt] if fmt else Hc

    def digest(self):
        h = hashlib.sha256()
        h.update(repr(sorted(self.props.items())).encode())
        h.update(repr((sorted(self.env.items()), self.time_tiled)).encode())
        for p in self.packets:
            h.update(("%s:%d;" % (p.dtype.str, p.size)).encode())
            h.update(np.ascontiguousarray(p).tobytes())
        return h.hexdigest()

    def blocks(self):
        """blocks per call"""
        return [-(-n // KB) for n in self.emit]


@functools.lru_cache(maxsize=None)
def rows(path):
    """the rows of one path, in the Makefile's order"""
    assert path in PATHS, path
    out = []
    units = makefile_units()
    for unit in units["float"] + units["format"] + units["tile"]:
        p, S, H, E, fmt = path_of(unit)
        if p != path:
            continue
        seed = "psk_fast_S%d_H0_E0/settle_in_place" % S if path == "settle_in_place_h8" else "%s/%s" % (unit, path)
        out.append(Row(unit, path, S, H, fmt, seed))
    return tuple(out)


def all_rows():
    return [r for p in PATHS for r in rows(p)]


def oracle_calls(oracle_mod, row):
    """the oracle's four streams of every call of the row (a format's values cast to float32: exact)"""
    o = oracle_mod.OracleComponent()
    for k, v in row.props.items():
        setattr(o, k, v)
    out = []
    for k, p in enumerate(row.packets):
        r = o.service(np.asarray(p).astype(np.float32), 0.01, sriChanged=(k == 0))
        out.append(dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index))
    return out


def _check_totals():
    units = makefile_units()
    got = {k: len(v) for k, v in units.items()}
    assert got == TOTALS, "the Makefile builds %s units, the census knows %s" % (got, TOTALS)
    per_path = dict.fromkeys(PATHS, 0)
    for kind in units.values():
        for u in kind:
            per_path[path_of(u)[0]] += 1
    assert per_path == PATH_COUNTS, per_path


_check_totals()
