"""The census of the front stages that take samplesPerBaud and numAvg at run time -- psk_tile_front_any_kernel<1>, <4> and <16>
(psk_tile.hip), the wide front stage (psk_wide.hip) and both behind the far fit -- with stimuli for what no stream of ordinary
size reaches: exact ties, the exactness certificate on finite samples, partial chunks and carried partial symbols (DESIGN.md
section 4.8).  A plain module: tests/test_front_census.py checks the table and the conditions of every draw without a GPU,
tests/test_gpu_front_census.py runs the rows on one, the rows of a variant as the channels of one handle, so that the launch
picks the body the rows are about.

Every row draws from a generator of its own, seeded by the row's name (section 4.2's rule), and takes the first attempt that
meets the conditions of its kind; the conditions are evaluated with the float64 models below, never with the code under test.

Kinds:
  tie     integer-valued rectangular pulses, the amplitude doubled at the two timing phases of a pair that changes every 8 .. 40
          symbols: the window sums of the pair tie exactly, the first maximum is the lower phase
  drift   rectangular pulses of one energy (in exact arithmetic every phase ties, the pick is 0); one symbol in the first tile
          of the second call holds samples 2e4 .. 2e6 strong, each phase its own magnitude and angle.
          While it is in the window the small energies round at its scale, a phase at a time; once it has left, what the
          reference's running sums kept of that decides every pick to the end of the call.  A tile after the first starts from a
          fresh sum, and so must refuse.
  kept    the same stream with a burst small enough for the certificate to hold with 4 bits to spare: nothing rounds
  before  the drift stream cut so that the burst is in the window of every symbol of call 1 and leaves it with that call's
          last one; calls 2 and 3 are clean
"""
import functools
import hashlib

import numpy as np

KB = 128  # symbols of a block
TILE = dict(any=2 * KB, wide=KB)  # symbols of a tile, the launch sets of these rows being small (place_tiles: k_min blocks)
VARIANTS = ("any1", "any4", "any16", "wide", "far")
S_RANGE = dict(any1=(2, 64), any4=(65, 256), any16=(257, 1024), wide=(1025, 65535))  # the S field of the variant's front launch
KINDS = ("tie", "drift", "kept", "before")
FORMAT_DTYPE = dict(cs16=np.int16, cs8=np.int8, cf16=np.float16)
FORMAT_SCALE = dict(cs16=512, cs8=8, cf16=64)  # times a point of components 1 .. 4, doubled: exact in the format
CLEAN_AMPLITUDE = 0.7310586
FAR_PHASE_AVG = 32641
SEED_TRIES = 64
BIG_TAILS = (1, 7, 63, 127, 65, 15)  # what the call of three tiles emits beyond two of them
SMALL_CALLS = (1, 7, 9, 15, 63, 65, 127)
UNAMBIGUOUS = 2.0 ** -30  # relative top-two gap far above what 2^-52 times a few thousand additions can move

# variant: (samplesPerBaud, kind, numAvg, packet format or None)
TABLE = dict(
    any1=[(33, "tie", 1), (33, "drift", 16), (33, "kept", 17), (33, "before", 15),      # 512 // 33 = 15 symbols a staging batch
          (40, "tie", 2), (40, "drift", 13), (40, "kept", 14), (40, "before", 100),     # 12
          (63, "tie", 9), (63, "drift", 10), (63, "kept", 2), (63, "before", 60),       # 8
          (64, "tie", 10), (64, "drift", 2), (64, "kept", 9), (64, "before", 33),       # 8
          (2, "tie", 1025), (2, "drift", 1026), (2, "kept", 1030), (2, "before", 1100),
          (8, "tie", 1100), (8, "drift", 1100), (8, "kept", 1025), (8, "before", 1500),
          (16, "tie", 1025), (16, "drift", 1027), (16, "kept", 1100), (16, "before", 1040)],  # (<= 1024 is the wave-scan kernel's)
    any4=[(65, "tie", 1), (65, "drift", 10), (65, "kept", 4), (65, "before", 6),
          (65, "tie", 2, "cs16"), (65, "tie", 5, "cs8"), (65, "tie", 8, "cf16"),
          (128, "tie", 2), (128, "drift", 5), (128, "kept", 3), (128, "before", 4),
          (255, "tie", 4), (255, "drift", 8), (255, "kept", 9), (255, "before", 2),
          (256, "tie", 3), (256, "drift", 4), (256, "kept", 6), (256, "before", 5),
          (40, "tie", 7), (40, "drift", 100), (40, "kept", 20), (40, "before", 14)],
    any16=[(257, "tie", 1), (257, "drift", 3), (257, "kept", 2), (257, "before", 4),
           (1000, "tie", 2), (1000, "drift", 2), (1000, "kept", 3), (1000, "before", 3),
           (1023, "tie", 3), (1023, "drift", 4), (1023, "kept", 1), (1023, "before", 2),
           (1024, "tie", 4), (1024, "drift", 3), (1024, "kept", 2), (1024, "before", 2),
           (40, "tie", 50), (40, "drift", 30), (40, "kept", 10), (40, "before", 5),
           (100, "tie", 5), (100, "drift", 17), (100, "kept", 8), (100, "before", 3)],
    wide=[(1025, "tie", 2), (1025, "drift", 3), (1025, "kept", 1), (1025, "before", 2),
          (2048, "tie", 3), (2048, "drift", 2), (2048, "kept", 2), (2048, "before", 3),
          (2049, "tie", 1), (2049, "drift", 2), (2049, "kept", 3), (2049, "before", 2),
          (5000, "tie", 2), (5000, "drift", 2), (5000, "kept", 1), (5000, "before", 2)],
    far=[(8, "drift", 10), (1025, "drift", 2)],
)


def _rng(name, attempt=0):
    d = hashlib.sha256(("%s#%d" % (name, attempt)).encode()).digest()
    return np.random.default_rng(int.from_bytes(d[:16], "little"))


def tile_symbols(S):
    return TILE["wide" if S > 1024 else "any"]


def terms_log2(A):
    """bits of the count of additions the certificate allows for (tile_fold: numAvg + two blocks)"""
    return int(A + 2 * KB).bit_length()


# ---- the float64 models of the window sums ------------------------------------------------------------------------------

def energies(packets, S):
    """(symbols, samplesPerBaud) energies of the whole stream as the kernels and the reference form them: re*re + im*im in
    binary32, each operation rounded"""
    iq = np.concatenate([np.asarray(p).astype(np.float32) for p in packets])
    re, im = iq[0::2], iq[1::2]
    e = re * re + im * im
    assert e.dtype == np.float32
    n = e.size // S
    return e[: n * S].reshape(n, S).astype(np.float64)


def exact_picks(e, A):
    """(first, last) maximum of the exact window sums of every output symbol of the stream.  An energy is split into its
    multiple of 2^12 and the rest: both parts of every window sum are exact in binary64 (asserted), and the sums compare as
    the pairs do once the carry is moved over."""
    assert np.isfinite(e).all() and e.max() < 2.0 ** 43 and e.shape[0] < 1 << 12
    hi = np.floor(e / 4096.0) * 4096.0
    lo = e - hi
    assert np.array_equal(lo * 2.0 ** 24, np.rint(lo * 2.0 ** 24))
    z = np.zeros((1, e.shape[1]))
    ch, cl = np.concatenate([z, np.cumsum(hi, axis=0)]), np.concatenate([z, np.cumsum(lo, axis=0)])
    Wh, Wl = ch[A:] - ch[:-A], cl[A:] - cl[:-A]
    carry = np.floor(Wl / 4096.0) * 4096.0
    Wh, Wl = Wh + carry, Wl - carry
    top = Wh == Wh.max(axis=1, keepdims=True)
    top &= Wl == np.where(top, Wl, -1.0).max(axis=1, keepdims=True)
    S = e.shape[1]
    first = top.argmax(axis=1)
    return first, S - 1 - top[:, ::-1].argmax(axis=1), (Wh, Wl)


def running_picks(e, A, emit, tile=None):
    """The picks of sums kept in binary64 in the reference's order, per call: a call starts from a fresh sum of the numAvg - 1
    symbols in front of it, added in order; a symbol's energies arrive, the first maximum is the pick, the oldest symbol's
    leave.  tile: a fresh sum in front of every `tile` symbols of a call as well -- what a tile of the front stage has."""
    out, pos = [], 0
    for n in emit:
        picks = np.zeros(n, np.int64)
        for t0 in range(0, n, tile or max(n, 1)):
            W = np.zeros(e.shape[1])
            for tau in range(pos + t0, pos + t0 + A - 1):
                W += e[tau]
            for i in range(pos + t0, pos + min(t0 + (tile or n), n)):
                W += e[i + A - 1]
                picks[i - pos] = int(np.argmax(W))
                W -= e[i]
        out.append(picks)
        pos += n
    return out


def per_call(x, emit):
    cuts = np.concatenate([[0], np.cumsum(emit)])
    return [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def emitted(S, A, lens):
    """symbols each call emits from a cold start, and what each leaves of a symbol (psk_ctl.h: plan_call, regular window mode)"""
    ring, out, rem = 0, [], []
    for n in lens:
        total = ring + n
        n_out = max(total // S - (A - 1), 0)
        ring = total - n_out * S
        out.append(n_out)
        rem.append(ring % S)
    return out, rem


# ---- shapes -------------------------------------------------------------------------------------------------------------

def _small(rng, S):
    return int(rng.choice(SMALL_CALLS if S < 1000 else SMALL_CALLS[:5]))


def _emit(rng, kind, S, A):
    """(symbols per call, the burst's symbol in the stream or None).  One call of every row has three tiles."""
    T = tile_symbols(S)
    big = 2 * T + int(rng.choice(BIG_TAILS))
    if kind == "tie":
        emit = [_small(rng, S) for _ in range(3)]
        emit[int(rng.integers(0, 3))] = big
        return emit, None
    if kind == "before":
        # symbol g of the stream is in the window of outputs 0 .. g (g < numAvg) and leaves with output g, the first call's last
        g = 0 if A == 1 else int(rng.integers(max(0, A - 1 - 40), A))
        rest = [big, _small(rng, S)]
        return [g + 1] + (rest if rng.integers(0, 2) else rest[::-1]), g
    # drift, kept: the burst enters the window with output u of the second call, in that call's first tile, and has left it
    # before the call's second half begins
    u = int(rng.integers(1, T // 2))
    e0 = _small(rng, S)
    need = 2 * (A + u)
    e1 = max(2 * T, -(-need // KB) * KB) + int(rng.choice(BIG_TAILS))
    return [e0, e1, _small(rng, S)], e0 + A - 1 + u


def _lens(rng, S, A, emit):
    """packet lengths (complex samples) that emit these: every packet leaves a part of a symbol behind, another than the one
    before where samplesPerBaud allows it, so that the carried samples of calls 2 and 3 end inside a symbol"""
    rem, lens = 0, []
    for k, n in enumerate(emit):
        pool = [r for r in range(1, S) if r != rem] or [1]
        new = int(rng.choice(pool))
        lens.append((n + (A - 1 if k == 0 else 0)) * S + new - rem)
        rem = new
    return lens


def _interleave(x, dtype=np.float32):
    out = np.empty(2 * x.size, dtype)
    out[0::2] = x.real
    out[1::2] = x.imag
    return out


def _cut(iq, lens):
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [iq[2 * a : 2 * b] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- stimuli ------------------------------------------------------------------------------------------------------------

def tie_pairs(rng, S):
    """the pairs of timing phases a tie row raises, one after the other: both sides of every DPP row boundary and of the
    half-wave, the same lane one phase apart (k, k + 64), the first and the last phase, both sides of the first chunk boundary
    of a wide symbol (the last chunk's only phase at 1025 and 2049 is S - 1)"""
    pairs = [(0, S - 1)] if S > 2 else [(0, 1)]
    pairs += [(k, k + 1) for k in (15, 31, 47) if S > k + 1]
    if S > 64:
        ks = {0, S - 65} | {int(k) for k in rng.integers(0, S - 64, 3)}
        pairs += [(k, k + 64) for k in sorted(ks)]
    if S > 1024:
        pairs.append((1023, 1024))
    if 2 < S <= 16:
        pairs += [(k, k + 1) for k in range(1, S - 1, 3)]
    return pairs


def _points(c, s, M):
    """the stimulus' constellation: a point (c, s) and its quarter turns (half turns for constelationSize 2) -- components
    swapped and negated, so that every point has the same energy to the bit"""
    return np.array([complex(c, s), complex(-s, c), complex(-c, -s), complex(s, -c)][:: 2 if M == 2 else 1])


def _tie_stream(rng, S, M, n_sym, fmt):
    pairs = tie_pairs(rng, S)
    scale = FORMAT_SCALE.get(fmt, 1)
    p, q = (int(v) for v in rng.choice(4, 2, replace=False) + 1)
    pts = _points(scale * p, scale * q, M)
    x = np.repeat(pts[rng.integers(0, pts.size, n_sym)], S)
    order, pos, seg = rng.permutation(len(pairs)), 0, 0
    raised = np.empty((n_sym, 2), np.int64)
    while pos < n_sym:
        L = int(rng.integers(8, 41))
        raised[pos : pos + L] = pairs[order[seg % len(pairs)]]
        pos, seg = pos + L, seg + 1
    at = (np.arange(n_sym)[:, None] * S + raised).ravel()
    x[at] *= 2
    return x, dict(pairs=pairs)


def burst_range(kind, M, A):
    """magnitudes of the burst's samples, two decades (one octave for the kept kind), drawn log-uniformly per phase"""
    if kind == "kept":
        # 24 + (exponent of the largest energy - exponent of the clean one, -1) + terms_log2 <= 48: four below the rule's 52
        top = np.sqrt(2.0 ** (24 - terms_log2(A))) * 0.99
        return top / 2, top
    assert M in (2, 4)  # (2e6^4 = 1.6e25: the M-th power of the picked sample stays finite)
    return 2e4, 2e6


def _burst_stream(rng, kind, S, M, A, n_sym, g):
    turn = rng.uniform(0.2, 0.8) * 2 * np.pi / M
    c, s = np.float32(CLEAN_AMPLITUDE * np.cos(turn)), np.float32(CLEAN_AMPLITUDE * np.sin(turn))
    pts = _points(float(c), float(s), M)
    x = np.repeat(pts[rng.integers(0, pts.size, n_sym)], S)
    lo, hi = burst_range(kind, M, A)
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), S))
    x[g * S : (g + 1) * S] = mag * np.exp(2j * np.pi * rng.random(S))
    return x, dict(symbol=g, magnitudes=(float(mag.min()), float(mag.max())))


def spread_exponent(e):
    """exponent of the largest energy minus exponent of the smallest (tile_fold's, on binary32 energies that are normal)"""
    return int(np.frexp(e.max())[1] - np.frexp(e.min())[1])


def condition(kind, S, A, M, emit, g, e):
    """does the stream meet what its kind is for?  (None, or the reason it does not)"""
    T = tile_symbols(S)
    first, last, (Wh, Wl) = exact_picks(e, A)
    assert first.size == sum(emit)
    if kind == "tie":
        for k, (f, l) in enumerate(zip(per_call(first, emit), per_call(last, emit))):
            if (f != l).mean() < 0.25:
                return "call %d: first and last maximum differ in %.2f of the symbols" % (k, (f != l).mean())
        return None
    run = running_picks(e, A, emit)
    exact = per_call(first, emit)
    certificate = 24 + spread_exponent(e) + terms_log2(A)
    if kind == "kept":
        if certificate > 48:
            return "certificate %d" % certificate
        return None if all(np.array_equal(r, x) for r, x in zip(run, exact)) else "the running sums round"
    if certificate < 56:
        return "certificate %d: the refusal is not sure" % certificate
    # while the burst is in the window it decides: the top two sums of those symbols are far apart
    pos = np.concatenate([[0], np.cumsum(emit)])
    inside = np.arange(max(g - A + 1, 0), g + 1)
    W = Wh[inside] + Wl[inside]
    two = np.partition(W, S - 2, axis=1)[:, S - 2 :]
    if ((two[:, 1] - two[:, 0]) < UNAMBIGUOUS * two[:, 1]).any():
        return "the burst's own pick is close"
    if kind == "before":
        if not (inside[0] == 0 and inside[-1] == emit[0] - 1):
            return "the burst is not in every window of the first call"
        return None if all(np.array_equal(r, x) and not x.any() for r, x in zip(run[1:], exact[1:])) else "a later call is not clean"
    # drift
    k = int(np.searchsorted(pos, g - A + 1, side="right") - 1)
    if k != 1 or not (0 < g - A + 1 - pos[1] < T) or g + 1 - pos[1] > emit[1] // 2:
        return "the burst is misplaced"
    if exact[0].any() or exact[2].any() or not all(np.array_equal(run[j], exact[j]) for j in (0, 2)):
        return "a clean call is not clean"
    half = np.arange(emit[1] // 2, emit[1])
    differs = run[1][half] != exact[1][half]
    tiles = {int(t) for t in half[differs] // T if t >= 1}
    if differs.mean() < 0.25 or len(tiles) < 2:
        return "drifted picks in %.2f of the second half, tiles %s" % (differs.mean(), sorted(tiles))
    return None


class Row:
    """variant, S, kind, fmt, name; props; far (PSK_SOFT_OPT_FAR_FIT); packets (one array per call, its dtype the format);
    emit (symbols per call); burst_call (drift: the call that must be handed over, else None); draw (what was settled on)"""

    def __init__(self, variant, S, kind, A, fmt=None):
        self.variant, self.S, self.kind, self.A, self.fmt = variant, S, kind, A, fmt
        self.name = "%s/S%d/A%d/%s" % (variant, S, A, kind) + ("/" + fmt if fmt else "")
        self.far = variant == "far"
        self.front = "wide" if S > 1024 else "any"
        ki = KINDS.index(kind)
        # constelationSize cycles 2 / 4 / 8 by samplesPerBaud, numAvg and kind, not by position, so that a new row moves no
        # other.  The two kinds whose strong burst is picked cycle 2 / 4: a window of 512 or 1024 equal energies has no bit
        # below 2^-15 of them, only an energy of 2^38 rounds it, and the 8th power of such a sample is not finite -- which
        # refuses the call through another flag than the one these rows are about.
        M = (2, 4)[(S + A + ki) % 2] if kind in ("drift", "before") else (2, 4, 8)[(S + A + ki) % 3]
        for attempt in range(SEED_TRIES):
            rng = _rng(self.name, attempt)
            self.props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, differentialDecoding=int((S + A + 2 * ki) % 5 == 0),
                              phaseAvg=FAR_PHASE_AVG if self.far else int(rng.choice((1, 2, 50, 385))))
            emit, g = _emit(rng, kind, S, A)
            lens = _lens(rng, S, A, emit)
            n = sum(lens)
            n_sym = n // S + 1
            if kind == "tie":
                x, draw = _tie_stream(rng, S, M, n_sym, fmt)
            else:
                x, draw = _burst_stream(rng, kind, S, M, A, n_sym, g)
            iq = _interleave(x[:n], np.float64 if fmt else np.float32)
            if fmt:
                assert np.array_equal(iq, iq.astype(FORMAT_DTYPE[fmt]).astype(np.float64))
                iq = iq.astype(FORMAT_DTYPE[fmt])
            packets = _cut(iq, lens)
            got, rem = emitted(S, A, lens)
            assert got == emit and all(rem[:2]), (self.name, got, emit, rem)
            why = condition(kind, S, A, M, emit, g, energies(packets, S))
            if why is None:
                self.packets, self.emit, self.lens, self.rem = packets, emit, lens, rem
                self.burst_symbol = g
                self.burst_call = 1 if kind == "drift" else None
                self.draw = dict(draw, attempt=attempt)
                return
        raise AssertionError("%s: no draw in %d meets the conditions of its kind (the last: %s)" % (self.name, SEED_TRIES, why))

    def digest(self):
        h = hashlib.sha256()
        h.update(repr((sorted(self.props.items()), self.far)).encode())
        for p in self.packets:
            h.update(("%s:%d;" % (p.dtype.str, p.size)).encode())
            h.update(np.ascontiguousarray(p).tobytes())
        return h.hexdigest()

    def tiles(self):
        """tiles per call"""
        T = tile_symbols(self.S)
        return [-(-n // T) for n in self.emit]


@functools.lru_cache(maxsize=None)
def rows(variant):
    assert variant in VARIANTS, variant
    return tuple(Row(variant, *spec) for spec in TABLE[variant])


def all_rows():
    return [r for v in VARIANTS for r in rows(v)]


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
