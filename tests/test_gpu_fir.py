"""psk_soft_process_device_filtered on a real MI355X: packets filtered and decimated on the GPU (psk_fir.hip) in front of the
demodulator.  Every stream, count and SRI field of a call is, as bit patterns, what a second handle gives through
psk_soft_process_device on the contract's packets -- tests/fir_model.py (behind tests/tune_model.py, in front of
tests/resample_model.py) on the packet's samples, CF32, contiguous, with the scaled sample period --; the history behind every
call is the model's.

Both handles write rows of tests/row_guards.py: every output row has exactly n_symbols of capacity (the counts come from a
control-plane-only handle fed the contract's packets) and 1024 guard bytes in front of it and behind it that must come back
untouched, as must every byte of the arena the packets lie in -- frame-major matrices among them."""
import numpy as np
import pytest

from tests import fir_model as fm
from tests import resample_model as rm
from tests import row_guards as rg
from tests import tune_model as tm
from tests.test_strided_control import OUT_FIELDS

pytestmark = pytest.mark.gpu

F32 = np.float32
DT = (np.float32, np.int16, np.int8, np.float16)
XD = 0.01
STEP_837 = int(8.37 / 8 * 2.0 ** 32)
NO_FIR, NO_RS, NO_TUNE = (0, 0, 0, 0), (0, 0, 0), (0, 0)


def _signal(rng, n, dt, M=4, sps=8):
    """n complex samples of a PSK signal at sps samples a symbol in noise, interleaved, in the packet dtype dt (the integer and
    half formats hold small integers, float32 every mantissa bit)"""
    sym = rng.integers(0, M, n // sps + 2)
    s = np.repeat(np.exp(1j * (2 * np.pi * sym / M + 0.3)), sps)[:n]
    x = s + 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = x.real, x.imag
    if np.dtype(dt) == np.float32:
        return (iq * 37.3).astype(F32)
    return np.clip(np.rint(iq * 40), -127, 127).astype(dt)


def _taps(rng, T):
    h = (rng.standard_normal(T) / np.sqrt(T)).astype(F32)
    return h


class Image:
    """the arena the packets of one call lie in: contiguous packets and frame-major matrices between guards"""

    def __init__(self, C, rng):
        self.C, self.rng, self.size, self.parts = C, rng, 0, []
        self.at, self.stride = [None] * C, [1] * C

    def _place(self, arr, align, bare):
        start = rg._start(self.size + rg.GUARD, align, bare)
        self.parts.append((start, np.ascontiguousarray(arr).view(np.uint8).reshape(-1)))
        self.size = start + arr.nbytes + rg.GUARD
        return start

    def packet(self, c, x):
        fmt = rg.FORMAT_OF[x.dtype]
        self.at[c] = (self._place(x, rg.FORMAT_ALIGN[fmt], c % 2 == 0), x.size, fmt)

    def matrix(self, cols, width, first):
        """cols: [(channel, x)] in adjacent columns from `first` of a matrix `width` complex samples wide, junk elsewhere"""
        dt = cols[0][1].dtype
        fmt = rg.FORMAT_OF[dt]
        rows = max(x.size // 2 for _, x in cols)
        m = _signal(self.rng, rows * width, dt).reshape(rows, width, 2)
        for j, (c, x) in enumerate(cols):
            assert x.dtype == dt
            m[: x.size // 2, first + j] = x[: 2 * (x.size // 2)].reshape(-1, 2)
        start = self._place(m, rg.FORMAT_ALIGN[fmt], False)
        for j, (c, x) in enumerate(cols):
            self.at[c] = (start + (first + j) * rg.FORMAT_ALIGN[fmt], 2 * (x.size // 2), fmt)
            self.stride[c] = width

    def image(self):
        img = np.full(max(self.size, 2 * rg.GUARD), rg.GUARD_BYTE, np.uint8)
        for start, b in self.parts:
            img[start: start + b.size] = b
        return img, self.at


class Case:
    """C channels through a sequence of calls: the handle under test, the handle that runs the contract's packets, the
    control-plane-only handle that gives the counts, and the model's state per channel."""

    def __init__(self, props, taps, options=(), seed=1):
        from psk_soft_amd import lib as pl

        self.pl, self.C, self.props, self.taps = pl, len(props), props, dict(taps)
        self.got, self.ref = pl.Handle(self.C, device=0), pl.Handle(self.C, device=0)
        self.plan = pl.Handle(self.C, device=pl.DEVICE_NONE)
        for h in (self.got, self.ref, self.plan):
            h.configure(0, props)
            for opt, v in options:
                h.set_option(opt, v)
        for slot, t in self.taps.items():
            self.got.fir_define(slot, t)
        self.rows_got, self.rows_ref = rg.DeviceRows(self.got), rg.DeviceRows(self.ref)
        self.fhist = [np.zeros(2 * fm.HIST, F32) for _ in range(self.C)]
        self.rhist = [np.zeros(6, F32) for _ in range(self.C)]
        self.calls = 0
        self.held = None  # (the counts of a call that was refused on purpose: the control plane has moved, the next call is that one)
        self.rng = np.random.default_rng(seed)

    def close(self):
        self.rows_got.close()
        self.rows_ref.close()
        for h in (self.got, self.ref, self.plan):
            h.close()

    def set_history(self, c, floats):
        self.got.set_fir_history(c, floats)
        self.fhist[c] = np.asarray(floats, F32).copy()

    def model(self, data, modes, tunes, firs, rss):
        """the contract's packet of every channel ((array or None, sample period)), and the histories behind the call (the
        model's own state moves in call(), once the call went through)"""
        out, fh, rh = [], list(self.fhist), list(self.rhist)
        for c in range(self.C):
            x, xd = data[c], XD
            if x is None or x.size < 2 or modes[c] != 1:
                out.append((x, xd))
                continue
            (ph, st), (slot1, D, pos, ffl), (rpos, rstep, rfl) = tunes[c], firs[c], rss[c]
            touched = bool(ph | st) or bool(slot1) or bool(rstep)
            s = tm.apply(ph, st, x) if (ph | st) else x[: 2 * (x.size // 2)].astype(F32)
            if slot1:
                s, fh[c] = fm.apply(self.taps[slot1 - 1], D, pos, s, fh[c], bool(ffl & 1))
                xd = xd * float(D)
            if rstep and s.size >= 2:
                s, rh[c] = rm.apply(rpos, rstep, s, rh[c], bool(rfl & 1))
                xd = xd * (rstep * 2.0 ** -32)
            out.append((s if touched else x, xd))
        return out, fh, rh

    def counts(self, want, modes, sri_changed):
        pl = self.pl
        pk, out = (pl.Packet * self.C)(), (pl.Output * self.C)()
        for c, (x, xd) in enumerate(want):
            if x is None:
                continue
            pk[c].n_floats, pk[c].format, pk[c].sri_xdelta = x.size, rg.FORMAT_OF[x.dtype], xd
            pk[c].sri_mode, pk[c].sriChanged, pk[c].present = modes[c], int(sri_changed), 1
            out[c].cap_symbols = 1 << 62
        self.plan.process_device(0, pk, out)
        return [{k: int(getattr(o, k)) for k in ("n_symbols", "n_bits", "n_sampleIndex")} for o in out]

    def call(self, data, image, tunes=None, firs=None, rss=None, modes=None, short=None, histories=True):
        """one call of both handles; data[c]: the packet (None: absent), image: the Image the packets of the handle under test
        lie in.  short = (channel, symbols): the call is made with that channel's cap_symbols that much below what it emits,
        must be refused with PSK_SOFT_ERR_CAPACITY, and nothing moves: the same arguments without `short` are the next
        call.  Returns the streams of the handle under test."""
        pl, C = self.pl, self.C
        tunes, firs, rss = tunes or [NO_TUNE] * C, firs or [NO_FIR] * C, rss or [NO_RS] * C
        modes = modes or [1] * C
        want, fh, rh = self.model(data, modes, tunes, firs, rss)
        first = self.calls == 0
        if self.held is None:
            self.held = self.counts(want, modes, first)
        counts = list(self.held)
        assert sum(k["n_symbols"] for k in counts) > 0, "a call that emits nothing shows nothing"
        if short:
            assert counts[short[0]]["n_symbols"] > short[1]
            counts[short[0]] = dict(counts[short[0]], n_symbols=counts[short[0]]["n_symbols"] - short[1])
        else:
            self.held = None
        strides = list(image.stride)

        def fix(pk, xds):
            for c in range(C):
                pk[c].sri_xdelta, pk[c].sri_mode = xds[c], modes[c]

        def run_got(pk, out, bases):
            fix(pk, [XD] * C)
            self.got.process_device_filtered(0, pk, strides, tunes, firs, rss, out)

        def run_ref(pk, out, bases):
            fix(pk, [xd for _, xd in want])
            self.ref.process_device(0, pk, out)

        lay_got = rg.Layout(counts, packet_image=image.image(), call=self.calls)
        if short:
            with pytest.raises(pl.PskSoftError) as ei:
                self.rows_got.run(lay_got, sri_changed=first, call=run_got)
            assert ei.value.status == 6, ei.value
            self.got.synchronize()
            self.check_histories()
            return None
        got, found, out_g = self.rows_got.run(lay_got, sri_changed=first, call=run_got)
        assert not found, rg.messages(found)[:5]
        lay_ref = rg.Layout(counts, packets=[x for x, _ in want], call=self.calls)
        ref, found, out_r = self.rows_ref.run(lay_ref, sri_changed=first, call=run_ref)
        assert not found, rg.messages(found)[:5]
        self.calls += 1
        self.fhist, self.rhist = fh, rh
        for c in range(C):
            a, b = [getattr(out_g[c], f) for f in OUT_FIELDS], [getattr(out_r[c], f) for f in OUT_FIELDS]
            assert _bits(a) == _bits(b), (self.calls, c, a, b)
            for s in rg.STREAMS:
                assert got[c][s].tobytes() == ref[c][s].tobytes(), (self.calls, c, s, _first_difference(got[c][s], ref[c][s]))
        if histories:
            self.check_histories()
        return got

    def check_histories(self):
        for c in range(self.C):
            h = self.got.fir_history(c)
            assert np.array_equal(h.view(np.uint32), self.fhist[c].view(np.uint32)), ("history", self.calls, c)


def _bits(fields):
    return [np.float64(v).view(np.uint64) if isinstance(v, float) else v for v in fields]


def _first_difference(a, b):
    if a.size != b.size:
        return "sizes %d / %d" % (a.size, b.size)
    w = np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))
    return "first of %d bytes at %d" % (w.size, w[0]) if w.size else "none"


def _props(C, S=8, numAvg=(10, 16, 25)):
    return [dict(samplesPerBaud=S, constelationSize=(2, 4, 8)[c % 3], numAvg=numAvg[c % 3], phaseAvg=(5, 20, 50)[(c // 3) % 3],
                 differentialDecoding=int(c % 5 == 3)) for c in range(C)]


def _length_for(n_out, D, pos, extra=0):
    """a packet length with exactly n_out outputs at (D, pos): the last output's newest input, and up to D - 1 more"""
    n = pos + (n_out - 1) * D + 1 + extra % D
    assert fm.count(pos, D, n) == n_out
    return n


TS = (1, 2, 127, 128)
NEG = (1 << 63) + 12345


# ---- 1. every format, every place a packet can lie, tuned or not, the edges of a piece -------------------------------------------------

@pytest.mark.parametrize("D", [1, 2, 3, 4, 7, 9, 15, 16])
@pytest.mark.parametrize("dt", DT, ids=["cf32", "cs16", "cs8", "cf16"])
def test_formats_places_and_piece_edges(dt, D):
    """ten kinds of length -- n_out = P-1, P, P+1, 2P-1, 2P, 2P+1 (P = psk_soft_fir_piece(D)), one sample, T-1 samples, a
    packet with pos >= n, a small odd n_out -- x {a run of ten adjacent columns (the tile gather, then the filter on its
    rows), single strided columns (read where they lie), contiguous packets} x {untuned, tuned}: sixty channels, one call, the
    taps of four slots of 1, 2, 127 and 128 taps, every pos below D."""
    from psk_soft_amd import lib as pl

    P = pl.fir_piece(D)
    assert P == fm.piece(D)
    kinds = 10
    C = 6 * kinds
    rng = np.random.default_rng(97000 + D)
    taps = {s: _taps(rng, T) for s, T in enumerate(TS)}
    props = _props(C)
    case = Case(props, taps)
    try:
        data, firs, tunes = [None] * C, [None] * C, [None] * C
        img = Image(C, rng)
        for c in range(C):
            kind, place, tuned = c % kinds, (c // kinds) % 3, c // (3 * kinds)
            slot = (kind + c // kinds) % 4  # (every kind meets every tap count)
            T = TS[slot]
            pos = (c * 7 + kind) % D
            if kind < 6:
                n = _length_for((P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1)[kind], D, pos, c)
            elif kind == 6:
                n, pos = 1, 0
            elif kind == 7:
                n = max(1, T - 1)
            elif kind == 8:
                pos = D - 1
                n = max(1, pos)  # (pos >= n: no output, unless D = 1, where every sample is one)
            else:
                n = _length_for(37, D, pos, c)
            data[c] = _signal(rng, n, dt, props[c]["constelationSize"])
            firs[c] = (1 + slot, D, pos, pl.FIR_RESTART if c % 4 == 1 else 0)
            case.set_history(c, (rng.standard_normal(2 * fm.HIST) * 25).astype(F32))  # (in front of every packet; the restarted ones must not show it)
            tunes[c] =((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), (tm.step_word(0.003), tm.step_word(-0.01), 1, NEG)[c % 4]) if tuned else NO_TUNE
        assert len({(c % kinds, firs[c][0]) for c in range(C)}) == 4 * kinds
        for tuned in range(2):
            base = tuned * 3 * kinds
            img.matrix([(base + k, data[base + k]) for k in range(kinds)], kinds + 3, 2)
            for k in range(kinds):
                img.matrix([(base + kinds + k, data[base + kinds + k])], 3, 1 + k % 2)
                img.packet(base + 2 * kinds + k, data[base + 2 * kinds + k])
        want, _, _ = case.model(data, [1] * C, tunes, firs, [NO_RS] * C)
        n_outs = [w[0].size // 2 for w in want]
        assert {P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 37} <= set(n_outs) and (D == 1 or 0 in n_outs)
        case.call(data, img, tunes, firs)
    finally:
        case.close()


# ---- 2. the history ---------------------------------------------------------------------------------------------------------------------

def test_history_carried_set_restarted_and_kept_by_a_refused_call():
    """three consecutive calls per channel are the one long packet; psk_soft_fir_get_history is the model's after each call;
    odd channels start from a history set with psk_soft_fir_set_history, even ones restart on top of one that must not show;
    a call refused with PSK_SOFT_ERR_CAPACITY between the second and the third changes neither outputs nor histories."""
    from psk_soft_amd import lib as pl

    C = 12
    rng = np.random.default_rng(97100)
    taps = {0: _taps(rng, 128), 1: _taps(rng, 8), 7: _taps(rng, 33)}
    props = _props(C)
    case = Case(props, taps)
    try:
        Ds = [(1, 2, 3, 16, 5, 8)[c % 6] for c in range(C)]
        slots = [(0, 1, 7)[c % 3] for c in range(C)]
        lens = [[60 + 11 * c for c in range(C)], [pl.fir_piece(Ds[c]) * Ds[c] + 300 + c for c in range(C)], [2000 + 7 * c for c in range(C)]]
        streams = [_signal(rng, sum(l[c] for l in lens), DT[c % 4], props[c]["constelationSize"]) for c in range(C)]
        hist0 = [(rng.standard_normal(2 * fm.HIST) * 30).astype(F32) for c in range(C)]
        for c in range(C):
            case.set_history(c, hist0[c])
        case.check_histories()
        pos, at, parts = [Ds[c] - 1 for c in range(C)], [0] * C, [[] for _ in range(C)]
        for k in range(3):
            data = [streams[c][2 * at[c]: 2 * (at[c] + lens[k][c])] for c in range(C)]
            img = Image(C, rng)
            for c in range(C):
                img.packet(c, data[c])
            firs = [(1 + slots[c], Ds[c], pos[c], pl.FIR_RESTART if k == 0 and c % 2 == 0 else 0) for c in range(C)]
            if k == 2:  # the same call with channel 3's capacity one symbol short: refused, and nothing moves
                assert case.call(data, img, None, firs, short=(3, 1)) is None
            want, _, _ = case.model(data, [1] * C, [NO_TUNE] * C, firs, [NO_RS] * C)
            case.call(data, img, None, firs)
            for c in range(C):
                parts[c].append(want[c][0])
                pos[c] = pl.fir_advance(firs[c], lens[k][c])
                assert pos[c] == fm.advance(firs[c][2], Ds[c], lens[k][c])
                at[c] += lens[k][c]
        for c in range(C):  # the three packets' outputs are those of the one long packet
            whole, _ = fm.apply(taps[slots[c]], Ds[c], Ds[c] - 1, streams[c], hist0[c], restart=c % 2 == 0)
            assert np.array_equal(np.concatenate(parts[c]).view(np.uint32), whole.view(np.uint32)), c
    finally:
        case.close()


# ---- 3. a launch in which workgroups walk several pieces ---------------------------------------------------------------------------------

def test_2100_packets_in_one_call():
    """2100 filtered packets in one call: the launch gives a packet one workgroup, so the twelve packets of two to three pieces
    are walked by a workgroup that takes all their pieces.  int8 and int16, D = 16, two slots of 33 and 128 taps; the long
    packets sit on channels with samplesPerBaud 1 and numAvg 0: every row sample is a symbol.  Every third channel restarts,
    the others start from the handle's zeros; every fourth is tuned."""
    from psk_soft_amd import lib as pl

    C, D = 2100, 16
    P = pl.fir_piece(D)
    rng = np.random.default_rng(97200)
    taps = {2: _taps(rng, 33), 40: _taps(rng, 128)}
    big = {5 + 170 * j: (2 * P + 1, 2 * P + P // 2, 3 * P - 1, 3 * P)[j % 4] for j in range(12)}
    props = [dict(samplesPerBaud=2, constelationSize=(2, 4, 8)[c % 3], numAvg=(2, 3, 5)[c % 3], phaseAvg=(2, 5)[c % 2]) for c in range(C)]
    for c in big:
        props[c] = dict(props[c], samplesPerBaud=1, numAvg=0)
    case = Case(props, taps)
    try:
        pos = [(c * 5) % D for c in range(C)]
        lens = [200 + (37 * c) % 300 for c in range(C)]
        for c, t in big.items():
            lens[c] = _length_for(t, D, pos[c], c)
        data = [_signal(rng, lens[c], (np.int8, np.int16)[c % 2], props[c]["constelationSize"], 32) for c in range(C)]
        img = Image(C, rng)
        for c in range(C):
            img.packet(c, data[c])
        firs = [(1 + (2, 40)[(c // 2) % 2], D, pos[c], pl.FIR_RESTART if c % 3 == 0 else 0) for c in range(C)]
        tunes = [NO_TUNE if c % 4 else (c << 40, tm.step_word(0.001 * (c % 50 + 1))) for c in range(C)]
        want, _, _ = case.model(data, [1] * C, tunes, firs, [NO_RS] * C)
        assert sorted(w[0].size // 2 for w in want)[-12:] == sorted(big.values()) and sorted(w[0].size // 2 for w in want)[-13] < 40
        case.call(data, img, tunes, firs)
    finally:
        case.close()


# ---- 4. everything in one call ------------------------------------------------------------------------------------------------------------

def test_a_mixed_call():
    """48 channels, two calls: filtered only, filtered and resampled (8.37 / 8), resampled only, tuned only, plain, absent,
    real (sri_mode 0) and empty packets, the four formats, single strided columns among them; channels 40 .. 47 are a run of
    int16 columns.  Each channel is its own model; absent, real and empty packets leave the filter's history as it was set."""
    from psk_soft_amd import lib as pl

    C = 48
    rng = np.random.default_rng(97300)
    taps = {0: np.full(8, 0.125, F32), 9: _taps(rng, 64)}
    props = _props(C, numAvg=(100, 64, 25))
    case = Case(props, taps)
    try:
        hist0 = [(rng.standard_normal(2 * fm.HIST) * 20).astype(F32) for c in range(C)]
        for c in range(C):
            case.set_history(c, hist0[c])
        fpos, rpos, ph = [c % 2 for c in range(C)], [(c * 0x9E3779B1) % STEP_837 for c in range(C)], [c << 50 for c in range(C)]
        quiet = [c for c in range(40) if c % 8 >= 5]
        for k in range(2):
            # (5, 6, 7: absent, real, empty, in both calls; the others move through the five live kinds)
            kind = [(c + 3 * k) % 5 if c >= 40 or c % 8 < 5 else c % 8 for c in range(C)]
            n = [2600 + 41 * c + 300 * k for c in range(C)]
            data = [None if kind[c] == 5 else _signal(rng, 1 if kind[c] == 7 else n[c], np.int16 if c >= 40 else DT[(c // 8 + c) % 4],
                                                      props[c]["constelationSize"])[: 1 if kind[c] == 7 else None] for c in range(C)]
            modes = [0 if kind[c] == 6 else 1 for c in range(C)]
            # every packet carries a filter, a resampler and a tune where its kind has none of its own only if quiet: those are not looked at
            firs = [(1 + (0, 9)[c % 2], 2, fpos[c], 0) if kind[c] in (0, 1, 5, 6, 7) else NO_FIR for c in range(C)]
            rss = [(rpos[c], STEP_837, 0) if kind[c] in (1, 2) else NO_RS for c in range(C)]
            tunes = [(ph[c], tm.step_word(0.002 * (c - 17))) if kind[c] == 3 or (kind[c] in (0, 1, 2) and c % 3 == 0) else NO_TUNE for c in range(C)]
            img = Image(C, rng)
            for c in range(40):
                if data[c] is None:
                    continue
                if c % 5 == 2 and kind[c] < 5:
                    img.matrix([(c, data[c])], 4, 1)
                else:
                    img.packet(c, data[c])
            img.matrix([(c, data[c]) for c in range(40, C)], 9, 1)
            case.call(data, img, tunes, firs, rss, modes)
            for c in range(C):
                live = data[c] is not None and data[c].size >= 2 and modes[c] == 1
                if not live:
                    continue
                m = data[c].size // 2
                if tunes[c] != NO_TUNE:
                    ph[c] = pl.tune_advance(tunes[c][0], tunes[c][1], m)
                if firs[c] != NO_FIR:
                    fpos[c] = pl.fir_advance(firs[c], m)
                    m = fm.count(firs[c][2], 2, m)
                if rss[c] != NO_RS:
                    rpos[c] = pl.resample_advance((rss[c][0], rss[c][1]), m)
        for c in quiet:
            assert np.array_equal(case.got.fir_history(c).view(np.uint32), hist0[c].view(np.uint32)), c
    finally:
        case.close()


# ---- 5. the other schedules ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["time_tiled", "deferred_join", "quality"])
def test_schedules_and_quality_records(schedule):
    from psk_soft_amd import lib as pl

    C, n = 12, 9000
    props = [dict(samplesPerBaud=4, constelationSize=(2, 4, 8)[c % 3], numAvg=(25, 100, 200, 400)[(c // 3) % 4] if schedule == "deferred_join" else 64,
                  phaseAvg=(10, 50)[c % 2]) for c in range(C)]
    options = {"time_tiled": [(pl.Handle.OPT_TIME_TILED, 2)], "deferred_join": [(pl.Handle.OPT_DEFERRED_JOIN, 1)],
               "quality": [(pl.Handle.OPT_QUALITY, 1)]}[schedule]
    rng = np.random.default_rng(97400)
    taps = {0: np.full(8, 0.125, F32), 1: _taps(rng, 32)}
    case = Case(props, taps, options)
    try:
        pos = [1] * C
        for k in range(2):
            lens = [n + 33 * c + 500 * k for c in range(C)]
            data = [_signal(rng, lens[c], DT[c % 4], props[c]["constelationSize"]) for c in range(C)]
            img = Image(C, rng)
            for c in range(C):
                img.packet(c, data[c])
            firs = [(1 + c % 2, 2, pos[c], pl.FIR_RESTART if k == 0 else 0) for c in range(C)]
            tunes = [NO_TUNE if c % 2 else (c << 40, tm.step_word(0.0005 * (c + 1))) for c in range(C)]
            rss = [(0, STEP_837, 0) if k == 0 and c % 4 == 3 else NO_RS for c in range(C)]
            case.call(data, img, tunes, firs, rss)
            pos = [pl.fir_advance(firs[c], lens[c]) for c in range(C)]
            if schedule == "quality":
                assert bytes(case.got.quality_records()) == bytes(case.ref.quality_records()), k
        if schedule == "time_tiled":
            assert case.got.stats()["channels_tiled"] > 0 and case.ref.stats()["channels_tiled"] > 0
    finally:
        case.close()


# ---- 6. a slot redefined between two calls --------------------------------------------------------------------------------------------------

def test_a_slot_redefined_between_two_calls():
    """the first call filters with the taps the slot held when it was made, the second with the new ones -- and of another
    length: the history serves both"""
    from psk_soft_amd import lib as pl

    C = 6
    rng = np.random.default_rng(97500)
    old, new = _taps(rng, 16), _taps(rng, 128)
    props = _props(C)
    case = Case(props, {3: old})
    try:
        for k in range(2):
            data = [_signal(rng, 5000 + 100 * c, DT[c % 4], props[c]["constelationSize"]) for c in range(C)]
            img = Image(C, rng)
            for c in range(C):
                img.packet(c, data[c])
            firs = [(4, 1, 0, pl.FIR_RESTART if k == 0 else 0)] * C
            case.call(data, img, None, firs)
            if k == 0:  # (no synchronize in between: psk_soft_fir_define waits for the launch that reads the slot)
                case.got.fir_define(3, new)
                case.taps[3] = new
    finally:
        case.close()
