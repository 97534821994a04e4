"""psk_soft_sync_device without a GPU: the exports and the layouts, the host-side definition (psk_soft_sync_host) against
tests/sync_model.py byte for byte, cut invariance and RESTART, the entry on control-plane-only handles (PSK_SOFT_DEVICE_NONE) -- it
checks, then leaves planned records and nothing else --, psk_soft_sync_derive, and what the pass is for: a known word found in the
soft symbols of the reference (the oracle), at every frame, with one rotation."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import sync_model as sm

F32 = np.float32
NEW = ("psk_soft_sync_define", "psk_soft_sync_device", "psk_soft_get_sync", "psk_soft_sync_get_history", "psk_soft_sync_set_history",
       "psk_soft_sync_derive", "psk_soft_sync_host", "psk_soft_sync_bytes", "psk_soft_sync_in_bytes", "psk_soft_sync_piece")
WORD_LENGTHS = (1, 2, 31, 64, 127, 128)


def test_the_symbols_are_exported_and_the_records_have_their_layout():
    L = pl.load()
    for name in NEW:
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    R, I, H = pl.SyncRecord, pl.SyncIn, pl.SyncHit
    assert ctypes.sizeof(R) == 456 == sm.RECORD_BYTES == L.psk_soft_sync_bytes()
    assert ctypes.sizeof(I) == 32 == sm.IN_BYTES == L.psk_soft_sync_in_bytes()
    assert ctypes.sizeof(H) == 24 == sm.HIT_BYTES
    names = ("n_symbols", "n_windows", "n_valid", "n_hits", "best", "hits", "word_len", "flags", "pad")
    assert [getattr(R, k).offset for k in names] == [0, 8, 16, 24, 32, 56, 440, 444, 448]
    assert [sm.RECORD_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 56, 440, 444, 448]
    assert [getattr(I, k).offset for k in ("soft", "n_symbols", "word", "flags", "threshold", "pad")] == [0, 8, 16, 20, 24, 28]
    assert [getattr(H, k).offset for k in ("pos", "cr", "ci", "e", "m")] == [0, 8, 12, 16, 20]
    assert ctypes.sizeof(pl.SyncDerived) == 40
    assert (pl.SYNC_RESTART, pl.SYNC_DATA, pl.SYNC_PLANNED) == (1, 1, 128) == (sm.RESTART, sm.DATA, sm.PLANNED)
    assert (pl.SYNC_MAX_WORD, pl.SYNC_SLOTS, pl.SYNC_HITS, pl.SYNC_HISTORY_FLOATS) == (128, 16, 16, 254)
    # the piece is a constant of the library, whole runs of a wave, and the model's
    assert pl.sync_piece() == sm.PIECE and sm.PIECE % sm.THREADS == 0


# ---- the definition ----------------------------------------------------------------------------------------------------------

def _word(L, seed):
    """L unit points of a QPSK word, interleaved"""
    rng = np.random.default_rng(seed)
    z = sm.psk_points(4, rng.integers(0, 4, L))
    w = np.empty(2 * L, F32)
    w[0::2], w[1::2] = z.real, z.imag
    return w


def _row(n, seed, word=None, at=(), gain=0.8 - 0.3j, sigma=0.05):
    """n noisy QPSK symbols, interleaved, with `word` (turned and scaled by `gain`) written at the positions `at`"""
    rng = np.random.default_rng(seed)
    z = sm.psk_points(4, rng.integers(0, 4, n)) * gain
    for p in at:
        wz = (word[0::2] + 1j * word[1::2]) * gain
        lo, hi = max(p, 0), min(p + len(wz), n)
        if hi > lo:
            z[lo:hi] = wz[lo - p: hi - p]
    z = z + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.empty(2 * n, F32)
    x[0::2], x[1::2] = z.real, z.imag
    return x


def _check_host(word, thr, x, flags, hist, ctx):
    rec, hout = pl.sync_host(word, thr, x, flags, hist)
    model, mh = sm.model_record(word, thr, x, flags, hist)
    sm.assert_same(rec, model, ctx)
    assert hout.tobytes() == mh.tobytes(), ctx + ": history"
    return rec, hout


@pytest.mark.parametrize("L", WORD_LENGTHS)
def test_sync_host_against_the_model(L):
    word = _word(L, 100 + L)
    hist = _row(127, 7 * L)
    for n in sorted({max(L - 1, 1), L, L + 1, 126, 127, 128, 129, 300}):
        x = _row(n, 1000 * L + n, word, at=(n // 3,))
        for flags in (0, pl.SYNC_RESTART):
            for h in (None, hist):
                for thr in (0.5, 1.0, 1e-6):
                    ctx = "L %d n %d flags %d hist %s thr %g" % (L, n, flags, h is not None, thr)
                    rec, _ = _check_host(word, thr, x, flags, h, ctx)
                    p0, nw = sm.windows(n, L, bool(flags))
                    assert (rec.n_symbols, rec.n_windows, rec.word_len, rec.flags) == (n, nw, L, pl.SYNC_DATA), ctx
                    assert nw == (max(0, n - L + 1) if flags else n), ctx


def test_sync_host_against_the_model_on_rows_of_up_to_130_pieces():
    """the rows the probe searches for the join's second and third trip (tests/prepass_probe_cases.py): 1 .. 130 pieces of 1024
    windows -- the first rows beyond four pieces the host definition meets -- with hits either side of piece 64"""
    from tests import prepass_probe_cases as pc

    rows = pc.sync_chunk_protos()
    for k, p in enumerate(rows):
        rec, _ = _check_host(p["word"], p["thr"], p["x"], pl.SYNC_RESTART if p["restart"] else 0, p["hist"], "chunk row %d" % k)
        assert -(-rec.n_windows // sm.PIECE) == pc.SYNC_CHUNK_PIECES[k], k
    assert max(pc.SYNC_CHUNK_PIECES) == 130 and sum(1 for n in pc.SYNC_CHUNK_PIECES if n > 64) >= 6


def test_a_word_at_every_position_across_the_history_boundary():
    """the stream's word starts k symbols in front of the row, k = 0 .. L: the hit is at -k (none at k = L: that window was the
    call before's), its metric that of the window wholly inside a row"""
    L = 31
    word = _word(L, 3)
    for k in range(0, L + 1):
        stream = _row(127 + 200, 50 + k, word, at=(127 - k,))
        hist, x = stream[: 2 * 127], stream[2 * 127:]
        rec, _ = _check_host(word, 0.9, x, 0, hist, "k %d" % k)
        whole, _ = pl.sync_host(word, 0.9, stream, pl.SYNC_RESTART)
        assert whole.n_hits == 1 and whole.hits[0].pos == 127 - k
        if k < L:
            assert rec.n_hits == 1 and rec.hits[0].pos == -k and rec.best.pos == -k, k
            assert bytes(rec.hits[0])[8:] == bytes(whole.hits[0])[8:], k  # (the same sums and metric, bit for bit)
        else:
            assert rec.n_hits == 0, k


def test_a_metric_exactly_at_the_threshold_is_a_hit():
    L = 64
    word = _word(L, 5)
    x = _row(400, 11, word, at=(100,), sigma=0.2)
    pos, cr, ci, e, m, valid, _ = sm.model_windows(word, x, pl.SYNC_RESTART)
    k = 100
    assert valid[k] and 0.5 < m[k] < 1.0
    rec, _ = _check_host(word, float(m[k]), x, pl.SYNC_RESTART, None, "at the threshold")
    assert rec.n_hits == 1 and rec.hits[0].pos == k and rec.hits[0].m == m[k]
    rec, _ = _check_host(word, float(np.nextafter(m[k], F32(2))), x, pl.SYNC_RESTART, None, "one ulp above")
    assert rec.n_hits == 0 and rec.best.pos == k


def test_two_equal_best_windows_give_the_first():
    L = 31
    word = _word(L, 6)
    half = _row(150, 12, word, at=(40,), sigma=0.1)
    x = np.concatenate([half, half])  # (every window wholly inside a half occurs twice, bit for bit)
    rec, _ = _check_host(word, 0.7, x, pl.SYNC_RESTART, None, "two equal bests")
    assert rec.n_hits == 2 and [h.pos for h in rec.hits[:2]] == [40, 190]
    assert bytes(rec.hits[0])[8:] == bytes(rec.hits[1])[8:] and rec.best.pos == 40


def test_seventeen_and_more_hits_keep_the_first_sixteen_and_count_all():
    L = 2
    word = _word(L, 8)
    for n_words in (16, 17, 40):
        at = tuple(5 + 7 * i for i in range(n_words))
        x = _row(5 + 7 * n_words + 10, 13, word, at=at, sigma=0.0)
        pos, cr, ci, e, m, valid, _ = sm.model_windows(word, x, pl.SYNC_RESTART)
        thr = 0.999
        want = np.flatnonzero(valid & (m >= F32(thr)))
        assert set(at) <= set(want.tolist())
        rec, _ = _check_host(word, thr, x, pl.SYNC_RESTART, None, "%d words" % n_words)
        assert rec.n_hits == len(want) and [h.pos for h in rec.hits[: min(16, len(want))]] == want[:16].tolist()
        if len(want) < 16:
            assert bytes(rec.hits[len(want)]) == bytes(24)


def test_non_finite_symbols_and_rows_without_energy():
    L = 31
    word = _word(L, 9)
    x = _row(300, 14, word, at=(150,))
    for bad in (np.inf, -np.inf, np.nan):
        y = x.copy()
        y[0] = bad  # (what the first symbol of a differential stream is)
        y[2 * 200 + 1] = bad
        rec, _ = _check_host(word, 0.9, y, pl.SYNC_RESTART, None, "bad %r" % bad)
        # the windows that meet a bad symbol are not valid: those at 0 and at 170 .. 200
        assert rec.n_valid == rec.n_windows - 1 - L and rec.n_hits == 1 and rec.hits[0].pos == 150
    # a bad symbol in the history reaches the windows in front of the row
    hist = _row(127, 15)
    hist[2 * 126] = np.nan
    rec, _ = _check_host(word, 0.9, x, 0, hist, "bad history")
    assert rec.n_valid == rec.n_windows - (L - 1)
    # an all-zero row: d = 0 is below FLT_MIN, no window is valid, best stays zero bytes
    rec, _ = _check_host(word, 0.9, np.zeros(2 * 300, F32), pl.SYNC_RESTART, None, "zeros")
    assert rec.n_windows == 270 and rec.n_valid == 0 and rec.n_hits == 0 and bytes(rec.best) == bytes(24)
    # denormal energies stay below FLT_MIN too; tiny but normal ones do not
    tiny = (x * F32(1e-22)).astype(F32)
    rec, _ = _check_host(word, 0.9, tiny, pl.SYNC_RESTART, None, "tiny")
    assert rec.n_valid == 0
    # symbols whose energy overflows
    rec, _ = _check_host(word, 0.9, (x * F32(3e19)).astype(F32), pl.SYNC_RESTART, None, "huge")
    assert rec.n_valid == 0


def test_a_row_without_symbols_gives_the_zero_record_and_keeps_the_history():
    word = _word(31, 9)
    hist = _row(127, 15)
    for flags in (0, pl.SYNC_RESTART):
        rec, hout = _check_host(word, 0.9, np.zeros(0, F32), flags, hist, "empty")
        assert bytes(rec) == bytes(456) and hout.tobytes() == hist.tobytes()


def test_sync_host_bad_arguments():
    L = pl.load()
    word, x = _word(4, 1), _row(10, 2)
    rec, hout = pl.SyncRecord(), np.zeros(254, F32)

    def call(w=word, n_w=4, thr=0.5, flags=0, soft=x, n=10, r=rec):
        return L.psk_soft_sync_host(w.ctypes.data if w is not None else None, n_w, thr, flags, None,
                                    soft.ctypes.data if soft is not None else None, n, ctypes.byref(r) if r is not None else None,
                                    hout.ctypes.data)

    assert call() == pl.OK
    for kw in (dict(w=None), dict(soft=None), dict(r=None), dict(n_w=0), dict(n_w=129), dict(thr=0.0), dict(thr=-1.0), dict(thr=1.0000001),
               dict(thr=float("nan")), dict(flags=2), dict(flags=0x80000001), dict(n=1 << 30)):
        assert call(**kw) == 1, kw
    assert call(thr=1.0) == pl.OK and call(soft=None, n=0) == pl.OK


# ---- cuts and RESTART --------------------------------------------------------------------------------------------------------------

def _shifted_hits(rec, shift, drop_below):
    """the stored hits of a record with their positions in the whole row; those that start in front of the stream are dropped"""
    assert rec.n_hits <= 16
    return [(p + shift, cr, ci, e, m) for p, cr, ci, e, m in sm.hits_of(rec) if p + shift >= drop_below]


def test_a_row_cut_into_two_calls_gives_the_hits_and_the_best_of_the_row_whole():
    L = 31
    word = _word(L, 21)
    n = 700
    words_at = (60, 180, 181 + L, 400, 640)
    x = _row(n, 22, word, at=words_at, sigma=0.1)
    whole, whole_hist = pl.sync_host(word, 0.8, x, pl.SYNC_RESTART)
    assert [h.pos for h in whole.hits[: whole.n_hits]] == list(words_at)
    want = sm.hits_of(whole)
    for cut in (1, 5, 30, 31, 59, 60, 75, 90, 91, 127, 128, 200, 410, 669, 670, 699):
        a, ha = pl.sync_host(word, 0.8, x[: 2 * cut], pl.SYNC_RESTART)
        b, hb = pl.sync_host(word, 0.8, x[2 * cut:], 0, ha)
        # every position starts exactly one window: none twice, none left out -- but for the windows of the second call that
        # start in the zeros in front of a short first row, which are the host's to drop
        assert a.n_windows + b.n_windows - max(0, (L - 1) - cut) == whole.n_windows, cut
        got = _shifted_hits(a, 0, 0) + _shifted_hits(b, cut, 0)
        assert got == want, cut
        bests = [h for h in ((a.best, 0), (b.best, cut)) if bytes(h[0]) != bytes(24) and h[0].pos + h[1] >= 0]
        first = max(bests, key=lambda h: (h[0].m, -(h[0].pos + h[1])))
        assert (first[0].pos + first[1], bytes(first[0])[8:]) == (whole.best.pos, bytes(whole.best)[8:]), cut
        assert hb.tobytes() == whole_hist.tobytes(), cut
    # and into three
    a, ha = pl.sync_host(word, 0.8, x[: 2 * 190], pl.SYNC_RESTART)
    b, hb = pl.sync_host(word, 0.8, x[2 * 190: 2 * 200], 0, ha)
    c, hc = pl.sync_host(word, 0.8, x[2 * 200:], 0, hb)
    assert _shifted_hits(a, 0, 0) + _shifted_hits(b, 190, 0) + _shifted_hits(c, 200, 0) == want
    assert hc.tobytes() == whole_hist.tobytes()


def test_restart_semantics():
    L = 31
    word = _word(L, 23)
    hist = _row(127, 24, word, at=(127 - 10,))  # (the word's first ten symbols end the history)
    x = _row(300, 25, word, at=(-10, 100))     # (... and the row begins with the rest)
    cont, hc = pl.sync_host(word, 0.8, x, 0, hist)
    assert [h.pos for h in cont.hits[: cont.n_hits]] == [-10, 100] and cont.n_windows == 300
    rest, hr = pl.sync_host(word, 0.8, x, pl.SYNC_RESTART, hist)
    none, hn = pl.sync_host(word, 0.8, x, pl.SYNC_RESTART, None)
    # with RESTART the history in front is zeros whatever is passed, and no window starts in front of the row
    assert bytes(rest) == bytes(none) and hr.tobytes() == hn.tobytes()
    assert [h.pos for h in rest.hits[: rest.n_hits]] == [100] and rest.n_windows == 300 - L + 1
    assert hr.tobytes() == x[2 * (300 - 127):].tobytes() == hc.tobytes()
    # a short first row leaves zeros in front of it in the history
    short, hs = pl.sync_host(word, 0.8, x[: 2 * 20], pl.SYNC_RESTART, hist)
    assert short.n_windows == 0 and short.n_symbols == 20 and short.flags == pl.SYNC_DATA
    assert hs[: 2 * 107].tobytes() == bytes(8 * 107) and hs[2 * 107:].tobytes() == x[: 2 * 20].tobytes()
    # ... and the next call's windows that reach into them are there for the host to drop: it knows its stream offset
    nxt, _ = pl.sync_host(word, 0.8, x[2 * 20:], 0, hs)
    assert nxt.n_windows == 280 and [h.pos + 20 for h in nxt.hits[: nxt.n_hits] if h.pos + 20 >= 0] == [100]


# ---- the entry on a control-plane-only handle ------------------------------------------------------------------------------------

def _dry(nch=4):
    h = pl.Handle(nch, device=pl.DEVICE_NONE)
    h.sync_define(0, _word(31, 1))
    h.sync_define(15, _word(128, 2))
    return h


def _in(soft=0x10000, n=1000, word=1, flags=0, thr=0.5, pad=0):
    return pl.SyncIn(soft, n, word, flags, thr, pad)


def test_the_planned_record():
    h = _dry()
    assert bytes(h.sync_records()) == bytes(4 * 456)
    h.sync_device(0, [_in(), _in(word=16, flags=pl.SYNC_RESTART), _in(word=0), _in(n=20, flags=pl.SYNC_RESTART)])
    r = h.sync_records()
    want = np.zeros(4, sm.RECORD_DTYPE)
    for k, (n, nw, L) in enumerate(((1000, 1000, 31), (1000, 1000 - 128 + 1, 128), (0, 0, 0), (20, 0, 31))):
        if L:
            want[k]["n_symbols"], want[k]["n_windows"], want[k]["word_len"], want[k]["flags"] = n, nw, L, pl.SYNC_PLANNED
    assert bytes(r) == want.tobytes()
    # a call covers what it covers: channel 0 keeps its record; not searched: the zero record
    h.sync_device(1, [_in(soft=0), _in(n=0)])
    r2 = h.sync_records()
    want[1] = want[2] = np.zeros((), sm.RECORD_DTYPE)
    assert bytes(r2) == want.tobytes()
    assert h.sync_history(0).tobytes() == bytes(4 * 254)
    h.close()


def test_every_refusal_leaves_everything_as_it_was():
    h = _dry()
    L = pl.load()
    h.sync_device(0, [_in(), _in(), _in(), _in()])
    before = bytes(h.sync_records())
    good = _in()
    bad = dict(
        slot_above_15=_in(word=17), slot_never_defined=_in(word=2), thr_nan=_in(thr=float("nan")), thr_zero=_in(thr=0.0),
        thr_negative=_in(thr=-0.5), thr_above_one=_in(thr=1.5), unknown_flags=_in(flags=2), high_flag=_in(flags=0x80000000),
        pad=_in(pad=1), misaligned=_in(soft=0x10004), too_long=_in(n=1 << 30))
    for name, k in bad.items():
        for place in (0, 2):  # (first and last of the call: the channels in front of a bad one are not touched either)
            ins = [good, good, good]
            ins[place] = k
            with pytest.raises(pl.PskSoftError) as e:
                h.sync_device(1, ins)
            assert e.value.status == 1, name
            assert bytes(h.sync_records()) == before, name
    # what is wrong on a channel that is not searched is not looked at
    h.sync_device(1, [_in(word=0, thr=9.0, flags=77, pad=3), _in(soft=0, word=99), _in(n=0, soft=0x10004)])
    assert bytes(h.sync_records())[456:] == bytes(3 * 456)
    # the range, the pointers
    arr = (pl.SyncIn * 2)(good, good)
    assert L.psk_soft_sync_device(h._h, 3, 2, arr, None) == 1
    assert L.psk_soft_sync_device(h._h, 0, 0, arr, None) == 1
    assert L.psk_soft_sync_device(h._h, 0, 2, None, None) == 1
    assert L.psk_soft_sync_device(None, 0, 2, arr, None) == 1
    assert L.psk_soft_get_sync(h._h, 3, 2, (pl.SyncRecord * 2)()) == 1 and L.psk_soft_get_sync(h._h, 0, 1, None) == 1
    buf = np.zeros(254, F32)
    assert L.psk_soft_sync_get_history(h._h, 4, buf.ctypes.data) == 1 and L.psk_soft_sync_set_history(h._h, 0, None) == 1
    # the words
    w = _word(128, 1)
    for slot, ptr, n in ((16, w.ctypes.data, 4), (0, None, 4), (0, w.ctypes.data, 0), (0, w.ctypes.data, 129)):
        assert L.psk_soft_sync_define(h._h, slot, ptr, n) == 1
    assert bytes(h.sync_records())[:456] == before[:456]
    h.close()


def test_the_call_leaves_the_control_plane_alone():
    h = _dry()
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=50, phaseAvg=50)
    blob, stats = [h.export_state(c) for c in range(4)], h.stats()
    h.sync_device(0, [_in()] * 4)
    assert [h.export_state(c) for c in range(4)] == blob and h.stats() == stats
    h.close()


# ---- the derivation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", (2, 4, 8))
def test_sync_derive_at_every_rotation(M):
    L, Ew, amp = 32, 32.0, 0.7
    for r in range(M):
        for off in (-0.4, -0.05, 0.0, 0.05, 0.4):  # (of a step 2 pi / M)
            angle = 2 * math.pi * (r + off) / M
            e = F32(L * amp * amp)
            c = amp * L * 0.98
            hit = pl.SyncHit(123, F32(c * math.cos(angle)), F32(c * math.sin(angle)), e, F32(0.96))
            d = pl.sync_derive(hit, M, L, Ew)
            assert d["rotation"] == r, (M, r, off)
            assert abs(d["residual"] - 2 * math.pi * off / M) < 1e-6
            wrapped = math.atan2(math.sin(angle), math.cos(angle))
            assert abs(d["angle"] - wrapped) < 1e-6
            assert abs(d["amplitude"] - amp) < 1e-6
            assert abs(d["metric"] - (float(hit.cr) ** 2 + float(hit.ci) ** 2) / (float(e) * Ew)) < 1e-12
    zero = pl.sync_derive(pl.SyncHit(), M, L, Ew)
    assert zero["rotation"] == -1 and all(math.isnan(zero[k]) for k in ("angle", "residual", "amplitude", "metric"))


def test_sync_derive_bad_arguments():
    hit = pl.SyncHit(0, 1.0, 0.0, 1.0, 1.0)
    for M, L in ((0, 4), (1, 4), (3, 4), (16, 4), (4, 0), (4, 129)):
        with pytest.raises(pl.PskSoftError) as e:
            pl.sync_derive(hit, M, L, 4.0)
        assert e.value.status == 1
    L = pl.load()
    assert L.psk_soft_sync_derive(None, 4, 4, 4.0, ctypes.byref(pl.SyncDerived())) == 1
    assert L.psk_soft_sync_derive(ctypes.byref(hit), 4, 4, 4.0, None) == 1
    assert abs(pl.sync_word_energy(_word(32, 1)) - 32.0) < 1e-4


# ---- what the pass is for: frames in the reference's soft symbols -----------------------------------------------------------------

# (M, word length, noise sigma per component, seed): a random word every 500 symbols in random data, 8 samples a symbol with a
# rectangular pulse, numAvg 50, phaseAvg 50, packets of 8192 samples through the oracle.  At sigma 0.3 the reference's tracker slips
# a cycle between two frames on some noise draws -- the rotation of the hits then changes, which is what the record is there to
# show --; the draw here is one on which it does not.
ORACLE_CASES = ((4, 32, 0.1, 1), (4, 32, 0.3, 4), (8, 48, 0.05, 1))
ORACLE_SYMBOLS, ORACLE_FIRST, ORACLE_PERIOD, ORACLE_S = 6200, 137, 500, 8
_oracle_runs = {}


def oracle_run(oracle_mod, case):
    """(the oracle's soft symbols, the word, the word positions that lie in them) -- computed once"""
    if case not in _oracle_runs:
        M, WL, sigma, seed = case
        iq, w, starts = sm.framed_stream(M, ORACLE_S, WL, ORACLE_PERIOD, ORACLE_SYMBOLS, ORACLE_FIRST, sigma, seed)
        o = oracle_mod.OracleComponent()
        o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = ORACLE_S, M, 50, 50
        soft = oracle_mod.run_stream(o, iq, 0.01, packet_complex=8192)["soft"]
        _oracle_runs[case] = (soft, w, [s for s in starts if s + WL <= soft.size // 2], iq)
    return _oracle_runs[case]


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_the_word_is_found_at_every_frame_of_the_reference_with_one_rotation(oracle_mod, case):
    M, WL, sigma, seed = case
    soft, w, starts, _ = oracle_run(oracle_mod, case)
    assert len(starts) == 12
    pos, cr, ci, e, m, valid, _ = sm.model_windows(w, soft, pl.SYNC_RESTART)
    assert valid[1:].all()
    at = np.zeros(len(m), bool)
    at[starts] = True
    print("case", case, "metric at the words", float(m[at].min()), "..", float(m[at].max()), "elsewhere at most", float(m[~at & valid].max()))
    assert (m[at] >= 0.8).all() and (m[~at & valid] < 0.6).all()
    # the host's definition finds the twelve, and the derivation gives one rotation with a small residual
    rec, _ = pl.sync_host(w, 0.7, soft, pl.SYNC_RESTART)
    sm.assert_same(rec, sm.model_record(w, 0.7, soft, pl.SYNC_RESTART)[0], str(case))
    assert [h.pos for h in rec.hits[: rec.n_hits]] == starts
    Ew = pl.sync_word_energy(w)
    der = [pl.sync_derive(h, M, WL, Ew) for h in rec.hits[: rec.n_hits]]
    assert len({d["rotation"] for d in der}) == 1
    # (a residual beyond a quarter of a step would leave the decision within a quarter of a step of the next rotation)
    assert max(abs(d["residual"]) for d in der) < 0.25 * 2 * math.pi / M
