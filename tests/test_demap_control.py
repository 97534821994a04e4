"""psk_soft_demap_device without a GPU: the exports and the layouts, the host-side definition (psk_soft_demap_host) against
tests/demap_model.py byte for byte, the edges of its arithmetic, the symbols in front of a row (PSK_SOFT_DEMAP_FRONT), the entry on
control-plane-only handles (PSK_SOFT_DEVICE_NONE) -- it checks, then leaves planned records and nothing else --,
psk_soft_demap_gain, and what the pass is for: the frames behind the words found in the soft symbols of the reference (the
oracle), demapped to the bits that were sent."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401  (in front of the library: psk_soft_amd.lib.load says why)

from psk_soft_amd import lib as pl
from tests import demap_model as dm
from tests import sync_model as sm
from tests.test_sync_control import ORACLE_FIRST, ORACLE_PERIOD, ORACLE_SYMBOLS, oracle_run

F32 = np.float32
NEW = ("psk_soft_demap_define", "psk_soft_demap_device", "psk_soft_get_demap", "psk_soft_demap_host", "psk_soft_demap_gain",
       "psk_soft_demap_bytes", "psk_soft_demap_in_bytes", "psk_soft_demap_piece")
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5 * 1024 + 3)
GAIN = (0.9, 0.5)  # (what noisy_row divides by)


def test_the_symbols_are_exported_and_the_records_have_their_layout():
    L = pl.load()
    for name in NEW:
        assert name in pl.EXPORTS and hasattr(L, name), name
    assert L.psk_soft_abi_version() == 2
    R, I = pl.DemapRecord, pl.DemapIn
    assert ctypes.sizeof(R) == 64 == dm.RECORD_BYTES == L.psk_soft_demap_bytes()
    assert ctypes.sizeof(I) == 64 == dm.IN_BYTES == L.psk_soft_demap_in_bytes()
    names = ("n_symbols", "n_finite", "n_clip", "n_nan", "sum_e", "sum_err", "bits", "flags", "pad")
    assert [getattr(R, k).offset for k in names] == [0, 8, 16, 24, 32, 40, 48, 52, 56]
    assert [dm.RECORD_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 40, 48, 52, 56]
    names = ("soft", "n_symbols", "pos", "out", "count", "channel", "map", "flags", "gain_re", "gain_im", "scale", "pad")
    assert [getattr(I, k).offset for k in names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 60]
    assert (pl.DEMAP_I8, pl.DEMAP_FRONT) == (1, 2) == (dm.I8, dm.FRONT)
    assert (pl.DEMAP_DATA, pl.DEMAP_REC_I8, pl.DEMAP_PLANNED) == (1, 2, 128) == (dm.DATA, dm.REC_I8, dm.PLANNED)
    assert pl.DEMAP_REC_I8 == pl.DEMAP_I8 << 1
    assert (pl.DEMAP_GAIN_RESIDUAL, pl.DEMAP_GAIN_UNIT) == (1, 2)
    assert (pl.DEMAP_SLOTS, pl.DEMAP_MAX_SEGMENTS, pl.DEMAP_FRONT_SYMBOLS) == (16, 1 << 20, 127) and dm.FRONT_SYMBOLS == 127
    assert pl.demap_piece() == dm.PIECE == 1024 and dm.PIECE % dm.THREADS == 0


# ---- the definition ----------------------------------------------------------------------------------------------------------

def check_host(points, labels, x, pos, count, gain, scale, flags, front, ctx):
    out, rec = pl.demap_host(points, labels, x, pos, count, gain, scale, flags, front)
    mout, mrec = dm.model_segment(points, labels, x, pos, count, gain, scale, flags, front)
    assert out.dtype == mout.dtype and out.tobytes() == mout.tobytes(), ctx + ": values"
    dm.assert_same(rec, mrec, ctx)
    return out, rec


@pytest.mark.parametrize("M", (2, 4, 8))
def test_demap_host_against_the_model(M):
    points, labels = dm.odd_map(M)
    assert list(labels) != list(dm.gray_labels(M)) and abs(np.hypot(points[0::2], points[1::2]) - 1).max() > 0.1
    for count in COUNTS:
        for pos in (0, 7):
            x = dm.noisy_row(M, pos + count + 3, 100 * M + count + pos)
            for flags, scale in ((0, 3.25), (pl.DEMAP_I8, 40.0)):
                ctx = "M %d count %d pos %d flags %d" % (M, count, pos, flags)
                out, rec = check_host(points, labels, x, pos, count, GAIN, scale, flags, None, ctx)
                assert (rec.n_symbols, rec.n_finite, rec.n_nan, rec.bits) == (count, count, 0, dm.bits_of(M)), ctx
                assert rec.flags == pl.DEMAP_DATA | (pl.DEMAP_REC_I8 if flags else 0) and out.size == count * dm.bits_of(M), ctx
                assert rec.sum_e > 0 and rec.sum_err > 0 and (flags or rec.n_clip == 0), ctx
    # the int8 values are the rounded float32 ones, and some were clamped
    x = dm.noisy_row(M, 2000, 77)
    f, _ = pl.demap_host(points, labels, x, 0, 2000, GAIN, 90.0, 0)
    b, rec = pl.demap_host(points, labels, x, 0, 2000, GAIN, 90.0, pl.DEMAP_I8)
    assert np.array_equal(b, np.clip(np.rint(f), -127, 127).astype(np.int8)) and 0 < rec.n_clip == int((np.abs(np.rint(f)) > 127).sum())


def test_two_segments_of_a_frame_add_their_counts():
    points, labels = dm.odd_map(8)
    x = dm.noisy_row(8, 3000, 5)
    whole, w = pl.demap_host(points, labels, x, 100, 2500, GAIN, 20.0, pl.DEMAP_I8)
    a, ra = pl.demap_host(points, labels, x, 100, 700, GAIN, 20.0, pl.DEMAP_I8)
    b, rb = pl.demap_host(points, labels, x, 800, 1800, GAIN, 20.0, pl.DEMAP_I8)
    assert np.concatenate([a, b]).tobytes() == whole.tobytes()
    assert (ra.n_symbols + rb.n_symbols, ra.n_finite + rb.n_finite, ra.n_clip + rb.n_clip) == (w.n_symbols, w.n_finite, w.n_clip)
    # (the sums are added in an order that depends on the segment: equal but for the last bits)
    assert abs(ra.sum_err + rb.sum_err - w.sum_err) <= 1e-12 * w.sum_err and abs(ra.sum_e + rb.sum_e - w.sum_e) <= 1e-12 * w.sum_e


# ---- edges of the arithmetic -----------------------------------------------------------------------------------------------------

BPSK = np.array([1, 0, -1, 0], F32)  # with labels (0, 1) and y = (a, 0): d0 = (a - 1)^2, d1 = (a + 1)^2, l = d1 - d0 = 4 a


def _row_of(*symbols):
    return np.array(symbols, F32).reshape(-1)


def test_a_symbol_between_two_points_takes_the_first_minimum():
    for labels in ((0, 1), (1, 0)):
        x = _row_of((0.0, 0.5), (0.0, -2.0))
        for scale in (1.0, -1.0):
            out, rec = check_host(BPSK, labels, x, 0, 2, (1.0, 0.0), scale, 0, None, "between %r %g" % (labels, scale))
            assert (out == 0).all() and (np.signbit(out) == (scale < 0)).all()  # (l = +0: d - d of equal values)
            assert rec.sum_err == float(F32(1.25)) + float(F32(5.0))
    # QPSK on the axes, a symbol on a diagonal: the two nearest points tie, the first of them is dmin's
    points, labels = np.array([1, 0, 0, 1, -1, 0, 0, -1], F32), (0, 1, 3, 2)
    out, rec = check_host(points, labels, _row_of((0.5, 0.5)), 0, 1, (1.0, 0.0), 1.0, 0, None, "diagonal")
    assert out[1] == 0 and out[0] == 2.0 and rec.sum_err == 0.5  # (bit 1 separates the two nearest; bit 0 does not)


def test_ties_go_to_even_and_the_clamp_counts_what_it_changes():
    x = _row_of((0.125, 0.0))  # l = 0.5 exactly
    for k in range(0, 9):
        for sign in (1, -1):
            out, rec = check_host(BPSK, (0, 1), x, 0, 1, (1.0, 0.0), sign * (2 * k + 1), pl.DEMAP_I8, None, "k %d" % k)
            want = sign * (k if k % 2 == 0 else k + 1)  # k + 0.5 to the even neighbour
            assert out[0] == want and rec.n_clip == 0, (k, sign)
    for scale, want, clip in ((254.98, 127, 0), (-254.98, -127, 0), (255.0, 127, 1), (-255.0, -127, 1), (253.0, 126, 0), (1e30, 127, 1)):
        out, rec = check_host(BPSK, (0, 1), x, 0, 1, (1.0, 0.0), scale, pl.DEMAP_I8, None, "scale %g" % scale)
        assert (out[0], rec.n_clip, rec.n_nan) == (want, clip, 0), scale
    # v = +-inf: l of a huge symbol times a huge scale; float32 keeps the inf, int8 clamps and counts it
    big = _row_of((100.0, 0.0), (-100.0, 0.0))  # l = +-400
    f, rf = check_host(BPSK, (0, 1), big, 0, 2, (1.0, 0.0), 1e37, 0, None, "inf f32")
    assert f[0] == np.inf and f[1] == -np.inf and (rf.n_clip, rf.n_nan, rf.n_finite) == (0, 0, 2)
    b, rb = check_host(BPSK, (0, 1), big, 0, 2, (1.0, 0.0), 1e37, pl.DEMAP_I8, None, "inf i8")
    assert list(b) == [127, -127] and (rb.n_clip, rb.n_nan) == (2, 0)


def test_non_finite_symbols_at_the_edges_of_lanes_waves_and_pieces():
    M = 8
    points, labels = dm.odd_map(M)
    n = 2 * 1024 + 37
    where = (0, 63, 64, 255, 256, 1023, 1024, 1024 + 255, 2 * 1024, n - 1)
    for flags in (0, pl.DEMAP_I8):
        x = dm.noisy_row(M, n, 31)
        for k, s in enumerate(where):
            x[2 * s + (k & 1)] = (np.nan, np.inf, -np.inf)[k % 3]
        out, rec = check_host(points, labels, x, 0, n, GAIN, 10.0, flags, None, "non-finite flags %d" % flags)
        # every value of a bad symbol is NaN (inf - inf): written as 0 in int8, counted, left out of n_finite and of the sums
        assert rec.n_finite == n - len(where) and rec.n_nan == 3 * len(where)
        v = out.reshape(n, 3)
        bad = np.zeros(n, bool)
        bad[list(where)] = True
        # (float32: the one quiet NaN, whatever sign and payload the arithmetic handed on)
        assert (v[bad] == 0).all() if flags else (v[bad].view(np.uint32) == 0x7FC00000).all()
        assert np.isfinite(v[~bad].astype(F32)).all() and math.isfinite(rec.sum_e) and math.isfinite(rec.sum_err)
        clean = x.copy().reshape(-1, 2)
        clean[list(where)] = 0
        e, dmin = dm.symbol_terms(points, labels, clean, GAIN, 10.0)[:2]
        assert rec.sum_err == dm.ordered_sum(dmin, ~bad) and rec.sum_e == dm.ordered_sum(e, ~bad)
    # a gain that overflows a finite symbol: y is not finite, the symbol is not counted
    out, rec = check_host(points, labels, _row_of((3e38, 3e38)), 0, 1, (2.0, 2.0), 1.0, 0, None, "overflow")
    assert rec.n_finite == 0 and rec.sum_e == 0.0


def test_denormal_energies_are_kept():
    points, labels = dm.odd_map(4)
    x = (dm.noisy_row(4, 1500, 3) * F32(1e-21)).astype(F32)
    out, rec = check_host(points, labels, x, 0, 1500, GAIN, 5.0, 0, None, "denormal")
    e = dm.symbol_terms(points, labels, x.reshape(-1, 2), GAIN, 5.0)[0]
    assert 0 < e.max() < np.finfo(F32).tiny and rec.sum_e > 0 and rec.n_finite == 1500


def test_demap_host_bad_arguments():
    L = pl.load()
    points, labels = dm.odd_map(4)
    lab = np.ascontiguousarray(labels, np.uint8)
    x, out = dm.noisy_row(4, 50, 1), np.zeros(64, F32)
    rec = pl.DemapRecord()

    def call(p=points, lb=lab, M=4, r=rec, **kw):
        f = dict(soft=x.ctypes.data, n_symbols=50, pos=0, out=out.ctypes.data, count=10, channel=0, map=0, flags=0, gain_re=1.0,
                 gain_im=0.0, scale=1.0, pad=0)
        f.update(kw)
        k = pl.DemapIn(**f)
        return L.psk_soft_demap_host(p.ctypes.data if p is not None else None, lb.ctypes.data if lb is not None else None, M,
                                     ctypes.byref(k), None, ctypes.byref(r) if r is not None else None)

    assert call() == pl.OK and rec.n_symbols == 10
    nanp = points.copy()
    nanp[3] = np.nan
    for kw in (dict(p=None), dict(lb=None), dict(r=None), dict(M=3), dict(M=16), dict(M=0), dict(p=nanp), dict(lb=np.array([0, 1, 1, 3], np.uint8)),
               dict(lb=np.array([0, 1, 2, 4], np.uint8)), dict(flags=4), dict(pad=1), dict(soft=x.ctypes.data + 4), dict(out=None),
               dict(out=out.ctypes.data + 2), dict(n_symbols=1 << 30), dict(pos=-1), dict(pos=-128, flags=pl.DEMAP_FRONT), dict(pos=41), dict(pos=(1 << 63) - 1), dict(pos=(1 << 63) - 10), dict(pos=51, count=1),
               dict(gain_re=float("inf")), dict(gain_im=float("nan")), dict(scale=float("inf"))):
        assert call(**kw) == 1, kw
    assert call(pos=40) == pl.OK and call(pos=-127, flags=pl.DEMAP_FRONT) == pl.OK and call(out=out.ctypes.data + 1, flags=pl.DEMAP_I8) == pl.OK
    assert call(count=0, pos=99, flags=77) == pl.OK and bytes(rec) == bytes(64)  # (skipped: the zero record, nothing looked at)


# ---- the symbols in front of a row ----------------------------------------------------------------------------------------------

def test_front_splices_the_history_in_front_of_the_row():
    M = 8
    points, labels = dm.odd_map(M)
    hist, row = dm.noisy_row(M, 127, 41), dm.noisy_row(M, 1500, 42)
    joined = np.concatenate([hist, row])
    for pos, count in ((-127, 127), (-127, 1400), (-64, 65), (-1, 1), (-1, 1200), (0, 10), (5, 100)):
        for flags in (0, pl.DEMAP_I8):
            ctx = "front pos %d count %d flags %d" % (pos, count, flags)
            a, ra = check_host(points, labels, row, pos, count, GAIN, 30.0, flags | pl.DEMAP_FRONT, hist, ctx)
            b, rb = pl.demap_host(points, labels, joined, pos + 127, count, GAIN, 30.0, flags)
            assert a.tobytes() == b.tobytes() and bytes(ra) == bytes(rb), ctx
            # zeros in front: what the history is behind PSK_SOFT_SYNC_RESTART
            z, rz = check_host(points, labels, row, pos, count, GAIN, 30.0, flags | pl.DEMAP_FRONT, None, ctx + " zeros")
            zz, rzz = pl.demap_host(points, labels, np.concatenate([np.zeros(254, F32), row]), pos + 127, count, GAIN, 30.0, flags)
            assert z.tobytes() == zz.tobytes() and bytes(rz) == bytes(rzz), ctx


# ---- the entry on a control-plane-only handle ------------------------------------------------------------------------------------

def _dry(nch=4):
    h = pl.Handle(nch, device=pl.DEVICE_NONE)
    h.demap_define(0, *dm.odd_map(4))
    h.demap_define(15, *dm.odd_map(8))
    h.demap_define(3, *dm.odd_map(2))
    return h


def _in(soft=0x10000, n=1000, pos=0, out=0x20000, count=100, channel=0, map=1, flags=0, gr=1.0, gi=0.5, scale=2.0, pad=0):
    return pl.DemapIn(soft, n, pos, out, count, channel, map, flags, gr, gi, scale, pad)


def _no_call_yet(h):
    return pl.load().psk_soft_get_demap(h._h, 0, 1, (pl.DemapRecord * 1)()) == 1


def test_the_planned_records():
    h = _dry()
    assert _no_call_yet(h)
    h.demap_device([_in(), _in(map=16, flags=pl.DEMAP_I8, out=0x20001, count=7), _in(count=0), _in(map=0), _in(soft=0), _in(map=4, pos=900)])
    r = h.demap_records(0, 6)
    want = np.zeros(6, dm.RECORD_DTYPE)
    for k, (n, B, fl) in {0: (100, 2, 128), 1: (7, 3, 130), 5: (100, 1, 128)}.items():
        want[k]["n_symbols"], want[k]["bits"], want[k]["flags"] = n, B, fl
    assert bytes(r) == want.tobytes()
    assert bytes(h.demap_records(5, 1)) == want[5].tobytes()
    L = pl.load()
    arr = (pl.DemapRecord * 7)()
    assert L.psk_soft_get_demap(h._h, 0, 7, arr) == 1 and L.psk_soft_get_demap(h._h, 6, 1, arr) == 1 and L.psk_soft_get_demap(h._h, 0, 0, arr) == 1
    assert L.psk_soft_get_demap(h._h, 0, 1, None) == 1 and L.psk_soft_get_demap(None, 0, 1, arr) == 1
    # the records are the LAST call's
    h.demap_device([_in(count=5)])
    assert h.demap_records(0, 1)[0].n_symbols == 5 and L.psk_soft_get_demap(h._h, 1, 1, arr) == 1
    h.close()


def test_every_refusal_leaves_everything_as_it_was():
    h = _dry()
    L = pl.load()
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=50, phaseAvg=50)
    h.demap_device([_in(), _in(count=33), _in(map=16)])
    before = bytes(h.demap_records(0, 3))
    blob, stats, peek = [h.export_state(c) for c in range(4)], h.stats(), [h.peek(c) for c in range(4)]
    good = _in()
    bad = dict(
        slot_above_15=_in(map=17), slot_never_defined=_in(map=2), unknown_flags=_in(flags=4), high_flag=_in(flags=0x80000000), pad=_in(pad=1),
        misaligned_soft=_in(soft=0x10004), null_out=_in(out=0), misaligned_f32_out=_in(out=0x20002), too_long=_in(n=1 << 30),
        beyond_row=_in(pos=901), pos_int64_max=_in(pos=(1 << 63) - 1), pos_wraps_with_count=_in(pos=(1 << 63) - 100), pos_past_row=_in(pos=1001, count=1),
        count_beyond_row=_in(count=1001), negative_pos=_in(pos=-1), front_below=_in(pos=-128, flags=pl.DEMAP_FRONT),
        front_channel_range=_in(flags=pl.DEMAP_FRONT, channel=4), front_never_searched=_in(flags=pl.DEMAP_FRONT, pos=-5, channel=1),
        gain_inf=_in(gr=float("inf")), gain_nan=_in(gi=float("nan")), scale_nan=_in(scale=float("nan")), scale_inf=_in(scale=float("-inf")))
    for name, k in bad.items():
        for place in (0, 2):  # (first and last of the call)
            ins = [good, good, good]
            ins[place] = k
            with pytest.raises(pl.PskSoftError) as e:
                h.demap_device(ins)
            assert e.value.status == 1, name
            assert bytes(h.demap_records(0, 3)) == before, name
    arr = (pl.DemapIn * 2)(good, good)
    assert L.psk_soft_demap_device(h._h, 0, arr, None) == 1 and L.psk_soft_demap_device(h._h, (1 << 20) + 1, arr, None) == 1
    assert L.psk_soft_demap_device(h._h, 2, None, None) == 1 and L.psk_soft_demap_device(None, 2, arr, None) == 1
    assert bytes(h.demap_records(0, 3)) == before
    # the maps: every refusal of a definition leaves the slot as it was (slot 1 undefined, slot 0 QPSK)
    p4, l4 = dm.odd_map(4)
    l4 = np.ascontiguousarray(l4, np.uint8)
    nanp = p4.copy()
    nanp[0] = np.inf
    for slot, M, pts, lab in ((16, 4, p4, l4), (1, 3, p4, l4), (1, 16, p4, l4), (1, 4, None, l4), (1, 4, p4, None), (1, 4, nanp, l4),
                              (0, 4, p4, np.array([0, 0, 1, 2], np.uint8)), (0, 4, p4, np.array([1, 2, 3, 4], np.uint8))):
        assert L.psk_soft_demap_define(h._h, slot, M, pts.ctypes.data if pts is not None else None, lab.ctypes.data if lab is not None else None) == 1
    with pytest.raises(pl.PskSoftError):
        h.demap_device([_in(map=2)])
    assert bytes(h.demap_records(0, 3)) == before and h.demap_records(0, 1)[0].bits == 2
    # what is wrong on a skipped segment is not looked at
    h.demap_device([_in(count=0, flags=99, pad=3, map=40), _in(map=0, soft=0x10004), _in(soft=0, out=0, n=1 << 40)])
    assert bytes(h.demap_records(0, 3)) == bytes(3 * 64)
    # the control plane has not moved
    assert [h.export_state(c) for c in range(4)] == blob and h.stats() == stats
    assert [h.peek(c) for c in range(4)] == peek
    h.close()


def test_front_needs_a_sync_call_that_searched_the_channel():
    h = _dry()
    h.sync_define(0, np.array([1, 0, 0, 1, -1, 0], F32))
    front = _in(flags=pl.DEMAP_FRONT, pos=-100, channel=2)
    with pytest.raises(pl.PskSoftError):
        h.demap_device([front])
    # a sync call that covers channel 2 without searching it does not do
    h.sync_device(1, [pl.SyncIn(0x10000, 1000, 1, 0, 0.5, 0), pl.SyncIn(0x10000, 1000, 0, 0, 0.5, 0)])
    with pytest.raises(pl.PskSoftError):
        h.demap_device([front])
    h.demap_device([_in(flags=pl.DEMAP_FRONT, pos=-127, channel=1)])
    # one that searches it does, with or without RESTART; a later one that covers it without searching takes it back
    for flags in (0, pl.SYNC_RESTART):
        h.sync_device(2, [pl.SyncIn(0x10000, 1000, 1, flags, 0.5, 0)])
        h.demap_device([front, _in()])
        assert h.demap_records(0, 2)[0].flags == pl.DEMAP_PLANNED
    h.sync_device(2, [pl.SyncIn(0, 1000, 1, 0, 0.5, 0)])
    with pytest.raises(pl.PskSoftError):
        h.demap_device([front])
    h.close()


# ---- the gain --------------------------------------------------------------------------------------------------------------------

def _derived(rotation, residual=0.0, amplitude=1.0):
    return dict(angle=0.0, residual=residual, amplitude=amplitude, metric=1.0, rotation=rotation)


@pytest.mark.parametrize("M", (2, 4, 8))
def test_demap_gain_at_every_rotation(M):
    s = math.sqrt(0.5)
    table = {0: (1, 0), 1: (s, s), 2: (0, 1), 3: (-s, s), 4: (-1, 0), 5: (-s, -s), 6: (0, -1), 7: (s, -s)}
    for r in range(M):
        c, sn = table[r * (8 // M)]
        for amp in (1.0, 0.7, 1.37):
            g = pl.demap_gain(_derived(r, 0.3, amp), M)
            assert g.dtype == F32 and g[0] == F32(c / amp) and g[1] == F32(-sn / amp), (M, r, amp)
            if r * (8 // M) % 2 == 0:  # a quadrant turn: one part is an exact 0
                assert (g[0] == 0) != (g[1] == 0)
            u = pl.demap_gain(_derived(r, 0.3, amp), M, pl.DEMAP_GAIN_UNIT)
            assert u[0] == F32(c) and u[1] == F32(-sn)
            for res in (-0.3, -1e-3, 0.0, 0.05, math.pi / M):
                theta = 2 * math.pi * r / M + res
                want = np.array([np.cos(theta) / amp, -np.sin(theta) / amp], np.float64)
                got = pl.demap_gain(_derived(r, res, amp), M, pl.DEMAP_GAIN_RESIDUAL)
                ulp = np.maximum(np.spacing(np.abs(want).astype(F32)), np.spacing(F32(1e-7))).astype(np.float64)
                assert (np.abs(got.astype(np.float64) - want) <= ulp).all(), (M, r, amp, res, got, want)
    # the gain undoes the turn: a point of the rotated constellation comes back to its place
    z = sm.psk_points(M, np.arange(M)) * 0.7 * np.exp(2j * math.pi * 1 / M)
    g = pl.demap_gain(_derived(1, 0.0, 0.7), M)
    assert np.abs(z * (complex(g[0]) + 1j * complex(g[1])) - sm.psk_points(M, np.arange(M))).max() < 1e-6


def test_demap_gain_bad_arguments():
    for d, M, flags in ((_derived(-1), 4, 0), (_derived(4), 4, 0), (_derived(2), 2, 0), (_derived(0, 0.0, 0.0), 4, 0), (_derived(0, 0.0, -1.0), 4, 0),
                        (_derived(0, 0.0, float("nan")), 4, 0), (_derived(0, 0.0, float("inf")), 4, 0), (_derived(0), 3, 0), (_derived(0), 16, 0),
                        (_derived(0), 4, 4), (_derived(0, float("nan")), 4, pl.DEMAP_GAIN_RESIDUAL)):
        with pytest.raises(pl.PskSoftError) as e:
            pl.demap_gain(d, M, flags)
        assert e.value.status == 1
    L = pl.load()
    g = (ctypes.c_float * 2)()
    assert L.psk_soft_demap_gain(None, 4, 0, g) == 1 and L.psk_soft_demap_gain(ctypes.byref(pl.SyncDerived(0, 0, 1.0, 1, 0, 0)), 4, 0, None) == 1
    assert pl.demap_gain(_derived(0, float("nan")), 4)[0] == 1.0  # (the residual is not looked at without its flag)


# ---- what the pass is for: the frames of the reference's soft symbols as the bits that were sent ------------------------------------

# (M, word length, noise sigma per component, seed), as tests/test_sync_control.py builds them
CLEAN_CASES = ((4, 32, 0.1, 1), (8, 48, 0.05, 1), (2, 32, 0.2, 3))
NOISY_CASE = (4, 32, 0.3, 4)
FRAME = 500


def demap_frames(oracle_mod, case):
    """the frames of 500 symbols behind the twelve hits: (the bits sent, the LLRs by the host, by the model, the records)"""
    M, WL, sigma, seed = case
    B = dm.bits_of(M)
    soft, w, starts, _ = oracle_run(oracle_mod, case)
    data, _, _ = sm.framed_symbols(M, WL, ORACLE_PERIOD, ORACLE_SYMBOLS, ORACLE_FIRST, seed)
    rec, _ = pl.sync_host(w, 0.7, soft, pl.SYNC_RESTART)
    hits = list(rec.hits[: rec.n_hits])
    assert [h.pos for h in hits] == starts and len(hits) == 12
    labels = dm.gray_labels(M)
    pz = sm.psk_points(M, np.arange(M))
    points = np.empty(2 * M, F32)
    points[0::2], points[1::2] = pz.real, pz.imag
    Ew = pl.sync_word_energy(w)
    sent, host, model, recs = [], [], [], []
    for h in hits:
        gain = pl.demap_gain(pl.sync_derive(h, M, WL, Ew), M)
        assert h.pos + FRAME <= soft.size // 2
        out, r = pl.demap_host(points, labels, soft, h.pos, FRAME, gain, 1.0, 0)
        mout, mr = dm.model_segment(points, labels, soft, h.pos, FRAME, gain, 1.0, 0)
        dm.assert_same(r, mr, "%r frame at %d" % (case, h.pos))
        lab = labels[data[h.pos: h.pos + FRAME]]
        sent.append(np.array([[(v >> (B - 1 - j)) & 1 for j in range(B)] for v in lab]).reshape(-1))
        host.append(out), model.append(mout), recs.append(r)
    return np.concatenate(sent), np.concatenate(host), np.concatenate(model), recs


@pytest.mark.parametrize("case", CLEAN_CASES)
def test_the_signs_of_the_llrs_are_the_bits_that_were_sent(oracle_mod, case):
    M, WL, sigma, seed = case
    sent, host, model, recs = demap_frames(oracle_mod, case)
    assert host.tobytes() == model.tobytes() and sent.size == 12 * FRAME * dm.bits_of(M)
    errors = int(((host < 0).astype(int) != sent).sum())  # (a positive value: bit 0 is the nearer)
    print("case", case, "bit errors", errors, "of", sent.size, "smallest |l|", float(np.abs(host).min()))
    assert errors == 0
    # the decision-directed noise power per component, from the record alone
    est = [r.sum_err / (2 * r.n_finite) for r in recs]
    print("case", case, "sigma^2", sigma * sigma, "estimated", min(est), "..", max(est))
    assert all(r.n_finite == FRAME for r in recs) and all(abs(v - sigma * sigma) <= 0.25 * sigma * sigma for v in est)


def test_a_noisy_stream_has_the_errors_theory_gives_it(oracle_mod):
    sent, host, model, recs = demap_frames(oracle_mod, NOISY_CASE)
    errors, merrors = int(((host < 0).astype(int) != sent).sum()), int(((model < 0).astype(int) != sent).sum())
    print("case", NOISY_CASE, "bit errors", errors, "of", sent.size, "(theory for one picked sample a symbol: Q(0.707 / 0.3) = 0.92 %)")
    assert errors == merrors and host.tobytes() == model.tobytes()
    assert errors < 0.02 * sent.size
