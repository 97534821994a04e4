"""psk_soft_process_device_strided on control-plane-only handles (PSK_SOFT_DEVICE_NONE): the entry checks the strides, then
plans and counts exactly like psk_soft_process_device -- a packet's stride changes where its samples lie, never how many there
are.  No GPU: nothing here touches data."""
import ctypes

import pytest

from psk_soft_amd import lib as pl

FORMATS = (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8)
OUT_FIELDS = ("ret", "n_symbols", "n_bits", "n_sampleIndex", "sri_pushed", "sri_soft_xdelta", "sri_bits_xdelta", "n_warn")
LIMITS = dict(max_window_samples=64 * 1025 + 64, max_phase_avg=40000)


def _table():
    """the configuration table of tests.test_control_plane.test_which_kernel_a_configuration_is_planned_for"""
    return [(S, A, n) for S in list(range(2, 35)) + [40, 64] for A in (1, 100, 128, 129, 256, 257, 512, 513, 1024, 1025)
            for n in (50,)] + [(8, 100, n) for n in (1, 384, 385, 1920, 1921, 4000, 32640, 32641)] + [(24, 300, 1000), (16, 1024, 1920)]


def _packets(cfgs, fmt, k, odd=False):
    pk, out = (pl.Packet * len(cfgs))(), (pl.Output * len(cfgs))()
    for i, (S, A, n) in enumerate(cfgs):
        pk[i].n_floats = 2 * S * (A + 300) + (1 if odd and i % 3 == 0 else 0)
        pk[i].sri_xdelta, pk[i].sri_mode, pk[i].sriChanged, pk[i].present, pk[i].format = 0.01, 1, int(k == 0), 1, fmt
        out[i].cap_symbols = 1 << 62
    return pk, out


def _results(out):
    return [tuple(getattr(o, f) for f in OUT_FIELDS) for o in out]


def _handle(cfgs):
    h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, **LIMITS)
    h.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
    return h


def _peeks(h):
    return [h.peek(c) for c in range(h.n_channels)]


def _queries(h):
    return [tuple(getattr(h.query(c), k) for k in pl.PROP_NAMES) for c in range(h.n_channels)]


def test_the_symbol_is_exported_and_the_abi_version_stays():
    assert "psk_soft_process_device_strided" in pl.EXPORTS
    L = pl.load()
    assert hasattr(L, "psk_soft_process_device_strided")
    assert L.psk_soft_abi_version() == 2
    assert ctypes.sizeof(pl.Packet) == 32 and ctypes.sizeof(pl.Output) == 104 and ctypes.sizeof(pl.Stats) == 96


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stride", [1, 7, 4096])
def test_counts_sri_warnings_stats_and_peek_equal_the_contiguous_call(fmt, stride):
    cfgs = _table()
    ref, got = _handle(cfgs), _handle(cfgs)
    for k in range(2):
        pk, out_r = _packets(cfgs, fmt, k, odd=True)
        _, out_g = _packets(cfgs, fmt, k, odd=True)
        if k == 1:  # a missing packet and a real (mode 0) one: dropped with a warning
            pk[3].present = 0
            pk[4].sri_mode = 0
        ref.process_device(0, pk, out_r)
        # (every second packet of the stride-7 case stays contiguous: one call may mix)
        strides = [1 if stride == 7 and i % 2 else stride for i in range(len(cfgs))]
        got.process_device_strided(0, pk, strides, out_g)
        assert _results(out_g) == _results(out_r), (k, stride)
        assert got.stats() == ref.stats()
        assert _peeks(got) == _peeks(ref)
    assert [got.channel_stats(c, 1) for c in (0, 5, len(cfgs) - 1)] == [ref.channel_stats(c, 1) for c in (0, 5, len(cfgs) - 1)]
    ref.close()
    got.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_null_and_all_ones_are_the_contiguous_call(fmt):
    cfgs = _table()[::7]
    hs = [_handle(cfgs) for _ in range(3)]
    for k in range(3):
        outs = []
        for j, h in enumerate(hs):
            pk, out = _packets(cfgs, fmt, k)
            if j == 0:
                h.process_device(0, pk, out)
            elif j == 1:
                h.process_device_strided(0, pk, None, out)
            else:
                h.process_device_strided(0, pk, (ctypes.c_uint64 * len(cfgs))(*([1] * len(cfgs))), out)
            outs.append(_results(out))
        assert outs[1] == outs[0] and outs[2] == outs[0]
        assert [h.stats() for h in hs[1:]] == [hs[0].stats()] * 2
        assert [_peeks(h) for h in hs[1:]] == [_peeks(hs[0])] * 2
    for h in hs:
        h.close()


def test_quality_records_of_a_control_plane_handle_are_the_contiguous_ones():
    cfgs = _table()[::11]
    ref, got = _handle(cfgs), _handle(cfgs)
    for h in (ref, got):
        h.set_option(pl.Handle.OPT_QUALITY, 1)
    for k in range(2):
        pk, out = _packets(cfgs, pl.FORMAT_CS16, k)
        ref.process_device(0, pk, out)
        got.process_device_strided(0, pk, [33] * len(cfgs), out)
    assert bytes(got.quality_records()) == bytes(ref.quality_records())
    ref.close()
    got.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_stride_of_zero_and_an_overflowing_extent_are_refused_and_change_nothing(fmt):
    cfgs = _table()[::5]
    C = len(cfgs)
    h, fresh = _handle(cfgs), _handle(cfgs)
    L = pl.load()
    sample_bytes = pl.FORMAT_SAMPLE_BYTES[fmt]
    for k in range(2):
        pk, out = _packets(cfgs, fmt, k)
        before = (_peeks(h), _queries(h), h.stats())
        n_last = int(pk[C - 1].n_floats) // 2
        bad = [
            [1] * 4 + [0] + [1] * (C - 5),                                         # a stride of 0
            [3] * (C - 1) + [(1 << 64) // (sample_bytes * n_last) + 1],            # stride x bytes x samples >= 2^64
            [(1 << 64) - 1] + [1] * (C - 1),                                       # stride x bytes alone overflows
        ]
        for strides in bad:
            arr = (ctypes.c_uint64 * C)(*strides)
            _, out_bad = _packets(cfgs, fmt, k)
            st = L.psk_soft_process_device_strided(h._h, 0, C, pk, arr, out_bad, None)
            assert st == 1, strides  # PSK_SOFT_ERR_INVALID_ARG
            assert b"stride" in L.psk_soft_last_error()
            with pytest.raises(pl.PskSoftError) as ei:
                h.process_device_strided(0, pk, strides, out_bad)
            assert ei.value.status == 1
            assert (_peeks(h), _queries(h), h.stats()) == before
        # the largest extent that fits is accepted (nothing is read on a control-plane-only handle) ...
        fits = [((1 << 64) - 1) // (sample_bytes * (int(pk[i].n_floats) // 2)) for i in range(C)]
        h.process_device_strided(0, pk, fits, out)
        # ... and the sequence goes on as a fresh one does
        _, out_f = _packets(cfgs, fmt, k)
        fresh.process_device(0, pk, out_f)
        assert _results(out) == _results(out_f)
        assert _peeks(h) == _peeks(fresh) and h.stats() == fresh.stats()
    # a packet that is absent is not looked at: its stride may be anything
    pk, out = _packets(cfgs, fmt, 2)
    pk[2].present = 0
    h.process_device_strided(0, pk, [5, 5, 0] + [5] * (C - 3), out)
    _, out_f = _packets(cfgs, fmt, 2)
    fresh.process_device(0, pk, out_f)
    assert _results(out) == _results(out_f) and _peeks(h) == _peeks(fresh)
    h.close()
    fresh.close()


def test_an_unknown_format_is_refused_as_by_the_contiguous_call():
    cfgs = _table()[:4]
    h = _handle(cfgs)
    pk, out = _packets(cfgs, pl.FORMAT_CF32, 0)
    pk[1].format = 2
    before = _peeks(h)
    with pytest.raises(pl.PskSoftError) as ei:
        h.process_device_strided(0, pk, [9] * 4, out)
    assert ei.value.status == 1 and "unknown packet format 2" in str(ei.value)
    assert _peeks(h) == before
    h.close()


def test_frame_major_packets_helper():
    pk, strides = pl.frame_major_packets(0x10000, [100, 90, 80], 128, 5, 3, pl.FORMAT_CS16, xdelta=0.25, sriChanged=True)
    assert [int(p.data) for p in pk] == [0x10000 + 4 * 5, 0x10000 + 4 * 6, 0x10000 + 4 * 7]
    assert [int(p.n_floats) for p in pk] == [200, 180, 160] and list(strides) == [128] * 3
    assert all(p.present == 1 and p.sri_mode == 1 and p.sriChanged == 1 and p.format == pl.FORMAT_CS16 and p.sri_xdelta == 0.25 for p in pk)
    pk, strides = pl.frame_major_packets(0, 10, 4, 0, 4, pl.FORMAT_CS8)
    assert [int(p.data or 0) for p in pk] == [0, 2, 4, 6] and [int(p.n_floats) for p in pk] == [20] * 4
    with pytest.raises(ValueError):
        pl.frame_major_packets(0, 10, 4, 2, 3)
