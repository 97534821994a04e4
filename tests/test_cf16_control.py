"""Complex binary16 packets (PSK_SOFT_FORMAT_CF16 = 4: interleaved IEEE half I/Q, torch.complex32) on the control plane, without a
GPU: format 4 is accepted on the per-channel and the stamped path and planned exactly like float packets of the same element
count, in batches that mix all four formats too; 5 and 6 stay refused with nothing committed; counts and SRI are the oracle's
on the widened data; a strided packet whose `data` is only 2-byte aligned is refused."""
import ctypes
import math

import numpy as np
import pytest

from psk_soft_amd import lib as pl

ALL_FORMATS = (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, getattr(pl, "FORMAT_CF16", None))


def _peek_all(h):
    return [h.peek(c) for c in range(h.n_channels)]


def _routing_cfgs():
    # the table of test_cs16_control.py (test_control_plane.py::test_which_kernel_a_configuration_is_planned_for)
    return [(S, A, n) for S in list(range(2, 35)) + [40, 64] for A in (1, 100, 128, 129, 256, 257, 512, 513, 1024, 1025)
            for n in (50,)] + [(8, 100, n) for n in (1, 384, 385, 1920, 1921, 4000, 32640, 32641)] + [(24, 300, 1000), (16, 1024, 1920)]


def _bits16(u):
    return np.asarray(u, np.uint16).view(np.float16)


def test_numpy_widens_as_the_contract_says():
    """the oracle's input is x.astype(np.float32): value-exact for every finite encoding, subnormals become normal floats, a
    quiet NaN keeps sign and payload (shifted left by 13)"""
    u = np.arange(65536, dtype=np.uint32)
    finite = (u & 0x7C00) != 0x7C00
    w = _bits16(u.astype(np.uint16)).astype(np.float32).view(np.uint32)
    sign, e, m = (u >> 15) << 31, (u >> 10) & 31, u & 1023
    norm = (e > 0) & finite
    assert np.array_equal(w[norm], (sign | ((e + 112) << 23) | (m << 13))[norm])
    sub = (e == 0) & (m > 0)
    assert np.array_equal(_bits16(u[sub].astype(np.uint16)).astype(np.float64), np.where(u[sub] >> 15, -1.0, 1.0) * m[sub] * 2.0 ** -24)
    assert ((w[sub] >> 23) & 255).min() >= 103  # (normal floats)
    for enc, want in ((0x7C00, 0x7F800000), (0xFC00, 0xFF800000), (0x7E00, 0x7FC00000), (0xFE00, 0xFFC00000), (0x7E01, 0x7FC02000)):
        assert int(w[enc]) == want, hex(enc)


def test_format_constant_and_unchanged_struct_layout():
    assert (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8, pl.FORMAT_CF16) == (0, 1, 3, 4)
    assert pl.FORMAT_SAMPLE_BYTES[pl.FORMAT_CF16] == 4
    assert pl.Packet.format.offset == 31 and pl.Packet.format.size == 1
    assert ctypes.sizeof(pl.Packet) == 32 and ctypes.sizeof(pl.Output) == 104 and ctypes.sizeof(pl.Stats) == 96
    assert pl.load().psk_soft_abi_version() == 2


@pytest.mark.parametrize("bad", [2, 5, 6, 7, 255])
def test_format_4_is_accepted_and_the_others_stay_refused_with_nothing_committed(bad):
    h = pl.Handle(4, device=pl.DEVICE_NONE)
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=100)
    h.plan_only(0, [dict(n_floats=2 * 1000, xdelta=0.01, sriChanged=True, format=pl.FORMAT_CF16)] * 4)
    before = _peek_all(h)
    assert before[0]["ring_len"] > 0
    pk = [dict(n_floats=2 * 3000, xdelta=0.01, format=pl.FORMAT_CF16)] * 4
    pk[1] = dict(pk[1], format=bad)
    with pytest.raises(pl.PskSoftError) as e:
        h.plan_only(0, pk)
    assert e.value.status == 1 and "format %d" % bad in str(e.value) and "CF16 = 4" in str(e.value)
    assert _peek_all(h) == before
    # a uniform batch (the stamped path) with the bad format in its first packet: the same
    with pytest.raises(pl.PskSoftError) as e:
        h.plan_only(0, [dict(n_floats=2 * 3000, xdelta=0.01, format=bad)] * 4)
    assert e.value.status == 1
    assert _peek_all(h) == before
    # the host-buffer entry checks it too (a control-plane handle: no data is read) and takes format 4
    arr = (pl.Packet * 1)()
    out = (pl.Output * 1)()
    arr[0].n_floats, arr[0].sri_xdelta, arr[0].sri_mode, arr[0].present, arr[0].format = 64, 0.01, 1, 1, bad
    out[0].cap_symbols = 1 << 40
    assert pl.load().psk_soft_process_host(h._h, 0, 1, arr, out) == 1
    assert _peek_all(h) == before
    arr[0].format = pl.FORMAT_CF16
    assert pl.load().psk_soft_process_host(h._h, 0, 1, arr, out) == 0
    h.close()


def test_cf16_packets_are_routed_like_float_packets():
    cfgs = _routing_cfgs()
    got = {}
    for fmt in (pl.FORMAT_CF32, pl.FORMAT_CF16):
        h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
        h.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
        res = []
        for k in range(2):
            res.append(h.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1, xdelta=0.01, sriChanged=(k == 0), format=fmt)
                                       for S, A, n in cfgs]))
        got[fmt] = (h.stats(), res, _peek_all(h))
        h.close()
    st_f, res_f, peek_f = got[pl.FORMAT_CF32]
    st_c, res_c, peek_c = got[pl.FORMAT_CF16]
    n_fast = sum(1 for S, A, n in cfgs if 2 <= S <= 1024 and n <= 32640)
    assert st_c["channels_fast"] == n_fast and st_c["channels_sequential"] == len(cfgs) - n_fast, st_c
    assert st_c == st_f
    assert res_c == res_f and peek_c == peek_f


def test_a_batch_mixing_the_four_formats_is_planned_like_float():
    cfgs = _routing_cfgs()
    ref = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
    h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
    for x in (ref, h):
        x.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
    for k in range(4):
        r_f = ref.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1 + k, xdelta=0.01, sriChanged=(k == 0)) for S, A, n in cfgs])
        r_m = h.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1 + k, xdelta=0.01, sriChanged=(k == 0), format=ALL_FORMATS[(i + k) % 4])
                              for i, (S, A, n) in enumerate(cfgs)])
        assert r_m == r_f
    assert _peek_all(h) == _peek_all(ref)
    assert h.stats() == ref.stats()
    h.close()
    ref.close()


@pytest.mark.parametrize("n_ch", [16, 64])
def test_stamped_batches_of_cf16_packets(n_ch):
    """Uniform batches (the stamped path: 16 channels or more with equal packets) of format 4, then batches that switch
    between the formats call by call and batches whose packets differ only in their format: every result and every
    channel's state as the float batch gives them."""
    fmts = [pl.FORMAT_CF16, pl.FORMAT_CF16, pl.FORMAT_CS16, pl.FORMAT_CF32, pl.FORMAT_CF16, pl.FORMAT_CS8, pl.FORMAT_CF16]
    ref = pl.Handle(n_ch, device=pl.DEVICE_NONE)
    h = pl.Handle(n_ch, device=pl.DEVICE_NONE)
    for x in (ref, h):
        x.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=100, phaseAvg=50)
    for k, fmt in enumerate(fmts):
        n = 2 * 8 * (1000 + 37 * k) + (k % 2)
        r_f = ref.plan_only(0, [dict(n_floats=n, xdelta=0.01, sriChanged=(k == 0))] * n_ch)
        r_c = h.plan_only(0, [dict(n_floats=n, xdelta=0.01, sriChanged=(k == 0), format=fmt)] * n_ch)
        assert r_c == r_f
    # the stamp key tells the formats apart: one channel's packet in another format breaks the uniform run, the plans
    # stay the float plans -- CF16 among CS16 (the same bytes per sample) as well as the others
    n = 2 * 8 * 1500
    for base, odd in ((pl.FORMAT_CF16, pl.FORMAT_CS16), (pl.FORMAT_CS16, pl.FORMAT_CF16), (pl.FORMAT_CF16, pl.FORMAT_CF32)):
        r_f = ref.plan_only(0, [dict(n_floats=n, xdelta=0.01)] * n_ch)
        pk = [dict(n_floats=n, xdelta=0.01, format=base)] * n_ch
        pk[n_ch // 2] = dict(pk[n_ch // 2], format=odd)
        pk[n_ch - 1] = dict(pk[n_ch - 1], format=pl.FORMAT_CS8)
        assert h.plan_only(0, pk) == r_f
    assert _peek_all(h) == _peek_all(ref)
    st = h.stats()
    assert st == ref.stats() and st["channels_sequential"] == 0
    h.close()
    ref.close()


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_counts_and_sri_equal_the_oracles_on_the_widened_data(oracle_mod):
    """A sequence of CF16 calls with ragged sizes, an odd last element, a real-data packet, a queue flush and an xdelta
    change: counts, SRI pushes and xdeltas, warnings and the carried lengths are what the oracle gives for
    x.astype(np.float32)."""
    rng = np.random.default_rng(11)
    h = pl.Handle(1, device=pl.DEVICE_NONE, max_window_samples=1 << 16, max_phase_avg=4096)
    o = oracle_mod.OracleComponent()
    for name, v in (("samplesPerBaud", 8), ("constelationSize", 8), ("numAvg", 100), ("phaseAvg", 50)):
        h.configure(0, [{name: v}])
        setattr(o, name, v)
    sizes = [2 * 1000 * 8, 6, 2 * 333 + 1, 2 * 4096, 0, 2 * 17 * 8, 2 * 2500 + 1, 1]
    for i, n in enumerate(sizes):
        x = rng.standard_normal(n).astype(np.float16)
        xd = 0.01 if i < 3 else 0.02
        mode = 0 if i == 5 else 1
        kw = dict(mode=mode, sriChanged=(i in (0, 3)), inputQueueFlushed=(i == 6))
        ro = o.service(x.astype(np.float32), xd, **kw)
        rg = h.plan_only(0, [dict(n_floats=n, xdelta=xd, format=pl.FORMAT_CF16, **kw)])[0]
        assert rg["ret"] == ro.ret, i
        assert rg["n_symbols"] == ro.phase.size and 2 * rg["n_symbols"] == ro.soft.size, i
        assert rg["n_bits"] == ro.bits.size and rg["n_sampleIndex"] == ro.index.size, i
        assert rg["sri_pushed"] == ro.sri_pushed, i
        if ro.sri_pushed:
            assert _same(rg["sri_soft_xdelta"], ro.sri_soft_xdelta) and _same(rg["sri_bits_xdelta"], ro.sri_bits_xdelta), i
        assert rg["n_warn"] == ro.n_warn, i
        pk = h.peek(0)
        assert (pk["ring_len"], pk["index"], pk["fit_len"]) == (o.ring_size, o.index, o.fit_history().size), i
    h.close()


def test_a_2_byte_aligned_strided_cf16_packet_is_refused_and_changes_nothing():
    """`data` of a CF16 packet is 4-byte aligned (whole samples).  A control-plane-only handle never looks at the pointer of a
    contiguous packet; the strided entry checks the alignment of what it would gather before anything is planned, on such a
    handle too: 2-byte aligned is refused with PSK_SOFT_ERR_INVALID_ARG and the text names the format, 4-byte aligned goes
    through and counts like the contiguous call."""
    C = 12
    h, ref = pl.Handle(C, device=pl.DEVICE_NONE), pl.Handle(C, device=pl.DEVICE_NONE)
    for x in (h, ref):
        x.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=100)
    base = 1 << 20  # (an address: nothing is read)
    pk, strides = pl.frame_major_packets(base, 4000, 64, 3, C, fmt=pl.FORMAT_CF16, xdelta=0.01, sriChanged=True)
    assert [pk[i].data for i in (0, 1)] == [base + 12, base + 16]
    out = (pl.Output * C)()
    for o in out:
        o.cap_symbols = 1 << 62
    before = (_peek_all(h), h.stats())
    good = pk[5].data
    pk[5].data = good + 2
    with pytest.raises(pl.PskSoftError) as e:
        h.process_device_strided(0, pk, strides, out)
    assert e.value.status == 1 and "(CF16: 4)" in str(e.value) and "aligned (CS16: 4)" in str(e.value)
    assert (_peek_all(h), h.stats()) == before
    pk[5].data = good
    h.process_device_strided(0, pk, strides, out)
    out_r = (pl.Output * C)()
    for o in out_r:
        o.cap_symbols = 1 << 62
    ref.process_device(0, pk, out_r)
    fields = ("ret", "n_symbols", "n_bits", "n_sampleIndex", "sri_pushed", "sri_soft_xdelta", "sri_bits_xdelta", "n_warn")
    assert [tuple(getattr(o, f) for f in fields) for o in out] == [tuple(getattr(o, f) for f in fields) for o in out_r]
    assert _peek_all(h) == _peek_all(ref) and h.stats() == ref.stats()
    h.close()
    ref.close()
