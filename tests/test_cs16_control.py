"""Complex int16 packets (PSK_SOFT_FORMAT_CS16) on the control plane, without a GPU: the format field is checked, a
refused call commits nothing, CS16 packets are planned for the same kernels as float ones, and the C++ host class with a
short input port counts and pushes what the oracle does on the float cast of the same packets."""
import ctypes

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from psk_soft_amd import sandbox


def _peek_all(h):
    return [h.peek(c) for c in range(h.n_channels)]


@pytest.mark.parametrize("bad", [2, 7, 255])
def test_unknown_format_is_refused_and_nothing_is_committed(bad):
    h = pl.Handle(4, device=pl.DEVICE_NONE)
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=100)
    h.plan_only(0, [dict(n_floats=2 * 1000, xdelta=0.01, sriChanged=True)] * 4)
    before = _peek_all(h)
    pk = [dict(n_floats=2 * 3000, xdelta=0.01, format=pl.FORMAT_CS16)] * 4
    pk[2] = dict(pk[2], format=bad)
    with pytest.raises(pl.PskSoftError) as e:
        h.plan_only(0, pk)
    assert e.value.status == 1  # PSK_SOFT_ERR_INVALID_ARG
    assert "format" in str(e.value)
    assert _peek_all(h) == before
    # a uniform batch (the stamped path) with the bad format in its first packet: the same
    with pytest.raises(pl.PskSoftError) as e:
        h.plan_only(0, [dict(n_floats=2 * 3000, xdelta=0.01, format=bad)] * 4)
    assert e.value.status == 1
    assert _peek_all(h) == before
    # the host-buffer entry checks it too (a control-plane handle: no data is read)
    arr = (pl.Packet * 1)()
    out = (pl.Output * 1)()
    arr[0].n_floats, arr[0].sri_xdelta, arr[0].sri_mode, arr[0].present, arr[0].format = 64, 0.01, 1, 1, bad
    out[0].cap_symbols = 1 << 40
    assert pl.load().psk_soft_process_host(h._h, 0, 1, arr, out) == 1
    assert _peek_all(h) == before
    # both known formats go through, and an absent packet's format is not looked at
    h.plan_only(0, [dict(n_floats=2 * 3000, xdelta=0.01, format=f) for f in (0, 1, 0, 1)])
    arr[0].present, arr[0].format = 0, bad
    assert pl.load().psk_soft_process_device(h._h, 0, 1, arr, out, None) == 0
    h.close()


def test_packet_struct_layout_is_unchanged():
    """`format` took the place of the old `reserved` byte: same offsets, same size (ABI version 2)."""
    assert pl.Packet.format.offset == 31 and pl.Packet.format.size == 1
    assert ctypes.sizeof(pl.Packet) == 32
    assert pl.load().psk_soft_abi_version() == 2


def _routing_cfgs():
    # the table of test_control_plane.py::test_which_kernel_a_configuration_is_planned_for
    return [(S, A, n) for S in list(range(2, 35)) + [40, 64] for A in (1, 100, 128, 129, 256, 257, 512, 513, 1024, 1025)
            for n in (50,)] + [(8, 100, n) for n in (1, 384, 385, 1920, 1921, 4000, 32640, 32641)] + [(24, 300, 1000), (16, 1024, 1920)]


def test_cs16_packets_are_routed_like_float_packets():
    cfgs = _routing_cfgs()
    got = {}
    for fmt in (pl.FORMAT_CF32, pl.FORMAT_CS16):
        h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
        h.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
        res = []
        for k in range(2):
            res.append(h.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1, xdelta=0.01, sriChanged=(k == 0), format=fmt)
                                       for S, A, n in cfgs]))
        got[fmt] = (h.stats(), res, _peek_all(h))
        h.close()
    st_f, res_f, peek_f = got[pl.FORMAT_CF32]
    st_s, res_s, peek_s = got[pl.FORMAT_CS16]
    n_fast = sum(1 for S, A, n in cfgs if 2 <= S <= 1024 and n <= 32640)
    assert st_s["channels_fast"] == n_fast and st_s["channels_sequential"] == len(cfgs) - n_fast, st_s
    assert (st_s["channels_fast"], st_s["channels_sequential"]) == (st_f["channels_fast"], st_f["channels_sequential"])
    assert res_s == res_f and peek_s == peek_f
    # a batch that mixes the formats channel by channel plans the same too
    h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
    h.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
    for k in range(2):
        r = h.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1, xdelta=0.01, sriChanged=(k == 0), format=(i + k) % 2)
                            for i, (S, A, n) in enumerate(cfgs)])
        assert r == res_f[k]
    assert h.stats()["channels_fast"] == n_fast
    h.close()


def test_host_class_with_a_short_input_port_control_plane(oracle_mod):
    """A psk_soft variant with a dataShort_in port, on a control-plane-only handle: output counts, the three SRI pushes
    and their xdeltas, warnings -- packet by packet what the oracle does with the float cast of the same int16 data."""
    comp = sandbox.Component(device=pl.DEVICE_NONE, input="short")
    o = oracle_mod.OracleComponent()
    for name, v in (("samplesPerBaud", 8), ("constelationSize", 8), ("numAvg", 100)):
        setattr(comp, name, v)
        setattr(o, name, v)
    assert comp.service() == pl.NOOP
    rng = np.random.default_rng(3)
    sizes = [2 * 1000 * 8, 6, 2 * 333 + 1, 2 * 4096, 0, 2 * 17 * 8]
    n_soft = n_bits = 0
    sri = 0
    for i, n in enumerate(sizes):
        data = rng.integers(-3000, 3000, n).astype(np.int16)
        xd = 0.01 if i < 3 else 0.02
        comp.push(data, xdelta=xd, sriChanged=(i in (0, 3)), streamID="s%d" % i, EOS=(i == len(sizes) - 1))
        assert comp.service() == pl.NORMAL
        r = o.service(data.astype(np.float32), xd, sriChanged=(i in (0, 3)))
        n_soft += r.soft.size
        n_bits += r.bits.size
        sri += int(r.sri_pushed)
        log = comp.sri_log("softDecision_dataFloat_out")
        assert len(log) == sri
        if r.sri_pushed:
            assert log[-1] == (r.sri_soft_xdelta, 1)
            assert comp.sri_log("bits_dataShort_out")[-1] == (r.sri_bits_xdelta, 0)
            assert comp.sri_log("phase_dataFloat_out")[-1] == (r.sri_soft_xdelta, 0)
    assert comp.getData("softDecision_dataFloat_out").size == n_soft
    assert comp.getData("bits_dataShort_out").size == n_bits
    assert comp.getData("phase_dataFloat_out").size == n_soft // 2
    assert comp.getData("sampleIndex_dataShort_out").size == n_soft // 2
    assert comp.last_eos and comp.last_stream == "s%d" % (len(sizes) - 1)
    # real data: a warning, nothing pushed
    comp.push(np.zeros(64, np.int16), xdelta=0.01, complexData=False)
    assert comp.service() == pl.NORMAL and comp.warnings == 1
    with pytest.raises(TypeError):
        comp.push(np.zeros(64, np.float32), xdelta=0.01)
    comp.close()
