"""Complex int8 packets (PSK_SOFT_FORMAT_CS8 = 3) on the control plane, without a GPU: format 3 is accepted on the per-channel and
the stamped path and planned exactly like float packets of the same element count, in batches that mix all three formats too,
and the C++ host class with a char input port counts and pushes what the oracle does on the float cast of the same packets."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from psk_soft_amd import sandbox


def _peek_all(h):
    return [h.peek(c) for c in range(h.n_channels)]


def _routing_cfgs():
    # the table of test_cs16_control.py (test_control_plane.py::test_which_kernel_a_configuration_is_planned_for)
    return [(S, A, n) for S in list(range(2, 35)) + [40, 64] for A in (1, 100, 128, 129, 256, 257, 512, 513, 1024, 1025)
            for n in (50,)] + [(8, 100, n) for n in (1, 384, 385, 1920, 1921, 4000, 32640, 32641)] + [(24, 300, 1000), (16, 1024, 1920)]


def test_format_constants():
    assert (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8) == (0, 1, 3)


def test_cs8_packets_are_routed_like_float_packets():
    cfgs = _routing_cfgs()
    got = {}
    for fmt in (pl.FORMAT_CF32, pl.FORMAT_CS8):
        h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
        h.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
        res = []
        for k in range(2):
            res.append(h.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1, xdelta=0.01, sriChanged=(k == 0), format=fmt)
                                       for S, A, n in cfgs]))
        got[fmt] = (h.stats(), res, _peek_all(h))
        h.close()
    st_f, res_f, peek_f = got[pl.FORMAT_CF32]
    st_c, res_c, peek_c = got[pl.FORMAT_CS8]
    n_fast = sum(1 for S, A, n in cfgs if 2 <= S <= 1024 and n <= 32640)
    assert st_c["channels_fast"] == n_fast and st_c["channels_sequential"] == len(cfgs) - n_fast, st_c
    assert (st_c["channels_fast"], st_c["channels_sequential"]) == (st_f["channels_fast"], st_f["channels_sequential"])
    assert res_c == res_f and peek_c == peek_f


def test_a_batch_mixing_the_three_formats_is_planned_like_float():
    cfgs = _routing_cfgs()
    fmts = (pl.FORMAT_CF32, pl.FORMAT_CS16, pl.FORMAT_CS8)
    ref = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
    h = pl.Handle(len(cfgs), device=pl.DEVICE_NONE, max_window_samples=64 * 1025 + 64, max_phase_avg=40000)
    for x in (ref, h):
        x.configure(0, [dict(samplesPerBaud=S, numAvg=A, phaseAvg=n) for S, A, n in cfgs])
    for k in range(3):
        r_f = ref.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1 + k, xdelta=0.01, sriChanged=(k == 0)) for S, A, n in cfgs])
        r_m = h.plan_only(0, [dict(n_floats=2 * S * (A + 300) + 1 + k, xdelta=0.01, sriChanged=(k == 0), format=fmts[(i + k) % 3])
                              for i, (S, A, n) in enumerate(cfgs)])
        assert r_m == r_f
    assert _peek_all(h) == _peek_all(ref)
    assert h.stats()["channels_fast"] == ref.stats()["channels_fast"]
    h.close()
    ref.close()


@pytest.mark.parametrize("n_ch", [16, 64])
def test_stamped_batches_of_cs8_packets(n_ch):
    """Uniform batches (the stamped path: 16 channels or more with equal packets) of format 3, then batches that switch
    between the formats call by call and a batch whose packets differ only in their format: every result and every
    channel's state as the float batch gives them."""
    fmts = [pl.FORMAT_CS8, pl.FORMAT_CS8, pl.FORMAT_CS16, pl.FORMAT_CF32, pl.FORMAT_CS8]
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
    # stay the float plans
    n = 2 * 8 * 1500
    r_f = ref.plan_only(0, [dict(n_floats=n, xdelta=0.01)] * n_ch)
    pk = [dict(n_floats=n, xdelta=0.01, format=pl.FORMAT_CS8)] * n_ch
    pk[n_ch // 2] = dict(pk[n_ch // 2], format=pl.FORMAT_CS16)
    pk[n_ch - 1] = dict(pk[n_ch - 1], format=pl.FORMAT_CF32)
    assert h.plan_only(0, pk) == r_f
    assert _peek_all(h) == _peek_all(ref)
    st = h.stats()
    assert st["channels_fast"] == ref.stats()["channels_fast"] and st["channels_sequential"] == 0
    h.close()
    ref.close()


def test_format_2_stays_refused_next_to_format_3():
    h = pl.Handle(4, device=pl.DEVICE_NONE)
    h.configure_all(samplesPerBaud=8, constelationSize=4, numAvg=100)
    h.plan_only(0, [dict(n_floats=2 * 1000, xdelta=0.01, sriChanged=True, format=pl.FORMAT_CS8)] * 4)
    before = _peek_all(h)
    pk = [dict(n_floats=2 * 3000, xdelta=0.01, format=pl.FORMAT_CS8)] * 4
    pk[1] = dict(pk[1], format=2)
    with pytest.raises(pl.PskSoftError) as e:
        h.plan_only(0, pk)
    assert e.value.status == 1 and "format 2" in str(e.value) and "CS8 = 3" in str(e.value)
    assert _peek_all(h) == before
    h.close()


def test_host_class_with_a_char_input_port_control_plane(oracle_mod):
    """A psk_soft variant with a dataChar_in port (the port's buffer typed as plain char), on a control-plane-only handle:
    output counts, the three SRI pushes and their xdeltas, warnings -- packet by packet what the oracle does with the float
    cast of the same int8 data."""
    comp = sandbox.Component(device=pl.DEVICE_NONE, input="char")
    o = oracle_mod.OracleComponent()
    for name, v in (("samplesPerBaud", 8), ("constelationSize", 8), ("numAvg", 100)):
        setattr(comp, name, v)
        setattr(o, name, v)
    assert comp.service() == pl.NOOP
    rng = np.random.default_rng(5)
    sizes = [2 * 1000 * 8, 6, 2 * 333 + 1, 2 * 4096, 0, 2 * 17 * 8]
    n_soft = n_bits = 0
    sri = 0
    for i, n in enumerate(sizes):
        data = rng.integers(-128, 128, n).astype(np.int8)
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
    comp.push(np.zeros(64, np.int8), xdelta=0.01, complexData=False)
    assert comp.service() == pl.NORMAL and comp.warnings == 1
    for bad in (np.zeros(64, np.int16), np.zeros(64, np.float32), np.zeros(64, np.uint8)):
        with pytest.raises(TypeError):
            comp.push(bad, xdelta=0.01)
    comp.close()
