"""The host class (psk_soft_amd/host/psk_soft_gpu.h) under the traffic of a REDHAWK domain, without a GPU: a control-plane-only
component (PSK_SOFT_DEVICE_NONE) of each input type and the oracle run the scripts of tests/host_script.py side by side, and after
EVERY serviceFunction() call the return value, the sizes of what the four ports received and their packet counts
(push-only-if-non-empty), the three SRI logs value for value, the warning count, resetState as the component reports it and
psk_soft_peek of the component's own handle (ring_len, index, fit_len) are the oracle's.

The directed scripts are the ways in which the host class once differed from the C ABI under it: it cleared resetState after
every call and handed the cleared value back with the next call's properties, so that a reset the library still held -- behind a
flushed real-data packet, or a resetState set in front of a real-data packet -- was wiped, where the reference does the three
resets at the next complex packet (cpp/psk_soft.cpp:353-372); and it leaked the packet when the properties were refused."""
import numpy as np
import pytest

from psk_soft_amd import lib as pl
from psk_soft_amd import sandbox
from tests import host_script as hs

INPUTS = ("float", "short", "char")


def _pair(oracle_mod, input):
    comp = sandbox.Component(device=pl.DEVICE_NONE, input=input)
    return comp, hs.ComponentSide(comp, input), hs.OracleSide(oracle_mod, input)


@pytest.mark.parametrize("input", INPUTS)
@pytest.mark.parametrize("seed", hs.SEEDS)
def test_drawn_scripts(oracle_mod, seed, input):
    comp, got, ref = _pair(oracle_mod, input)
    records = hs.run(hs.draw(seed), got, ref, "seed %d %s" % (seed, input), data=False)
    assert records and comp.live_packets == 0
    comp.close()


@pytest.mark.parametrize("input", INPUTS)
@pytest.mark.parametrize("name", sorted(hs.DIRECTED))
def test_directed_script(oracle_mod, name, input):
    comp, got, ref = _pair(oracle_mod, input)
    records = hs.run(hs.DIRECTED[name](), got, ref, "%s %s" % (name, input), data=False)
    assert comp.live_packets == 0
    if name in ("flushed_real_packet", "reset_then_real_packet"):
        # the numbers of the reproduction: 50 fit points before, the real-data packet leaves the reset standing, the 80 complex
        # samples behind it emit 10 symbols into a CLEARED history
        assert [r["peek"]["fit_len"] for r in records[:3]] == [50, 50, 10]
        assert [r["resetState"] for r in records[:3]] == [0, 1, 0]
    if name == "reset_then_noop_services":
        assert [(r["ret"], r["resetState"]) for r in records[1:4]] == [(pl.NOOP, 1), (pl.NOOP, 1), (pl.NORMAL, 0)]
        assert records[3]["peek"]["fit_len"] == 10
    comp.close()


@pytest.mark.parametrize("input", INPUTS)
def test_refused_properties_leave_no_packet_behind(oracle_mod, input):
    """numAvg has no listener: raised past the window between two calls it reaches the library with the next call's properties,
    which the library refuses (PSK_SOFT_ERR_LIMIT).  service() raises, the packet it took is deleted, nothing of the component
    or the library has changed, and with numAvg set back the component goes on where the oracle -- which has seen neither the
    refused value nor the dropped packet -- stands."""
    nrng = np.random.default_rng(7)
    comp, got, ref = _pair(oracle_mod, input)
    head = hs.Script([("set", "samplesPerBaud", 8), ("push", hs.packet(hs.signal(nrng, 8, 4, 3000), sriChanged=True)), ("service",)])
    hs.run(head, got, ref, "head", data=False)
    before = got.handle.peek(0)
    comp.numAvg = 65536 // 8 + 1
    got.apply(("push", hs.packet(hs.signal(nrng, 8, 4, 500))))
    assert comp.live_packets == 1
    with pytest.raises(RuntimeError) as e:
        comp.service()
    assert "psk_soft_configure" in str(e.value) and "limits" in str(e.value)
    assert comp.live_packets == 0
    assert got.handle.peek(0) == before and comp.packets(hs.PORTS[0]) == 1
    comp.numAvg = 100
    tail = hs.Script([("push", hs.packet(hs.signal(nrng, 8, 4, 1000))), ("service",), ("set", "phaseAvg", 20),
                      ("push", hs.packet(hs.signal(nrng, 8, 4, 777), flushed=True)), ("service",), ("service",)])
    records = hs.run(tail, got, ref, "tail", data=False)
    assert [r["ret"] for r in records] == [pl.NORMAL, pl.NORMAL, pl.NOOP] and comp.live_packets == 0
    comp.close()


def test_the_draws_hold_what_the_tests_are_named_for():
    """conditions of the draw, from the operations alone: over the committed seeds every kind of event occurs, and each of the two
    paths on which a reset was lost occurs with a complex packet behind it"""
    kinds, total = set(), {}
    for seed in hs.SEEDS:
        sc = hs.draw(seed)
        kinds |= set(sc.kinds)
        f = hs.facts(sc)
        for k, v in f.items():
            total[k] = (total.get(k, set()) | v) if isinstance(v, set) else total.get(k, 0) + v
        cur = dict(hs.DEFAULTS)
        for op in sc.ops:  # the limits, at every pair the component can hand to the library
            if op[0] == "set":
                cur[op[1]] = op[2]
                if op[1] != "numAvg":
                    assert cur["samplesPerBaud"] * cur["numAvg"] <= hs.WINDOW, (seed, cur)
            elif op[0] == "service":
                assert cur["samplesPerBaud"] * cur["numAvg"] <= hs.WINDOW, (seed, cur)
            assert 1 <= cur["samplesPerBaud"] and 1 <= cur["phaseAvg"] <= hs.PHASE_AVG
            if op[0] == "push":
                assert op[1]["x"].size <= 2 * 4096 + 1
    assert kinds == set(hs.KINDS), set(hs.KINDS) - kinds
    assert total["sets"] == set(hs.DEFAULTS)
    for k in ("noop", "complex", "real", "flushed", "empty", "odd", "queued_two"):
        assert total[k] > 0, k
    assert total["lost_flush"] >= 3 and total["lost_user"] >= 3, total
    for name in ("flushed_real_packet", "reset_then_real_packet"):
        f = hs.facts(hs.DIRECTED[name]())
        assert f["lost_flush" if name == "flushed_real_packet" else "lost_user"] == 1 and f["complex"] == 3


@pytest.mark.parametrize("seed", hs.GPU_SEEDS)
def test_the_scripts_that_run_with_data_emit(oracle_mod, seed):
    """by the oracle alone: more than 1000 symbols, in eight calls or more"""
    ref = hs.OracleSide(oracle_mod)
    recs = [r for r in map(ref.apply, hs.draw(seed, hs.GPU_EVENTS, hs.GPU_SIZES).ops) if r is not None]
    emitted = [r["data"]["phase"].size for r in recs if r["data"]["phase"].size]
    assert len(emitted) >= 8 and sum(emitted) > 1000, emitted


def test_the_draw_of_a_seed_is_the_same_every_time():
    a, b = hs.draw(5), hs.draw(5)
    assert a.kinds == b.kinds and len(a.ops) == len(b.ops)
    for x, y in zip(a.ops, b.ops):
        if x[0] == "push":
            assert np.array_equal(x[1]["x"].view(np.uint32), y[1]["x"].view(np.uint32)) and {k: v for k, v in x[1].items() if k != "x"} == {
                k: v for k, v in y[1].items() if k != "x"}
        else:
            assert x == y
