"""Several handles in one process, each driven from a thread of its own (no GPU): the control plane of a handle is its own, so
eight control-plane-only handles that run scripts of tests/test_control_plane.py's kind side by side -- released together by a
barrier; ctypes lets go of the interpreter lock inside every call -- give, result for result and peek for peek, what the same
scripts give one after the other; and psk_soft_last_error is the calling thread's own."""
import random
import threading

import pytest

from psk_soft_amd import lib as pl
from tests.thread_workers import run_workers

N_HANDLES = 8


def _script(seed, calls=150):
    """property traffic and packets of one handle: [("set", {name: value}) | ("call", packet)]"""
    rng = random.Random(seed)
    ops, xdelta = [], 0.01
    for call in range(calls):
        for _ in range(rng.choice([0, 0, 0, 1, 2])):
            what = rng.choice(["samplesPerBaud", "numAvg", "constelationSize", "phaseAvg", "differentialDecoding", "resetState"])
            value = {"samplesPerBaud": [1, 2, 3, 4, 5, 8, 10, 16, 7], "numAvg": [0, 1, 2, 5, 20, 100], "constelationSize": [2, 4, 8, 16, 3, 1],
                     "phaseAvg": [1, 2, 5, 50, 200], "differentialDecoding": [0, 1], "resetState": [1]}[what]
            ops.append(("set", {what: rng.choice(value)}))
        if rng.random() < 0.2:
            xdelta = rng.choice([0.01, 1.0, 0.5, 1e-6])
        ops.append(("call", dict(n_floats=2 * rng.choice([0, 1, 3, 7, 64, 100, 777, 1000, 2500]) + (rng.random() < 0.1), xdelta=xdelta,
                                 mode=0 if rng.random() < 0.05 else 1, sriChanged=call == 0 or rng.random() < 0.1,
                                 inputQueueFlushed=rng.random() < 0.05)))
    return ops


def _play(h, ops, out):
    for op in ops:
        if op[0] == "set":
            h.configure(0, [op[1]])
        else:
            out.append((repr(h.plan_only(0, [op[1]])[0]), h.peek(0)))  # (repr: a NaN xdelta compares equal to itself)


def _handle():
    return pl.Handle(1, device=pl.DEVICE_NONE, max_window_samples=1 << 16, max_phase_avg=4096)


def test_eight_handles_from_eight_threads_equal_the_serial_run():
    scripts = [_script(100 + i) for i in range(N_HANDLES)]
    serial = []
    for ops in scripts:
        h, out = _handle(), []
        _play(h, ops, out)
        h.close()
        serial.append(out)
    assert all(len(out) == 150 for out in serial) and len({repr(out) for out in serial}) == N_HANDLES  # (eight different scripts)
    handles = [_handle() for _ in range(N_HANDLES)]
    got = [[] for _ in range(N_HANDLES)]
    barrier = threading.Barrier(N_HANDLES)

    def worker(i):
        def run():
            barrier.wait(60)
            _play(handles[i], scripts[i], got[i])
        return run

    run_workers([worker(i) for i in range(N_HANDLES)])
    for i in range(N_HANDLES):
        assert got[i] == serial[i], "handle %d: first difference at call %d" % (
            i, next(k for k in range(150) if k >= len(got[i]) or got[i][k] != serial[i][k]))
        handles[i].close()


def test_the_last_error_is_the_calling_threads_own():
    """two threads provoke different refusals at the same moment, many times over: each reads the text of its own"""
    a, b = _handle(), _handle()
    b.configure(0, [dict(samplesPerBaud=0)])
    barrier = threading.Barrier(2)
    rounds = 200
    seen = {"limit": [], "unsupported": []}

    def limit():
        for _ in range(rounds):
            barrier.wait(60)
            with pytest.raises(pl.PskSoftError) as e:
                a.configure(0, [dict(samplesPerBaud=8, numAvg=1 << 20)])
            seen["limit"].append((e.value.status, str(e.value), pl.load().psk_soft_last_error().decode()))

    def unsupported():
        for _ in range(rounds):
            barrier.wait(60)
            with pytest.raises(pl.PskSoftError) as e:
                b.plan_only(0, [dict(n_floats=16, xdelta=0.01)])
            seen["unsupported"].append((e.value.status, str(e.value), pl.load().psk_soft_last_error().decode()))

    run_workers([limit, unsupported])
    assert len(seen["limit"]) == len(seen["unsupported"]) == rounds
    assert {s for s, _, _ in seen["limit"]} == {4} and {s for s, _, _ in seen["unsupported"]} == {5}
    assert len({t for _, t, _ in seen["limit"]}) == 1 and len({t for _, t, _ in seen["unsupported"]}) == 1
    assert all("psk_soft_configure" in t and "psk_soft_configure" in last for _, t, last in seen["limit"])
    assert all("psk_soft_configure" not in t and "psk_soft_configure" not in last for _, t, last in seen["unsupported"])
    # (a thread that has had no refusal reads an empty text, not another thread's)
    fresh = []
    t = threading.Thread(target=lambda: fresh.append(pl.load().psk_soft_last_error()))
    t.start()
    t.join(60)
    assert fresh == [b""]
    a.close()
    b.close()
