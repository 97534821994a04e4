"""The host class (psk_soft_amd/host/psk_soft_gpu.h) on a real MI355X under the scripts of tests/host_script.py: everything
tests/test_host_class_control.py compares after every serviceFunction() call, and the data all four ports received in that call,
bit for bit (uint32 / int16 patterns) against the oracle fed the float32 cast of the packet -- for a float, a short and a char
input port.

The family scripts carry a one-channel component through every kernel family a single stream reaches, on fresh components and,
with property changes between the packets, on ONE component; each call that is named for a family asserts from the statistics of
the component's own handle (psk_soft_get_channel_stats) and from the names of the call's launches (PSK_SOFT_TRACE_LAUNCHES=2: the
statistics alone do not tell the three front stages of the time-tiled kernels apart) that the family did the work:

    wave_scan        a call under 2048 symbols of a window class with an instantiation
    tiled_pfit       one call of 2048 symbols or more: the time-tiled kernels with the parallel fit (the only packet above 4096)
    any_front        samplesPerBaud 40, no instantiation: the time-tiled kernels behind the run-time front stage
    wide             samplesPerBaud 2000 with numAvg 4: the wide front stage
    s1               samplesPerBaud 1, emitting: planned for the time-tiled kernels behind the run-time front stage
    reference_order  the reference-order kernel.  No plan sends a component inside its limits (phaseAvg <= 4096, packets far
                     below 2^20 symbols) there; a call reaches it at run time, handed over by the exactness guard -- here a NaN
                     sample in a samplesPerBaud 1 call, which only a float port can deliver."""
import numpy as np
import pytest

from psk_soft_amd import sandbox
from tests import host_script as hs

pytestmark = pytest.mark.gpu

INPUTS = ("float", "short", "char")

def _names(rec):
    return {name for name, _ in rec["launches"]}


def _front_S(rec, name):
    """samplesPerBaud on the lines of the front stage `name` (the wide one's name goes on: "wide_front (chunk, pick)")"""
    return {int(S) for what, S in rec["launches"] if what == name or what.startswith(name + " (")}


# what a call named for a family must show: the statistics of the handle, and the launches of the call by their names in the trace
# (psk_capi.cpp: "fast (screened tier)" / "fast (exact tier)" the wave-scan kernels, "tile_front" the front stage of a window class,
# "tile_front_any" the run-time front stage with the largest samplesPerBaud of its set, "wide_front" the wide one, "pfit" the
# parallel fit).  The reference-order kernel's launch line is written for every call, whatever it covers: the statistics tell.
REACHED = dict(
    wave_scan=lambda r: r["stats"]["channels_fast"] == 1 and r["stats"]["channels_tiled"] == 0 and r["stats"]["channels_sequential"] == 0
    and any(n.startswith("fast (") for n in _names(r)) and not any(n.startswith(("tile_", "wide_")) for n in _names(r)),
    tiled_pfit=lambda r: r["stats"]["channels_tiled"] == 1 and r["stats"]["channels_parallel_fit"] == 1 and r["stats"]["channels_sequential"] == 0
    and {"tile_front", "pfit", "tile_back"} <= _names(r),
    any_front=lambda r: r["stats"]["channels_fast"] == 1 and r["stats"]["channels_tiled"] == 1 and r["stats"]["channels_sequential"] == 0
    and _front_S(r, "tile_front_any") == {40} and not _front_S(r, "wide_front") and "tile_front" not in _names(r),
    wide=lambda r: r["stats"]["channels_fast"] == 1 and r["stats"]["channels_tiled"] == 1 and r["stats"]["channels_sequential"] == 0
    and _front_S(r, "wide_front") == {2000} and not _front_S(r, "tile_front_any"),
    s1=lambda r: r["stats"]["channels_fast"] == 1 and r["stats"]["channels_tiled"] == 1 and r["stats"]["channels_sequential"] == 0
    and _front_S(r, "tile_front_any") == {1} and not _front_S(r, "wide_front"),
    reference_order=lambda r: r["stats"]["channels_sequential"] == 1 and r["stats"]["channels_guard"] == 1 and r["stats"]["channels_fast"] == 0
    and "seq (reference order)" in _names(r),
)


@pytest.fixture(autouse=True)
def _two_host_threads(monkeypatch):
    monkeypatch.setenv("PSK_SOFT_HOST_THREADS", "2")  # (a handle would otherwise start seven copy threads)


class _Builder:
    """operations, and which service is named for which family"""

    def __init__(self, seed):
        self.nrng = np.random.default_rng(seed)
        self.ops, self.named, self.services = [], {}, 0
        self.S, self.M = 10, 4
        self.first = True

    def set(self, **kw):
        for k in ("numAvg", "samplesPerBaud", "constelationSize", "phaseAvg", "differentialDecoding", "resetState"):  # numAvg first
            if k in kw:
                self.ops.append(("set", k, kw[k]))
        self.S, self.M = kw.get("samplesPerBaud", self.S), kw.get("constelationSize", self.M)

    def call(self, n, family=None, odd=False, nan_at=None, noise=0.05, **kw):
        x = hs.signal(self.nrng, self.S, self.M, n, 2 * n + (1 if odd else 0), noise=noise)
        if nan_at is not None:
            x[2 * nan_at] = np.nan
        self.ops += [("push", hs.packet(x, sriChanged=self.first, **kw)), ("service",)]
        self.first = False
        if family:
            self.named[self.services] = family
        self.services += 1


def _wave_scan(b):
    b.set(samplesPerBaud=8, numAvg=100, constelationSize=4)
    b.call(3000, "wave_scan")
    b.call(1001, "wave_scan", odd=True)
    b.set(constelationSize=8, differentialDecoding=1)
    b.call(2000, "wave_scan")
    b.call(1500, "wave_scan", flushed=True)


def _tiled_pfit(b):
    b.set(samplesPerBaud=2, numAvg=20, constelationSize=4, phaseAvg=50)
    b.call(1000, "wave_scan", noise=0.02)
    b.call(4800, "tiled_pfit", noise=0.02)  # 2400 symbols in one call
    b.call(1500, "wave_scan", noise=0.02)


def _any_front(b):
    b.set(samplesPerBaud=40, numAvg=20, constelationSize=4, phaseAvg=20)
    b.call(4000, "any_front")
    b.call(4000, "any_front")
    b.call(3001, "any_front")


def _wide(b):
    b.set(numAvg=4, samplesPerBaud=2000, constelationSize=2, phaseAvg=20)
    b.call(4000)
    b.call(4000)
    for _ in range(5):
        b.call(4000, "wide")


def _s1(b):
    b.set(samplesPerBaud=1)  # (numAvg as it is: the window, trimmed to numAvg samples by the resync, is full, and every sample a symbol)
    b.call(600, "s1")
    b.call(400, "s1")


def _handed_over(b):
    """(a float port, at the end of a script) a NaN sample in a samplesPerBaud 1 call: the exactness guard hands the call to the
    reference-order kernel, and the next one too -- the NaN lives on in the fit"""
    b.set(samplesPerBaud=1)
    b.call(600, "reference_order", nan_at=300)
    b.call(400, "reference_order")


def _family_script(name, input):
    b = _Builder(sum(map(ord, name)))
    if name == "every_family_on_one_component":
        # (in the order of their windows, 40, 800, 800, 8000 samples: a window made smaller than what the deque holds stalls, as in
        # the reference; samplesPerBaud 1 emits from a full window, and the last window grows again from its 4 samples)
        _tiled_pfit(b)
        _wave_scan(b)
        _any_front(b)
        _wide(b)
        _s1(b)
        b.set(numAvg=100, samplesPerBaud=8, constelationSize=4, differentialDecoding=0, phaseAvg=50)
        b.call(3000, "wave_scan")
        b.call(2000, "wave_scan")
    elif name == "s1":
        b.set(samplesPerBaud=8, numAvg=50, constelationSize=4)
        b.call(3000, "wave_scan")
        _s1(b)
        b.set(samplesPerBaud=8)
        b.call(3000, "wave_scan")
    else:
        dict(wave_scan=_wave_scan, tiled_pfit=_tiled_pfit, any_front=_any_front, wide=_wide)[name](b)
    if input == "float" and name in ("s1", "every_family_on_one_component"):
        _handed_over(b)
    return hs.Script(b.ops), b.named


def _run(oracle_mod, script, input, ctx, trace=None):
    comp = sandbox.Component(device=0, input=input)
    try:
        records = hs.run(script, hs.ComponentSide(comp, input, stats=True, trace=trace), hs.OracleSide(oracle_mod, input), ctx, data=True)
        assert comp.live_packets == 0
        return records
    finally:
        comp.close()


@pytest.mark.parametrize("input", INPUTS)
@pytest.mark.parametrize("name", ["wave_scan", "tiled_pfit", "any_front", "wide", "s1", "every_family_on_one_component"])
def test_family_script(oracle_mod, capfd, monkeypatch, name, input):
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")  # (read when the component creates its handle)
    script, named = _family_script(name, input)
    assert all(op[1]["x"].size // 2 <= 4096 or named.get(i) == "tiled_pfit" for i, op in enumerate(o for o in script.ops if o[0] == "push"))
    records = _run(oracle_mod, script, input, "%s %s" % (name, input), trace=lambda: capfd.readouterr().err)
    reached = set()
    for k, family in sorted(named.items()):
        rec = records[k]
        n = rec["data"]["phase"].size
        print("%s %s service %d %s: %d symbols %s %s" % (name, input, k, family, n, {a: b for a, b in rec["stats"].items() if b}, rec["launches"]))
        assert n > 0, "service %d (%s) emitted nothing" % (k, family)
        assert (n >= 2048) == (family == "tiled_pfit"), (k, family, n)
        assert REACHED[family](rec), "service %d did not reach %s: %s %s" % (k, family, rec["stats"], rec["launches"])
        reached.add(family)
    want = {"every_family_on_one_component": {"wave_scan", "tiled_pfit", "any_front", "wide", "s1"}, "s1": {"wave_scan", "s1"},
            "tiled_pfit": {"wave_scan", "tiled_pfit"}}.get(name, {name})
    if input == "float" and name in ("s1", "every_family_on_one_component"):
        want = want | {"reference_order"}
    assert reached == want


@pytest.mark.parametrize("input", INPUTS)
@pytest.mark.parametrize("name", sorted(hs.DIRECTED))
def test_directed_script(oracle_mod, name, input):
    records = _run(oracle_mod, hs.DIRECTED[name](), input, "%s %s" % (name, input))
    assert sum(r["data"]["phase"].size for r in records) > 1900


@pytest.mark.parametrize("input", INPUTS)
@pytest.mark.parametrize("seed", hs.GPU_SEEDS)
def test_drawn_script(oracle_mod, seed, input):
    script = hs.draw(seed, hs.GPU_EVENTS, hs.GPU_SIZES)
    records = _run(oracle_mod, script, input, "seed %d %s" % (seed, input))
    assert sum(r["data"]["phase"].size for r in records) > 1000, "the script emits"
