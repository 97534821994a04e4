"""A script model of the host class (psk_soft_amd/host/psk_soft_gpu.h): what a REDHAWK domain does to one component -- property
sets through configure() (the listener fires on a change only), resetState, packets queued on the input port (complex or real,
inputQueueFlushed, sriChanged, an xdelta that changes, no elements, an odd element count), serviceFunction() calls on a full and
on an empty queue -- as a flat list of operations, a seeded draw of such lists, and one runner per side:

    OracleSide      the oracle's component (oracle/pyoracle.py: OracleComponent) behind a queue and four sinks of its own
    ComponentSide   psk_soft_amd.sandbox.Component, input "float", "short" or "char"

Both answer a "service" operation with the same record (ret, the data the four ports received in that call, the packet counts,
the three SRI logs, the warning count, resetState as the component reports it, ring_len / index / fit_len), and same() compares
two records value for value: counts and logs always, the data bit for bit (uint32 / int16 patterns, as assert_parity does) where
the component has a device.  tests/test_host_class_control.py runs it without a GPU, tests/test_gpu_host_class.py on one.

Operations:  ("set", name, value)   ("push", packet)   ("service",)
packet: dict(x float32 elements, complex, flushed, sriChanged, xdelta); a short port gets rint(4000 x) as int16, a char port
rint(40 x) as int8, and the oracle the float32 cast of what the port got."""
import math
import random
import re

import numpy as np

PORTS = ("softDecision_dataFloat_out", "bits_dataShort_out", "phase_dataFloat_out", "sampleIndex_dataShort_out")
KEYS = ("soft", "bits", "phase", "index")
WINDOW, PHASE_AVG = 65536, 4096  # the component's limits (psk_soft_gpu.h: the constructor's defaults)
DEFAULTS = dict(samplesPerBaud=10, numAvg=100, constelationSize=4, phaseAvg=50, differentialDecoding=0, resetState=0)
SEEDS = tuple(range(12))  # the committed seeds of the drawn scripts
# ... and the ones that run with data on a GPU, in packets of a few hundred to a few thousand samples: seeds whose script does not
# spend itself in the reference's stalled state (a window made smaller than what the deque holds never emits again)
# -- a condition of the draw that tests/test_host_class_control.py checks with the oracle
GPU_SEEDS, GPU_EVENTS, GPU_SIZES = (0, 2, 7, 9), 36, (300, 777, 1000, 2047, 2500, 4000)

KINDS = ("set_samplesPerBaud", "set_numAvg", "set_constelationSize", "set_phaseAvg", "set_differentialDecoding", "set_and_back",
         "window_class", "reset", "packet", "real", "flushed", "flushed_real", "reset_real", "sri_changed", "xdelta", "empty", "odd",
         "double", "noop")


def signal(nrng, S, M, n_complex, n_elems=None, noise=0.05, freq=3e-5):
    """n_complex samples of an M-PSK signal at S samples a symbol (rectangular pulses with a raised middle: a timing peak; a
    carrier offset; noise), interleaved float32 I/Q of n_elems elements (2 n_complex, or one more: an odd count)"""
    M = M if M in (2, 4, 8) else 4
    n_sym = n_complex // S + 2
    sym = np.exp(1j * (2 * np.pi * nrng.integers(0, M, n_sym) / M + np.pi / 4))
    k = np.arange(S)
    shape = 1.0 + 0.5 * np.exp(-(((k - S // 2)) / (0.15 * S + 0.5)) ** 2)
    x = (sym[:, None] * shape[None, :]).ravel()[:n_complex]
    x = x * np.exp(1j * freq * np.arange(x.size)) + noise * (nrng.standard_normal(x.size) + 1j * nrng.standard_normal(x.size))
    out = np.zeros(2 * n_complex if n_elems is None else n_elems, np.float32)
    out[0 : 2 * n_complex : 2], out[1 : 2 * n_complex : 2] = x.real, x.imag
    return out


def port_data(x, input):
    """the elements a port of type `input` is given for the float32 elements x"""
    if input == "short":
        return np.rint(np.asarray(x, np.float64) * 4000.0).clip(-32767, 32767).astype(np.int16)
    if input == "char":
        return np.rint(np.asarray(x, np.float64) * 40.0).clip(-127, 127).astype(np.int8)
    return np.ascontiguousarray(x, np.float32)


def packet(x, complex=True, flushed=False, sriChanged=False, xdelta=0.01):
    return dict(x=np.ascontiguousarray(x, np.float32), complex=bool(complex), flushed=bool(flushed), sriChanged=bool(sriChanged),
                xdelta=float(xdelta))


class Script:
    def __init__(self, ops, kinds=(), seed=None):
        self.ops, self.kinds, self.seed = list(ops), list(kinds), seed


def draw(seed, n_events=48, sizes=(1, 3, 7, 64, 100, 777, 1000, 2500), wide=True):
    """The script of a seed.  Every state the component passes through is inside its limits (window, phaseAvg), away from
    samplesPerBaud == 0 and phaseAvg == 0: a property set whose listener fires hands ALL properties to the library."""
    rng = random.Random(1000003 * seed + 17)
    nrng = np.random.default_rng(seed)
    cur = dict(DEFAULTS)
    S_choices = [1, 2, 3, 4, 5, 7, 8, 10, 16, 40] + ([2000] if wide else [])
    A_choices = [0, 1, 2, 5, 20, 100, 300]
    M_choices = [2, 4, 8, 16, 3, 1]
    n_choices = [1, 2, 5, 50, 200, 4096]
    xd_choices = [0.01, 1.0, 0.5, 1e-3]
    ops, kinds = [], []
    xd = [0.01]
    first = [True]

    def fits(S, A):
        return S * A <= WINDOW

    def push(n_complex=None, odd=False, **kw):
        n = rng.choice(sizes) if n_complex is None else n_complex
        x = signal(nrng, max(1, cur["samplesPerBaud"]), cur["constelationSize"], n, 2 * n + (1 if odd else 0))
        kw.setdefault("sriChanged", first[0] or rng.random() < 0.1)
        first[0] = False
        ops.append(("push", packet(x, xdelta=xd[0], **kw)))

    def set_(name, value):
        ops.append(("set", name, value))
        cur[name] = value

    weights = [("packet", 30), ("set_samplesPerBaud", 5), ("set_numAvg", 5), ("set_constelationSize", 5), ("set_phaseAvg", 5),
               ("set_differentialDecoding", 3), ("set_and_back", 3), ("window_class", 3), ("reset", 4), ("real", 4), ("flushed", 4),
               ("flushed_real", 3), ("reset_real", 3), ("sri_changed", 3), ("xdelta", 3), ("empty", 2), ("odd", 3), ("double", 3),
               ("noop", 3)]
    names = [k for k, _ in weights]
    for _ in range(n_events):
        kind = rng.choices(names, [w for _, w in weights])[0]
        if kind == "set_samplesPerBaud":
            ok = [S for S in S_choices if fits(S, cur["numAvg"])]
            set_("samplesPerBaud", rng.choice(ok))
        elif kind == "set_numAvg":
            ok = [A for A in A_choices if fits(cur["samplesPerBaud"], A)]
            set_("numAvg", rng.choice(ok))
        elif kind == "window_class":  # both: numAvg first (it has no listener), so that no pair handed over leaves the window
            S = rng.choice(S_choices)
            A = rng.choice([A for A in A_choices if fits(S, A)])
            set_("numAvg", A)  # (the component holds it until the listener of samplesPerBaud, or the next call, hands over the pair)
            set_("samplesPerBaud", S)
        elif kind == "set_constelationSize":
            set_("constelationSize", rng.choice(M_choices))
        elif kind == "set_phaseAvg":
            set_("phaseAvg", rng.choice(n_choices))
        elif kind == "set_differentialDecoding":
            set_("differentialDecoding", rng.choice([0, 1]))
        elif kind == "set_and_back":  # both listeners fire between two calls
            name = rng.choice(["samplesPerBaud", "constelationSize", "phaseAvg"])
            old = cur[name]
            other = {"samplesPerBaud": [s for s in (2, 8, 10) if fits(s, cur["numAvg"]) and s != old],
                     "constelationSize": [m for m in (2, 4, 8) if m != old], "phaseAvg": [n for n in (5, 50, 200) if n != old]}[name]
            set_(name, rng.choice(other))
            set_(name, old)
        elif kind == "reset":
            set_("resetState", 1)
        elif kind == "packet":
            push()
            ops.append(("service",))
        elif kind == "real":
            push(complex=False)
            ops.append(("service",))
        elif kind == "flushed":
            push(flushed=True)
            ops.append(("service",))
        elif kind == "flushed_real":  # the library is left holding the reset of the flush ...
            push(n_complex=32, complex=False, flushed=True)
            ops.append(("service",))
            push()  # ... which the next complex packet has to find
            ops.append(("service",))
        elif kind == "reset_real":  # the same for a reset of the user's
            set_("resetState", 1)
            push(n_complex=32, complex=False)
            ops.append(("service",))
            push()
            ops.append(("service",))
        elif kind == "sri_changed":
            push(sriChanged=True)
            ops.append(("service",))
        elif kind == "xdelta":
            xd[0] = rng.choice([v for v in xd_choices if v != xd[0]])
            push(sriChanged=rng.random() < 0.7)  # (a source announces a new rate; the reference also survives one that does not)
            ops.append(("service",))
        elif kind == "empty":
            push(n_complex=0)
            ops.append(("service",))
        elif kind == "odd":
            push(odd=True)
            ops.append(("service",))
        elif kind == "double":
            push()
            push()
            ops.append(("service",))
            ops.append(("service",))
        elif kind == "noop":
            ops.append(("service",))
        kinds.append(kind)
    return Script(ops, kinds, seed)


def facts(script):
    """What a script holds, from its operations alone: the services by what they took, and the two paths on which the parent
    host class lost a reset -- a real-data packet taken while resetState was up (set by the user: "reset_real", or by the
    packet's own flush: "flushed_real") with a complex packet serviced later."""
    queue, out = [], dict(noop=0, complex=0, real=0, flushed=0, empty=0, odd=0, queued_two=0, lost_user=0, lost_flush=0, sets=set())
    reset_up, pending = False, []
    for op in script.ops:
        if op[0] == "set":
            out["sets"].add(op[1])
            if op[1] == "resetState" and op[2]:
                reset_up = True
        elif op[0] == "push":
            queue.append(op[1])
            out["queued_two"] += len(queue) >= 2
        else:
            if not queue:
                out["noop"] += 1
                continue
            p = queue.pop(0)
            out["flushed"] += p["flushed"]
            out["empty"] += p["x"].size == 0
            out["odd"] += p["x"].size % 2
            if not p["complex"]:
                out["real"] += 1
                if p["flushed"]:
                    pending.append("lost_flush")
                if reset_up:
                    pending.append("lost_user")
            else:
                out["complex"] += 1
                for k in pending:
                    out[k] += 1
                pending, reset_up = [], False
    return out


LAUNCH = re.compile(r"\[psk_soft\] ok; next: (.+?) S=(-?\d+) H=")  # a launch line of PSK_SOFT_TRACE_LAUNCHES=2: name, S


def _same_value(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


class OracleSide:
    """The oracle's component with what the host class adds around the loop: the input queue, NOOP on an empty one, the three
    pushSRI calls (reference cpp/psk_soft.cpp:399-404), push-only-if-non-empty (:605-615)."""

    def __init__(self, po, input="float"):
        self.o = po.OracleComponent()
        self.input = input
        self.queue = []
        self.packets = [0, 0, 0, 0]
        self.sri = [[], [], [], []]
        self.warnings = 0

    def apply(self, op):
        if op[0] == "set":
            setattr(self.o, op[1], op[2])
            return None
        if op[0] == "push":
            self.queue.append(op[1])
            return None
        o = self.o
        data = {k: np.zeros(0, np.float32 if k in ("soft", "phase") else np.int16) for k in KEYS}
        ret = 0
        if self.queue:
            p = self.queue.pop(0)
            r = o.service(port_data(p["x"], self.input).astype(np.float32), p["xdelta"], mode=1 if p["complex"] else 0,
                          sriChanged=p["sriChanged"], inputQueueFlushed=p["flushed"])
            ret = r.ret
            data = dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index)
            self.warnings += r.n_warn
            if r.sri_pushed:
                self.sri[0].append((r.sri_soft_xdelta, 1))
                self.sri[2].append((r.sri_soft_xdelta, 0))
                self.sri[1].append((r.sri_bits_xdelta, 0))
            for i, k in enumerate(KEYS):
                self.packets[i] += data[k].size > 0
        return dict(ret=ret, data=data, packets=list(self.packets), sri=[list(s) for s in self.sri], warnings=self.warnings,
                    resetState=int(o.resetState), peek=dict(ring_len=o.ring_size, index=o.index, fit_len=int(o.fit_history().size)))


class ComponentSide:
    def __init__(self, comp, input="float", stats=False, trace=None):
        """stats: the record of a service holds the statistics of the component's handle; trace: a function that returns what the
        library has written to stderr since it was last called (a component created under PSK_SOFT_TRACE_LAUNCHES): the record
        holds the launch lines of the call"""
        self.comp, self.input, self.stats, self.trace = comp, input, stats, trace
        self.handle = comp.handle()

    def apply(self, op):
        comp = self.comp
        if op[0] == "set":
            setattr(comp, op[1], op[2])
            return None
        if op[0] == "push":
            p = op[1]
            comp.push(port_data(p["x"], self.input), xdelta=p["xdelta"], complexData=p["complex"], sriChanged=p["sriChanged"],
                      inputQueueFlushed=p["flushed"])
            return None
        if self.trace:
            self.trace()
        ret = comp.service()
        launches = self.trace() if self.trace else None
        rec = dict(ret=ret, data={k: comp.getData(port) for k, port in zip(KEYS, PORTS)}, packets=[comp.packets(port) for port in PORTS],
                   sri=[comp.sri_log(port) for port in PORTS], warnings=comp.warnings, resetState=int(comp.resetState),
                   peek=self.handle.peek(0))
        if self.stats:
            rec["stats"] = self.handle.channel_stats()[0]
        if launches is not None:
            rec["launches"] = LAUNCH.findall(launches)  # [(name, S)]
        return rec


def same(got, ref, ctx, data=True):
    """the record of the component against the oracle's; data=False (a component without a device): the sizes of the data only"""
    assert got["ret"] == ref["ret"], ctx
    for k in KEYS:
        assert got["data"][k].size == ref["data"][k].size, "%s: %s has %d elements, the oracle %d" % (ctx, k, got["data"][k].size, ref["data"][k].size)
    assert got["packets"] == ref["packets"], "%s: packets %s, the oracle %s" % (ctx, got["packets"], ref["packets"])
    for port, a, b in zip(PORTS, got["sri"], ref["sri"]):
        assert len(a) == len(b) and all(_same_value(x[0], y[0]) and x[1] == y[1] for x, y in zip(a, b)), "%s: SRI log of %s: %s, the oracle %s" % (
            ctx, port, a[-3:], b[-3:])
    assert got["warnings"] == ref["warnings"], "%s: warnings %d, the oracle %d" % (ctx, got["warnings"], ref["warnings"])
    assert got["resetState"] == ref["resetState"], "%s: resetState %d, the oracle %d" % (ctx, got["resetState"], ref["resetState"])
    assert got["peek"] == ref["peek"], "%s: %s, the oracle %s" % (ctx, got["peek"], ref["peek"])
    if data:  # as tests/test_gpu_parity.py: assert_parity -- every finite float by its uint32 pattern, the same non-finite pattern
        for k in KEYS:
            a, b = got["data"][k], ref["data"][k]
            if k in ("soft", "phase"):
                a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), "%s: non-finite pattern of %s differs" % (ctx, k)
                fin = np.isfinite(b)
                a, b = a.view(np.uint32)[fin], b.view(np.uint32)[fin]
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, "%s: %s differs in %d of %d elements, first at %d" % (ctx, k, bad.size, a.size, bad[0])


def run(script, got_side, ref_side, ctx="", data=True):
    """every operation on both sides; every service compared.  Returns the component's records."""
    records = []
    for i, op in enumerate(script.ops):
        g, r = got_side.apply(op), ref_side.apply(op)
        if op[0] == "service":
            same(g, r, "%s op %d (service %d)" % (ctx, i, len(records)), data)
            records.append(g)
    return records


# -- directed scripts ------------------------------------------------------------------------------------------------------------


def _base(nrng, S=8, A=100, n_sym=2000):
    return [("set", "samplesPerBaud", S), ("set", "numAvg", A), ("push", packet(signal(nrng, S, 4, n_sym * S), sriChanged=True)), ("service",)]


def flushed_real_packet():
    """2000 symbols at samplesPerBaud 8 / numAvg 100, a flushed real-data packet of 64 elements, 80 complex samples: the flush's
    reset is done at the complex packet (the fit history holds its 10 symbols, not the 50 it held before)"""
    nrng = np.random.default_rng(101)
    return Script(_base(nrng) + [("push", packet(np.zeros(64, np.float32), complex=False, flushed=True)), ("service",),
                                 ("push", packet(signal(nrng, 8, 4, 80))), ("service",),
                                 ("push", packet(signal(nrng, 8, 4, 1000))), ("service",)])


def reset_then_real_packet():
    nrng = np.random.default_rng(102)
    return Script(_base(nrng) + [("set", "resetState", 1), ("push", packet(np.zeros(64, np.float32), complex=False)), ("service",),
                                 ("push", packet(signal(nrng, 8, 4, 80))), ("service",),
                                 ("push", packet(signal(nrng, 8, 4, 1000))), ("service",)])


def reset_then_noop_services():
    nrng = np.random.default_rng(103)
    return Script(_base(nrng) + [("set", "resetState", 1), ("service",), ("service",), ("push", packet(signal(nrng, 8, 4, 80))), ("service",),
                                 ("push", packet(signal(nrng, 8, 4, 1000))), ("service",)])


def set_and_set_back():
    """every listened-to property set and set back between two calls: both listeners of each have fired"""
    nrng = np.random.default_rng(104)
    ops = _base(nrng)
    for name, other, old in (("samplesPerBaud", 10, 8), ("constelationSize", 8, 4), ("phaseAvg", 200, 50)):
        ops += [("set", name, other), ("set", name, old), ("push", packet(signal(nrng, 8, 4, 1500))), ("service",),
                ("push", packet(signal(nrng, 8, 4, 700))), ("service",)]
    return Script(ops)


DIRECTED = dict(flushed_real_packet=flushed_real_packet, reset_then_real_packet=reset_then_real_packet,
                reset_then_noop_services=reset_then_noop_services, set_and_set_back=set_and_set_back)
