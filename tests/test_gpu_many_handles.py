"""Many handles in one process on a real MI355X, the shape a REDHAWK domain runs the library in: eight handles on device 0, created
up front, each with buffers and a non-blocking stream of its own, five calls each, chosen so that together they touch everything a
call can share with the call of another handle --

    H0  64 channels alike (samplesPerBaud 8, numAvg 100, QPSK), process_device: the stamped plan, wave-scan; an acquire_device
        look behind every call
    H1  48 channels of mixed window classes (samplesPerBaud 4 / 8 / 10, numAvg 25 / 100 / 400), PSK_SOFT_OPT_DEFERRED_JOIN, one
        psk_soft_join at the end: the side streams
    H2  2 channels, 2^15 samples a call at samplesPerBaud 4: time-tiled, parallel fit
    H3  16 cs16 columns of one frame-major matrix, process_device_tuned, PSK_SOFT_OPT_QUALITY: gather, tune and quality launches
    H4  8 channels, cs8 and cf16 packets through process_host: staging slots, the copy pool
    H5  4 channels, samplesPerBaud 10, numAvg 25, phaseAvg 20000 (max_phase_avg 32768), 1500 symbols a call  } two different
    H6  4 channels, samplesPerBaud 10, numAvg 100, phaseAvg 30000, the same otherwise                        } dynamic-LDS grants
        above 64 KiB on ONE wave-scan kernel: 4 x (y_len + samplesPerBaud x r_len) = 137232 and 140192 bytes
    H7  a sandbox.Component: the host class

Each handle first runs its script ALONE, on a fresh handle in the same process, traced (PSK_SOFT_TRACE_LAUNCHES=2): that run is
compared with the oracle on the handle's first and last channel, bit for bit, and is where reach is asserted.  Then the combined
runs -- interleaved from one thread; one thread per handle behind a barrier, and with a barrier in front of every call; the same
with H2 destroyed and created again while the others are in flight -- must give every handle, byte for byte, what it gave alone:
all four streams, every count and SRI field, the per-channel statistics, the quality and acquire records, the exported states.

Inside this process the runs alone come first, so by the time the threads of a combined run start, the record of every grant
(psk_fast_kernel.h: LdsGrant) already shows what H5 and H6 ask for: they take the lock, compare and return.  The test that has
two threads be the FIRST of a process to ask -- H5 for the smaller grant, H6 for the larger, a barrier in front of every call --
starts a child process for it, and compares with the runs alone that the child does afterwards.  Even that cannot force the two
threads between the compare and the update at the same instant."""
import contextlib
import ctypes
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from psk_soft_amd import lib as pl
from psk_soft_amd import sandbox
from psk_soft_amd.stimulus import synth_channel
from tests import host_script as hs
from tests import tune_model as tm
from tests.test_gpu_parity import assert_parity
from tests.thread_workers import WorkerStuck, run_workers

pytestmark = pytest.mark.gpu

K = 5  # calls per handle
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("soft", "bits", "phase", "index")
_LINE = re.compile(r"\[psk_soft\] ok; next: (?P<what>.+?) S=(?P<S>-?\d+) H=(?P<H>-?\d+) ch0=\d+ cnt=(?P<cnt>\d+) tiles=\d+ y_len=(?P<y_len>\d+) "
                   r"r_len=(?P<r_len>\d+) slot=-?\d+ stream=(?P<stream>\S+)")


@pytest.fixture(autouse=True)
def _two_host_threads(monkeypatch):
    monkeypatch.setenv("PSK_SOFT_HOST_THREADS", "2")  # (eight handles would otherwise start seven copy threads each)


def _al(n):
    return (n + 127) // 128 * 128


def _signals(base, props, n, sigma=0.01):
    return [synth_channel(base + c, p["constelationSize"], p["samplesPerBaud"], n, sigma=sigma) for c, p in enumerate(props)]


def _cs16(x):
    return np.rint(x.astype(np.float64) * 4000.0).clip(-32767, 32767).astype(np.int16)


def _cs8(x):
    return np.rint(x.astype(np.float64) * 40.0).clip(-127, 127).astype(np.int8)


def _fields(o):
    return (o.ret, o.n_symbols, o.n_bits, o.n_sampleIndex, o.sri_pushed, o.sri_soft_xdelta, o.sri_bits_xdelta, o.n_warn)


class DeviceRig:
    """a handle fed device-resident packets on a stream of its own.  data[k][c]: the packet of channel c in call k"""

    entry = "device"
    options = ()
    deferred = False
    looks = False
    limits = {}

    def __init__(self, name, props, data, device=0):
        self.name, self.props, self.data, self.device = name, props, data, device
        self.C = len(props)

    # -- what the oracle is fed for channel c in call k
    def model(self, k, c):
        return np.asarray(self.data[k][c]).astype(np.float32)

    def create(self):
        L = pl.load()
        self.h = h = pl.Handle(self.C, device=self.device, **self.limits)
        h.configure(0, self.props)
        for opt, val in self.options:
            h.set_option(opt, val)
        self.stream = ctypes.c_void_p()
        assert L.hipSetDevice(self.device) == 0 and L.hipStreamCreateWithFlags(ctypes.byref(self.stream), 1) == 0  # (non-blocking)
        self.lay, tot = {}, [0, 0, 0, 0, 0]
        for k in range(K):
            for c in range(self.C):
                cap = h.output_capacity(c, self.frames(k, c))
                self.lay[k, c] = (cap, tuple(tot))
                for i, s in enumerate((self.in_bytes(k, c), 8 * cap, 4 * cap, 6 * cap, 2 * cap)):
                    tot[i] += _al(s)
        self.tot = tot
        self.bufs = [h.device_alloc(max(t, 128)) for t in tot]
        self.upload_inputs()
        h.synchronize()
        self.outs = []
        return self

    def frames(self, k, c):
        return self.data[k][c].size // 2

    def in_bytes(self, k, c):
        return self.data[k][c].nbytes

    def upload_inputs(self):  # (one copy)
        host = np.zeros(max(self.tot[0], 128), np.uint8)
        for (k, c), (_, o) in self.lay.items():
            raw = np.frombuffer(np.ascontiguousarray(self.data[k][c]).tobytes(), np.uint8)
            host[o[0] : o[0] + raw.size] = raw
        self.h.upload(self.bufs[0], host)

    def packets(self, k):
        pk = (pl.Packet * self.C)()
        fmt = {np.dtype(np.float32): pl.FORMAT_CF32, np.dtype(np.int16): pl.FORMAT_CS16, np.dtype(np.int8): pl.FORMAT_CS8,
               np.dtype(np.float16): pl.FORMAT_CF16}
        for c in range(self.C):
            x = self.data[k][c]
            pk[c].data, pk[c].n_floats, pk[c].sri_xdelta, pk[c].sri_mode = self.bufs[0] + self.lay[k, c][1][0], x.size, 0.01, 1
            pk[c].sriChanged, pk[c].present, pk[c].format = int(k == 0), 1, fmt[x.dtype]
        return pk

    def outputs(self, k):
        out = (pl.Output * self.C)()
        d_in, d_soft, d_phase, d_bits, d_sidx = self.bufs
        for c in range(self.C):
            cap, o = self.lay[k, c]
            out[c].soft, out[c].phase, out[c].bits, out[c].sampleIndex = d_soft + o[1], d_phase + o[2], d_bits + o[3], d_sidx + o[4]
            out[c].cap_symbols = cap
        return out

    def call(self, k):
        """enqueue call k: no host wait"""
        pk, out = self.packets(k), self.outputs(k)
        self.process(k, pk, out)
        if self.looks:
            self.h.acquire_device(0, pk, None, None, self.stream.value)
        self.outs.append((pk, out))

    def process(self, k, pk, out):
        self.h.process_device(0, pk, out, self.stream.value)

    def finish(self, calls=K):
        h = self.h
        if self.deferred:
            h.join(self.stream.value)
        assert pl.load().hipStreamSynchronize(self.stream) == 0
        h.synchronize()
        soft, phase, bits, sidx = (h.download(b, (max(t, 128),), np.uint8) for b, t in zip(self.bufs[1:], self.tot[1:]))  # (one copy each)
        streams, fields = {}, []
        for k in range(calls):
            out = self.outs[k][1]
            fields.append([_fields(out[c]) for c in range(self.C)])
            for c in range(self.C):
                o, (cap, off) = out[c], self.lay[k, c]
                ns, nb, nx = int(o.n_symbols), int(o.n_bits), int(o.n_sampleIndex)
                assert ns <= cap and nb <= 3 * cap and nx <= cap
                streams[k, c] = dict(soft=soft[off[1] : off[1] + 8 * ns].view(np.float32), phase=phase[off[2] : off[2] + 4 * ns].view(np.float32),
                                     bits=bits[off[3] : off[3] + 2 * nb].view(np.int16), index=sidx[off[4] : off[4] + 2 * nx].view(np.int16))
        return dict(streams=streams, fields=fields, chstats=h.channel_stats(), quality=bytes(h.quality_records()),
                    acquire=bytes(h.acquire_records()) if self.looks else b"", state=[h.export_state(c) for c in range(self.C)])

    def destroy(self):
        if self.h._h is None:  # (gone already)
            return
        for b in self.bufs:
            self.h.device_free(b)
        self.h.close()
        assert pl.load().hipStreamDestroy(self.stream) == 0


class H0(DeviceRig):
    looks = True


class H1(DeviceRig):
    options = ((pl.Handle.OPT_DEFERRED_JOIN, 1),)
    deferred = True


class H2(DeviceRig):
    limits = dict(max_packet_complex=1 << 16)


class H3(DeviceRig):
    """sixteen cs16 columns of one frame-major matrix per call, every channel shifted by a tune of its own"""

    options = ((pl.Handle.OPT_QUALITY, 1),)
    WIDTH = 16

    def __init__(self, name, props, data, steps):
        DeviceRig.__init__(self, name, props, data)
        self.tunes = []
        phase = [(0x123456789ABCDEF * (c + 1)) & tm.MASK for c in range(self.C)]
        for k in range(K):
            self.tunes.append([(phase[c], steps[c]) for c in range(self.C)])
            phase = [tm.advance(phase[c], steps[c], data[k][c].size // 2) for c in range(self.C)]

    def model(self, k, c):
        return tm.apply(self.tunes[k][c][0], self.tunes[k][c][1], self.data[k][c])

    def in_bytes(self, k, c):  # (the matrix of call k lies at the place of its channel 0)
        return self.data[k][0].nbytes * self.WIDTH if c == 0 else 0

    def upload_inputs(self):
        host = np.zeros(max(self.tot[0], 128), np.uint8)
        for k in range(K):
            mat = np.stack([self.data[k][c].reshape(-1, 2) for c in range(self.C)], axis=1)  # [frames, width, 2]
            raw, o = np.frombuffer(np.ascontiguousarray(mat).tobytes(), np.uint8), self.lay[k, 0][1][0]
            host[o : o + raw.size] = raw
        self.h.upload(self.bufs[0], host)

    def process(self, k, pk, out):
        frames = self.data[k][0].size // 2
        pk2, strides = pl.frame_major_packets(self.bufs[0] + self.lay[k, 0][1][0], frames, self.WIDTH, 0, self.C, pl.FORMAT_CS16, 0.01, k == 0)
        for c in range(self.C):
            pk[c] = pk2[c]
        self.h.process_device_tuned(0, pk, strides, self.tunes[k], out, self.stream.value)


class H4:
    """cs8 and cf16 packets through process_host"""

    def __init__(self, name, props, data):
        self.name, self.props, self.data, self.C = name, props, data, len(props)

    def model(self, k, c):
        return np.asarray(self.data[k][c]).astype(np.float32)

    def create(self):
        self.h = pl.Handle(self.C, device=0)
        self.h.configure(0, self.props)
        self.res = []
        return self

    def call(self, k):
        self.res.append(self.h.process_host(0, [dict(data=self.data[k][c], xdelta=0.01, sriChanged=(k == 0)) for c in range(self.C)]))

    def finish(self, calls=K):
        h = self.h
        h.synchronize()
        streams = {(k, c): {key: self.res[k][c][key].copy() for key in KEYS} for k in range(calls) for c in range(self.C)}
        fields = [[tuple(self.res[k][c][f] for f in ("ret", "sri_pushed", "sri_soft_xdelta", "sri_bits_xdelta", "n_warn")) for c in range(self.C)]
                  for k in range(calls)]
        return dict(streams=streams, fields=fields, chstats=h.channel_stats(), quality=bytes(h.quality_records()), acquire=b"",
                    state=[h.export_state(c) for c in range(self.C)])

    def destroy(self):
        self.h.close()


class H7:
    """the host class: one component, a packet and a serviceFunction() per call"""

    C = 1

    def __init__(self, name, props, data):
        self.name, self.props, self.data = name, props, data

    def model(self, k, c):
        return self.data[k][0]

    def create(self):
        self.comp = sandbox.Component(device=0)
        for key in ("numAvg", "samplesPerBaud", "constelationSize", "phaseAvg"):
            setattr(self.comp, key, self.props[0][key])
        self.handle = self.comp.handle()
        self.res = []
        return self

    def call(self, k):
        comp = self.comp
        comp.push(self.data[k][0], xdelta=0.01, sriChanged=(k == 0))
        ret = comp.service()
        self.res.append((ret, {key: comp.getData(port) for key, port in zip(KEYS, hs.PORTS)}))

    def finish(self, calls=K):
        comp, h = self.comp, self.handle
        return dict(streams={(k, 0): self.res[k][1] for k in range(calls)},
                    fields=[[(self.res[k][0],)] for k in range(calls)] + [[tuple(comp.packets(p) for p in hs.PORTS), tuple(map(tuple, (comp.sri_log(p) for p in hs.PORTS))),
                                                                            comp.warnings, comp.resetState, comp.live_packets]],
                    chstats=h.channel_stats(), quality=bytes(h.quality_records()), acquire=b"", state=[h.export_state(0)])

    def destroy(self):
        self.comp.close()


def _cut(xs, n):
    """K packets of n complex samples from every signal: data[k][c]"""
    return [[x[2 * n * k : 2 * n * (k + 1)] for x in xs] for k in range(K)]


def _h0():
    p = [dict(samplesPerBaud=8, numAvg=100, constelationSize=4, phaseAvg=50)] * 64
    d = _cut(_signals(1000, p, K * 2000), 2000)
    return lambda: H0("H0", p, d)


def _h1():
    classes = [(4, 25), (8, 100), (10, 400)]
    p = [dict(samplesPerBaud=classes[c % 3][0], numAvg=classes[c % 3][1], constelationSize=(2, 4, 8)[(c // 3) % 3], phaseAvg=50) for c in range(48)]
    d = _cut(_signals(2000, p, K * 1500), 1500)
    return lambda: H1("H1", p, d)


def _h2():
    p = [dict(samplesPerBaud=4, numAvg=100, constelationSize=4, phaseAvg=50), dict(samplesPerBaud=4, numAvg=100, constelationSize=8, phaseAvg=200)]
    d = _cut(_signals(3000, p, K << 15), 1 << 15)
    return lambda: H2("H2", p, d)


def _h3():
    p = [dict(samplesPerBaud=8, numAvg=100, constelationSize=(2, 4, 8)[c % 3], phaseAvg=50) for c in range(16)]
    d = _cut([_cs16(x) for x in _signals(4000, p, K * 2000)], 2000)
    steps = [tm.step_word(1e-4 * (c - 7)) for c in range(16)]  # (channel 7: a constant rotation)
    return lambda: H3("H3", p, d, steps)


def _h4():
    p = [dict(samplesPerBaud=(4, 8)[c % 2], numAvg=100, constelationSize=(2, 4, 8)[c % 3], phaseAvg=50) for c in range(8)]
    x = _cut(_signals(5000, p, K * 2000), 2000)
    d = [[_cs8(v) if k % 2 == 0 else v.astype(np.float16) for v in x[k]] for k in range(K)]
    return lambda: H4("H4", p, d)


def _big_grant(name, numAvg, phaseAvg, base):
    """samplesPerBaud 10 keeps its energy ring in dynamic LDS beside the fit ring (psk_plan.h: ering_dynamic), so the grant of a
    wave-scan call is 4 x (y_len + 10 x r_len) bytes with r_len = (numAvg + 129) & ~1 and, above phaseAvg 16384, y_len = 32768: two
    values of numAvg under 128 are two sizes on one kernel, psk_fast_kernel<10,1,.>.  1500 symbols a call: wave-scan, not tiled."""
    def make():
        p = [dict(samplesPerBaud=10, numAvg=numAvg, constelationSize=(4, 8, 2, 4)[c], phaseAvg=phaseAvg) for c in range(4)]
        d = _cut(_signals(base, p, K * 15000), 15000)
        cls = type(name, (DeviceRig,), dict(limits=dict(max_phase_avg=32768)))
        return lambda device=0: cls(name, p, d, device)
    return make


def _h7():
    p = [dict(samplesPerBaud=8, numAvg=100, constelationSize=8, phaseAvg=50)]
    d = _cut(_signals(8000, p, K * 2000), 2000)
    return lambda: H7("H7", p, d)


_BUILD = dict(H0=_h0, H1=_h1, H2=_h2, H3=_h3, H4=_h4, H5=_big_grant("H5", 25, 20000, 6000), H6=_big_grant("H6", 100, 30000, 7000), H7=_h7)
_specs = {}


def spec(name):
    """the script of one handle, drawn once: a function that makes a fresh rig of it"""
    if name not in _specs:
        _specs[name] = _BUILD[name]()
    return _specs[name]


def specs():
    return {name: spec(name) for name in _BUILD}


@contextlib.contextmanager
def _traced(path):
    """handles created inside are traced (the variable is read at psk_soft_create), and file descriptor 2 goes to `path`"""
    sys.stderr.flush()
    saved, f = os.dup(2), os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    os.dup2(f, 2)
    os.close(f)
    os.environ["PSK_SOFT_TRACE_LAUNCHES"] = "2"
    try:
        yield
    finally:
        os.environ.pop("PSK_SOFT_TRACE_LAUNCHES", None)
        os.dup2(saved, 2)
        os.close(saved)


def _alone(make):
    rig = make().create()
    try:
        for k in range(K):
            rig.call(k)
        return rig.finish()
    finally:
        rig.destroy()


_solo = {}


@pytest.fixture
def solo(tmp_path):
    """every script alone on a fresh handle, traced: name -> (result, launch lines).  Computed once."""
    if not _solo:
        done = {}
        for name, make in specs().items():
            path = str(tmp_path / (name + ".trace"))
            with _traced(path):
                res = _alone(make)
            with open(path) as f:
                lines = [m.groupdict() for m in map(_LINE.search, f) if m]
            done[name] = (res, lines)
        _solo.update(done)  # (published whole: a run alone that raised leaves nothing half filled behind)
    return _solo


def _equal(got, ref, ctx):
    """byte for byte"""
    assert sorted(got["streams"]) == sorted(ref["streams"]), ctx
    for kc in ref["streams"]:
        for key in KEYS:
            a, b = got["streams"][kc][key], ref["streams"][kc][key]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %s of call %d channel %d differs from the run alone" % ((ctx, key) + kc)
    assert repr(got["fields"]) == repr(ref["fields"]), ctx + ": counts / SRI fields"
    assert got["chstats"] == ref["chstats"], ctx + ": per-channel statistics"
    assert got["quality"] == ref["quality"], ctx + ": quality records"
    assert got["acquire"] == ref["acquire"], ctx + ": acquire records"
    assert got["state"] == ref["state"], ctx + ": exported state"


def test_every_script_alone_reaches_what_it_is_for_and_matches_the_oracle(oracle_mod, solo):
    sp = specs()
    for name, (res, lines) in solo.items():
        rig = sp[name]()
        what = [ln["what"] for ln in lines]
        st = res["chstats"]
        print(name, sorted(set(what)), "streams", len({ln["stream"] for ln in lines}), "y_len", sorted({int(ln["y_len"]) for ln in lines}),
              {k: sum(s[k] for s in st) for k in st[0] if any(s[k] for s in st)})
        assert sum(res["streams"][k, c]["phase"].size for k in range(K) for c in range(rig.C)) > 500 * rig.C, name
        assert all(s["channels_sequential"] == 0 and s["channels_guard"] == 0 for s in st), name
        for c in sorted({0, rig.C - 1}):  # the oracle, on the first and the last channel
            o = oracle_mod.OracleComponent()
            for key, v in rig.props[c].items():
                setattr(o, key, v)
            for k in range(K):
                r = o.service(rig.model(k, c), 0.01, sriChanged=(k == 0))
                assert_parity(res["streams"][k, c], dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index), "%s alone, call %d channel %d" % (name, k, c))
    lines = {name: solo[name][1] for name in solo}
    stats = {name: solo[name][0]["chstats"] for name in solo}
    whats = {name: {ln["what"] for ln in lines[name]} for name in solo}
    # H0: every channel on the wave-scan kernels, one launch for all 64 (the stamped plan); the looks
    assert all(s["channels_fast"] == 1 and s["channels_tiled"] == 0 for s in stats["H0"])
    assert any(ln["what"].startswith("fast (") and int(ln["cnt"]) == 64 for ln in lines["H0"]) and "acquire_fold" in whats["H0"]
    assert len(solo["H0"][0]["acquire"]) == 64 * pl.load().psk_soft_acquire_bytes() and any(solo["H0"][0]["acquire"])
    # H1: three window classes, launches on more than one stream
    assert len({ln["S"] for ln in lines["H1"] if ln["what"].startswith("fast (")}) == 3
    assert len({ln["stream"] for ln in lines["H1"] if ln["what"].startswith("fast (")}) >= 2
    # H2: time-tiled, parallel fit
    assert all(s["channels_tiled"] == 1 and s["channels_parallel_fit"] == 1 for s in stats["H2"]) and "pfit" in whats["H2"]
    # H3: gather, tune and quality launches
    assert whats["H3"] & {"gather_tiles", "gather_singles"} and {"tune", "quality_fold", "quality_join"} <= whats["H3"]
    assert any(solo["H3"][0]["quality"])
    # H4, H7: the wave-scan kernels behind process_host
    assert all(s["channels_fast"] == 1 for s in stats["H4"] + stats["H7"])
    # H5 / H6: two different dynamic-LDS grants above 64 KiB on one wave-scan kernel, 4 x (y_len + samplesPerBaud x r_len) bytes
    grants, kernels = {}, {}
    for name in ("H5", "H6"):
        assert all(s["channels_fast"] == 1 and s["channels_tiled"] == 0 for s in stats[name]), name
        fast = [ln for ln in lines[name] if ln["what"] == "fast (screened tier)"]
        assert fast and {ln["S"] for ln in fast} == {"10"} and len({ln["H"] for ln in fast}) == 1, (name, fast[:2])
        kernels[name] = (fast[0]["S"], fast[0]["H"])
        grants[name] = {4 * (int(ln["y_len"]) + int(ln["S"]) * int(ln["r_len"])) for ln in fast}
        assert all(4 * int(ln["y_len"]) > 65536 for ln in fast), name
    print("grants", grants, kernels)
    assert kernels["H5"] == kernels["H6"]  # (one kernel: the same window class, the same history depth)
    assert grants == {"H5": {137232}, "H6": {140192}}, grants  # (both above 65536; H5's the smaller)


def _combined(solo, run):
    sp = specs()
    rigs = [sp[name]().create() for name in sp]  # all eight, up front
    stuck = False
    try:
        got = run(rigs)
        for rig in rigs:
            _equal(got[rig.name], solo[rig.name][0], rig.name)
    except WorkerStuck:
        stuck = True  # (a worker may still be inside the library: nothing it uses is destroyed)
        raise
    finally:
        if not stuck:
            for rig in rigs:
                rig.destroy()


def test_interleaved_from_one_thread(solo):
    """call k of every handle is enqueued before call k + 1 of any; no host wait until the end (process_host and the host class
    return their data: they wait for their own handle, for nobody else's)"""
    def run(rigs):
        for k in range(K):
            for rig in rigs:
                rig.call(k)
        return {rig.name: rig.finish() for rig in rigs}

    _combined(solo, run)


@pytest.mark.parametrize("every_call", [False, True], ids=["barrier_at_the_start", "barrier_at_every_call"])
def test_one_thread_per_handle(solo, every_call):
    def run(rigs):
        barrier, got = threading.Barrier(len(rigs)), {}

        def worker(rig):
            def go():
                barrier.wait(60)
                for k in range(K):
                    if every_call and k:
                        barrier.wait(60)
                    rig.call(k)
                got[rig.name] = rig.finish()
            return go

        run_workers([worker(rig) for rig in rigs])
        return got

    _combined(solo, run)


def test_a_handle_destroyed_and_created_again_while_the_others_are_in_flight(solo):
    """H2 stops after two calls, synchronises, destroys its handle, creates a new one and runs its whole script on that"""
    def run(rigs):
        barrier, got = threading.Barrier(len(rigs)), {}
        again = {}

        def worker(rig):
            def go():
                barrier.wait(60)
                if rig.name == "H2":
                    rig.call(0)
                    rig.call(1)
                    rig.finish(calls=2)
                    rig.destroy()
                    again["H2"] = new = spec("H2")().create()
                    for k in range(K):
                        new.call(k)
                    got["H2"] = new.finish()
                    return
                for k in range(K):
                    rig.call(k)
                got[rig.name] = rig.finish()
            return go

        try:
            run_workers([worker(rig) for rig in rigs])
        finally:
            if "H2" in again:  # (the first H2 is gone: the clean-up of _combined gets the second)
                rigs[[r.name for r in rigs].index("H2")] = again["H2"]
        return got

    _combined(solo, run)


def _first_grants_main():
    """(the child process of the test below) H5 and H6 from a thread each, before anything else in the process has asked for a
    grant; then each alone"""
    names = ("H5", "H6")
    rigs = [spec(name)().create() for name in names]
    barrier, got = threading.Barrier(len(rigs)), {}

    def worker(rig):
        def go():
            for k in range(K):
                barrier.wait(60)
                rig.call(k)
            got[rig.name] = rig.finish()
        return go

    run_workers([worker(rig) for rig in rigs])
    for rig in rigs:
        rig.destroy()
    for name in names:
        _equal(got[name], _alone(spec(name)), name)
    print("first grants ok", {name: sum(st["channels_fast"] for st in got[name]["chstats"]) for name in names})


def test_the_first_grants_of_a_process_asked_for_from_two_threads():
    """In this process every grant is on record once the runs alone are through.  A fresh process, where the two threads are the
    first to ask: H5 for 137232 bytes and H6 for 140192 on the same kernel, released together in front of every call -- and every
    byte as in the runs alone that follow in that process."""
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_many_handles import _first_grants_main; _first_grants_main()"], cwd=ROOT,
                       env=dict(os.environ, PSK_SOFT_HOST_THREADS="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first grants ok {'H5': 4, 'H6': 4}" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_two_devices(request):
    """H5 on device 0 and H6 on device 1, interleaved: skipped where one device is visible"""
    n = ctypes.c_int()
    assert pl.load().hipGetDeviceCount(ctypes.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device visible: the two-device case did not run")
    solo = request.getfixturevalue("solo")
    rigs = [spec("H5")(0).create(), spec("H6")(1).create()]
    try:
        for k in range(K):
            for rig in rigs:
                rig.call(k)
        for rig in rigs:
            _equal(rig.finish(), solo[rig.name][0], rig.name + " on device %d" % rig.device)
    finally:
        for rig in rigs:
            rig.destroy()
