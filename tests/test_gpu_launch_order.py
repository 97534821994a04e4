"""The schedule of a call, pinned launch by launch: for every case below two consecutive calls on a fresh handle under
PSK_SOFT_TRACE_LAUNCHES=1 and PSK_SOFT_VALIDATE=1, the whole trace -- every launch line and every channel line behind it --
compared with the one recorded in test_gpu_launch_order.json.

The recorded traces come from `python -m tests.test_gpu_launch_order --record [--commit HASH] [--out FILE]` run on a build of
the commit BEFORE a change to the routing of a call (psk_capi.cpp: process_round), never on the code under test; the file names
that commit.  The test itself never writes the file.

A launch line is compared on what, S, H, cnt, tiles, y_len, r_len and slot, its stream pointer replaced by the order of first
appearance within the case; a channel line on every field but in= (K, tbase and toff included).  The packets are random
values of the right length: the trace is a matter of the control plane alone, and the parity of these paths is checked
elsewhere."""

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_launch_order.json")
_LAUNCH = re.compile(r"\[psk_soft\] ok; next: (?P<what>.+?) S=(?P<S>-?\d+) H=(?P<H>-?\d+) ch0=\d+ cnt=(?P<cnt>\d+) tiles=(?P<tiles>\d+) "
                     r"y_len=(?P<y_len>\d+) r_len=(?P<r_len>\d+) slot=(?P<slot>\d+) stream=(?P<stream>\S+)")
_CHANNEL = re.compile(r"\[psk_soft\]   (?P<fields>ch \d+ .*?) in=\S+")
_LAUNCH_KEYS = ("S", "H", "cnt", "tiles", "y_len", "r_len", "slot")
OPT_TIME_TILED, OPT_DEFERRED_JOIN, OPT_FAR_FIT = 3, 5, 7


def first_call(S, A, n_sym):
    """complex samples of a first call that emits n_sym symbols (the window fills first)"""
    return (n_sym + A - 1) * S


def _chan(S, A, n_sym, phaseAvg=50, M=4, dtype=np.float32, second=None):
    """one channel: its properties, the lengths of its two calls in complex samples, the element type of its packets"""
    return dict(props=dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=phaseAvg),
                lens=(first_call(S, A, n_sym), n_sym * S if second is None else second), dtype=dtype)


def _two_classes():
    # (two window classes, H=1 and H=4, and a channel fed half a symbol a call: it never emits)
    quiet = dict(props=dict(samplesPerBaud=8, constelationSize=4, numAvg=25, phaseAvg=50), lens=(4, 4), dtype=np.float32)
    return [_chan(8, 25, 600 + c) for c in range(3)] + [_chan(4, 400, 610 + c) for c in range(3)] + [quiet]


# name -> environment, limits of the handle, options, channels, configured alike in one go (the stamped path)
CASES = {
    "01_two_classes_and_a_quiet_channel": dict(chans=_two_classes()),
    "02_deferred_join": dict(chans=_two_classes(), options={OPT_DEFERRED_JOIN: 1}),
    "03_automatic_tiling": dict(chans=[_chan(8, 100, 2304), _chan(8, 100, 2304)]),
    "04_pipelined_ranges": dict(chans=[_chan(8, 100, 2304), _chan(8, 100, 2304)], env=dict(PSK_SOFT_PIPELINED=2)),
    "05_any_set": dict(chans=[_chan(40, 25, 600), _chan(40, 25, 603)]),
    "06_wide_set": dict(chans=[_chan(2048, 3, 300, phaseAvg=20)]),
    # (the third channel gets three samples in its second call: nothing emitted, the far window holds values)
    "07_far_fit": dict(chans=[_chan(8, 10, 600, phaseAvg=40000), _chan(2048, 3, 200, phaseAvg=40000), _chan(8, 10, 600, phaseAvg=40000, second=3)],
                       limits=dict(max_phase_avg=65535), options={OPT_FAR_FIT: 1}),
    "08_in_place_classes": dict(chans=[_chan(8, 25, 300, dtype=np.int16), _chan(8, 25, 301, dtype=np.int8), _chan(8, 25, 302, dtype=np.float16)]),
    "09_cs16_moved_back": dict(chans=[_chan(8, 100, 2304, dtype=np.int16), _chan(8, 100, 2304, dtype=np.int16)]),
    "10_stamped": dict(chans=[_chan(8, 100, 600)] * 16, uniform=True),
    "11_stamped_and_moved_back": dict(chans=[_chan(8, 100, 600, dtype=np.int16)] * 16, uniform=True, options={OPT_TIME_TILED: 2}),
    # (one case more than the eleven the schedule was pinned for: the pre-passes of the other two formats, CS8 and CF16 at a
    # numAvg without in-place kernels, so that every launch name of a call is in the file)
    "12_cs8_cf16_pre_pass": dict(chans=[_chan(4, 400, 300, dtype=np.int8), _chan(4, 400, 301, dtype=np.float16)]),
}
# every launch name of a call, but for the two that other trace tests cover: the pieces of a batch cut in time (the same names
# in more rounds) and "seq_wide" without the tiled scratch
WHATS = {
    "cs16_convert", "cs8_convert", "cf16_convert", "fast<0,1> (calls that emit nothing)", "tile_front_any", "pfit (any)", "tile_fit (any)",
    "tile_back (any)", "wide_front (chunk, pick)", "pfit (wide)", "tile_fit (wide)", "tile_back (wide)", "far_quiet (calls that emit nothing)",
    "tile_front_any (far)", "far_fit (any)", "tile_back (any, far)", "wide_front (chunk, pick; far)", "far_fit (wide)", "tile_back (wide, far)",
    "pipe_front", "pipe_fit", "pipe_back", "tile_front", "pfit", "tile_fit", "tile_back", "fast (screened tier)", "fast (exact tier)",
    "seq (reference order)", "seq_wide (reference order, samplesPerBaud > 1024)",
}


class _Stderr:
    """file descriptor 2 into a file while the library writes its trace (it writes with fprintf, past sys.stderr)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def text(self):
        self.tmp.seek(0)
        return self.tmp.read().decode("utf-8", "replace")

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.out = self.text()
        self.tmp.close()


def normalise(text, streams):
    """the trace of one call as a list of strings: 'what|S|H|cnt|tiles|y_len|r_len|slot|stream number' per launch, the channel
    lines behind it without their in= field"""
    out = []
    for line in text.splitlines():
        m = _LAUNCH.search(line)
        if m:
            n = streams.setdefault(m["stream"], len(streams))
            out.append("|".join([m["what"]] + [m[k] for k in _LAUNCH_KEYS] + [str(n)]))
            continue
        m = _CHANNEL.search(line)
        if m:
            out.append("  " + m["fields"])
    return out


def _packet_data(rng, dtype, n_complex):
    if dtype == np.int16:
        return rng.integers(-20000, 20000, 2 * n_complex).astype(np.int16)
    if dtype == np.int8:
        return rng.integers(-100, 100, 2 * n_complex).astype(np.int8)
    return rng.standard_normal(2 * n_complex).astype(dtype)


def run_case(name):
    """the normalised traces of the case's two calls"""
    from psk_soft_amd import lib as pl

    case = CASES[name]
    chans = case["chans"]
    C = len(chans)
    fmt = {np.int16: pl.FORMAT_CS16, np.int8: pl.FORMAT_CS8, np.float16: pl.FORMAT_CF16}
    env = dict(case.get("env", {}), PSK_SOFT_TRACE_LAUNCHES=1, PSK_SOFT_VALIDATE=1)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    h, bufs = None, []
    try:
        h = pl.Handle(C, device=0, **case.get("limits", {}))
        for opt, v in case.get("options", {}).items():
            h.set_option(opt, v)
        if case.get("uniform"):
            h.configure_all(**chans[0]["props"])
        else:
            h.configure(0, [c["props"] for c in chans])
        rng = np.random.default_rng(20261017)
        calls = []
        for k in range(2):
            pk, out = (pl.Packet * C)(), (pl.Output * C)()
            for c, ch in enumerate(chans):
                x = _packet_data(rng, ch["dtype"], ch["lens"][k])
                cap = h.output_capacity(c, ch["lens"][k])
                rows = [h.device_alloc(max(n, 128)) for n in (x.nbytes, 8 * cap, 4 * cap, 6 * cap, 2 * cap)]
                bufs += rows
                h.upload(rows[0], x)
                pk[c].data, pk[c].n_floats, pk[c].sri_xdelta, pk[c].sri_mode = rows[0], x.size, 0.01, 1
                pk[c].sriChanged, pk[c].present, pk[c].format = int(k == 0), 1, fmt.get(ch["dtype"], pl.FORMAT_CF32)
                out[c].soft, out[c].phase, out[c].bits, out[c].sampleIndex, out[c].cap_symbols = rows[1], rows[2], rows[3], rows[4], cap
            calls.append((pk, out))
        h.synchronize()
        traces, streams = [], {}
        for pk, out in calls:
            with _Stderr() as err:
                h.process_device(0, pk, out)
            traces.append(normalise(err.out, streams))
            h.synchronize()  # (the next call reads the note the parallel fit's kernels leave the host: not while they run)
        return traces
    finally:
        if h is not None:
            for b in bufs:
                h.device_free(b)
            h.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _whats(traces):
    return {line.split("|")[0] for call in traces for line in call if not line.startswith("  ")}


def _recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_order_is_the_recorded_one(name):
    want = _recorded()["cases"][name]
    got = run_case(name)
    assert len(got) == len(want) == 2
    for k in range(2):
        for i, (g, w) in enumerate(zip(got[k], want[k])):
            assert g == w, "%s, call %d, line %d of the trace" % (name, k, i)
        assert len(got[k]) == len(want[k]), "%s, call %d: %d lines, recorded %d" % (name, k, len(got[k]), len(want[k]))


def test_recorded_traces_hold_every_launch_name():
    """(of the file alone: what it was recorded from is another commit)"""
    rec = _recorded()
    assert re.fullmatch(r"[0-9a-f]{40}", rec["commit"]), rec["commit"]
    assert sorted(rec["cases"]) == sorted(CASES)
    seen = set()
    for traces in rec["cases"].values():
        seen |= _whats(traces)
    assert seen == WHATS, (sorted(WHATS - seen), sorted(seen - WHATS))


def _record():
    ap = argparse.ArgumentParser(description="record the traces of the build in the tree (a build of the commit to pin against)")
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", default=None, help="the commit the build was made from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=RECORDED)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
    cases = {}
    for name in sorted(CASES):
        cases[name] = run_case(name)
        print(name, [len(t) for t in cases[name]], sorted(_whats(cases[name])), flush=True)
    seen = set().union(*(_whats(t) for t in cases.values()))
    print("missing:", sorted(WHATS - seen), "unexpected:", sorted(seen - WHATS), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(commit=commit, cases=cases), f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    _record()
