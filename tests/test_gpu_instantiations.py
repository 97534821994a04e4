"""Every compiled unit of the wave-scan family through each of its paths, on a real MI355X: the rows of
tests/instantiation_census.py, one test per path, the rows of a test the channels of one batch -- a
wave each, three calls, every call ending in a partial block.

For every row: all four streams of every call are the oracle's bit for bit; the per-channel statistics say that the named
tier did the work (Handle.channel_stats); the launch trace of a second, traced handle fed the same input holds the launch
line of the row's class, and its outputs are the untraced run's.  PSK_SOFT_VALIDATE=1 throughout.

The trace names the window class, not the variant of the numAvg 513 .. 1024 class: H0 (the symbols leaving the window read a
second time, the default) and H8_E0 (eight blocks of history in registers) both show as H=8.  Which of the two ran is decided
by PSK_SOFT_REREAD, which the library reads once per process: the evidence for H0 is that the suite's process runs without
it, the evidence for H8_E0 that its rows run in a child process started with PSK_SOFT_REREAD=0."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import instantiation_census as ic
from tests import row_guards as rg
from tests.test_gpu_cs16_schedules import KEYS, parse_trace, untraced_then_traced
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = {"settle_in_place": "fast (screened tier)", "settle_in_place_h8": "fast (screened tier)", "format_settle": "fast (screened tier)",
        "exact_tier": "fast (exact tier)", "exact_tier_h1": "fast (exact tier)", "format_exact": "fast (exact tier)",
        "tile_front": "tile_front"}
# format_exact rows whose driver does not reach launch_fast_<format>_S*_H1_E1 (DESIGN.md section 4.3 lists each with its reason);
# only rows of that path may be named here
UNREACHABLE = frozenset()


def _wrong_stats(row, k, st):
    """what the statistics of call k of a row's channel say against the table of section 4.3, or None"""
    p = row.path
    if p in ("settle_in_place", "settle_in_place_h8", "format_settle"):
        ok = (st["channels_fast"] == 1 and st["channels_exact_timing"] == 0 and st["channels_tiled"] == 0 and
              st["channels_sequential"] == 0 and st["timing_exact_blocks"] >= row.blocks()[k])
    elif p == "exact_tier":
        ok = st["channels_exact_timing"] == 1 and st["channels_guard"] == 0 and st["channels_sequential"] == 0
    elif p == "exact_tier_h1":
        ok = st["channels_sequential"] == 0 and (k < 2 or (st["channels_exact_timing"] == 1 and st["channels_guard"] == 0))
    elif p == "format_exact":
        ok = k == 0 or (st["channels_exact_timing"] == 1 and st["channels_guard"] == 0)
    else:
        ok = st["channels_tiled"] == 1 and st["timing_exact_blocks"] > 0 and st["channels_sequential"] == 0
    if ok:
        return None
    return "call %d (%d blocks): %s" % (k, row.blocks()[k], {key: v for key, v in st.items() if v})


def run_rows(oracle_mod, monkeypatch, capfd, rows, guarded=False):
    """The rows as one batch of one handle, untraced and traced; returns {row name: [what is wrong with it]} (empty: nothing).
    guarded: the calls go through psk_soft_process_device on rows of exactly n_symbols between guard words (tests/row_guards.py)
    instead of psk_soft_process_host, and a changed guard or packet byte is one more thing wrong with a row; a third handle
    then takes the same calls with the rows cycling over the sets of absent streams (row_guards.NULL_SETS): the streams it has
    pointers for, its statistics and its state blobs must be the first handle's."""
    from psk_soft_amd import lib as pl

    rows = [r for r in rows if r.name not in UNREACHABLE]
    n = len(rows)
    env = {"PSK_SOFT_VALIDATE": "1"}
    for r in rows:
        assert r.env == rows[0].env and r.time_tiled == rows[0].time_tiled
    env.update(rows[0].env)
    window = max(r.props["samplesPerBaud"] * r.props["numAvg"] for r in rows) + 64
    overruns, blobs = [], []  # (the findings and the state blobs of every handle)

    def body(h, cap, absent=None):
        h.configure(0, [r.props for r in rows])
        if rows[0].time_tiled is not None:
            h.set_option(pl.Handle.OPT_TIME_TILED, rows[0].time_tiled)
        if guarded:
            planner, dev = rg.Planner(n, max_window_samples=window, max_phase_avg=512), rg.DeviceRows(h)
            planner.h.configure(0, [r.props for r in rows])
        got, traces, stats = {c: [] for c in range(n)}, [], []
        try:
            for k in range(3):
                if guarded:
                    packets = [r.packets[k] for r in rows]
                    lay = rg.Layout(planner.counts(0, packets, k == 0), absent=absent, packets=packets, call=k)
                if cap:
                    cap.readouterr()
                if guarded:
                    res, found, _ = dev.run(lay, 0, sri_changed=(k == 0))
                    overruns.extend(found)
                else:
                    res = h.process_host(0, [dict(data=r.packets[k], xdelta=0.01, sriChanged=(k == 0)) for r in rows])
                if cap:
                    traces.append(parse_trace(cap.readouterr().err))
                stats.append(h.channel_stats())
                for c in range(n):
                    got[c].append({key: res[c][key] for key in KEYS})
            if guarded:
                blobs.append([h.export_state(c) for c in range(n)])
        finally:
            if guarded:
                dev.close()
                planner.h.close()
        return got, traces, stats

    t0 = time.perf_counter()
    ref = [ic.oracle_calls(oracle_mod, r) for r in rows]
    t1 = time.perf_counter()
    (got, _, stats), (_, traces, stats_traced) = untraced_then_traced(monkeypatch, capfd, env, n, body, max_window_samples=window,
                                                                       max_phase_avg=512)
    sets = [rg.NULL_SETS[c % len(rg.NULL_SETS)] for c in range(n)]
    if guarded:
        h = pl.Handle(n, device=0, max_window_samples=window, max_phase_avg=512)  # (under `env` still)
        try:
            got_part, _, stats_part = body(h, None, sets)
        finally:
            h.close()
    t2 = time.perf_counter()
    wrong = {}
    for c, r in enumerate(rows):
        w = []
        if guarded:
            for k in range(3):
                for key in KEYS:
                    x = got_part[c][k][key]
                    if (x is None) != (key in sets[c]) or (x is not None and x.tobytes() != got[c][k][key].tobytes()):
                        w.append("absent streams %s: call %d, %s is not the stream of the call with all rows" % (list(sets[c]), k, key))
                if stats_part[k][c] != stats[k][c]:
                    w.append("absent streams %s: the statistics of call %d differ" % (list(sets[c]), k))
            if blobs[2][c] != blobs[0][c]:
                w.append("absent streams %s: the state blob differs from the one after the calls with all rows" % list(sets[c]))
        for k in range(3):
            try:
                assert_parity(got[c][k], ref[c][k], "call %d" % k)
            except AssertionError as e:
                w.append("parity: " + str(e).splitlines()[0][:200])
            for which, s in (("", stats), (" (traced)", stats_traced)):
                bad = _wrong_stats(r, k, s[k][c])
                if bad:
                    w.append("statistics%s: %s" % (which, bad))
            H = 1 if r.path == "format_exact" and k == 0 else r.trace_H  # (the poisoned first call is a CF32 packet)
            if not any(t["what"] == LINE[r.path] and t["S"] == r.S and t["H"] == H for t in traces[k]):
                w.append("trace: call %d has no '%s' S=%d H=%d" % (k, LINE[r.path], r.S, H))
            if r.path == "format_settle" and any(t["what"].endswith("_convert") for t in traces[k]):
                w.append("trace: call %d converts packets in front of the kernels" % k)
        w += ["guards: " + f["message"] for f in overruns if f["channel"] == c or (c == 0 and f["channel"] is None)]
        if w:
            wrong[r.name] = w
    print("%s: %d rows, oracle %.2f s, %s handles x three calls %.2f s, %d rows wrong" % (rows[0].path, n, t1 - t0, "three" if guarded else "two", t2 - t1, len(wrong)))
    for name, w in wrong.items():
        print("  %s %s\n    %s" % (name, next(r.props for r in rows if r.name == name), "\n    ".join(w)))
    return wrong


def test_settle_in_place(oracle_mod, monkeypatch, capfd):
    """The 108 screened float units (H 1/2/4 at samplesPerBaud 2 .. 32, H 0 at 2 .. 16) settle a near-tie in every block of
    every call themselves: exact_block_from_ring (H 1), window_end_f64 (H 2/4), window_end_reread_f64 (H 0)."""
    assert os.environ.get("PSK_SOFT_REREAD") in (None, "1"), "the H 0 rows need the default variant of the numAvg 513 .. 1024 class"
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("settle_in_place"))


def test_exact_tier(oracle_mod, monkeypatch, capfd):
    """The 77 exact-tier float units with window history (H 2/4 at samplesPerBaud 2 .. 32, H 8 at 2 .. 16): with
    PSK_SOFT_TIES_IN_PLACE=0 the screened tier hands every call of the near-tie signal over."""
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("exact_tier"))


def test_exact_tier_h1(oracle_mod, monkeypatch, capfd):
    """The 31 exact-tier float units of numAvg <= 128: the third call holds a symbol whose M-th power overflows; the screened
    tier refuses it and <S, 1, true> redoes the call from its first symbol, with the state two calls carried there."""
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("exact_tier_h1"))


def test_format_settle(oracle_mod, monkeypatch, capfd):
    """The 45 screened packet-format units: integer-valued ties read in place as CS16 / CS8 / CF16 (classes H 3 / 5 / 6, no
    conversion launch) and settled by the kernel itself."""
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("format_settle"))


def test_format_exact(oracle_mod, monkeypatch, capfd):
    """The 45 exact-tier packet-format units: a NaN sample in a first CF32 call leaves a feedback the screened tier's fit stage
    refuses, so the two calls in the row's format are the exact tier's.  Their phase is NaN or astronomically large; bits,
    sampleIndex, the non-finite patterns and every finite value are compared."""
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("format_exact"))


def test_tile_front(oracle_mod, monkeypatch, capfd):
    """The 15 time-tiled front units, PSK_SOFT_OPT_TIME_TILED = 2: the front stage settles the near-ties of its tiles."""
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("tile_front"))


def run_child_with_reread_0(test_file, child_test):
    """`child_test` of `test_file` in a fresh process started with PSK_SOFT_REREAD=0; it must pass there, not skip"""
    env = dict(os.environ, PSK_SOFT_REREAD="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", test_file, "-k", child_test, "-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, "the child ended with status %d" % r.returncode
    assert "1 passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-500:]


def test_settle_in_place_h8_child(oracle_mod, monkeypatch, capfd):
    """The 15 H8_E0 units (the body of test_settle_in_place_h8, which starts it in a process of its own)."""
    if os.environ.get("PSK_SOFT_REREAD") != "0":
        pytest.skip("runs in the child process of test_settle_in_place_h8, which sets PSK_SOFT_REREAD=0")
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("settle_in_place_h8"))


def test_settle_in_place_h8():
    """psk_fast_S{2..16}_H8_E0: the H 0 rows over again in a fresh process with PSK_SOFT_REREAD=0 (launch_fast reads the
    variable once per process).  This process does not touch the GPU here, whatever becomes of the child."""
    run_child_with_reread_0(os.path.abspath(__file__), "test_settle_in_place_h8_child")
