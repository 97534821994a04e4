"""The front stages that take samplesPerBaud and numAvg at run time, on a real MI355X: the rows of tests/front_census.py
(DESIGN.md section 4.8), one test per variant, the rows of a variant the channels of one handle -- so that the launch picks
psk_tile_front_any_kernel<1>, <4> or <16>, or sizes the wide front stage for its widest channel, as the rows need it --,
three calls a channel.

For every row: all four streams of every call are the oracle's bit for bit; Handle.channel_stats says that the time-tiled
kernels carried every call of a tie, kept or before row, and that a drift row's call with the burst was refused by the exactness
guard and the call after it carried again; the launch trace of a second, traced handle fed the same input holds the front
launch of the variant, one a call, with its S field inside the variant's range (and the far fit's lines for the far rows), and its outputs
are the untraced run's.  PSK_SOFT_VALIDATE=1 throughout.  A test reports every row that is wrong, not the first.

compare() takes results and nothing else, so that tests/test_front_census.py can hand it stand-ins built from the models and see
them reported (no GPU there)."""
import time

import pytest

from tests import front_census as fc
from tests.test_gpu_cs16_schedules import KEYS, parse_trace, untraced_then_traced
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

FRONT_LINE = dict(any="tile_front_any", wide="wide_front (chunk, pick)")
FAR_LINES = dict(any=("tile_front_any (far)", "far_fit (any)"), wide=("wide_front (chunk, pick; far)", "far_fit (wide)"))
LAUNCHES = "launch lines"  # the key of what is wrong with a call's launches: they belong to the handle, not to a row


def wrong_stats(row, k, st):
    """what the statistics of call k of a row's channel say against section 4.8, or None"""
    if row.burst_call == k:
        ok = st["channels_guard"] == 1 and st["channels_tiled"] == 0
    else:
        ok = st["channels_tiled"] == 1 and st["channels_guard"] == 0 and st["channels_sequential"] == 0
    return None if ok else "call %d: %s" % (k, {key: v for key, v in st.items() if v})


def wrong_launches(variant, rows, k, lines):
    """what the launch lines of call k say against the variant, as a list"""
    out = []
    fronts = {r.front for r in rows if r.emit[k]}
    for front in sorted(fronts):
        S = max(r.S for r in rows if r.front == front and r.emit[k])
        names = FAR_LINES[front] if variant == "far" else (FRONT_LINE[front],)
        lo, hi = fc.S_RANGE["wide" if front == "wide" else variant if variant != "far" else "any1"]
        for what in names:
            hit = [t for t in lines if t["what"] == what]
            if not hit:
                out.append("call %d has no '%s'" % (k, what))
            elif len(hit) != 1 or not (lo <= hit[0]["S"] <= hi and hit[0]["S"] == S):  # one launch, sized by its widest row
                out.append("call %d: '%s' with S %s, the variant's is one launch with S %d (%d .. %d)" % (k, what, [t["S"] for t in hit], S, lo, hi))
    other = [t["what"] for t in lines if t["what"].split(" (")[0] in ("tile_front_any", "wide_front") and
             {"tile_front_any": "any", "wide_front": "wide"}[t["what"].split(" (")[0]] not in fronts]
    if other:
        out.append("call %d launches %s as well" % (k, sorted(set(other))))
    return out


def compare(variant, rows, got, ref, stats, stats_traced, traces):
    """{row name or LAUNCHES: [what is wrong]} -- got[c][k], ref[c][k]: the four streams of call k of row c; stats[k][c],
    stats_traced[k][c]: its statistics in the two runs; traces[k]: the parsed launch lines of call k"""
    wrong = {}
    for c, r in enumerate(rows):
        w = []
        for k in range(len(r.packets)):
            try:
                assert_parity(got[c][k], ref[c][k], "call %d" % k)
            except AssertionError as e:
                w.append("parity: " + str(e).splitlines()[0][:200])
            for which, s in (("", stats), (" (traced)", stats_traced)):
                bad = wrong_stats(r, k, s[k][c])
                if bad:
                    w.append("statistics%s: %s" % (which, bad))
        if w:
            wrong[r.name] = w
    w = [m for k in range(len(traces)) for m in wrong_launches(variant, rows, k, traces[k])]
    if w:
        wrong[LAUNCHES] = w
    return wrong


def run_variant(oracle_mod, monkeypatch, capfd, variant):
    from psk_soft_amd import lib as pl

    t0 = time.perf_counter()
    rows = fc.rows(variant)
    n = len(rows)
    far = variant == "far"
    t1 = time.perf_counter()
    ref = [fc.oracle_calls(oracle_mod, r) for r in rows]
    t2 = time.perf_counter()

    def body(h, cap):
        if far:
            h.set_option(pl.Handle.OPT_FAR_FIT, 1)
        h.configure(0, [r.props for r in rows])
        got, traces, stats = {c: [] for c in range(n)}, [], []
        for k in range(3):
            if cap:
                cap.readouterr()
            res = h.process_host(0, [dict(data=r.packets[k], xdelta=0.01, sriChanged=(k == 0)) for r in rows])
            if cap:
                traces.append(parse_trace(cap.readouterr().err))
            stats.append(h.channel_stats())
            for c in range(n):
                got[c].append({key: res[c][key] for key in KEYS})
        return got, traces, stats

    limits = dict(max_window_samples=max(r.S * r.A for r in rows) + 64, max_phase_avg=65535 if far else 512,
                  max_packet_complex=1 << 21)
    assert max(p.size // 2 for r in rows for p in r.packets) <= limits["max_packet_complex"]
    # (PSK_SOFT_STAGE_MB: psk_soft_process_host cuts a batch into chunks of channels of 32 MiB of input, a launch set each -- the
    # rows of a variant are to share one, so the chunk is made to hold the variant's largest call, and no more: a slot's pinned
    # buffers are sized by it)
    stage_mb = max(32, -(-max(sum(r.packets[k].nbytes for r in rows) for k in range(3)) >> 20) + 8)
    env = {"PSK_SOFT_VALIDATE": "1", "PSK_SOFT_STAGE_MB": str(stage_mb)}
    (got, _, stats), (_, traces, stats_traced) = untraced_then_traced(monkeypatch, capfd, env, n, body, **limits)
    t3 = time.perf_counter()
    wrong = compare(variant, rows, got, ref, stats, stats_traced, traces)
    print("%s: %d rows, draw %.2f s, oracle %.2f s, two handles x three calls %.2f s, %d wrong" % (variant, n, t1 - t0, t2 - t1, t3 - t2, len(wrong)))
    for name, w in wrong.items():
        print("  %s %s\n    %s" % (name, next((r.props for r in rows if r.name == name), ""), "\n    ".join(w)))
    return wrong


def test_any_one_phase_a_lane(oracle_mod, monkeypatch, capfd):
    """psk_tile_front_any_kernel<1>: samplesPerBaud 33, 40, 63, 64, and 2, 8, 16 with windows of more than 1024 symbols --
    the window staged through LDS in batches of 512 samples (numAvg - 1 of exactly one batch and one symbol more among the
    rows), eight symbols a step through the level-by-level reductions, a last chunk of 1 and of 7 symbols"""
    assert not run_variant(oracle_mod, monkeypatch, capfd, "any1")


def test_any_four_phases_a_lane(oracle_mod, monkeypatch, capfd):
    """<4>: 65 (a lane's second phase), 128, 255, 256, with a channel of 40 in the same launch (nk = 1); the window rebuilt
    four symbols at a time with (numAvg - 1) mod 4 of 0, 1, 2 and 3; the CS16, CS8 and CF16 ties at 65"""
    assert not run_variant(oracle_mod, monkeypatch, capfd, "any4")


def test_any_sixteen_phases_a_lane(oracle_mod, monkeypatch, capfd):
    """<16>: 257 (the fifth phase), 1000, 1023, 1024 (the sixteenth), with channels of 40 and 100 in the same launch"""
    assert not run_variant(oracle_mod, monkeypatch, capfd, "any16")


def test_wide(oracle_mod, monkeypatch, capfd):
    """psk_wide_chunk_kernel and psk_wide_pick_kernel sized for samplesPerBaud 5000 (zmax 5) with channels of two chunks (1025:
    the second holds one phase; 2048) and three (2049) beside: ties across the chunk boundary, the certificate through WideStat"""
    assert not run_variant(oracle_mod, monkeypatch, capfd, "wide")


def test_far_fit(oracle_mod, monkeypatch, capfd):
    """PSK_SOFT_OPT_FAR_FIT with phaseAvg 32641: a drift row behind far_fit (any) at samplesPerBaud 8 and one behind far_fit
    (wide) at 1025 -- the fold of psk_farfit.hip refuses the burst's call and carries the next"""
    assert not run_variant(oracle_mod, monkeypatch, capfd, "far")
