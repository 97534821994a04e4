"""Every kernel family through psk_soft_process_device on rows of exactly n_symbols between guard words (tests/row_guards.py,
DESIGN.md section 4.5), on a real MI355X.

Every family is one batch, run twice on two fresh handles: once with all four rows for every channel, once with the channels
cycling over the sets of absent streams (row_guards.NULL_SETS: none, each single one, bits only, bits + sampleIndex only,
nothing at all with cap_symbols 0).  Both runs: every stream the call had a pointer for is the oracle's bit for bit
(assert_parity), no guard byte, no byte in the place of an absent row and no packet byte changed, and the statistics say the
family's kernels did the work -- what the family's own test asserts.  Across the runs: the per-channel statistics of every
call and the state blob of every channel after the last are identical -- which rows a caller asks for reaches neither.

The stimuli are the suite's own (the cases of the tests named in each family), cut down to calls of at most 2^16 samples.
The census paths run through tests/test_gpu_instantiations.py: run_rows with the guarded rows, its assertions unchanged."""
import os
import time

import numpy as np
import pytest

from tests import instantiation_census as ic
from tests import row_guards as rg
from tests.test_gpu_cs16_schedules import parse_trace, rounds, screened, whats
from tests.test_gpu_instantiations import run_child_with_reread_0, run_rows
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

KEYS = rg.STREAMS


# ---- the census paths ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", [p for p in ic.PATHS if p != "settle_in_place_h8"])
def test_census_path_on_guarded_rows(oracle_mod, monkeypatch, capfd, path):
    """the rows of the path (three calls ending in tails of 1 .. 3, 60 .. 100 and 127 symbols: odd and even tails and a partial
    last block for every unit) with everything test_gpu_instantiations asserts, the guards, and a third handle whose rows
    cycle over the sets of absent streams"""
    if path == "settle_in_place":
        assert os.environ.get("PSK_SOFT_REREAD") in (None, "1")
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows(path), guarded=True)


def test_census_h8_on_guarded_rows_child(oracle_mod, monkeypatch, capfd):
    """The 15 H8_E0 units (the body of test_census_h8_on_guarded_rows, which starts it in a process of its own)."""
    if os.environ.get("PSK_SOFT_REREAD") != "0":
        pytest.skip("runs in the child process of test_census_h8_on_guarded_rows, which sets PSK_SOFT_REREAD=0")
    assert not run_rows(oracle_mod, monkeypatch, capfd, ic.rows("settle_in_place_h8"), guarded=True)


def test_census_h8_on_guarded_rows():
    """psk_fast_S{2..16}_H8_E0 in a fresh process with PSK_SOFT_REREAD=0, as test_settle_in_place_h8 starts its own.  This
    process does not touch the GPU here, whatever becomes of the child."""
    run_child_with_reread_0(os.path.abspath(__file__), "test_census_h8_on_guarded_rows_child")


# ---- a family: kinds of channels, a batch of them, two runs --------------------------------------------------------------

class Kind:
    """one channel's properties and its packets, call by call (None: no packet in that call)"""

    def __init__(self, props, iq, cuts):
        self.props = props
        self.packets = [None if c is None else np.ascontiguousarray(iq[2 * c[0] : 2 * c[1]]) for c in cuts]
        assert self.packets[0] is not None  # (sriChanged goes with call 0)
        self._ref = None

    def ref(self, oracle_mod):
        """the oracle's streams of every call, computed once"""
        if self._ref is None:
            o = oracle_mod.OracleComponent()
            for k, v in self.props.items():
                setattr(o, k, v)
            self._ref = []
            for k, p in enumerate(self.packets):
                if p is None:
                    self._ref.append(None)
                    continue
                r = o.service(np.asarray(p).astype(np.float32), 0.01, sriChanged=(k == 0))
                self._ref.append(dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index))
        return self._ref


def by_packet(n, packet):
    """the cuts of n complex samples into calls of `packet`"""
    return [(a, min(a + packet, n)) for a in range(0, n, packet)]


def synth_kind(seed, M, S, diff, A, n_ph, N, packet, max_calls=None, signal_M=None, **kw):
    """signal_M: the modulation of the stimulus where it is not constelationSize (16 has no constellation to synthesise)"""
    from psk_soft_amd.stimulus import synth_channel

    cuts = by_packet(N, packet or N)[:max_calls]
    assert max(b - a for a, b in cuts) <= 1 << 16
    props = dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n_ph, differentialDecoding=diff)
    return Kind(props, synth_channel(seed, signal_M or M, S, cuts[-1][1], **kw), cuts)


class Run:
    pass


def run_batch(oracle_mod, kinds, absent, setup=None, limits=None, ch0=0, n_handle=None, entry=None, capfd=None):
    """kinds[c]: the Kind of channel ch0 + c of a fresh handle of n_handle channels; absent[c]: the streams its calls leave
    out.  Every call on guarded rows; parity of every stream asked for; returns a Run: found (guard findings), stats[k],
    chstats[k][c], blobs[c], traces[k], seconds.  entry(h, dev, lay, k, first): another way to make call k (default:
    DeviceRows.run through psk_soft_process_device)."""
    from psk_soft_amd import lib as pl

    limits = dict(limits or {})
    C, n_handle = len(kinds), n_handle or len(kinds)
    n_calls = max(len(kd.packets) for kd in kinds)
    out = Run()
    out.found, out.stats, out.chstats, out.traces = [], [], [], []
    t0 = time.perf_counter()
    h = pl.Handle(n_handle, device=0, **limits)
    planner = rg.Planner(n_handle, **limits)
    dev = rg.DeviceRows(h)
    try:
        for hh in (h, planner.h):
            hh.configure(ch0, [kd.props for kd in kinds])
        if setup:
            setup(h)
        for k in range(n_calls):
            packets = [kd.packets[k] if k < len(kd.packets) else None for kd in kinds]
            sri = k == 0
            lay = rg.Layout(planner.counts(ch0, packets, sri), absent=absent, packets=packets, call=k)
            if capfd:
                capfd.readouterr()
            if entry:
                res, found = entry(h, dev, lay, k, sri)
            else:
                res, found, _ = dev.run(lay, ch0, sri_changed=sri)
            if capfd:
                out.traces.append(parse_trace(capfd.readouterr().err))
            out.found += found
            out.stats.append(h.stats())
            out.chstats.append(h.channel_stats(ch0, C))
            for c, kd in enumerate(kinds):
                if packets[c] is None:
                    assert all(res[c][s] is None or res[c][s].size == 0 for s in KEYS), (k, c)
                    continue
                ref = kd.ref(oracle_mod)[k]
                got = {s: ref[s] if res[c][s] is None else res[c][s] for s in KEYS}  # (an absent stream: nothing to compare)
                assert_parity(got, ref, "call %d channel %d without %s, %s" % (k, c, list(absent[c]) if absent else [], kd.props))
        out.blobs = [h.export_state(ch0 + c) for c in range(C)]
    finally:
        dev.close()
        planner.h.close()
        h.close()
    out.seconds = time.perf_counter() - t0
    return out


def null_sets(C, n_kinds=1):
    """the sets of absent streams over the channels of a batch whose channel c is of kind c % n_kinds: every kind meets every set"""
    assert C >= n_kinds * len(rg.NULL_SETS) or n_kinds == 1
    return [rg.NULL_SETS[(c // n_kinds) % len(rg.NULL_SETS)] for c in range(C)]


def both_runs(oracle_mod, name, kinds, check_stats, n_kinds=1, **kw):
    """the batch with all rows, then with the channels cycling over the sets of absent streams; check_stats(run) asserts what
    the family's own test asserts of the statistics"""
    C = len(kinds)
    assert C >= len(rg.NULL_SETS), "every set of absent streams is seen"
    full = run_batch(oracle_mod, kinds, [()] * C, **kw)
    sets = null_sets(C, n_kinds)
    part = run_batch(oracle_mod, kinds, sets, **kw)
    print("%s: %d channels, %d calls, %.2f s with all rows, %.2f s with absent streams" % (name, C, len(full.stats), full.seconds, part.seconds))
    for run, what in ((full, "all rows"), (part, "absent streams")):
        assert not run.found, "%s, %s:\n  %s" % (name, what, "\n  ".join(rg.messages(run.found)))
        check_stats(run)
    for k in range(len(full.stats)):
        assert part.chstats[k] == full.chstats[k], "%s: the statistics of call %d depend on the rows the call had" % (name, k)
    for c in range(C):
        assert part.blobs[c] == full.blobs[c], "%s: the state of channel %d (without %s) depends on the rows its calls had" % (
            name, c, list(sets[c]))
    return full, part


def times(kinds, n):
    """the kinds over and over: channel c is kinds[c % len]"""
    return [kinds[c % len(kinds)] for c in range(n)]


# ---- the families --------------------------------------------------------------------------------------------------------

def test_reference_order_kernel(oracle_mod):
    """set_force_sequential(1): psk_kernels.hip, one lane per channel; constelationSize 2, 4, 8 and 16 (no bits, a warning per
    symbol), samplesPerBaud 1 (no sampleIndex) and > 1, differential decoding; two calls with ragged cuts"""
    kinds = [synth_kind(300 + i, M, S, diff, A, 9, 2300 + 7 * i, 1201 + i, signal_M=(4 if M == 16 else None))
             for i, (M, S, diff, A) in enumerate(((2, 1, 0, 0), (4, 5, 0, 7), (8, 3, 1, 20), (16, 4, 0, 10), (8, 1, 0, 0)))]
    C = 40

    def stats(run):
        for k, st in enumerate(run.stats):
            assert st["channels_sequential"] == C and st["channels_fast"] == 0, (k, st)

    both_runs(oracle_mod, "reference order", times(kinds, C), stats, n_kinds=5, setup=lambda h: h.set_force_sequential(1))


def test_exactness_guard_hands_over(oracle_mod):
    """test_gpu_parity.test_exactness_guard_hands_over: the wave-scan kernel refuses at run time, the reference-order kernel
    writes the rows"""
    from psk_soft_amd.stimulus import synth_channel

    iq = synth_channel(9, 4, 8, 1 << 14).copy()
    iq[: 2 * 4000] *= np.float32(1e-6)
    iq[2 * 9000 : 2 * 9100] *= np.float32(3e4)
    kd = Kind(dict(samplesPerBaud=8, constelationSize=4, numAvg=100), iq, [(0, 1 << 14)])

    def stats(run):
        assert all(st["channels_guard"] == 1 for st in run.chstats[0]), run.stats

    both_runs(oracle_mod, "guard hand-over", [kd] * 8, stats)


def _tiled(mode=2, pfit=None):
    from psk_soft_amd import lib as pl

    def setup(h):
        h.set_option(pl.Handle.OPT_TIME_TILED, mode)
        if pfit is not None:
            h.set_option(pl.Handle.OPT_PARALLEL_FIT, pfit)
    return setup


def _tiled_kinds():
    """test_gpu_tiled.CASES with a packet length: their first three calls"""
    from tests.test_gpu_tiled import CASES

    cases = [c for c in CASES if c[6] is not None and c[6] > 8 * c[1]]
    assert len(cases) == 6
    return [synth_kind(31 * M + S, M, S, diff, A, n, N, packet, max_calls=3) for M, S, diff, A, n, N, packet in cases]


_TILED = []


def tiled_kinds():
    if not _TILED:
        _TILED.extend(_tiled_kinds())
    return _TILED


@pytest.mark.parametrize("pfit", [1, 0])
def test_tiled_front_fit_back(oracle_mod, pfit):
    """PSK_SOFT_OPT_TIME_TILED = 2: the tiled front, fit and back stages; with the parallel fit (from the second call on, the
    window full) and with PSK_SOFT_OPT_PARALLEL_FIT = 0, the fit walked block by block"""
    kinds = times(tiled_kinds(), 48)  # (6 kinds x 8 sets)
    assert all(len(kd.packets) == 3 for kd in kinds)

    def stats(run):
        for k, per in enumerate(run.chstats):
            for c, st in enumerate(per):
                assert st["channels_fast"] == 1 and st["channels_sequential"] == 0 and st["channels_tiled"] == 1, (k, c, st)
                if pfit == 0:
                    assert st["channels_parallel_fit"] == 0, (k, c, st)
                elif k == len(run.chstats) - 1 and kinds[c].props["phaseAvg"] >= 2 and os.environ.get("PSK_SOFT_PIPELINED") != "2":
                    assert st["channels_parallel_fit"] == 1 and st["parallel_fit_refusals"] == 0, (k, c, st)

    both_runs(oracle_mod, "tiled, parallel fit %d" % pfit, kinds, stats, n_kinds=6, setup=_tiled(2, pfit))


@pytest.mark.skipif(os.environ.get("PSK_SOFT_PIPELINED") == "2", reason="counts the parallel fit, which the forced pipelined mode replaces")
def test_parallel_fit_second_round(oracle_mod):
    """test_gpu_tiled.test_parallel_fit_second_round with the round always enqueued: 16 channels at 16 dB, eight calls"""
    C, N, calls = 16, 1 << 15, 8
    kinds = [synth_kind(100 + c, 4, 8, 0, 100, 50, calls * N, N, sigma=0.15) for c in range(C)]

    def stats(run):
        for st in run.stats:
            assert st["channels_fast"] == C and st["channels_sequential"] == 0, st
        assert sum(st["channels_parallel_fit"] for st in run.stats) >= (calls - 1) * C * 3 // 4, run.stats
        assert sum(st["channels_parallel_fit_second_round"] for st in run.stats) >= 1, run.stats

    both_runs(oracle_mod, "second round", kinds, stats, setup=_tiled(2, 2))


@pytest.mark.skipif(os.environ.get("PSK_SOFT_PIPELINED") == "2", reason="counts the parallel fit, which the forced pipelined mode replaces")
def test_parallel_fit_walker(oracle_mod):
    """test_gpu_tiled.test_parallel_fit_walks_runs_of_blocks_itself, its cases of at most 2^16 samples a call: a constellation
    a few hundredths of a radian off zero phase, exactly zero phase with a partial last block, 2-PSK"""
    cases = ((4, 8, 50, 0, 0.0766, 1 << 16), (4, 8, 50, 0, 0.0, (1 << 16) - 40), (2, 4, 17, 0, 0.03, 1 << 15))
    kinds = [synth_kind(131 + M, M, S, diff, 100, n, 3 * npk, npk, cfo=0.0, phi0=mphi0 / M) for M, S, n, diff, mphi0, npk in cases]
    batch = times(kinds, 24)

    def stats(run):
        for c, st in enumerate(run.chstats[-1]):
            assert st["channels_parallel_fit"] == 1 and st["parallel_fit_refusals"] == 0, (c, st)
        # (test_parallel_fit_walks_runs_of_blocks_itself's bound: a quarter of some call's blocks walked by the wave itself -- runs)
        walked = [(run.chstats[-1][c]["fit_chain_blocks"], (npk // S + 127) // 128) for c, (_, S, _, _, _, npk) in enumerate(cases)]
        assert any(w >= nb // 4 for w, nb in walked), walked

    both_runs(oracle_mod, "walker", batch, stats, n_kinds=3, setup=_tiled(2))


def test_pipelined_ranges(oracle_mod, monkeypatch):
    """test_gpu_tiled.test_pipelined_ranges, its smallest case (samplesPerBaud 4, 2-PSK): ranges of three tiles, ragged lengths,
    a noisy channel handed over in the middle of a call; an eighth channel so that every set of absent streams is seen"""
    monkeypatch.setenv("PSK_SOFT_PIPELINED", "2")
    S, M, diff, n_ph, calls = 4, 2, 0, 10, 3
    lens = [40000, 40000, 1000 * S, 23456, 40000, 17 * 128 * S + 5 * S, 40000, 31111]
    C = len(lens)
    kinds = [synth_kind(500 + 7 * S + c, M, S, diff, 100, n_ph, calls * lens[c], lens[c], sigma=(0.35 if c == 4 else 0.01)) for c in range(C)]

    def stats(run):
        for st in run.stats:
            assert st["channels_fast"] == C and st["channels_sequential"] == 0 and st["channels_parallel_fit"] == 0, st
        assert sum(st["channels_tiled"] for st in run.stats) >= calls * (C - 2), run.stats

    both_runs(oracle_mod, "pipelined ranges", kinds, stats, setup=_tiled(2))


def test_run_time_front_stages(oracle_mod):
    """test_gpu_tiled.ANY_CASES -- samplesPerBaud 1, samplesPerBaud >= 33, numAvg > 1024: the time-tiled kernels behind the front
    stage that takes both at run time -- and samplesPerBaud 1025 (test_gpu_wide_symbols): the wide front stage, psk_wide.hip"""
    from tests.test_gpu_wide_symbols import psk_signal

    kinds = [synth_kind(53 * M + S, M, S, diff, A, n, N, packet) for M, S, diff, A, n, N, packet in
             ((4, 1, 0, 0, 50, 20000, 7001), (8, 33, 0, 60, 200, 33 * 2600, 33 * 900), (4, 10, 0, 1025, 385, 10 * 6000, 20000))]
    wide = psk_signal(np.random.default_rng(1025 * 16 + 4 * 2), 1025, 60, 4)
    kinds.append(Kind(dict(samplesPerBaud=1025, constelationSize=4, numAvg=3, phaseAvg=20, differentialDecoding=0), wide,
                      [(0, 20011), (20011, 40960), (40960, 61500)]))
    assert all(len(kd.packets) == 3 for kd in kinds)
    batch = times(kinds, 32)

    def stats(run):
        for k, per in enumerate(run.chstats):
            for c, st in enumerate(per):
                assert st["channels_sequential"] == 0 and st["channels_guard"] == 0, (k, c, st)
        for c, st in enumerate(run.chstats[-1]):
            assert st["channels_fast"] == 1, (c, st)
            if c % 4 == 3:  # (samplesPerBaud 1025: test_wide_symbols_match_the_oracle's rule)
                assert any(per[c]["channels_tiled"] == 1 for per in run.chstats), (c, st)
            else:  # (ANY_CASES: after the last call, as test_window_classes_without_an_instantiation)
                assert st["channels_tiled"] == 1, (c, st)

    both_runs(oracle_mod, "run-time front stages", batch, stats, n_kinds=4, limits=dict(max_window_samples=10 * 1025 + 64, max_phase_avg=512))


def test_far_fit(oracle_mod):
    """test_gpu_far_fit.test_filling_crossing_steady, its smallest case (samplesPerBaud 2, 2-PSK, phaseAvg 32641) with the option
    on: the window filling, becoming steady in the middle of a block of the second call, a call shorter than a block"""
    from psk_soft_amd.stimulus import synth_channel
    from tests.test_gpu_far_fit import OPT_FAR_FIT, _cuts_by_symbols

    S, M, n, A = 2, 2, 32641, 10
    c0 = int(0.6 * n) | 1
    while (n - c0) % 128 == 0:
        c0 += 2
    counts = [c0, c0, 101]
    assert counts[0] < n < counts[0] + counts[1] and (n - counts[0]) % 128
    cuts = _cuts_by_symbols(S, A, counts, S - 1)[:3]
    kd = Kind(dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=n, differentialDecoding=0), synth_channel(4100 + S + M, M, S, cuts[-1][1]), cuts)

    def stats(run):
        for k, per in enumerate(run.chstats):
            for st in per:
                assert st["channels_fast"] == 1 and st["channels_sequential"] == 0 and st["channels_guard"] == 0 and st["channels_tiled"] == 1, (k, st)

    both_runs(oracle_mod, "far fit", [kd] * 8, stats, setup=lambda h: h.set_option(OPT_FAR_FIT, 1),
              limits=dict(max_window_samples=16384, max_phase_avg=65535))


@pytest.mark.parametrize("pieces", [2, 3])
def test_mixed_batch_cut_in_time(oracle_mod, monkeypatch, capfd, pieces):
    """test_gpu_parity.test_mixed_batch_cut_in_time, "untiled", at samplesPerBaud 2 so that a call of 128 blocks stays under
    2^16 samples: five window classes in one batch, every channel's call cut into `pieces` pieces of whole blocks, the rows
    written piece by piece (process_device_call advances every pointer the call has).  A channel too short to cut, odd symbol
    counts.  The launch trace of the run itself shows the cut: every class's screened-tier launch once per piece."""
    monkeypatch.setenv("PSK_SOFT_SPLIT_CLASSES", str(pieces))
    monkeypatch.setenv("PSK_SOFT_TIME_TILED", "0")
    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    S, C, calls = 2, 16, 2
    Ms = [(2, 4, 8)[c % 3] for c in range(C)]
    lens = [36000 + 2 * (37 * c % 1000) + (2 if c % 2 else 0) for c in range(C)]
    lens[3] = 2300
    kinds = [synth_kind(4200 + c, Ms[c], S, int(c % 4 == 1), (25, 100, 200, 400, 1000)[c % 5], (10, 50, 200)[(c // 5) % 3], calls * lens[c], lens[c],
                        cfo=(0.02 if c % 7 == 0 else None)) for c in range(C)]
    classes = {(S, {25: 1, 100: 1, 200: 2, 400: 4, 1000: 8}[kd.props["numAvg"]]) for kd in kinds}

    def stats(run):
        for st in run.stats:
            assert st["channels_fast"] == C and st["channels_sequential"] == 0, st
        for k, lines in enumerate(run.traces):
            assert rounds(lines) == pieces and screened(lines) == {cl: pieces for cl in classes}, (k, screened(lines))
            assert "tile_front" not in whats(lines), (k, whats(lines))

    both_runs(oracle_mod, "cut in %d" % pieces, kinds, stats, capfd=capfd, limits=dict(max_window_samples=16384, max_phase_avg=512))


@pytest.mark.parametrize("entry", ["strided", "tuned"])
def test_frame_matrix(oracle_mod, monkeypatch, capfd, entry):
    """psk_soft_process_device_strided / _tuned: a frame-major matrix 12 columns wide, columns 1 .. 8 a run the tiled transpose
    takes and column 10 alone, gathered sample by sample.  The packet guard is the rest of the matrix: columns 0, 9 and 11 and
    the frames behind a shorter channel's last.  Tuned: every other channel shifted; the reference is the oracle on
    psk_soft_tune_apply of the column."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel
    from tests.test_gpu_strided import gathers

    monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
    W, cols, calls, F = 12, list(range(1, 9)) + [10], 2, 3001
    C = len(cols)
    props = [dict(samplesPerBaud=(4, 5, 8)[c % 3], constelationSize=(2, 4, 8)[(c // 2) % 3], numAvg=(30, 100)[c % 2], phaseAvg=(10, 50)[(c // 3) % 2],
                  differentialDecoding=int(c == 4)) for c in range(C)]
    frames = [[F - 7 * ((c + k) % 4) for c in range(C)] for k in range(calls)]
    tunes = [(0, 0) if entry == "strided" or c % 2 == 0 else ((c * 0x1234567890ABCDEF) & (2 ** 64 - 1), pl.tune_step(1e-4 * (c - 4))) for c in range(C)]
    raw, kinds = [], []
    for c in range(C):
        n = sum(frames[k][c] for k in range(calls))
        iq = synth_channel(8100 + c, props[c]["constelationSize"], props[c]["samplesPerBaud"], n)
        cuts = [(sum(frames[j][c] for j in range(k)), sum(frames[j][c] for j in range(k + 1))) for k in range(calls)]
        raw.append([iq[2 * a : 2 * b] for a, b in cuts])
        seen, ph = [], tunes[c][0]
        for a, b in cuts:  # (what the demodulator sees: the column shifted, the oscillator running on from call to call)
            seen.append(iq[2 * a : 2 * b] if tunes[c] == (0, 0) else pl.tune_apply(ph, tunes[c][1], iq[2 * a : 2 * b]))
            ph = pl.tune_advance(ph, tunes[c][1], b - a)
        kinds.append(Kind(props[c], np.concatenate(seen), cuts))
    phase = [t[0] for t in tunes]

    def call(h, dev, lay, k, sri):
        m = np.full((F, W, 2), np.float32(-7.5e8))
        for c, col in enumerate(cols):
            m[: frames[k][c], col] = raw[c][k].reshape(-1, 2)
        image = (m.view(np.uint8).reshape(-1), [(8 * col, 2 * frames[k][c], pl.FORMAT_CF32) for c, col in enumerate(cols)])
        lay = rg.Layout(lay.counts, absent=lay.absent, packet_image=image, call=k)

        def go(pk, out, bases):
            tn = [(phase[c], tunes[c][1]) if tunes[c] != (0, 0) else (0, 0) for c in range(C)]
            if entry == "strided":
                h.process_device_strided(0, pk, [W] * C, out)
            else:
                h.process_device_tuned(0, pk, [W] * C, tn, out)
        res, found, _ = dev.run(lay, 0, sri_changed=sri, call=go)
        for c in range(C):
            phase[c] = pl.tune_advance(phase[c], tunes[c][1], frames[k][c])
        return res, found

    def stats(run):
        for k, (st, lines) in enumerate(zip(run.stats, run.traces)):
            assert st["channels_fast"] == C and st["channels_sequential"] == 0, st
            assert gathers(lines) == (1, 1, 1, 1), (k, lines)
            assert ("tune" in whats(lines)) == (entry == "tuned"), (k, whats(lines))

    def reset(h):
        phase[:] = [t[0] for t in tunes]

    both_runs(oracle_mod, "frame matrix, %s" % entry, kinds, stats, setup=reset, entry=call, capfd=capfd)


def test_a_call_in_the_middle_of_a_handle_leaves_its_neighbours_alone(oracle_mod):
    """One call covers [5, 13) of 18 channels, on guarded rows with the channels cycling over the sets of absent streams; the
    channels on either side -- in the middle of their own streams, windows and fits full -- keep their state byte for byte."""
    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channel

    n_all, ch0, nch = 18, 5, 8
    props = [dict(samplesPerBaud=(8, 5, 10)[c % 3], constelationSize=(4, 8, 2)[c % 3], numAvg=(100, 25, 200)[c % 3], phaseAvg=(50, 10)[c % 2])
             for c in range(n_all)]
    iqs = [synth_channel(6100 + c, props[c]["constelationSize"], props[c]["samplesPerBaud"], 9000 + 4137 + c) for c in range(n_all)]
    h = pl.Handle(n_all, device=0)
    planner, dev = rg.Planner(n_all), rg.DeviceRows(h)
    try:
        for hh in (h, planner.h):
            hh.configure(0, props)
        h.process_host(0, [dict(data=iq[: 2 * 9000], xdelta=0.01, sriChanged=True) for iq in iqs])
        planner.counts(0, [iq[: 2 * 9000] for iq in iqs], True)
        before = [h.export_state(c) for c in range(n_all)]
        packets = [iqs[ch0 + c][2 * 9000 :] for c in range(nch)]
        lay = rg.Layout(planner.counts(ch0, packets, False), absent=null_sets(nch), packets=packets)
        res, found, _ = dev.run(lay, ch0)
        assert not found, rg.messages(found)
        after = [h.export_state(c) for c in range(n_all)]
        for c in range(n_all):
            assert (after[c] == before[c]) == (not ch0 <= c < ch0 + nch), "channel %d" % c
        for c in range(nch):
            o = oracle_mod.OracleComponent()
            for k, v in props[ch0 + c].items():
                setattr(o, k, v)
            o.service(iqs[ch0 + c][: 2 * 9000], 0.01, sriChanged=True)
            r = o.service(packets[c], 0.01, sriChanged=False)
            ref = dict(soft=r.soft, bits=r.bits, phase=r.phase, index=r.index)
            assert_parity({s: ref[s] if res[c][s] is None else res[c][s] for s in KEYS}, ref, "channel %d" % (ch0 + c))
    finally:
        dev.close()
        planner.h.close()
        h.close()


def test_a_short_row_is_refused_on_the_device_too(oracle_mod):
    """The capacity rule (tests/test_output_contract_control.py) on a real handle: a bits-only and a sampleIndex-only row one
    symbol short are refused before anything is enqueued -- the state blobs are as before --, and the same call on exact rows
    is the oracle's.  (Were the call not refused, the symbol too many would land in the guard behind the row.)"""
    from psk_soft_amd import lib as pl

    kinds = [synth_kind(7300 + c, M, S, 0, 20, 10, 3000 + c, 3000 + c) for c, (M, S) in enumerate(((4, 8), (8, 5), (2, 4)))]
    absent = [(), ("soft", "phase", "index"), ("soft", "phase", "bits")]

    def entry(h, dev, lay, k, sri):
        def go(pk, out, bases):
            before = [h.export_state(c) for c in range(3)]
            for c in (1, 2):
                out[c].cap_symbols -= 1
                with pytest.raises(pl.PskSoftError) as e:
                    h.process_device(0, pk, out)
                assert e.value.status == 6, e.value
                out[c].cap_symbols += 1
            assert [h.export_state(c) for c in range(3)] == before
            h.process_device(0, pk, out)
        res, found, _ = dev.run(lay, 0, sri_changed=sri, call=go)
        return res, found

    run = run_batch(oracle_mod, kinds, absent, entry=entry)
    assert not run.found, rg.messages(run.found)
    assert run.stats[0]["channels_fast"] == 3, run.stats


# ---- the host entry ------------------------------------------------------------------------------------------------------

def _host_arenas(lay):
    """the layout's arenas in host memory, each on a line: ({arena: address}, {arena: uint8 view}), filled as they go up"""
    bases, views = {}, {}
    for name, img in lay.images().items():
        buf = np.empty(img.size + rg.LINE, np.uint8)
        off = -buf.ctypes.data % rg.LINE
        views[name] = buf[off : off + img.size]
        views[name][:] = img
        bases[name] = buf.ctypes.data + off
    return bases, views


def test_host_entry_on_a_real_handle(oracle_mod):
    """psk_soft_process_host has a capacity check of its own (a control-plane handle never reaches it: there the host entry
    is the device entry).  On a real handle, with HOST rows of exactly n_symbols between guard words: a bits-only and a
    sampleIndex-only row one symbol short are refused and the state blobs are as before; exact rows are accepted, the
    oracle's, and the copies back write nothing outside them; a channel with all four pointers null and cap_symbols 0 is
    accepted; after both calls every channel's blob is that of a handle whose calls had all rows."""
    from psk_soft_amd import lib as pl

    kinds = [synth_kind(7400 + c, M, S, 0, 20, 10, 6100 + 2 * c, 3000 + c, max_calls=2) for c, (M, S) in enumerate(((4, 8), (8, 5), (2, 4), (8, 3)))]
    C = len(kinds)
    absent = [(), ("soft", "phase", "index"), ("soft", "phase", "bits"), rg.STREAMS]
    blobs = []
    for sets in ([()] * C, absent):
        h = pl.Handle(C, device=0)
        planner = rg.Planner(C)
        try:
            for hh in (h, planner.h):
                hh.configure(0, [kd.props for kd in kinds])
            for k in range(2):
                packets = [kd.packets[k] for kd in kinds]
                lay = rg.Layout(planner.counts(0, packets, k == 0), absent=sets, packets=packets, call=k)
                bases, views = _host_arenas(lay)
                pk, out = (pl.Packet * C)(), (pl.Output * C)()
                lay.fill(bases, pk, out, sri_changed=(k == 0))
                if k == 1:
                    before = [h.export_state(c) for c in range(C)]
                    for c in range(C):
                        if not 0 < len(sets[c]) < 4:
                            continue
                        out[c].cap_symbols -= 1
                        st = h._L.psk_soft_process_host(h._h, 0, C, pk, out)
                        assert st == 6, "channel %d, a row without %s one symbol short: status %d" % (c, list(sets[c]), st)
                        out[c].cap_symbols += 1
                    assert [h.export_state(c) for c in range(C)] == before, "a refused call changed the state"
                pl._check(h._L.psk_soft_process_host(h._h, 0, C, pk, out))
                found = lay.check(views)
                assert not found, rg.messages(found)
                for c, kd in enumerate(kinds):
                    assert int(out[c].n_symbols) == lay.counts[c]["n_symbols"] > 0
                    got, ref = lay.extract(views, c), kd.ref(oracle_mod)[k]
                    assert all((got[s] is None) == (s in sets[c]) for s in KEYS)
                    assert_parity({s: ref[s] if got[s] is None else got[s] for s in KEYS}, ref, "host entry, call %d channel %d without %s" % (k, c, list(sets[c])))
            assert h.stats()["channels_fast"] == C
            blobs.append([h.export_state(c) for c in range(C)])
        finally:
            planner.h.close()
            h.close()
    for c in range(C):
        assert blobs[1][c] == blobs[0][c], "the state of channel %d (without %s) depends on the rows its calls had" % (c, list(absent[c]))
