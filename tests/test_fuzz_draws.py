"""tools/fuzz_gpu.py without a GPU: the draws of the cited seeds are what they were (tests/golden/fuzz_draws.json, recorded from
the tool before draw_round() existed, see tests/golden/make_fuzz_draws.py), and a rehearsal of every named configuration that
tests/test_gpu_randomised.py runs -- the draw respects the handle's limits and the entries' preconditions, the draw alone meets
the counts behind that file's reached-path assertions, and the oracle side of every round (tests/tune_model.py and the model
records included) runs to its end."""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_gpu as fz  # noqa: E402

from psk_soft_amd import lib as pl  # noqa: E402
from tests import tune_model as tm  # noqa: E402
from tests.golden.make_fuzz_draws import RECORDED, channel_digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fuzz_draws.json")
CASES = [(name, seed, rnd) for name, (_, _, rounds) in fz.CONFIGS.items() for seed, rnd in rounds]
_done = {}


def _pin(entry):
    rd = fz.draw_round(entry["seed"], entry["round"], entry["channels"], fz.Config())
    return [channel_digest(p, ev, s) for p, ev, s in zip(rd.props, rd.scripts, rd.sigs)]


def _rehearse(case):
    name, seed, rnd = case
    cfg, C, _ = fz.CONFIGS[name]
    rd = fz.draw_round(seed, rnd, C, cfg)
    tk = fz.ticks(rd)
    return rd, tk, fz.reference(rd, tk), fz.draw_facts(rd, tk)


def _pins():
    """every pinned draw, once, side by side (numpy leaves the interpreter lock alone)"""
    if "pins" not in _done:
        with open(GOLDEN) as f:
            entries = json.load(f)["entries"]
        with ThreadPoolExecutor(8) as ex:
            _done["pins"] = list(zip(entries, ex.map(_pin, entries)))
    return _done["pins"]


def _runs():
    """every rehearsal, once, side by side; the oracle is built and loaded before the threads start"""
    if "runs" not in _done:
        fz.po.build()
        fz.po.lib()
        with ThreadPoolExecutor(8) as ex:
            _done["runs"] = dict(zip(CASES, ex.map(_rehearse, CASES)))
    return _done["runs"]


def test_the_draws_of_the_cited_seeds_are_what_they_were():
    pins = _pins()
    assert [(e["seed"], e["round"], e["channels"]) for e, _ in pins] == [(s, r, C) for s, rs, C in RECORDED for r in rs]
    for e, now in pins:
        assert len(e["sha256"]) == e["channels"]
        changed = [c for c in range(e["channels"]) if now[c] != e["sha256"][c]]
        assert not changed, "seed %d round %d: the draws of channels %s changed" % (e["seed"], e["round"], changed[:20])


def test_the_variables_are_parsed_into_the_configuration_and_nowhere_else():
    env = dict(PSK_FUZZ_NONFINITE="0.05", PSK_FUZZ_EXTREME="0.1", PSK_FUZZ_MORE="1", PSK_FUZZ_S="2,4,100", PSK_FUZZ_CS16="0.3", PSK_FUZZ_CS8="0.2",
               PSK_FUZZ_CF16="0.1", PSK_FUZZ_QUALITY="1", PSK_FUZZ_FAR_FIT="0.5", PSK_FUZZ_STRICT="0", PSK_FUZZ_PACKET="4096", PSK_FUZZ_XD="0.01,0.5")
    cfg = fz.config_from_env(env)
    assert (cfg.nonfinite, cfg.extreme, cfg.more, cfg.s_choices, cfg.cs16, cfg.cs8, cfg.cf16, cfg.quality, cfg.far_fit, cfg.strict, cfg.packet,
            cfg.xd_choices) == (0.05, 0.1, True, (2, 4, 100), 0.3, 0.2, 0.1, True, 0.5, False, 4096, (0.01, 0.5))
    assert fz.config_from_env({}) == fz.Config() and fz.config_from_env(dict(PSK_FUZZ_MORE="0")).more is False
    assert fz.config_from_env(dict(PSK_FUZZ_QUALITY="1"), fz.CONFIGS["strided"][0]).entry == "strided"
    src = open(os.path.join(ROOT, "tools", "fuzz_gpu.py")).read()
    assert src.count("os.environ") == 1  # (main() hands it to config_from_env)


def test_a_new_kind_of_draw_leaves_the_others_as_they_were():
    """seed 7 round 0 with every later draw on: properties and scripts equal the default draw's, and so does the signal of every
    channel that stays float32"""
    base = fz.draw_round(7, 0, 40, fz.Config())
    cfg = fz.Config(entry="tuned", layout=True, looks=0.5, cs16=0.25, cs8=0.25, cf16=0.25, far_fit=0.0)
    rd = fz.draw_round(7, 0, 40, cfg)
    assert rd.props == base.props and rd.scripts == base.scripts
    same = [c for c in range(40) if rd.formats[c] is None]
    assert same and all(np.array_equal(rd.sigs[c].view(np.uint32), base.sigs[c].view(np.uint32)) for c in same)
    assert {f for f in rd.formats if f} & {"cf16", "rot4"} and any(t is not None for t in rd.tunes) and any(p is not None for p in rd.layout)


@pytest.mark.parametrize("case", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_the_draw_respects_limits_and_preconditions(case):
    rd, tk, _, _ = _runs()[case]
    cfg, lim = rd.cfg, rd.limits
    P = pl.acquire_piece()
    assert cfg.piece == P  # (the draw takes the piece length from its configuration, not from the library)
    assert rd.C <= 160 and all(t["packets"] and len(t["packets"]) == rd.C for t in tk)
    for c, place in enumerate(rd.layout):
        if place is not None:
            assert cfg.entry != "host" and 0 <= place[1] < rd.widths[place[0]] and rd.widths[place[0]] in fz.WIDTHS
    runs = {}
    for c, place in enumerate(rd.layout):
        if place is not None:
            runs.setdefault(place[0], []).append((c, place[1]))
    for m, cols in runs.items():  # adjacent channels in adjacent columns, 1 .. 12 of them
        assert 1 <= len(cols) <= 12 and all(b[0] - a[0] == 1 and b[1] - a[1] == 1 for a, b in zip(cols, cols[1:])), (m, cols)
    for t, tick in enumerate(tk):
        for c, p in enumerate(tick["packets"]):
            cur = tick["props"][c]
            assert cur["samplesPerBaud"] * cur["numAvg"] <= lim["max_window_samples"], (t, c, cur)
            assert cur["phaseAvg"] <= lim["max_phase_avg"] and cur["phaseAvg"] <= (65535 if cfg.far_fit else 32640), (t, c, cur)
            if p is None:
                continue
            n = p["data"].size // 2
            assert 1 <= n <= lim["max_packet_complex"] and p["data"].size == 2 * n and p["model"].dtype == np.float32 and p["model"].size == 2 * n
            assert p["mode"] in (0, 1) and (cfg.real or p["mode"] == 1)
            assert p["tune"] == (0, 0) or cfg.entry == "tuned"
            if p["tune"] != (0, 0):  # the next phase word: a plain 64-bit product, the library's and the model's
                ph, step = p["tune"]
                assert pl.tune_advance(ph, step, n) == (ph + step * n) % (1 << 64) == tm.advance(ph, step, n)
        for m, cols in runs.items():  # the channels of a matrix share a format within a call
            assert len({tick["packets"][c]["data"].dtype for c, _ in cols if tick["packets"][c] is not None}) <= 1, (t, m)
        if tick["look"] is not None:
            ch0, items, place, widths, tunes = tick["look"]
            assert 0 <= ch0 and ch0 + len(items) <= rd.C and (tunes is None or len(tunes) == len(items))
            by_m = {}
            for i, x in enumerate(items):
                if place[i] is not None:
                    assert 0 <= place[i][1] < widths[place[i][0]]
                    if x is not None:
                        by_m.setdefault(place[i][0], set()).add(x.dtype)
                assert x is None or 1 <= x.size // 2 <= 2 * P + 130
            assert all(len(v) == 1 for v in by_m.values())
    if cfg.entry == "tuned":  # the carried phase words: a tuned channel's consecutive packets continue each other unless redrawn
        carried = redrawn = 0
        for c in range(rd.C):
            t = rd.tunes[c]
            pk = [e for e in rd.scripts[c] if e[0] == "packet"]
            for i in range(1, len(pk) if t else 0):
                ok = t[i][0] == (t[i - 1][0] + t[i - 1][1] * (pk[i - 1][2] - pk[i - 1][1])) % (1 << 64)
                carried, redrawn = carried + ok, redrawn + (not ok)
        assert carried > redrawn > 0, (carried, redrawn)


def _planned_sequential(rd, tk):
    """channels the plan sends to the reference-order kernel, per tick: a control-plane handle fed the lengths of the round"""
    fmt = {fz.F32: pl.FORMAT_CF32, fz.I16: pl.FORMAT_CS16, fz.I8: pl.FORMAT_CS8, fz.F16: pl.FORMAT_CF16}
    h = pl.Handle(rd.C, device=pl.DEVICE_NONE, **rd.limits)
    try:
        h.configure(0, rd.props)
        if rd.options["far_fit"]:
            h.set_option(pl.Handle.OPT_FAR_FIT, 1)
        out = []
        for tick in tk:
            for c, key, val in tick["sets"]:
                h.configure(c, [{key: val}])
            h.plan_only(0, [None if p is None else dict(n_floats=p["data"].size, xdelta=p["xdelta"], mode=p["mode"], sriChanged=p["sriChanged"],
                                                        inputQueueFlushed=p["inputQueueFlushed"], format=fmt[p["data"].dtype]) for p in tick["packets"]])
            out.append(h.stats()["channels_sequential"])
        return out
    finally:
        h.close()


@pytest.mark.parametrize("case", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_the_draw_reaches_what_the_case_is_named_for(case):
    """the counts behind the reached-path assertions of tests/test_gpu_randomised.py, from the draw and the oracle alone"""
    rd, tk, (ref, look_models), facts = _runs()[case]
    name, cfg = case[0], rd.cfg
    assert len(ref) == rd.C and all(len(rows) == len(tk) for rows in ref)
    assert sum(r["soft"].size for rows in ref for r in rows if r is not None) > 1000 * rd.C  # (the round emits)
    if cfg.cs16 and cfg.cs8 and cfg.cf16:
        assert all(facts["sent"].get(f, 0) > 0 for f in ("cf32", "cs16", "cs8", "cf16")), facts["sent"]
        assert {"all", "alt", "cs8", "rot", "cf16", "rot4"} <= set(rd.formats)
    if name == "formats":  # half infinities and half NaNs reach the library in packets sent as CF16 throughout
        half = [c for c in range(rd.C) if rd.formats[c] == "cf16"]
        assert any(np.isinf(rd.sigs[c]).any() for c in half) and any(np.isnan(rd.sigs[c]).any() for c in half)
        assert all(rd.sigs[c].dtype == np.float16 and float(np.abs(rd.sigs[c][np.isfinite(rd.sigs[c])]).max()) <= 65504.0 for c in half)
        sent = [p["data"] for tick in tk for c, p in enumerate(tick["packets"]) if p is not None and c in half]
        assert all(x.dtype == np.float16 for x in sent) and any(np.isinf(x).any() for x in sent) and any(np.isnan(x).any() for x in sent)
    if cfg.layout:
        assert sum(facts["tiles"]) > 0 and sum(facts["singles"]) > 0, facts
        assert any(p is None for p in rd.layout) and any(None in t["packets"] for t in tk)
    if cfg.entry == "tuned":
        assert all(n > 0 for n in facts["tuned"][:2]), facts["tuned"]
        steps = {t[0][1] for t in rd.tunes if t}
        assert 0 in steps and 1 in steps and any(s > 1 << 63 for s in steps) and any(t is None for t in rd.tunes)
    if cfg.looks:
        assert facts["looked"] > 0 and sorted(look_models) == sorted(rd.looks)
        assert any(m["flags"] & pl.A_TUNED for ms in look_models.values() for m in ms)
    if cfg.far_fit:
        far = [c for c in range(rd.C) for t, tick in enumerate(tk)
               if tick["props"][c]["phaseAvg"] > 32640 and ref[c][t] is not None and ref[c][t]["soft"].size]
        assert len(set(far)) >= 2, far
        assert _planned_sequential(rd, tk) == [0] * len(tk)
    if cfg.real:
        real = [p for tick in tk for p in tick["packets"] if p is not None and p["mode"] == 0]
        assert any(p["inputQueueFlushed"] for p in real) and any(not p["inputQueueFlushed"] for p in real)
    if cfg.extreme:
        peaks = [float(np.abs(s[np.isfinite(s)]).max()) for s in rd.sigs if s.dtype == np.float32 and np.isfinite(s).any()]
        assert max(peaks) > 1e9 or min(peaks) < 1e-17
        assert any(not np.isfinite(s).all() for s in rd.sigs)
        assert any(p["samplesPerBaud"] > 33 for p in rd.props)
        assert any(e[0] == "set" and e[1] == "samplesPerBaud" for ev in rd.scripts for e in ev)
    if cfg.crowded:
        classes = {}
        for c, p in enumerate(rd.props):
            classes.setdefault((p["samplesPerBaud"], p["numAvg"], rd.formats[c]), []).append(c)
        assert len(classes) == cfg.crowded and all(len(v) >= 65 for v in classes.values())
        A = sorted(k[1] for k in classes)
        assert A[0] <= 128 < A[1] <= 256 and all(2 <= k[0] <= 16 for k in classes)
        assert len(tk) == 3 and all(None not in t["packets"] for t in tk)
        # eligible for the cut and the deferred join: no packet a conversion pre-pass would take (CS16 calls are neither cut nor
        # deferred where one converts them); the formats read in place go with numAvg up to 128
        assert all(f in (None, "cs8", "cf16") for f in rd.formats)
        assert all(rd.props[c]["numAvg"] <= 128 for c in range(rd.C) if rd.formats[c] is not None)
        assert all(p["phaseAvg"] <= 1920 and p["constelationSize"] in (2, 4, 8) for p in rd.props)
        first = [ref[c][0]["soft"].size // 2 for c in range(rd.C)]
        assert 128 * 128 <= min(first) and max(first) < 192 * 128, (min(first), max(first))  # (cut in time, not time-tiled)
    if name == "crowded_deferred":
        assert any(f is not None for f in rd.formats)  # (a class read in place)
