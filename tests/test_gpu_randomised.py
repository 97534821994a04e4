"""The named configurations of tools/fuzz_gpu.py on a real MI355X: random rounds with fixed seeds through every entry
(psk_soft_process_host, _device_strided, _device_tuned, psk_soft_acquire_device between the calls), every packet format, layout
and handle option.  All four streams of every channel are, bit for bit, the oracle's on the packet's float32 cast (tuned by
tests/tune_model.py where the call tunes it); quality and acquire records are held to their models' own assert_record; the source
buffers come back as they were uploaded.  Every round runs twice, untraced and on a handle created with PSK_SOFT_TRACE_LAUNCHES=2
(a traced run waits for the device in front of every launch, which would hide a missing stream wait), both with
PSK_SOFT_VALIDATE=1, so that a bad plan is refused on the host and not launched.

Every case asserts that it reached what it is named for, from the launch lines and the statistics.  These are conditions of the
draw, not measurements: tests/test_fuzz_draws.py checks without a GPU that the seeds meet them.  A failure names the command that
replays that one round alone."""
import os
import sys

import pytest

from tests.test_gpu_cs16_schedules import rounds, screened, whats

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_gpu as fz  # noqa: E402

pytestmark = pytest.mark.gpu


def _message(findings):
    lines = ["%d findings; replay: %s" % (len(findings), findings[0]["replay"])]
    for f in findings[:12]:
        lines.append("round %d channel %d %s: %s  format=%s layout=%s props=%s script=%s" % (
            f["round"], f["channel"], f["stream"], f["what"], f.get("format"), f.get("layout"), f["props"], f["script"]))
        lines.extend(f.get("detail", []))
    return "\n".join(lines)


def _launches(info):
    return [t for lines in info["traces"] for t in lines]


def _reached_formats(rd, info):
    assert all(info["sent"].get(f, 0) > 0 for f in ("cf32", "cs16", "cs8", "cf16")), info["sent"]
    # ... and the library saw them: every integer and half format on the class that reads it in place (psk_ctl.h: kPktFormats) or
    # through its conversion pre-pass, float32 on a class of the float kernels
    lines = _launches(info)
    classes = {H for _, H in screened(lines)}
    for H, convert in ((3, "cs16_convert"), (5, "cs8_convert"), (6, "cf16_convert")):
        assert H in classes or convert in whats(lines), (H, classes, whats(lines))
    assert classes - {3, 5, 6}, classes


def _reached_strided(rd, info):
    assert {"gather_tiles", "gather_singles"} <= whats(_launches(info)), whats(_launches(info))


def _reached_tuned(rd, info):
    got = [sum(t["cnt"] for t in lines if t["what"] == "tune") for lines in info["traces"]]
    assert got == info["tuned"] and sum(got) > 0, (got, info["tuned"])


def _reached_looks(rd, info):
    seen = [t["what"] for lines in info["look_traces"] for t in lines]
    assert "acquire_fold" in seen and "acquire_join" in seen and info["looks_seen"] > 0, seen


def _reached_quality_far_fit(rd, info):
    far = [t for t in _launches(info) if t["what"].startswith("far_fit") and t["cnt"] > 0]
    assert far, whats(_launches(info))
    assert all(st["channels_sequential"] - st["channels_guard"] == 0 for st in info["stats"]), info["stats"]
    assert info["quality_seen"] > 0 and "quality_join" in whats(_launches(info))


def _reached_wide(rd, info):
    assert any(p["samplesPerBaud"] > 33 for p in rd.props) and any(0 in m for m in rd.modes)
    assert any(e[0] == "set" and e[1] == "samplesPerBaud" for ev in rd.scripts for e in ev)
    # samplesPerBaud beyond the instantiated 2 .. 32 runs on the front stage for any samplesPerBaud, not on the reference-order
    # kernel: its launches say how wide their widest symbol is
    wide = [t for t in _launches(info) if t["what"].startswith("tile_front_any") and t["S"] > 33]
    assert wide, sorted(whats(_launches(info)))
    # every channel that had a packet was carried by some kernel: the statistics count it
    assert all(st["channels_fast"] + st["channels_sequential"] > 0 for st in info["stats"]), info["stats"]
    assert len(info["channel_stats"]) == rd.C


def _reached_crowded(rd, info):
    first = [t for t in info["traces"][0] if not t["what"].startswith("gather_")]
    classes = screened(first)
    assert len(classes) == rd.cfg.crowded and rounds(first) > 1 and all(n > 1 for n in classes.values()), first
    assert all(st["channels_tiled"] == 0 and st["channels_fast"] > 0 for st in info["stats"]), info["stats"]


def _reached_crowded_deferred(rd, info):
    # (a deferred call: its classes end on their own streams, without the reference-order launch over the whole batch)
    assert len(info["traces"]) == 3 and len(info["stats"]) == 1  # (three calls back to back, then join)
    for lines in info["traces"]:
        assert len(screened(lines)) == rd.cfg.crowded and "seq (reference order)" not in whats(lines), lines
    assert info["stats"][0]["channels_tiled"] == 0 and info["stats"][0]["channels_fast"] > 0, info["stats"]


def _reached_everything(rd, info):
    for f in (_reached_formats, _reached_strided, _reached_tuned, _reached_looks, _reached_wide):
        f(rd, info)
    assert info["quality_seen"] > 0 and any(t["what"].startswith("far_fit") for t in _launches(info))


REACHED = dict(wide=_reached_wide, formats=_reached_formats, quality_far_fit=_reached_quality_far_fit, strided=_reached_strided,
               tuned=_reached_tuned, looks=_reached_looks, crowded=_reached_crowded, crowded_deferred=_reached_crowded_deferred,
               everything=_reached_everything)


@pytest.mark.parametrize("name", list(fz.CONFIGS))
def test_randomised_configuration(oracle_mod, monkeypatch, capfd, name):
    cfg, C, seeds = fz.CONFIGS[name]
    assert set(REACHED) == set(fz.CONFIGS)
    monkeypatch.setenv("PSK_SOFT_VALIDATE", "1")
    for seed, rnd in seeds:
        rd = fz.draw_round(seed, rnd, C, cfg)
        tk = fz.ticks(rd)
        ref = fz.reference(rd, tk)
        monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
        findings, info = fz.run_round(rd, tk, ref, None, name)
        assert not findings, _message(findings)
        monkeypatch.setenv("PSK_SOFT_TRACE_LAUNCHES", "2")
        try:
            capfd.readouterr()
            findings, traced = fz.run_round(rd, tk, ref, capfd, name)
        finally:
            monkeypatch.delenv("PSK_SOFT_TRACE_LAUNCHES", raising=False)
        assert not findings, "traced run: " + _message(findings)
        REACHED[name](rd, traced)
