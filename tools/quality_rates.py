#!/usr/bin/env python3
"""quality_rates.py -- what PSK_SOFT_OPT_QUALITY costs on one MI355X: the same device-resident calls with the option off and on,
alternating in one process, timed with events on the caller's stream (the pass runs there, behind the call).

Shapes (QPSK, samplesPerBaud 8, numAvg 100, phaseAvg 50, packets and rows resident in HBM, rows on 128-byte boundaries):

  headline    4096 channels x 2^18 samples
  one         1 channel x 2^20 samples      (the calls where two more launches weigh most)
  few         64 channels x 2^20 samples

Per shape: median and spread of the off and the on step in ms, their difference (the pass as the step sees it), the bytes the pass
reads (10 a symbol: soft 8, sampleIndex 2) and psk_soft_probe_read_ms over as many bytes -- the read ceiling the pass is held
against.  The records of the on handle are compared with the model (tests/quality_model.py) on two channels of the first step.
With --pass-only the tool just runs `steps` on-steps of one shape: the run to put under a kernel trace for the kernel times
of quality_fold and quality_join by themselves.  One JSON object on stdout (and in --out).

    python tools/quality_rates.py [--steps 10] [--warmup 3] [--shapes headline,one,few] [--out FILE] [--pass-only SHAPE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from cs16_rates import A, M, NPH, S, outputs, packets  # noqa: E402

SHAPES = {"headline": (4096, 1 << 18), "one": (1, 1 << 20), "few": (64, 1 << 20)}


def run_shape(pl, torch, name, steps, warmup, pass_only=False):
    from psk_soft_amd.stimulus import synth_channels_torch
    from tests import quality_model as qm

    C, N = SHAPES[name]
    dev = torch.device("cuda", 0)
    src = synth_channels_torch(C, M, S, N, dev).contiguous()
    cap = (N // S + 2 + 63) // 64 * 64
    soft = torch.empty((C, 2 * cap), dtype=torch.float32, device=dev)
    phase = torch.empty((C, cap), dtype=torch.float32, device=dev)
    sidx = torch.empty((C, cap), dtype=torch.int16, device=dev)
    bits = torch.empty((C, 2 * cap), dtype=torch.int16, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    row, base = src.stride(0) * src.element_size(), src.data_ptr()
    out = outputs(pl, C, cap, lambda c: soft[c].data_ptr(), lambda c: bits[c].data_ptr(), lambda c: phase[c].data_ptr(),
                  lambda c: sidx[c].data_ptr())
    pk0 = packets(pl, C, lambda c: base + c * row, 2 * N, 0, True)
    pk = packets(pl, C, lambda c: base + c * row, 2 * N, 0, False)
    handles = {}
    for mode in ("on",) if pass_only else ("off", "on"):
        h = pl.Handle(C, device=0, max_packet_complex=N)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
        if mode == "on":
            h.set_option(pl.Handle.OPT_QUALITY, 1)
        h.process_device(0, pk0, out, stream.cuda_stream)
        h.synchronize()
        handles[mode] = h
    res = {"shape": [C, N]}
    n_sym = int(out[0].n_symbols)
    # the records of the first step against the model
    recs = handles["on"].quality_records()
    torch.cuda.synchronize()
    ok = True
    for c in (0, C - 1):
        g = dict(soft=soft[c, : 2 * n_sym].cpu().numpy(), phase=phase[c, :n_sym].cpu().numpy(), index=sidx[c, :n_sym].cpu().numpy())
        try:
            qm.assert_record(recs[c], qm.model_record(g["soft"], g["phase"], g["index"], M, S, 0), "channel %d" % c)
        except AssertionError as e:
            ok = False
            print("record differs from the model:", e, file=sys.stderr)
    res["records_ok"] = ok
    res["lock_channel0"] = pl.quality_derive(recs[0])["lock"]
    res["snr_db_channel0"] = pl.quality_derive(recs[0])["snr_db"]
    times = {m: [] for m in handles}
    for k in range(warmup + steps):
        for mode, h in handles.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h.process_device(0, pk, out, stream.cuda_stream)
            e1.record(stream)
            h.synchronize()
            stream.synchronize()
            if k >= warmup:
                times[mode].append(e0.elapsed_time(e1))
    for mode, t in times.items():
        res[mode + "_ms"] = statistics.median(t)
        res[mode + "_ms_min_max"] = [min(t), max(t)]
    if not pass_only:
        res["on_minus_off_ms"] = res["on_ms"] - res["off_ms"]
        res["on_over_off"] = res["on_ms"] / res["off_ms"]
        nbytes = 10 * n_sym * C
        res["pass_bytes"] = nbytes
        probe = torch.empty(((nbytes + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        res["probe_read_ms"] = handles["on"].probe_read_ms(probe.data_ptr(), probe.numel(), 5)
        res["pass_over_probe"] = res["on_minus_off_ms"] / res["probe_read_ms"] if res["probe_read_ms"] > 0 else None
    for h in handles.values():
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="headline,one,few")
    ap.add_argument("--pass-only", default=None, help="run only on-steps of this shape (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from psk_soft_amd import lib as pl

    if not torch.cuda.is_available():
        raise SystemExit("quality_rates.py measures on an MI355X; no GPU visible")
    result = {"tool": "quality_rates", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)}
    if args.pass_only:
        result[args.pass_only] = run_shape(pl, torch, args.pass_only, args.steps, args.warmup, pass_only=True)
    else:
        for name in args.shapes.split(","):
            result[name] = run_shape(pl, torch, name, args.steps, args.warmup)
            torch.cuda.empty_cache()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(v.get("records_ok", True) for v in result.values() if isinstance(v, dict) and "shape" in v) else 1


if __name__ == "__main__":
    sys.exit(main())
