#!/usr/bin/env python3
"""far_fit_rates.py -- what PSK_SOFT_OPT_FAR_FIT buys: phaseAvg 40000 on the reference-order kernel (option 0, or a library built
from the commit before the option existed) against the far fit (option 1), on one MI355X, packets resident in HBM.

  a  one channel x 2^19 samples, QPSK, samplesPerBaud 8, numAvg 100, phaseAvg 40000, the fit window full (steady state)
  b  4096 channels x 2^16 samples, the same configuration at phaseAvg 50 -- but channel 0, which has phaseAvg 40000
  c  the batch of b with no far channel (phaseAvg 50 everywhere)

Every step is one psk_soft_process_device call timed with a pair of HIP events on the stream of the call; the median of --steps
steps after --warmup (at least six: the far window of b is full after five calls).  The far channel's outputs of the last step are
compared with the CPU oracle run over the same calls (a, b).  One JSON object on stdout (and in --out).

    python tools/far_fit_rates.py [--far 0|1|none] [--lib FILE.so] [--cases a,b,c] [--steps 10] [--warmup 6] [--out FILE]

--far none leaves the option alone (a library without it); --lib measures another build of the library, e.g. the parent
commit's, copied into the tree in front of the run as tools/ab_libs.sh expects its libraries.
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

from cs16_rates import outputs, packets  # noqa: E402

S, M, A, N_NEAR, N_FAR = 8, 4, 100, 50, 40000
OPT_FAR_FIT = 7
STAT_KEYS = ("channels_fast", "channels_sequential", "channels_guard", "channels_tiled")


def run_case(pl, torch, C, N, far_channel, far_opt, steps, warmup, check):
    from psk_soft_amd.stimulus import synth_channels_torch

    dev = torch.device("cuda", 0)
    src = synth_channels_torch(C, M, S, N, dev, periodic=True).contiguous()
    cap = (N // S + 2 + 63) // 64 * 64
    soft = torch.empty((C, 2 * cap), dtype=torch.float32, device=dev)
    phase = torch.empty((C, cap), dtype=torch.float32, device=dev)
    sidx = torch.empty((C, cap), dtype=torch.int16, device=dev)
    bits = torch.empty((C, 2 * cap), dtype=torch.int16, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    h = pl.Handle(C, device=0, max_phase_avg=65535)
    if far_opt is not None:
        h.set_option(OPT_FAR_FIT, far_opt)
    props = [dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=(N_FAR if far_channel and c == 0 else N_NEAR)) for c in range(C)]
    h.configure(0, props)
    row, base = src.stride(0) * src.element_size(), src.data_ptr()
    out = outputs(pl, C, cap, lambda c: soft[c].data_ptr(), lambda c: bits[c].data_ptr(), lambda c: phase[c].data_ptr(),
                  lambda c: sidx[c].data_ptr())
    pk0 = packets(pl, C, lambda c: base + c * row, 2 * N, pl.FORMAT_CF32, True)
    pk = packets(pl, C, lambda c: base + c * row, 2 * N, pl.FORMAT_CF32, False)
    h.process_device(0, pk0, out, stream.cuda_stream)
    for _ in range(warmup - 1):
        h.process_device(0, pk, out, stream.cuda_stream)
    stream.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h.process_device(0, pk, out, stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = h.stats()
    res = {"shape": [C, N], "ms_per_step": statistics.median(ms), "ms_min_max": [min(ms), max(ms)],
           "symbols_per_s_of_channel_0": (N // S) / (statistics.median(ms) * 1e-3), "stats": {k: st[k] for k in STAT_KEYS},
           "fit_len_channel_0": h.peek(0)["fit_len"]}
    if check:
        from oracle import pyoracle as po

        po.build()
        o = po.OracleComponent()
        for k, v in props[0].items():
            setattr(o, k, v)
        iq = src[0].cpu().numpy()
        for k in range(warmup + steps):
            r = o.service(iq, 0.01, sriChanged=(k == 0))
        ns = int(out[0].n_symbols)
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))  # noqa: E731
        res["oracle_ok"] = bool(ns == r.phase.size and same(soft[0, : 2 * ns].cpu().numpy(), r.soft) and same(phase[0, :ns].cpu().numpy(), r.phase) and
                                same(sidx[0, :ns].cpu().numpy(), r.index) and same(bits[0, : int(out[0].n_bits)].cpu().numpy(), r.bits))
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--far", default="1", choices=["0", "1", "none"])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from psk_soft_amd import lib as pl

    if args.lib:
        pl.LIB_PATH = os.path.abspath(args.lib)
    if not torch.cuda.is_available():
        raise SystemExit("far_fit_rates.py measures on an MI355X; no GPU visible")
    far_opt = None if args.far == "none" else int(args.far)
    warmup = max(args.warmup, 6)
    result = {"tool": "far_fit_rates", "device": torch.cuda.get_device_name(0), "lib": pl.LIB_PATH, "far_fit": args.far,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg_far=N_FAR, phaseAvg=N_NEAR), "steps": args.steps,
              "warmup": warmup}
    shapes = {"a": (1, 1 << 19, True), "b": (4096, 1 << 16, True), "c": (4096, 1 << 16, False)}
    for case in args.cases.split(","):
        C, N, far = shapes[case]
        result[case] = run_case(pl, torch, C, N, far, far_opt, args.steps, warmup, far and not args.no_check)
        torch.cuda.empty_cache()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(v.get("oracle_ok", True) for v in result.values() if isinstance(v, dict) and "shape" in v) else 1


if __name__ == "__main__":
    sys.exit(main())
