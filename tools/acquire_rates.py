#!/usr/bin/env python3
"""acquire_rates.py -- what one look of psk_soft_acquire_device costs on one MI355X, next to the demodulator call on the same
packets: everything resident in HBM, everything on ONE stream, every step between two HIP events on that stream, medians over
--steps steps after --warmup.

Per shape (channels x samples) and format (cf32 / sc16 / sc8; int8 values, round(40 x), cast), QPSK, samplesPerBaud 8, contiguous:

  t_contig    psk_soft_process_device of the packets (the ordinary call)
  t_acquire   psk_soft_acquire_device of the same packets, with the samples it looks at per second
  t_acquire_tuned   the same, every packet tuned

and one frame-major group (--group-nsamp samples of every channel, adjacent columns of one matrix): t_acquire of the columns,
which go through the tile gather first, next to t_acquire of the contiguous rows.  The condition the pass was built to is t_acquire <= 2 x t_contig: the
smallest search over `step` that watches `lock` is two trial demodulator calls.
The derived offsets of a few channels of the first look are checked against psk_soft_acquire_host on the same samples.
One JSON object on stdout (and in --out).

    python tools/acquire_rates.py [--steps 10] [--warmup 3] [--formats cf32,sc16,sc8] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import A, M, NPH, S, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402
from strided_rates import Outs, _formats, timed  # noqa: E402


def host_check(pl, np, h, data, channels):
    """the device's derived offsets of `channels` against psk_soft_acquire_host of the same samples (cast to float32)"""
    worst = 0.0
    for c in channels:
        rec = h.acquire_records(c, 1)[0]
        want = pl.acquire_derive(pl.acquire_host(M, data[c].cpu().numpy().astype(np.float32)))
        got = pl.acquire_derive(rec)
        if got["lags_used"] != want["lags_used"] or not rec.n_valid:
            return False, float("nan")
        worst = max(worst, abs(got["offset_cycles_per_sample"] - want["offset_cycles_per_sample"]))
    return worst <= 1e-12, worst


def run_shape(pl, torch, np, iq8, fmt, tdt, steps, warmup):
    dev = iq8.device
    C, N = iq8.shape[0], iq8.shape[1] // 2
    cap = (N // S + 2 + 63) // 64 * 64
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    data = iq8.to(tdt).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    res = {"shape": [C, N], "sample_bytes": sb}
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
    pk0 = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, True)
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, False)
    o = Outs(pl, torch, C, cap, dev)
    h.process_device(0, pk0, o.out, raw)
    h.synchronize()
    res["t_contig"] = timed(torch, st, lambda: h.process_device(0, pk, o.out, raw), steps, warmup)
    h.acquire_device(0, pk, None, None, raw)
    res["offsets_equal_host"], res["offset_worst_difference"] = host_check(pl, np, h, data, sorted({0, 1, C // 2, C - 1}))
    res["t_acquire"] = timed(torch, st, lambda: h.acquire_device(0, pk, None, None, raw), steps, warmup)
    tunes = (pl.Tune * C)(*[pl.Tune((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), pl.tune_step(-0.00625)) for c in range(C)])
    res["t_acquire_tuned"] = timed(torch, st, lambda: h.acquire_device(0, pk, None, tunes, raw), steps, warmup)
    h.synchronize()
    h.close()
    res["samples_per_s"] = C * N / (res["t_acquire"]["median_ms"] * 1e-3)
    res["read_tb_per_s"] = C * N * sb / (res["t_acquire"]["median_ms"] * 1e-3) / 1e12
    res["ratio_acquire_over_contig"] = res["t_acquire"]["median_ms"] / res["t_contig"]["median_ms"]
    res["within_two_calls"] = res["ratio_acquire_over_contig"] <= 2.0
    return res


def run_group(pl, torch, iq8, fmt, tdt, steps, warmup):
    """all channels as adjacent columns of one frame-major matrix: the look at the columns (gathered, then folded), next to the look at the rows"""
    dev = iq8.device
    C, N = iq8.shape[0], iq8.shape[1] // 2
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    contig = iq8.to(tdt).contiguous()
    frame = contig.view(C, N, 2).permute(1, 0, 2).contiguous()  # [frame][column][I, Q]
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
    row = contig.stride(0) * contig.element_size()
    pk_c = packets(pl, C, lambda c: contig.data_ptr() + c * row, 2 * N, fmt, False)
    pk_s = packets(pl, C, lambda c: frame.data_ptr() + sb * c, 2 * N, fmt, False)
    strides = (pl.ctypes.c_uint64 * C)(*([C] * C))
    res = {"shape": [C, N], "sample_bytes": sb, "matrix_width": C}
    h.acquire_device(0, pk_c, None, None, raw)
    want = bytes(h.acquire_records())
    h.acquire_device(0, pk_s, strides, None, raw)
    res["records_identical"] = bytes(h.acquire_records()) == want
    res["t_acquire_contig"] = timed(torch, st, lambda: h.acquire_device(0, pk_c, None, None, raw), steps, warmup)
    res["t_acquire_group"] = timed(torch, st, lambda: h.acquire_device(0, pk_s, strides, None, raw), steps, warmup)
    h.synchronize()
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp", default="262144,4096", help="samples per channel of the contiguous shapes")
    ap.add_argument("--group-nsamp", type=int, default=1 << 16)
    ap.add_argument("--group-format", default="sc16")
    ap.add_argument("--formats", default="cf32,sc16,sc8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("acquire_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    result = {"tool": "acquire_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "piece": pl.acquire_piece(),
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH), "steps": args.steps, "warmup": args.warmup,
              "timing": "HIP events on one stream around every step; medians", "shapes": {}}
    fmts = {name: (fmt, tdt) for name, fmt, tdt, _ in _formats(pl, torch)}
    for n in [int(v) for v in args.nsamp.split(",")]:
        iq8 = quantise_torch(synth_channels_torch(args.channels, M, S, n, dev)).contiguous()
        shape = result["shapes"]["%dx%d" % (args.channels, n)] = {}
        for name in args.formats.split(","):
            shape[name] = run_shape(pl, torch, np, iq8, fmts[name][0], fmts[name][1], args.steps, args.warmup)
            torch.cuda.empty_cache()
        del iq8
    if args.group_nsamp:
        iq8 = quantise_torch(synth_channels_torch(args.channels, M, S, args.group_nsamp, dev)).contiguous()
        fmt, tdt = fmts[args.group_format]
        result["frame_major_group"] = dict(run_group(pl, torch, iq8, fmt, tdt, args.steps, args.warmup), format=args.group_format)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(v["offsets_equal_host"] for s in result["shapes"].values() for v in s.values())
    return 0 if ok and result.get("frame_major_group", {}).get("records_identical", True) else 1


if __name__ == "__main__":
    sys.exit(main())
