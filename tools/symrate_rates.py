#!/usr/bin/env python3
"""symrate_rates.py -- what one look of psk_soft_symrate_device costs on one MI355X, next to the demodulator call and the
carrier look on the same packets: everything resident in HBM, everything on ONE stream, every step between two HIP events on that
stream, medians over --steps steps after --warmup.

Per shape (channels x samples) and format (cf32 / sc16 / sc8; int8 values, round(40 x), cast), QPSK, samplesPerBaud 8, contiguous:

  t_contig    psk_soft_process_device of the packets (the ordinary call)
  t_acquire   psk_soft_acquire_device of the same packets (it reads all of them)
  t_symrate   psk_soft_symrate_device of the same packets (it reads the first min(n, 4096 x samplesPerBaud) samples of each),
              with the samples it looks at per second
  t_symrate_tuned   the same, every packet tuned

and one frame-major group (--group-nsamp samples of every channel, adjacent columns of one matrix): t_symrate of the columns,
which go through the tile gather first, next to t_symrate of the contiguous rows.
The records of a few channels of the first look are checked against psk_soft_symrate_host on the same samples (derived values
within 1e-9 relative).  One JSON object on stdout (and in --out).

    python tools/symrate_rates.py [--steps 10] [--warmup 3] [--formats cf32,sc16,sc8] [--out FILE.json]
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

MAX_BLOCKS = 4096


def host_check(pl, np, h, data, channels):
    """the device's derived values of `channels` against psk_soft_symrate_host of the same samples (cast to float32)"""
    worst = 0.0
    for c in channels:
        rec = h.symrate_records(c, 1)[0]
        want = pl.symrate_derive(pl.symrate_host(S, data[c].cpu().numpy().astype(np.float32)))
        got = pl.symrate_derive(rec)
        if got["lags_used"] != want["lags_used"] or got["detector"] != want["detector"] or not rec.n_valid:
            return False, float("nan")
        worst = max(worst, abs(got["samples_per_symbol"] / want["samples_per_symbol"] - 1.0))
    return worst <= 1e-9, worst


def run_shape(pl, torch, np, iq8, fmt, tdt, steps, warmup):
    dev = iq8.device
    C, N = iq8.shape[0], iq8.shape[1] // 2
    cap = (N // S + 2 + 63) // 64 * 64
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    data = iq8.to(tdt).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    used = min(N, MAX_BLOCKS * S) // S * S
    res = {"shape": [C, N], "sample_bytes": sb, "samples_looked_at": used}
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
    pk0 = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, True)
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, False)
    o = Outs(pl, torch, C, cap, dev)
    h.process_device(0, pk0, o.out, raw)
    h.synchronize()
    res["t_contig"] = timed(torch, st, lambda: h.process_device(0, pk, o.out, raw), steps, warmup)
    res["t_acquire"] = timed(torch, st, lambda: h.acquire_device(0, pk, None, None, raw), steps, warmup)
    h.symrate_device(0, pk, None, None, raw)
    res["derived_equal_host"], res["derived_worst_difference"] = host_check(pl, np, h, data, sorted({0, 1, C // 2, C - 1}))
    res["t_symrate"] = timed(torch, st, lambda: h.symrate_device(0, pk, None, None, raw), steps, warmup)
    tunes = (pl.Tune * C)(*[pl.Tune((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), pl.tune_step(-0.00625)) for c in range(C)])
    res["t_symrate_tuned"] = timed(torch, st, lambda: h.symrate_device(0, pk, None, tunes, raw), steps, warmup)
    h.synchronize()
    h.close()
    res["samples_per_s"] = C * used / (res["t_symrate"]["median_ms"] * 1e-3)
    res["ratio_symrate_over_contig"] = res["t_symrate"]["median_ms"] / res["t_contig"]["median_ms"]
    res["ratio_symrate_over_acquire"] = res["t_symrate"]["median_ms"] / res["t_acquire"]["median_ms"]
    return res


def run_group(pl, torch, iq8, fmt, tdt, steps, warmup):
    """all channels as adjacent columns of one frame-major matrix: the look at the columns (gathered, then folded), next to the look at the rows"""
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
    h.symrate_device(0, pk_c, None, None, raw)
    want = bytes(h.symrate_records())
    h.symrate_device(0, pk_s, strides, None, raw)
    res["records_identical"] = bytes(h.symrate_records()) == want
    res["t_symrate_contig"] = timed(torch, st, lambda: h.symrate_device(0, pk_c, None, None, raw), steps, warmup)
    res["t_symrate_group"] = timed(torch, st, lambda: h.symrate_device(0, pk_s, strides, None, raw), steps, warmup)
    h.synchronize()
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp", default="262144,32768,4096", help="samples per channel of the contiguous shapes")
    ap.add_argument("--group-nsamp", type=int, default=1 << 15)
    ap.add_argument("--group-format", default="sc16")
    ap.add_argument("--formats", default="cf32,sc16,sc8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("symrate_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    result = {"tool": "symrate_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "piece_blocks": pl.symrate_piece(),
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
    ok = all(v["derived_equal_host"] for s in result["shapes"].values() for v in s.values())
    return 0 if ok and result.get("frame_major_group", {}).get("records_identical", True) else 1


if __name__ == "__main__":
    sys.exit(main())
