#!/usr/bin/env python3
"""fir_rates.py -- what the filter pass of psk_soft_process_device_filtered costs on one MI355X, NEXT TO the tune pass on the
same packets in the same run: contiguous packets resident in HBM, everything on ONE stream, every step between two HIP events
on that stream, medians over --steps steps after --warmup.

Per format (cf32 / sc16; int8 values, round(40 x), cast), on handles created under PSK_SOFT_DIAG_GATHER_ONLY=1 (the pre-pass
runs, the ordinary call behind it is left out):

  t_tune              the tune pass alone: every packet tuned, none filtered (psk_tune_kernel)
  t_fir[T][D]         the filter pass alone: every packet filtered with T taps (8, 32, 128) and decimated by D (1, 2)

each with the bytes it reads and writes per second (the filter pass reads every sample once and writes one float2 per OUTPUT),
the filter pass also with its multiply-accumulates per second (2 T per output: re and im) and its time over the tune pass's.
No rate is fixed in advance: the tune pass of the same run, memory-bound, is the figure to stand beside.
A few channels of a full filtered call (32 taps, D = 2) are checked against psk_soft_fir_apply on the host fed through
psk_soft_process_device: the same bits out.
One JSON object on stdout (and in --out).

    python tools/fir_rates.py [--steps 10] [--warmup 3] [--formats cf32,sc16] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import M, NPH, S, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402
from strided_rates import Outs, timed  # noqa: E402
from tune_rates import _formats  # noqa: E402

TAPS = (8, 32, 128)
DECIMS = (1, 2)


def taps_of(T):
    """a unit-gain low-pass of T taps: a Hann-windowed boxcar (any finite taps cost the same)"""
    w = np.hanning(T + 2)[1:-1] if T > 2 else np.ones(T)
    return (w / w.sum()).astype(np.float32)


def host_check(pl, torch, data, fmt, numavg, channels, n_check, T, D):
    """the first n_check samples of `channels` through a full filtered call, against the CF32 packets the host-side definition
    makes of them, through psk_soft_process_device"""
    dev = data.device
    C = len(channels)
    h_t = taps_of(T)
    rows, n_out = [], []
    for c in channels:
        x = data[c, : 2 * n_check].to(torch.float32).cpu().numpy()
        y, _ = pl.fir_apply((1, D, D - 1, pl.FIR_RESTART), h_t, x)
        rows.append(torch.from_numpy(y).to(dev))
        n_out.append(y.size // 2)
    cap = (max(n_out) // S + 2 + 63) // 64 * 64  # (rows of every stream start aligned)
    got, want = Outs(pl, torch, C, cap, dev), Outs(pl, torch, C, cap, dev)
    sub = data[channels, : 2 * n_check].contiguous()
    row = sub.stride(0) * sub.element_size()
    for which in (0, 1):
        h = pl.Handle(C, device=0)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=numavg, phaseAvg=NPH)
        if which == 0:
            h.fir_define(0, h_t)
            pk = packets(pl, C, lambda i: sub.data_ptr() + i * row, 2 * n_check, fmt, True)
            h.process_device_filtered(0, pk, None, None, [(1, D, D - 1, pl.FIR_RESTART)] * C, None, got.out)
        else:
            pk = packets(pl, C, lambda i: rows[i].data_ptr(), 0, pl.FORMAT_CF32, True)
            for i in range(C):
                pk[i].n_floats = 2 * n_out[i]
                pk[i].sri_xdelta = 0.01 * float(D)
            h.process_device(0, pk, want.out)
        h.synchronize()
        h.close()
    ok = all(int(got.out[i].n_symbols) == int(want.out[i].n_symbols) > 0 for i in range(C))
    return ok and got.same(torch, want)


def run_format(pl, torch, iq8, name, fmt, tdt, numavg, cycles, steps, warmup):
    C, N = iq8.shape[0], iq8.shape[1] // 2
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    data = iq8.to(tdt).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    tstep = pl.tune_step(cycles)
    tunes = (pl.Tune * C)(*[pl.Tune((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), tstep) for c in range(C)])
    res = {"shape": [C, N], "sample_bytes": sb}
    res["first_step_identical"] = host_check(pl, torch, data, fmt, numavg, sorted({0, 1, C // 2, C - 1}), min(N, 1 << 14), 32, 2)

    os.environ["PSK_SOFT_DIAG_GATHER_ONLY"] = "1"
    h = pl.Handle(C, device=0)
    os.environ.pop("PSK_SOFT_DIAG_GATHER_ONLY")
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=numavg, phaseAvg=NPH)
    for slot, T in enumerate(TAPS):
        h.fir_define(slot, taps_of(T))
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, False)
    outs = (pl.Output * C)()  # (never looked at: the ordinary call is left out)
    moved = C * N * (sb + 8)
    res["t_tune"] = timed(torch, st, lambda: h.process_device_filtered(0, pk, None, tunes, None, None, outs, raw), steps, warmup)
    res["t_tune"]["bytes_read_plus_written"] = moved
    res["t_tune"]["tb_per_s"] = moved / (res["t_tune"]["median_ms"] * 1e-3) / 1e12
    res["t_fir"] = {}
    for slot, T in enumerate(TAPS):
        for D in DECIMS:
            firs = (pl.Fir * C)(*[pl.Fir(1 + slot, D, c % D, 0) for c in range(C)])
            n_out = sum(pl.fir_count(firs[c], N) for c in range(C))
            r = timed(torch, st, lambda: h.process_device_filtered(0, pk, None, None, firs, None, outs, raw), steps, warmup)
            moved = C * N * sb + 8 * n_out
            r.update(taps=T, decim=D, outputs=n_out, bytes_read_plus_written=moved, tb_per_s=moved / (r["median_ms"] * 1e-3) / 1e12,
                     gmac_per_s=2.0 * T * n_out / (r["median_ms"] * 1e-3) / 1e9, over_tune=r["median_ms"] / res["t_tune"]["median_ms"])
            res["t_fir"]["T%d_D%d" % (T, D)] = r
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp", type=int, default=1 << 18)
    ap.add_argument("--numavg", type=int, default=200)
    ap.add_argument("--cycles", type=float, default=-0.00625, help="shift in cycles per sample (the tune pass)")
    ap.add_argument("--formats", default="cf32,sc16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("fir_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    result = {"tool": "fir_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "cycles_per_sample": args.cycles,
              "pieces": {str(D): pl.fir_piece(D) for D in DECIMS},
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=args.numavg, phaseAvg=NPH), "steps": args.steps,
              "warmup": args.warmup, "timing": "HIP events on one stream around every step; medians", "formats": {}}
    iq8 = quantise_torch(synth_channels_torch(args.channels, M, S, args.nsamp, dev)).contiguous()
    for name, fmt, tdt in _formats(pl, torch):
        if name not in args.formats.split(","):
            continue
        result["formats"][name] = run_format(pl, torch, iq8, name, fmt, tdt, args.numavg, args.cycles, args.steps, args.warmup)
        torch.cuda.empty_cache()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(v["first_step_identical"] for v in result["formats"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
