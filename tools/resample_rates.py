#!/usr/bin/env python3
"""resample_rates.py -- what the resample pass of psk_soft_process_device_resampled costs on one MI355X, NEXT TO the tune pass
on the same packets in the same run: contiguous packets resident in HBM, everything on ONE stream, every step between two HIP
events on that stream, medians over --steps steps after --warmup.

Per format (cf32 / sc16 / sc8 / cf16; int8 values, round(40 x), cast), on handles created under PSK_SOFT_DIAG_GATHER_ONLY=1 (the
pre-pass runs, the ordinary call behind it is left out):

  t_tune              the tune pass alone: every packet tuned, none resampled (psk_tune_kernel)
  t_resample          the resample pass alone: every packet resampled at --ratio input samples per output, none tuned
  t_resample_tuned    the resample pass with the NCO inside it: every packet tuned and resampled (still one launch)

each with the bytes it reads and writes per second: the tune pass reads every sample once and writes one float2 for it; the
resample pass reads every sample once and writes one float2 per OUTPUT (n_out = about n / ratio).  No rate is fixed in advance:
the tune pass of the same run is the figure to stand beside.
A few channels of a full resampled-and-tuned call are checked against psk_soft_tune_apply + psk_soft_resample_apply on the host
fed through psk_soft_process_device: the same bits out.
One JSON object on stdout (and in --out).

    python tools/resample_rates.py [--steps 10] [--warmup 3] [--formats sc16] [--ratio 1.04625] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import M, NPH, S, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402
from strided_rates import Outs, timed  # noqa: E402
from tune_rates import _formats  # noqa: E402


def host_check(pl, torch, data, fmt, tunes, rss, numavg, channels, n_check):
    """the first n_check samples of `channels` through a full tuned and resampled call, against the CF32 packets the host-side
    definitions make of them, through psk_soft_process_device"""
    dev = data.device
    C = len(channels)
    rows, n_out = [], []
    for c in channels:
        x = data[c, : 2 * n_check].to(torch.float32).cpu().numpy()
        y, _ = pl.resample_apply((rss[c].pos, rss[c].step, pl.RS_RESTART), pl.tune_apply(tunes[c].phase, tunes[c].step, x))
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
            pk = packets(pl, C, lambda i: sub.data_ptr() + i * row, 2 * n_check, fmt, True)
            h.process_device_resampled(0, pk, None, [(tunes[c].phase, tunes[c].step) for c in channels],
                                       [(rss[c].pos, rss[c].step, pl.RS_RESTART) for c in channels], got.out)
        else:
            pk = packets(pl, C, lambda i: rows[i].data_ptr(), 0, pl.FORMAT_CF32, True)
            for i in range(C):
                pk[i].n_floats = 2 * n_out[i]
                pk[i].sri_xdelta = 0.01 * (rss[channels[i]].step * 2.0 ** -32)
            h.process_device(0, pk, want.out)
        h.synchronize()
        h.close()
    ok = all(int(got.out[i].n_symbols) == int(want.out[i].n_symbols) > 0 for i in range(C))
    return ok and got.same(torch, want)


def run_format(pl, torch, iq8, name, fmt, tdt, numavg, cycles, ratio, steps, warmup):
    dev = iq8.device
    C, N = iq8.shape[0], iq8.shape[1] // 2
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    data = iq8.to(tdt).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    tstep, rstep = pl.tune_step(cycles), pl.resample_step(ratio)
    tunes = (pl.Tune * C)(*[pl.Tune((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), tstep) for c in range(C)])
    rss = (pl.Resample * C)(*[pl.Resample((0x9E3779B1 * (c + 1)) % rstep, rstep, 0, 0) for c in range(C)])
    n_out = sum(pl.resample_count(rss[c], N) for c in range(C))
    res = {"shape": [C, N], "sample_bytes": sb, "outputs": n_out}
    res["first_step_identical"] = host_check(pl, torch, data, fmt, tunes, rss, numavg, sorted({0, 1, C // 2, C - 1}), min(N, 1 << 14))

    os.environ["PSK_SOFT_DIAG_GATHER_ONLY"] = "1"
    h = pl.Handle(C, device=0)
    os.environ.pop("PSK_SOFT_DIAG_GATHER_ONLY")
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=numavg, phaseAvg=NPH)
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, False)
    outs = (pl.Output * C)()  # (never looked at: the ordinary call is left out)
    # (the positions and phase words stay put from step to step: the pass costs the same wherever in the stream it stands)
    for key, tn, rs, moved in (("t_tune", tunes, None, C * N * (sb + 8)), ("t_resample", None, rss, C * N * sb + 8 * n_out),
                               ("t_resample_tuned", tunes, rss, C * N * sb + 8 * n_out)):
        res[key] = timed(torch, st, lambda: h.process_device_resampled(0, pk, None, tn, rs, outs, raw), steps, warmup)
        res[key]["bytes_read_plus_written"] = moved
        res[key]["tb_per_s"] = moved / (res[key]["median_ms"] * 1e-3) / 1e12
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp", type=int, default=1 << 18)
    ap.add_argument("--numavg", type=int, default=200)
    ap.add_argument("--cycles", type=float, default=-0.00625, help="shift in cycles per sample")
    ap.add_argument("--ratio", type=float, default=8.37 / 8, help="input samples per output sample")
    ap.add_argument("--formats", default="cf32,sc16,sc8,cf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("resample_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    result = {"tool": "resample_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "cycles_per_sample": args.cycles,
              "in_per_out": args.ratio, "piece": pl.resample_piece(),
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=args.numavg, phaseAvg=NPH), "steps": args.steps,
              "warmup": args.warmup, "timing": "HIP events on one stream around every step; medians", "formats": {}}
    iq8 = quantise_torch(synth_channels_torch(args.channels, M, S, args.nsamp, dev)).contiguous()
    for name, fmt, tdt in _formats(pl, torch):
        if name not in args.formats.split(","):
            continue
        result["formats"][name] = run_format(pl, torch, iq8, name, fmt, tdt, args.numavg, args.cycles, args.ratio, args.steps, args.warmup)
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
