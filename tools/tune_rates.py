#!/usr/bin/env python3
"""tune_rates.py -- what the frequency shift of psk_soft_process_device_tuned costs on one MI355X: tuned calls against untuned
calls on the same contiguous packets, resident in HBM, everything on ONE stream, every step between two HIP events on that
stream, medians over --steps steps after --warmup.

Per format (cf32 / sc16 / sc8 / cf16; int8 values, round(40 x), cast), QPSK, samplesPerBaud 8:

  t_untuned   psk_soft_process_device_tuned with tune = NULL (the ordinary call)
  t_tuned     the same packets, every one tuned (a step of --cycles cycles per sample, the phase word advanced from step to step)
  t_pass      the tune pass of t_tuned alone (a handle created under PSK_SOFT_DIAG_GATHER_ONLY=1), with the bytes it reads and
              writes per second

--numavg defaults to 200: a window class without in-place builds for the integer formats, so that the untuned sc16 call runs
the conversion pre-pass (psk_pkt_convert_kernel) -- the kernel with the same bytes in and out as the tune kernel on the same
packets.  Under `rocprofv3 --kernel-trace --stats -- python tools/tune_rates.py --formats sc16` the two show up side by side.
The first tuned step of a few channels is checked against psk_soft_tune_apply on the host: the same bits out.
One JSON object on stdout (and in --out).

    python tools/tune_rates.py [--steps 10] [--warmup 3] [--formats sc16] [--out FILE.json]
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


def _formats(pl, torch):
    return (("cf32", pl.FORMAT_CF32, torch.float32), ("sc16", pl.FORMAT_CS16, torch.int16), ("sc8", pl.FORMAT_CS8, torch.int8),
            ("cf16", pl.FORMAT_CF16, torch.float16))


def host_check(pl, torch, np, data, fmt, tunes, outs, numavg, channels):
    """channels of the first tuned step against the CF32 packets psk_soft_tune_apply makes of them on the host"""
    C, N = data.shape[0], data.shape[1] // 2
    cap = outs.soft.shape[1] // 2
    h = pl.Handle(len(channels), device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=numavg, phaseAvg=NPH)
    rows = torch.stack([torch.from_numpy(pl.tune_apply(tunes[c].phase, tunes[c].step, data[c].to(torch.float32).cpu().numpy()))
                        for c in channels]).to(data.device)
    o = Outs(pl, torch, len(channels), cap, data.device)
    pk = packets(pl, len(channels), lambda i: rows[i].data_ptr(), 2 * N, pl.FORMAT_CF32, True)
    h.process_device(0, pk, o.out)
    h.synchronize()
    h.close()
    ok = True
    for i, c in enumerate(channels):
        n = int(o.out[i].n_symbols)
        ok = ok and n == int(outs.out[c].n_symbols) and n > 0
        for a, b, k in ((o.soft, outs.soft, 2), (o.phase, outs.phase, 1), (o.sidx, outs.sidx, 1), (o.bits, outs.bits, 2)):
            x, y = a[i, : k * n], b[c, : k * n]
            ok = ok and bool(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y))
    return ok


def run_format(pl, torch, np, iq8, name, fmt, tdt, numavg, cycles, steps, warmup):
    dev = iq8.device
    C, N = iq8.shape[0], iq8.shape[1] // 2
    cap = (N // S + 2 + 63) // 64 * 64
    sb = 2 * torch.empty((), dtype=tdt).element_size()
    data = iq8.to(tdt).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    res = {"shape": [C, N], "sample_bytes": sb}
    step_word = pl.tune_step(cycles)
    tunes = (pl.Tune * C)(*[pl.Tune((0x9E3779B97F4A7C15 * (c + 1)) % (1 << 64), step_word) for c in range(C)])

    def handle(env=None):
        if env:
            os.environ[env] = "1"
        h = pl.Handle(C, device=0)
        if env:
            os.environ.pop(env)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=numavg, phaseAvg=NPH)
        return h

    pk0 = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, True)
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, fmt, False)

    def advance():
        for c in range(C):
            tunes[c].phase = pl.tune_advance(tunes[c].phase, step_word, N)

    # t_untuned
    h, o_u = handle(), Outs(pl, torch, C, cap, dev)
    h.process_device_tuned(0, pk0, None, None, o_u.out, raw)
    h.synchronize()
    res["t_untuned"] = timed(torch, st, lambda: h.process_device_tuned(0, pk, None, None, o_u.out, raw), steps, warmup)
    stt = h.stats()
    res["channels_fast"], res["channels_tiled"], res["channels_sequential"] = stt["channels_fast"], stt["channels_tiled"], stt["channels_sequential"]
    h.close()
    del o_u

    # t_tuned
    h, o_t = handle(), Outs(pl, torch, C, cap, dev)
    h.process_device_tuned(0, pk0, None, tunes, o_t.out, raw)
    h.synchronize()
    torch.cuda.synchronize()
    res["first_step_identical"] = host_check(pl, torch, np, data, fmt, tunes, o_t, numavg, sorted({0, 1, C // 2, C - 1}))
    advance()

    def tuned_step():
        h.process_device_tuned(0, pk, None, tunes, o_t.out, raw)
        advance()  # (host work of a real caller, outside the device's time line)

    res["t_tuned"] = timed(torch, st, tuned_step, steps, warmup)
    h.close()
    del o_t

    # t_pass
    h, o_p = handle("PSK_SOFT_DIAG_GATHER_ONLY"), Outs(pl, torch, C, cap, dev)
    res["t_pass"] = timed(torch, st, lambda: h.process_device_tuned(0, pk, None, tunes, o_p.out, raw), steps, warmup)
    h.close()
    del o_p

    moved = C * N * (sb + 8)  # the pass reads every sample once and writes one float2 for it
    res["pass_bytes_read_plus_written"] = moved
    res["pass_tb_per_s"] = moved / (res["t_pass"]["median_ms"] * 1e-3) / 1e12
    res["ratio_tuned_over_untuned"] = res["t_tuned"]["median_ms"] / res["t_untuned"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp", type=int, default=1 << 18)
    ap.add_argument("--numavg", type=int, default=200)
    ap.add_argument("--cycles", type=float, default=-0.00625, help="shift in cycles per sample")
    ap.add_argument("--formats", default="cf32,sc16,sc8,cf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("tune_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    result = {"tool": "tune_rates", "device": torch.cuda.get_device_name(0), "scale": 40.0, "cycles_per_sample": args.cycles,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=args.numavg, phaseAvg=NPH), "steps": args.steps,
              "warmup": args.warmup, "timing": "HIP events on one stream around every step; medians", "formats": {}}
    iq8 = quantise_torch(synth_channels_torch(args.channels, M, S, args.nsamp, dev)).contiguous()
    for name, fmt, tdt in _formats(pl, torch):
        if name not in args.formats.split(","):
            continue
        result["formats"][name] = run_format(pl, torch, np, iq8, name, fmt, tdt, args.numavg, args.cycles, args.steps, args.warmup)
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
