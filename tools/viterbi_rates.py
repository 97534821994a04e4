#!/usr/bin/env python3
"""viterbi_rates.py -- what psk_soft_viterbi_device costs on one MI355X, next to the demodulator call that wrote the soft rows and
to the demap call that made the LLRs it decodes: everything resident in HBM, everything on ONE stream, every step between two HIP
events on that stream, medians over --steps steps after --warmup.

One shape, --channels x --symbols QPSK soft symbols a channel (4096 x 32768), samplesPerBaud 8, sc16 packets (int8 values):

  t_process   psk_soft_process_device of the packets: --symbols x 8 samples a channel in, the four rows out
  t_demap     psk_soft_demap_device over the soft rows, one segment a row, int8: 2 LLRs a symbol, 65536 a channel
  t_viterbi   per code ("r12": K = 7 171/133 unpunctured; "r34": its rate 3/4), cut ("f4096": frames of 4096 steps, 8 a channel;
              "f32768": frames of 32768 steps, one a channel) and output form ("bytes", "packed"): psk_soft_viterbi_device over
              those LLRs (the values do not matter to the time), frames not terminated, with decoded bits per second and LLR
              bytes per second.  The time is the stream's: it holds the entry's own host work (one 32-byte descriptor a frame,
              checked, filled in and copied up) wherever the stream waits for it; t_host is the call's wall time on the host and
              host_share its part of the stream's time.  One wave decodes one frame, so the cut decides how many waves there are.

Outputs and records of a few frames are checked against psk_soft_viterbi_host on the downloaded LLRs, byte for byte.
One JSON object on stdout (and in --out).

    python tools/viterbi_rates.py [--steps 10] [--warmup 3] [--channels 4096] [--symbols 32768] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cs16_rates import A, M, NPH, S, packets  # noqa: E402
from cs8_rates import quantise_torch  # noqa: E402
from demap_rates import GAIN, SCALE, the_map  # noqa: E402
from strided_rates import Outs, timed  # noqa: E402

G = (0o171, 0o133)
CODES = {"r12": (0, 1, 0b11), "r34": (1, 3, 0b100111)}  # name: (slot, P, keep); 3/4: [1 1; 1 0; 0 1]
CUTS = {"f4096": 4096, "f32768": 32768}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--symbols", type=int, default=32768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("viterbi_rates.py measures on an MI355X; no GPU visible")
    dev = torch.device("cuda", 0)
    C, N = args.channels, args.symbols * S
    result = {"tool": "viterbi_rates", "device": torch.cuda.get_device_name(0), "code": "K 7, 171/133", "scratch_bytes": pl.VITERBI_SCRATCH_BYTES,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH), "steps": args.steps, "warmup": args.warmup,
              "timing": "HIP events on one stream around every step; medians", "shape": [C, args.symbols]}
    data = quantise_torch(synth_channels_torch(C, M, S, N, dev)).to(torch.int16).contiguous()
    row = data.stride(0) * data.element_size()
    st = torch.cuda.Stream()
    raw = st.cuda_stream
    cap = (N // S + 2 + 63) // 64 * 64
    h = pl.Handle(C, device=0)
    h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
    pk0 = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, pl.FORMAT_CS16, True)
    pk = packets(pl, C, lambda c: data.data_ptr() + c * row, 2 * N, pl.FORMAT_CS16, False)
    o = Outs(pl, torch, C, cap, dev)
    h.process_device(0, pk0, o.out, raw)
    h.synchronize()
    result["t_process"] = timed(torch, st, lambda: h.process_device(0, pk, o.out, raw), args.steps, args.warmup)
    h.synchronize()
    n_sym = [int(o.out[c].n_symbols) for c in range(C)]
    result["symbols_per_channel"] = [min(n_sym), max(n_sym)]
    # the LLRs: one segment a row, int8, a channel's values `pitch` bytes apart
    h.demap_define(0, *the_map(np, M))
    pitch = -(-2 * max(n_sym) // 16) * 16
    llr = torch.zeros(C * pitch, dtype=torch.int8, device=dev)
    dins = (pl.DemapIn * C)(*[pl.DemapIn(o.out[c].soft, n_sym[c], 0, llr.data_ptr() + c * pitch, n_sym[c], 0, 1, pl.DEMAP_I8, GAIN[0], GAIN[1], SCALE, 0)
                              for c in range(C)])
    result["t_demap"] = timed(torch, st, lambda: h.demap_device(dins, raw), args.steps, args.warmup)
    h.synchronize()
    for name, (slot, P, keep) in CODES.items():
        h.viterbi_define(slot, 7, G, P, keep)
    result["t_viterbi"] = {}
    ok = True
    for name, (slot, P, keep) in CODES.items():
        for cut, T in CUTS.items():
            n_llr = pl.viterbi_count(7, G, P, keep, T)
            per_channel = min(min(n_sym) * 2 // n_llr, 32768 // T)
            if not per_channel:
                continue
            for packed in (False, True):
                out_bytes = T // 8 if packed else T
                out = torch.zeros(C * per_channel * out_bytes, dtype=torch.uint8, device=dev)
                ins = (pl.ViterbiIn * (C * per_channel))(*[pl.ViterbiIn(llr.data_ptr() + c * pitch + k * n_llr, out.data_ptr() + (c * per_channel + k) * out_bytes,
                                                                         T, slot + 1, pl.VITERBI_PACKED if packed else 0, 0)
                                                           for c in range(C) for k in range(per_channel)])
                host_ms = []

                def step():
                    t0 = time.perf_counter()
                    h.viterbi_device(ins, raw)
                    host_ms.append((time.perf_counter() - t0) * 1e3)

                r = timed(torch, st, step, args.steps, args.warmup)
                for f in sorted({0, 1, len(ins) // 2, len(ins) - 1}):
                    at = ins[f].llr - llr.data_ptr()
                    want, rec = pl.viterbi_host(7, G, P, keep, llr[at: at + n_llr].cpu().numpy(), T, ins[f].flags)
                    got = out[f * out_bytes: (f + 1) * out_bytes].cpu().numpy().tobytes()
                    ok = ok and got == want.tobytes() and bytes(h.viterbi_records(f, 1)[0]) == bytes(rec)
                sec = r["median_ms"] * 1e-3
                frames = len(ins)
                t_host = sorted(host_ms[args.warmup:])[args.steps // 2]
                r.update(code=name, cut=cut, form="packed" if packed else "bytes", frames=frames, steps_per_frame=T, llr_bytes=frames * n_llr,
                         bits_per_s=frames * T / sec, llr_gbytes_per_s=frames * n_llr / sec / 1e9, t_host_median_ms=t_host,
                         host_share=t_host / r["median_ms"], over_process=r["median_ms"] / result["t_process"]["median_ms"],
                         over_demap=r["median_ms"] / result["t_demap"]["median_ms"])
                result["t_viterbi"]["%s_%s_%s" % (name, cut, r["form"])] = r
                del out
    result["outputs_and_records_equal_host"] = ok
    h.synchronize()
    h.close()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
