#!/usr/bin/env python3
"""wide_rates.py -- wide symbols (samplesPerBaud > 1024, psk_wide.hip) against the same sample count at samplesPerBaud 1024 (the
16-phases-a-lane front stage), packets resident in HBM, on one MI355X.

    1 channel    x 2^22 samples, samplesPerBaud 4096, numAvg 10   (and the CPU oracle's time for the same call)
    1024 channels x 2^20 samples, samplesPerBaud 2048, numAvg 4
    1 channel    x 2^24 samples, samplesPerBaud 65535, numAvg 2

ms per call (psk_soft_process_device + synchronize, QPSK, phaseAvg 50, noise-like stimulus), and the handle's statistics of
the last call.  One JSON object on stdout (and in --out).

    python tools/wide_rates.py [--steps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ms_per_call(pl, torch, C, N, S, A, steps, warmup):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(S * 7 + C)
    iq = torch.randn((C, 2 * N), generator=g, device=dev, dtype=torch.float32)
    cap = (N // S + 2 + 63) // 64 * 64
    soft = torch.empty((C, 2 * cap), dtype=torch.float32, device=dev)
    phase = torch.empty((C, cap), dtype=torch.float32, device=dev)
    sidx = torch.empty((C, cap), dtype=torch.int16, device=dev)
    bits = torch.empty((C, 2 * cap), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    h = pl.Handle(C, device=0, max_window_samples=max(S * A, 16384), max_phase_avg=512, max_packet_complex=N)
    h.configure_all(samplesPerBaud=S, constelationSize=4, numAvg=A, phaseAvg=50)

    def pkts(first):
        pk = (pl.Packet * C)()
        for c in range(C):
            pk[c].data = iq[c].data_ptr()
            pk[c].n_floats = 2 * N
            pk[c].sri_xdelta = 0.01
            pk[c].sri_mode = 1
            pk[c].sriChanged = int(first)
            pk[c].present = 1
        return pk

    out = (pl.Output * C)()
    for c in range(C):
        out[c].soft, out[c].bits, out[c].phase, out[c].sampleIndex = soft[c].data_ptr(), bits[c].data_ptr(), phase[c].data_ptr(), sidx[c].data_ptr()
        out[c].cap_symbols = cap
    h.process_device(0, pkts(True), out)
    h.synchronize()
    pk = pkts(False)
    for _ in range(warmup):
        h.process_device(0, pk, out)
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        h.process_device(0, pk, out)
    h.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    st = h.stats()
    h.close()
    del iq, soft, phase, sidx, bits
    torch.cuda.empty_cache()
    return dict(C=C, N=N, S=S, A=A, ms_per_call=ms, Msamples_per_s=C * N / ms / 1e3, symbols_per_call=int(N // S - A + 1), stats=st)


def oracle_ms(N, S, A):
    import numpy as np

    from oracle import pyoracle as po

    po.build()
    o = po.OracleComponent()
    o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, 4, A, 50
    x = np.random.default_rng(1).standard_normal(2 * N).astype(np.float32)
    t0 = time.perf_counter()
    o.service(x, 0.01, sriChanged=True)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from psk_soft_amd import lib as pl

    res = {}
    for name, C, N, S, A in (("one_channel", 1, 1 << 22, 4096, 10), ("1024_channels", 1024, 1 << 20, 2048, 4),
                             ("s65535", 1, 1 << 24, 65535, 2)):
        res[name] = dict(wide=ms_per_call(pl, torch, C, N, S, A, a.steps, a.warmup),
                         s1024=ms_per_call(pl, torch, C, N, 1024, A, a.steps, a.warmup))
        res[name]["wide_over_s1024_time"] = res[name]["wide"]["ms_per_call"] / res[name]["s1024"]["ms_per_call"]
    res["one_channel"]["oracle_cpu_ms"] = oracle_ms(1 << 22, 4096, 10)
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
