#!/usr/bin/env python3
"""cf16_rates.py -- complex binary16 (PSK_SOFT_FORMAT_CF16) against complex int16 (CS16) and float32 (CF32) packets on one
MI355X, in one process.

The same stimulus (QPSK, samplesPerBaud 8, numAvg 100, phaseAvg 50) is scaled by 1024 and rounded to integers of at most
+-2048: every value is then exact in half, in int16 and in float32, so the three formats carry the same numbers, give the same
bits and do the same arithmetic -- the CF16 and CS16 steps read the same bytes through the same loads and differ by the
conversion instructions only.  The paths of tools/cs8_rates.py:

  device      packets resident in HBM, 4096 channels x 2^18 samples, every step timed with a pair of HIP events on the stream
              of the call: the median of --steps steps after --warmup, in the order f32, cs16, cf16, cs16 again.  The two CS16
              medians give the run's own spread; `cf16_within_5_percent_of_cs16` is claimed only if that spread is inside the
              margin too, else `spread_exceeds_margin` says so
  zero_copy   packets and results in psk_soft_host_alloc memory, 4096 x 32768: Gsamples/s (recorded, no condition)
  host        psk_soft_process_host with pageable numpy packets and results, 4096 x 32768: Gsamples/s (recorded, no condition)

Every path checks that the three formats give the same bits on every channel of the first step, and compares channels 0 and
the last against the CPU oracle.  One JSON object on stdout (and in --out).

    python tools/cf16_rates.py [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from cs16_rates import A, M, NPH, S, oracle_check, outputs, packets  # noqa: E402

SCALE = 1024.0
LIMIT = 2048  # integers up to 2^11 are exact in half
MARGIN = 1.05
FORMATS = (("f32", 0, np.float32), ("cs16", 1, np.int16), ("cf16", 4, np.float16))  # (name, PSK_SOFT_FORMAT_*, numpy type)
STAT_KEYS = ("timing_exact_blocks", "channels_exact_timing", "fit_chain_blocks", "channels_sequential", "channels_fast")


def quantise_torch(x):
    import torch

    return torch.clamp(torch.round(x * SCALE), -LIMIT, LIMIT).to(torch.int16)


def _same(first, C, w=(2, 2, 1, 1)):
    """every format's first-step outputs equal to the float ones, bit for bit"""
    a = first["f32"]
    ns = a[4][0]
    ok = a[4] == [ns] * C
    for name, _, _ in FORMATS[1:]:
        b = first[name]
        ok = ok and b[4] == a[4] and all(np.array_equal(x[:, : k * ns].view(np.uint8), y[:, : k * ns].view(np.uint8))
                                         for x, y, k in zip(a[:4], b[:4], w))
    return bool(ok)


def _oracle_rows(first, C):
    b = first["cf16"]
    rows = []
    for c in (0, C - 1):
        ns = b[4][c]
        rows.append((b[0][c, : 2 * ns], b[1][c, : 2 * ns], b[2][c, :ns], b[3][c, :ns]))
    return rows


def run_device(pl, torch, C, N, steps, warmup):
    from psk_soft_amd.stimulus import synth_channels_torch

    dev = torch.device("cuda", 0)
    iq16 = quantise_torch(synth_channels_torch(C, M, S, N, dev)).contiguous()
    srcs = {"f32": iq16.to(torch.float32), "cs16": iq16, "cf16": iq16.to(torch.float16)}
    assert torch.equal(srcs["cf16"].to(torch.int16), iq16)
    cap = (N // S + 2 + 63) // 64 * 64
    stream = torch.cuda.Stream(device=dev)
    res, first = {}, {}
    fmt_of = {name: fmt for name, fmt, _ in FORMATS}
    for tag, name in (("f32", "f32"), ("cs16", "cs16"), ("cf16", "cf16"), ("cs16_again", "cs16")):
        src = srcs[name]
        soft = torch.empty((C, 2 * cap), dtype=torch.float32, device=dev)
        phase = torch.empty((C, cap), dtype=torch.float32, device=dev)
        sidx = torch.empty((C, cap), dtype=torch.int16, device=dev)
        bits = torch.empty((C, 2 * cap), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        h = pl.Handle(C, device=0)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
        row = src.stride(0) * src.element_size()
        base = src.data_ptr()
        out = outputs(pl, C, cap, lambda c: soft[c].data_ptr(), lambda c: bits[c].data_ptr(), lambda c: phase[c].data_ptr(),
                      lambda c: sidx[c].data_ptr())
        pk0 = packets(pl, C, lambda c: base + c * row, 2 * N, fmt_of[name], True)
        pk = packets(pl, C, lambda c: base + c * row, 2 * N, fmt_of[name], False)
        h.process_device(0, pk0, out, stream.cuda_stream)
        stream.synchronize()
        if tag == name:
            first[name] = (soft.clone(), bits.clone(), phase.clone(), sidx.clone(), [int(out[c].n_symbols) for c in range(C)])
            torch.cuda.synchronize()  # (the copies run on torch's stream: done before the next calls overwrite the outputs)
        for _ in range(warmup):
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
        res[tag + "_ms_per_step"] = statistics.median(ms)
        res[tag + "_ms_min_max"] = [min(ms), max(ms)]
        st = h.stats()
        res[tag + "_stats"] = {k: st[k] for k in STAT_KEYS}
        h.close()
        del soft, phase, sidx, bits
    a = first["f32"]
    ns = a[4][0]
    res["formats_identical"] = bool(a[4] == [ns] * C and all(
        first[name][4] == a[4] and all(torch.equal(x[:, : w * ns].view(torch.int32) if x.dtype == torch.float32 else x[:, : w * ns],
                                                   y[:, : w * ns].view(torch.int32) if y.dtype == torch.float32 else y[:, : w * ns])
                                       for x, y, w in zip(a[:4], first[name][:4], (2, 2, 1, 1)))
        for name in ("cs16", "cf16")))
    b = first["cf16"]
    rows = [(b[0][c, : 2 * b[4][c]].cpu().numpy(), b[1][c, : 2 * b[4][c]].cpu().numpy(), b[2][c, : b[4][c]].cpu().numpy(),
             b[3][c, : b[4][c]].cpu().numpy()) for c in (0, C - 1)]
    res["oracle_ok"] = oracle_check([srcs["cf16"][0].cpu().numpy(), srcs["cf16"][C - 1].cpu().numpy()], rows)
    cs16 = (res["cs16_ms_per_step"], res["cs16_again_ms_per_step"])
    res["cs16_spread"] = max(cs16) / min(cs16)
    res["ratio_cf16_over_cs16"] = res["cf16_ms_per_step"] / (sum(cs16) / 2)
    res["ratio_cf16_over_f32"] = res["cf16_ms_per_step"] / res["f32_ms_per_step"]
    res["margin"] = MARGIN
    res["spread_exceeds_margin"] = bool(res["cs16_spread"] > MARGIN)
    res["cf16_within_5_percent_of_cs16"] = bool(not res["spread_exceeds_margin"] and res["ratio_cf16_over_cs16"] <= MARGIN)
    res["shape"] = [C, N]
    return res


def run_zero_copy(pl, C, N, steps, warmup, host16):
    cap = (N // S + 2 + 63) // 64 * 64
    res, first = {}, {}
    for name, fmt, dt in FORMATS:
        buf = pl.host_alloc(C * 2 * N, dt).reshape(C, 2 * N)
        buf[:] = host16.astype(dt)
        soft = pl.host_alloc(C * 2 * cap, np.float32).reshape(C, 2 * cap)
        phase = pl.host_alloc(C * cap, np.float32).reshape(C, cap)
        sidx = pl.host_alloc(C * cap, np.int16).reshape(C, cap)
        bits = pl.host_alloc(C * 2 * cap, np.int16).reshape(C, 2 * cap)
        h = pl.Handle(C, device=0)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
        out = outputs(pl, C, cap, lambda c: soft[c].ctypes.data, lambda c: bits[c].ctypes.data, lambda c: phase[c].ctypes.data,
                      lambda c: sidx[c].ctypes.data)
        pk0 = packets(pl, C, lambda c: buf[c].ctypes.data, 2 * N, fmt, True)
        pk = packets(pl, C, lambda c: buf[c].ctypes.data, 2 * N, fmt, False)
        h.process_device(0, pk0, out)
        h.synchronize()
        first[name] = (soft.copy(), bits.copy(), phase.copy(), sidx.copy(), [int(out[c].n_symbols) for c in range(C)])
        for _ in range(warmup):
            h.process_device(0, pk, out)
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            h.process_device(0, pk, out)
        h.synchronize()
        res[name + "_gsamples_per_s"] = C * N * steps / (time.perf_counter() - t0) / 1e9
        h.close()
        for a in (buf, soft, phase, sidx, bits):
            pl.host_free(a.reshape(-1))
    res["formats_identical"] = _same(first, C)
    res["oracle_ok"] = oracle_check([host16[0], host16[C - 1]], _oracle_rows(first, C))
    res["ratio_cf16_over_cs16"] = res["cf16_gsamples_per_s"] / res["cs16_gsamples_per_s"]
    res["ratio_cf16_over_f32"] = res["cf16_gsamples_per_s"] / res["f32_gsamples_per_s"]
    res["shape"] = [C, N]
    return res


def run_host(pl, C, N, steps, warmup, host16):
    """psk_soft_process_host straight through the C ABI (pageable numpy buffers, descriptors built once)"""
    cap = (N // S + 2 + 63) // 64 * 64
    L = pl.load()
    res, first = {}, {}
    for name, fmt, dt in FORMATS:
        buf = np.ascontiguousarray(host16.astype(dt))
        soft = np.empty((C, 2 * cap), np.float32)
        phase = np.empty((C, cap), np.float32)
        sidx = np.empty((C, cap), np.int16)
        bits = np.empty((C, 2 * cap), np.int16)
        h = pl.Handle(C, device=0)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
        out = outputs(pl, C, cap, lambda c: soft[c].ctypes.data, lambda c: bits[c].ctypes.data, lambda c: phase[c].ctypes.data,
                      lambda c: sidx[c].ctypes.data)
        pk0 = packets(pl, C, lambda c: buf[c].ctypes.data, 2 * N, fmt, True)
        pk = packets(pl, C, lambda c: buf[c].ctypes.data, 2 * N, fmt, False)
        pl._check(L.psk_soft_process_host(h._h, 0, C, pk0, out))
        first[name] = (soft.copy(), bits.copy(), phase.copy(), sidx.copy(), [int(out[c].n_symbols) for c in range(C)])
        for _ in range(warmup):
            pl._check(L.psk_soft_process_host(h._h, 0, C, pk, out))
        t0 = time.perf_counter()
        for _ in range(steps):
            pl._check(L.psk_soft_process_host(h._h, 0, C, pk, out))
        res[name + "_gsamples_per_s"] = C * N * steps / (time.perf_counter() - t0) / 1e9
        h.close()
    res["formats_identical"] = _same(first, C)
    res["oracle_ok"] = oracle_check([host16[0], host16[C - 1]], _oracle_rows(first, C))
    res["ratio_cf16_over_cs16"] = res["cf16_gsamples_per_s"] / res["cs16_gsamples_per_s"]
    res["ratio_cf16_over_f32"] = res["cf16_gsamples_per_s"] / res["f32_gsamples_per_s"]
    res["shape"] = [C, N]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--nsamp-device", type=int, default=1 << 18)
    ap.add_argument("--nsamp-host", type=int, default=32768)
    ap.add_argument("--paths", default="device,zero_copy,host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from psk_soft_amd import lib as pl
    from psk_soft_amd.stimulus import synth_channels_torch

    if not torch.cuda.is_available():
        raise SystemExit("cf16_rates.py measures on an MI355X; no GPU visible")
    C = args.channels
    result = {"tool": "cf16_rates", "device": torch.cuda.get_device_name(0), "scale": SCALE, "limit": LIMIT,
              "config": dict(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH), "steps": args.steps,
              "warmup": args.warmup}
    paths = args.paths.split(",")
    if "device" in paths:
        result["device_resident"] = run_device(pl, torch, C, args.nsamp_device, args.steps, args.warmup)
        torch.cuda.empty_cache()
    if "zero_copy" in paths or "host" in paths:
        N = args.nsamp_host
        host16 = quantise_torch(synth_channels_torch(C, M, S, N, torch.device("cuda", 0))).cpu().numpy()
        if "zero_copy" in paths:
            result["zero_copy"] = run_zero_copy(pl, C, N, args.steps, args.warmup, host16)
        if "host" in paths:
            result["process_host"] = run_host(pl, C, N, args.steps, args.warmup, host16)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(v.get("formats_identical", True) and v.get("oracle_ok", True) for v in result.values() if isinstance(v, dict) and "shape" in v)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
