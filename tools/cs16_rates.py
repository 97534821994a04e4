#!/usr/bin/env python3
"""cs16_rates.py -- complex int16 (PSK_SOFT_FORMAT_CS16) against float32 (CF32) packets on one MI355X, in one process.

The same stimulus (QPSK, samplesPerBaud 8, numAvg 100, phaseAvg 50) quantised to int16 -- round(x * 8192), clipped -- is fed
once as int16 and once as its exact float32 cast, on three paths:

  device      packets resident in HBM, 4096 channels x 2^18 samples: ms per step (psk_soft_process_device + synchronize)
  zero_copy   packets and results in psk_soft_host_alloc memory, 4096 x 32768: Gsamples/s
  host        psk_soft_process_host with pageable numpy packets and results, 4096 x 32768: Gsamples/s

Every path checks that the two formats give the same bits on every channel of the first step, and compares channels 0 and the
last against the CPU oracle.  One JSON object on stdout (and in --out).

    python tools/cs16_rates.py [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SCALE = 8192.0
S, M, A, NPH = 8, 4, 100, 50


def quantise_torch(x):
    import torch

    return torch.clamp(torch.round(x * SCALE), -32768, 32767).to(torch.int16)


def packets(pl, C, ptr, n_elems, fmt, first):
    pk = (pl.Packet * C)()
    for c in range(C):
        pk[c].data = ptr(c)
        pk[c].n_floats = n_elems
        pk[c].sri_xdelta = 0.01
        pk[c].sri_mode = 1
        pk[c].sriChanged = int(first)
        pk[c].present = 1
        pk[c].format = fmt
    return pk


def outputs(pl, C, cap, soft, bits, phase, sidx):
    out = (pl.Output * C)()
    for c in range(C):
        out[c].soft, out[c].bits, out[c].phase, out[c].sampleIndex = soft(c), bits(c), phase(c), sidx(c)
        out[c].cap_symbols = cap
    return out


def oracle_check(iq16_rows, got_rows):
    """iq16_rows[i]: the int16 packet of a channel's first call; got_rows[i]: (soft, bits, phase, index) the library gave"""
    from oracle import pyoracle as po

    po.build()
    for iq, (soft, bits, phase, index) in zip(iq16_rows, got_rows):
        o = po.OracleComponent()
        o.samplesPerBaud, o.constelationSize, o.numAvg, o.phaseAvg = S, M, A, NPH
        r = o.service(iq.astype(np.float32), 0.01, sriChanged=True)
        for a, b in ((soft, r.soft), (phase, r.phase)):
            if not np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)):
                return False
        if not (np.array_equal(bits, r.bits) and np.array_equal(index, r.index)):
            return False
    return True


def run_device(pl, torch, C, N, steps, warmup):
    from psk_soft_amd.stimulus import synth_channels_torch

    dev = torch.device("cuda", 0)
    iq16 = quantise_torch(synth_channels_torch(C, M, S, N, dev)).contiguous()
    iqf = iq16.to(torch.float32)
    cap = (N // S + 2 + 63) // 64 * 64
    res = {}
    first_out = {}
    for name, fmt, src, esz in (("f32", pl.FORMAT_CF32, iqf, 4), ("cs16", pl.FORMAT_CS16, iq16, 2)):
        soft = torch.empty((C, 2 * cap), dtype=torch.float32, device=dev)
        phase = torch.empty((C, cap), dtype=torch.float32, device=dev)
        sidx = torch.empty((C, cap), dtype=torch.int16, device=dev)
        bits = torch.empty((C, 2 * cap), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        h = pl.Handle(C, device=0)
        h.configure_all(samplesPerBaud=S, constelationSize=M, numAvg=A, phaseAvg=NPH)
        row = src.stride(0) * esz
        base = src.data_ptr()
        out = outputs(pl, C, cap, lambda c: soft[c].data_ptr(), lambda c: bits[c].data_ptr(), lambda c: phase[c].data_ptr(),
                      lambda c: sidx[c].data_ptr())
        pk0 = packets(pl, C, lambda c: base + c * row, 2 * N, fmt, True)
        pk = packets(pl, C, lambda c: base + c * row, 2 * N, fmt, False)
        h.process_device(0, pk0, out)
        h.synchronize()
        n = [int(out[c].n_symbols) for c in (0, C - 1)]
        first_out[name] = (soft.clone(), bits.clone(), phase.clone(), sidx.clone(), n, [int(out[c].n_symbols) for c in range(C)])
        torch.cuda.synchronize()  # (the copies run on torch's stream: done before the next calls overwrite the outputs)
        for _ in range(warmup):
            h.process_device(0, pk, out)
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            h.process_device(0, pk, out)
        h.synchronize()
        res[name + "_ms_per_step"] = (time.perf_counter() - t0) * 1e3 / steps
        res[name + "_stats"] = h.stats()
        h.close()
        del soft, phase, sidx, bits
    a, b = first_out["f32"], first_out["cs16"]
    ns = a[5][0]  # (a uniform batch: every channel the same count; what lies behind it in the rows was never written)
    same = a[5] == b[5] == [ns] * C and all(
        torch.equal(x[:, : w * ns].view(torch.int32) if x.dtype == torch.float32 else x[:, : w * ns],
                    y[:, : w * ns].view(torch.int32) if y.dtype == torch.float32 else y[:, : w * ns])
        for x, y, w in zip(a[:4], b[:4], (2, 2, 1, 1)))
    rows = []
    for i, c in enumerate((0, C - 1)):
        ns = b[4][i]
        rows.append((b[0][c, : 2 * ns].cpu().numpy(), b[1][c, : 2 * ns].cpu().numpy(), b[2][c, :ns].cpu().numpy(), b[3][c, :ns].cpu().numpy()))
    res["formats_identical"] = bool(same)
    res["oracle_ok"] = oracle_check([iq16[0].cpu().numpy(), iq16[C - 1].cpu().numpy()], rows)
    res["ratio_cs16_over_f32"] = res["cs16_ms_per_step"] / res["f32_ms_per_step"]
    res["shape"] = [C, N]
    return res


def run_zero_copy(pl, C, N, steps, warmup, host16):
    cap = (N // S + 2 + 63) // 64 * 64
    res, first = {}, {}
    for name, fmt, dt in (("f32", pl.FORMAT_CF32, np.float32), ("cs16", pl.FORMAT_CS16, np.int16)):
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
    a, b = first["f32"], first["cs16"]
    ns = a[4][0]
    res["formats_identical"] = bool(a[4] == b[4] == [ns] * C and all(np.array_equal(x[:, : w * ns].view(np.uint8), y[:, : w * ns].view(np.uint8))
                                                                     for x, y, w in zip(a[:4], b[:4], (2, 2, 1, 1))))
    rows = []
    for c in (0, C - 1):
        ns = b[4][c]
        rows.append((b[0][c, : 2 * ns], b[1][c, : 2 * ns], b[2][c, :ns], b[3][c, :ns]))
    res["oracle_ok"] = oracle_check([host16[0], host16[C - 1]], rows)
    res["ratio_cs16_over_f32"] = res["cs16_gsamples_per_s"] / res["f32_gsamples_per_s"]
    res["shape"] = [C, N]
    return res


def run_host(pl, C, N, steps, warmup, host16):
    """psk_soft_process_host straight through the C ABI (pageable numpy buffers, descriptors built once)"""
    cap = (N // S + 2 + 63) // 64 * 64
    L = pl.load()
    res, first = {}, {}
    for name, fmt, dt in (("f32", pl.FORMAT_CF32, np.float32), ("cs16", pl.FORMAT_CS16, np.int16)):
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
    a, b = first["f32"], first["cs16"]
    ns = a[4][0]
    res["formats_identical"] = bool(a[4] == b[4] == [ns] * C and all(np.array_equal(x[:, : w * ns].view(np.uint8), y[:, : w * ns].view(np.uint8))
                                                                     for x, y, w in zip(a[:4], b[:4], (2, 2, 1, 1))))
    rows = []
    for c in (0, C - 1):
        ns = b[4][c]
        rows.append((b[0][c, : 2 * ns], b[1][c, : 2 * ns], b[2][c, :ns], b[3][c, :ns]))
    res["oracle_ok"] = oracle_check([host16[0], host16[C - 1]], rows)
    res["ratio_cs16_over_f32"] = res["cs16_gsamples_per_s"] / res["f32_gsamples_per_s"]
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
        raise SystemExit("cs16_rates.py measures on an MI355X; no GPU visible")
    C = args.channels
    result = {"tool": "cs16_rates", "device": torch.cuda.get_device_name(0), "scale": SCALE,
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
