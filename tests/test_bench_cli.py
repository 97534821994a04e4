"""bench.py's command line: a plain run reports the headline and nothing else, --dump-outputs writes what the last timed
step returned (a fixed, seeded sample within 64 MB), and the same arguments give the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("check", "cpu_baseline", "few_channels", "configs3_per_gpu", "mixed", "worst_case", "end_to_end")


def _bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PSK_BENCH_DRY"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, timeout=timeout)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout.decode()
    return json.loads(lines[0])


def _fake_outputs(C, n, bpb, cap):
    import torch

    from psk_soft_amd import lib as pl

    g = torch.Generator().manual_seed(1)
    out = (pl.Output * C)()
    for c in range(C):
        out[c].n_symbols, out[c].n_bits, out[c].n_sampleIndex = n, bpb * n, n
    soft = torch.randn((C, 2 * cap), generator=g)
    phase = torch.randn((C, cap), generator=g)
    bits = torch.randint(-1, 2, (C, bpb * cap), generator=g, dtype=torch.int16)
    sidx = torch.randint(0, 8, (C, cap), generator=g, dtype=torch.int16)
    return out, soft, bits, phase, sidx


@pytest.mark.parametrize("C,n,bpb,cap", [(4096, 32768, 2, 32832), (3, 100, 3, 128), (1, 3 << 20, 3, (3 << 20) + 64)])
def test_dump_outputs_layout_and_budget(tmp_path, C, n, bpb, cap):
    """The dump of bench.py on host tensors: channels 0 and C-1 always in the sample, every stream float32, each sampled
    channel's rows where counts.npy says, the whole within 64 MB, and the same sample every time."""
    sys.path.insert(0, ROOT)
    import bench

    out, soft, bits, phase, sidx = _fake_outputs(C, n, bpb, cap)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, soft, bits, phase, sidx)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["bits.npy", "counts.npy", "phase.npy", "sample_index.npy", "soft.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    counts = got["counts"].astype(np.int64)
    ch = counts[:, 0]
    assert ch[0] == 0 and (C == 1 or C - 1 in ch) and np.all(np.diff(ch) > 0)
    for f in ("soft", "bits", "phase", "sample_index"):
        assert got[f].dtype == np.float32
    off = {"soft": 0, "bits": 0, "phase": 0, "sample_index": 0}
    for (c, m, nb, ni) in counts:
        for f, t, k in (("soft", soft, 2 * m), ("bits", bits, nb), ("phase", phase, m), ("sample_index", sidx, ni)):
            assert np.array_equal(got[f][off[f] : off[f] + k], t[c, :k].numpy().astype(np.float32)), (f, c)
            off[f] += k
    assert all(off[f] == got[f].size for f in off)


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, timeout=120)
    assert out.returncode != 0 and b"--steps" in out.stderr


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path, oracle_mod):
    """A plain run: the headline fields, none of --full's; its dump is the last timed step's outputs (channel 0 against the
    oracle replayed over all warm-up and timed calls) and a second run with the same arguments dumps the same bytes."""
    from psk_soft_amd.stimulus import synth_channels_torch

    C, N, W, K = 64, 16384, 2, 3
    args = ["--steps", str(K), "--warmup", str(W), "--channels", str(C), "--nsamp", str(N)]
    r = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    assert all(k in r for k in PLAIN_KEYS) and not any(k in r for k in FULL_ONLY), sorted(r)
    assert r["steps"] == K and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "soft.npy" in files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    counts = np.load(tmp_path / "a" / "counts.npy").astype(np.int64)
    assert counts[:, 0].tolist() == list(range(C))  # (64 channels of 2048 symbols fit the budget whole)
    import torch

    x = synth_channels_torch(C, 4, 8, N, torch.device("cuda", 0), seed=0x5EED0000, periodic=True)[0].cpu().numpy()
    comp = oracle_mod.OracleComponent()
    comp.samplesPerBaud, comp.constelationSize, comp.numAvg, comp.phaseAvg = 8, 4, 100, 50
    for _ in range(W + K):
        ref = comp.service(x, 0.01, sriChanged=False)
    n = int(counts[0, 1])
    assert n == ref.phase.size
    soft, phase = np.load(tmp_path / "a" / "soft.npy"), np.load(tmp_path / "a" / "phase.npy")
    assert np.array_equal(soft[: 2 * n].view(np.uint32), np.ascontiguousarray(ref.soft, np.float32).view(np.uint32))
    assert np.array_equal(phase[:n].view(np.uint32), np.ascontiguousarray(ref.phase, np.float32).view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "a" / "bits.npy")[: int(counts[0, 2])], ref.bits.astype(np.float32))


@pytest.mark.gpu
def test_full_run_adds_the_check():
    r = _bench(["--steps", "3", "--warmup", "2", "--channels", "64", "--nsamp", "16384", "--full", "--no-cpu-baseline", "--no-few"])
    assert r["check"]["bits_index_exact"] and r["check"]["soft_phase_bit_identical"]
    assert r["roofline"]["empirical_read_ceiling"] > 0
