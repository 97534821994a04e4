"""Records tests/golden/fuzz_draws.json: one sha256 per channel over the properties, the script and the signal bytes that
tools/fuzz_gpu.py draws for a (seed, round, channels) in its default configuration.

usage: python tests/golden/make_fuzz_draws.py PATH_TO_A_FUZZ_GPU_PY [OUT.json]

The file is recorded from the tool as it was before draw_round() existed (git show f63e198:tools/fuzz_gpu.py > old_fuzz_gpu.py):
that version draws inside main(), so main() itself is run, unchanged, with the library's Handle replaced by a class that takes the
lists main() has drawn out of its frame and stops it there.  No GPU is needed.  The present tool draws through draw_round(), and
tests/test_fuzz_draws.py compares what that gives with the recorded file (it imports channel_digest from here).
"""
import hashlib
import importlib.util
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# (seed, rounds, channels): the suite's run of test_randomised_streams, and the rounds the regression tests cite
RECORDED = [(7, (0, 1, 2), 160), (702, (0,), 256), (1002, (5,), 256), (20261004, (129, 148), 256)]


def channel_digest(props, script, sig):
    """sha256 over a channel's draw: its properties, its script and the bytes of its signal"""
    h = hashlib.sha256()
    h.update(repr(sorted(props.items())).encode())
    h.update(repr([tuple(ev) for ev in script]).encode())
    h.update(str(sig.dtype).encode())
    h.update(sig.tobytes())
    return h.hexdigest()


class _Drawn(Exception):
    pass


class _StopAtTheHandle:
    """stands in for lib.Handle: main() has drawn the round when it creates the handle"""

    def __init__(self, *a, **kw):
        f = sys._getframe(1).f_locals
        raise _Drawn([channel_digest(p, ev, s) for p, ev, s in zip(f["props"], f["scripts"], f["sigs"])])


def record(tool_path):
    for k in [k for k in os.environ if k.startswith("PSK_FUZZ_")]:
        del os.environ[k]
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location("fuzz_gpu_recorded", tool_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.pl = types.SimpleNamespace(Handle=_StopAtTheHandle)
    entries = []
    argv = sys.argv
    try:
        for seed, rnds, C in RECORDED:
            for rnd in rnds:
                sys.argv = [tool_path, str(rnd + 1), str(C), str(seed), str(rnd)]
                try:
                    mod.main()
                except _Drawn as e:
                    entries.append(dict(seed=seed, round=rnd, channels=C, sha256=e.args[0]))
                else:
                    raise RuntimeError("main() did not reach the handle")
    finally:
        sys.argv = argv
    return dict(digest="sha256(repr(sorted(props.items())) + repr(script) + str(signal.dtype) + signal.tobytes()), utf-8", entries=entries)


if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_draws.json")
    doc = record(sys.argv[1])
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("%d rounds, %d channels -> %s" % (len(doc["entries"]), sum(len(e["sha256"]) for e in doc["entries"]), out))
