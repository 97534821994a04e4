"""Workers on threads of their own, for the tests that drive several handles at once (tests/test_many_handles_control.py,
tests/test_gpu_many_handles.py)."""
import threading
import time


class WorkerStuck(AssertionError):
    """a worker did not finish in time: it may still be inside the library, so what it uses must not be torn down"""


def run_workers(workers, seconds=120):
    """Start every worker on a daemon thread and wait for all of them, `seconds` for all together; whatever one of them raised is
    raised here.  A worker that is still running then raises WorkerStuck: the thread is a daemon, so it fails the test and holds
    up neither the rest of the suite nor the interpreter's exit."""
    errors = []

    def guard(fn):
        def run():
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 (handed to the caller's thread)
                errors.append(e)
        return run

    ts = [threading.Thread(target=guard(w), daemon=True) for w in workers]
    for t in ts:
        t.start()
    deadline = time.monotonic() + seconds
    for t in ts:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in ts):
        raise WorkerStuck("%d of %d workers did not finish" % (sum(t.is_alive() for t in ts), len(ts)))
    if errors:
        raise errors[0]
