"""Writes tests/golden/dev_prim_cases.json: name, number of cases and sha256 of the operand bytes of every case set of
tests/dev_prim_cases.py.  Run from the repository root (python tests/golden/make_dev_prim_cases.py) when a set changes on purpose."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import dev_prim_cases as dc  # noqa: E402

rows = []
for kind in dc.KINDS:
    c = dc.Cases(kind, digests=True)
    rows += [dict(name=n, cases=int(c.counts[n]), sha256=c.digests[n]) for n in c.sets]
with open(os.path.join(ROOT, "tests", "golden", "dev_prim_cases.json"), "w") as f:
    json.dump(rows, f, indent=0)
    f.write("\n")
print("%d case sets, %d cases" % (len(rows), sum(r["cases"] for r in rows)))
