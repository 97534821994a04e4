"""Writes tests/golden/front_census.json: name, the attempt whose draw met the conditions of the row's kind, and sha256 of
properties, options and packet bytes of every row of tests/front_census.py.  Run from the repository root
(python tests/golden/make_front_census.py) when a row changes on purpose."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import front_census as fc  # noqa: E402

rows = [dict(name=r.name, attempt=r.draw["attempt"], sha256=r.digest()) for r in fc.all_rows()]
with open(os.path.join(ROOT, "tests", "golden", "front_census.json"), "w") as f:
    json.dump(rows, f, indent=0)
    f.write("\n")
print("%d rows, attempts %s" % (len(rows), sorted({r["attempt"] for r in rows})))
