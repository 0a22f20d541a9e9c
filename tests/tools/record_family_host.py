"""Writes the fixtures of tests/test_family_host.py: tests/golden/family_host_<case>_in.npy (op code, then the case file of
tests/family_cases.py) and family_host_<case>.npy (what the program answered), plus family_host_refusals.json (the line each refused
case printed).

    python tests/tools/record_family_host.py PROGRAM

PROGRAM is any executable that speaks the protocol of tests/native/family_check.cpp (PROGRAM <op> <case file> <result file>).  The
committed recordings were made by a harness around cfs_api.hip as it was before the host numerics moved to csrc/cfs_family.cpp, so
the test holds the moved code to the numbers of the code it replaced, bit for bit.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from family_cases import OPS, cases, run  # noqa: E402


def main(program):
    refusals = {}
    for name, (op, data) in cases().items():
        got, refused = run(program, op, data)
        np.save(os.path.join(GOLDEN, f"family_host_{name}_in.npy"), np.concatenate([[OPS.index(op)], data]))
        if name.startswith("refuse_"):
            assert refused and got.size == 0, (name, refused)
            refusals[name] = refused
        else:
            assert refused is None and got.size, (name, refused)
            np.save(os.path.join(GOLDEN, f"family_host_{name}.npy"), got)
        print(name, op, data.size, got.size, refused or "")
    with open(os.path.join(GOLDEN, "family_host_refusals.json"), "w") as f:
        json.dump(refusals, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
