#!/usr/bin/env python3
"""Writes tests/golden/txq_model_observed.json: per transform size, what the CPU oracle's forward transform was observed to differ from
the float model of tests/txq_model.py by, beside the derived budget; the largest coefficient at 10 bit; and every range claim of the
kernels beside its limit.  tests/test_txq_model.py asserts the file against a fresh measurement."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import txq_model as M            # noqa: E402
from oracle import oracle as O   # noqa: E402


def main():
    O.build()
    out = [M.observe_size(O.fwd_txfm2d, ts) for ts in range(M.N_SIZES)]
    path = os.path.join(ROOT, "tests", "golden", "txq_model_observed.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
