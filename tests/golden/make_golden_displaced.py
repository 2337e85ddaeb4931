#!/usr/bin/env python3
"""Exact displaced traces Tr(A^-1 D_s) of schwinger128 at all 128 displacements, s = 2 L d = 256 d with
(D_s v)[i] = v[(i - s) mod n] (D_s = Pperm_s^T, multigrid.py:142-155): one sparse LU through the repo's
oracle, column-block solves, and every shifted diagonal read off the same block,
Tr(A^-1 D_s) = sum_c A^-1[(c - s) mod n, c].  d = 2 is the reference's own displacement (shift 512).
A one-off CPU job of a few minutes; run in the build container only (needs /root/reference for the
matrix file); writes tests/golden/displaced_traces128.json."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_path as rp          # noqa: E402

REF = "/root/reference"
MASS128 = -0.1320
L = 128
BLOCK = 512


def main():
    A = rp.load_matrix(os.path.join(REF, "schwinger128.mat"), MASS128)
    n = A.shape[0]
    assert n == 2 * L * L
    lu = rp.LUSolver(A)
    shifts = 2 * L * np.arange(L)
    tr = np.zeros(L, dtype=np.complex128)
    for c0 in range(0, n, BLOCK):
        cols = np.arange(c0, min(n, c0 + BLOCK))
        rhs = np.zeros((n, cols.size), dtype=np.complex128)
        rhs[cols, np.arange(cols.size)] = 1.0
        X = lu(rhs)                                    # A^-1[:, cols]
        for j, s in enumerate(shifts):
            tr[j] += np.sum(X[(cols - s) % n, np.arange(cols.size)])
        print("columns %d / %d" % (cols[-1] + 1, n), flush=True)
    out = {"displaced_traces128": [[float(v.real), float(v.imag)] for v in tr],
           "note": "Tr(A^-1 D_s), s = 256 d, d = 0..127, schwinger128 at mass -0.1320; exact sparse-LU column "
                   "solves (oracle.ref_path.LUSolver); entry d = [re, im]"}
    with open(os.path.join(HERE, "displaced_traces128.json"), "w") as f:
        json.dump(out, f)
    print("d=0:", tr[0], " d=2:", tr[2])


if __name__ == "__main__":
    main()
