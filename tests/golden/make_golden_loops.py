#!/usr/bin/env python3
"""Exact timeslice loops of schwinger128: G[p][a][b][t] = sum_x e^{-2 pi i p x / L} A^-1[idx(b,x,t), idx(a,x,t)]
for the momenta p = 0..3, the spin indices a, b in {0, 1} and every timeslice t = y, in the reference order
idx(s,x,y) = s L^2 + y L + x.  One sparse LU through the repo's oracle and the same column-block solves as
make_golden_displaced.py; of every column idx(a,x,t) only the two rows idx(0,x,t), idx(1,x,t) are read.
A one-off CPU job of a few minutes: python make_golden_loops.py PATH/schwinger128.mat (the reference's matrix
file); writes tests/golden/slice_loops128.json."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_path as rp          # noqa: E402

MASS128 = -0.1320
L = 128
BLOCK = 512
MOMENTA = (0, 1, 2, 3)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    A = rp.load_matrix(sys.argv[1], MASS128)
    n = A.shape[0]
    assert n == 2 * L * L
    lu = rp.LUSolver(A)
    G = np.zeros((len(MOMENTA), 2, 2, L), dtype=np.complex128)
    for c0 in range(0, n, BLOCK):
        cols = np.arange(c0, min(n, c0 + BLOCK))
        rhs = np.zeros((n, cols.size), dtype=np.complex128)
        rhs[cols, np.arange(cols.size)] = 1.0
        X = lu(rhs)                                    # A^-1[:, cols]
        a, site = cols // (L * L), cols % (L * L)      # column idx(a,x,t): site = t L + x
        t, x = site // L, site % L
        for b in range(2):
            vals = X[b * L * L + site, np.arange(cols.size)]
            for j, p in enumerate(MOMENTA):
                np.add.at(G[j, :, b, :], (a, t), np.exp(-2j * np.pi * p * x / L) * vals)
        print("columns %d / %d" % (cols[-1] + 1, n), flush=True)
    out = {"momenta": list(MOMENTA),
           "slice_loops128": [[float(v.real), float(v.imag)] for v in G.ravel()],
           "shape": list(G.shape),
           "note": "G[p][a][b][t] = sum_x exp(-2 pi i p x / L) A^-1[idx(b,x,t), idx(a,x,t)], p = 0..3, "
                   "schwinger128 at mass -0.1320; exact sparse-LU column solves (oracle.ref_path.LUSolver); "
                   "flattened in C order, entry = [re, im]"}
    with open(os.path.join(HERE, "slice_loops128.json"), "w") as f:
        json.dump(out, f)
    print("sum_t (G[0][0][0][t] + G[0][1][1][t]) =", np.sum(G[0, 0, 0] + G[0, 1, 1]))


if __name__ == "__main__":
    main()
