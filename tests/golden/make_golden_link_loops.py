#!/usr/bin/env python3
"""Exact point-split link loops of schwinger128, the four branches d = (F_x, B_x, F_t, B_t) of DESIGN 4i:

    F_mu[p][a][b][t] = sum_x e^{-2 pi i p x / L} U_mu(n)       A^-1[idx(b,n+mu), idx(a,n)]
    B_mu[p][a][b][t] = sum_x e^{-2 pi i p x / L} conj(U_mu(n)) A^-1[idx(b,n), idx(a,n+mu)]

for the momenta p = 0, 1, the spin indices a, b in {0, 1} and every timeslice t of n = (x, t), the site that owns the
link; n + x^ = ((x+1) mod L, t), n + t^ = (x, (t+1) mod L), idx(s,x,y) = s L^2 + y L + x, U_x(n) = -A[idx(0,n),
idx(0,n+x^)], U_t(n) = -A[idx(0,n), idx(0,n+t^)].  One sparse LU through the repo's oracle and the same column-block
solves as make_golden_loops.py; of every column idx(a,n) the rows idx(b,n+-mu) are read.
A one-off CPU job of a few minutes: python make_golden_link_loops.py PATH/schwinger128.mat (the reference's matrix
file); writes tests/golden/link_loops128.json."""
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
MOMENTA = (0, 1)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    A = rp.load_matrix(sys.argv[1], MASS128).tocsr()
    n = A.shape[0]
    V = L * L
    assert n == 2 * V
    sites = np.arange(V)
    sx, st = sites % L, sites // L
    fwd = (st * L + (sx + 1) % L, ((st + 1) % L) * L + sx)          # n + mu for mu = x, t
    U = [-np.asarray(A[sites, f]).ravel() for f in fwd]
    assert max(abs(np.abs(u) - 1).max() for u in U) < 1e-12
    bwd = (st * L + (sx - 1) % L, ((st - 1) % L) * L + sx)          # n - mu
    lu = rp.LUSolver(A)
    G = np.zeros((4, len(MOMENTA), 2, 2, L), dtype=np.complex128)
    for c0 in range(0, n, BLOCK):
        cols = np.arange(c0, min(n, c0 + BLOCK))
        rhs = np.zeros((n, cols.size), dtype=np.complex128)
        rhs[cols, np.arange(cols.size)] = 1.0
        X = lu(rhs)                                    # A^-1[:, cols]
        a, m = cols // V, cols % V                     # column idx(a,m)
        for mu in range(2):
            # F: the column's site owns the link, row at m + mu; B: the link's owner is m - mu, the row's site
            for d, owner, row in ((2 * mu, m, fwd[mu][m]), (2 * mu + 1, bwd[mu][m], bwd[mu][m])):
                link = U[mu][owner] if d % 2 == 0 else np.conj(U[mu][owner])
                t, x = owner // L, owner % L
                for b in range(2):
                    vals = link * X[b * V + row, np.arange(cols.size)]
                    for j, p in enumerate(MOMENTA):
                        np.add.at(G[d, j, :, b, :], (a, t), np.exp(-2j * np.pi * p * x / L) * vals)
        print("columns %d / %d" % (cols[-1] + 1, n), flush=True)
    out = {"momenta": list(MOMENTA),
           "link_loops128": [[float(v.real), float(v.imag)] for v in G.ravel()],
           "shape": list(G.shape),
           "note": "G[d][p][a][b][t], d = (F_x, B_x, F_t, B_t): F_mu = sum_x exp(-2 pi i p x / L) U_mu(n) "
                   "A^-1[idx(b,n+mu), idx(a,n)], B_mu = sum_x exp(-2 pi i p x / L) conj(U_mu(n)) A^-1[idx(b,n), "
                   "idx(a,n+mu)], n = (x,t) the link's owner, p = 0, 1, schwinger128 at mass -0.1320; exact sparse-LU "
                   "column solves (oracle.ref_path.LUSolver); flattened in C order, entry = [re, im]"}
    with open(os.path.join(HERE, "link_loops128.json"), "w") as f:
        json.dump(out, f)
    hp = np.array([[1, 1j], [-1j, 1]])
    hm = np.array([[1, -1j], [1j, 1]])
    jt = np.einsum('ab,abt->t', hp, G[2, 0]) - np.einsum('ab,abt->t', hm, G[3, 0])
    print("J_t(t, 0): mean", jt.mean(), "spread", np.abs(jt - jt.mean()).max())


if __name__ == "__main__":
    main()
