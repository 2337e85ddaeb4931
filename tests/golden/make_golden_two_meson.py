#!/usr/bin/env python3
"""Two-meson building blocks of schwinger128 at N = 32 Laplacian eigenvectors per timeslice, the source timeslice
t0 = 5 and the operators (g3, p = 0), (g3, p = 1) at the sink and at the source:

    C1[k][k'][t], C2[k][l][k'][l'][t] = utils.two_meson_sums(tau, M, [t0], ops, ops), entry [0]

with tau = utils.perambulators_from_solutions of the 64 sparse-LU solves of utils.laph_sources(V, L, [t0]) -- the
solves make_golden_distilled.py forms --, V = utils.laplacian_eigenvectors of the shipped links and M =
utils.laph_elementals(V, L, momenta).  The matrix is rebuilt from the link fixture the package ships.  A one-off CPU
job of under a minute: python make_golden_two_meson.py; writes tests/golden/two_meson128.json, 12 digits."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from deflatedmlmc_schwinger_amd import gateway, matrix, utils     # noqa: E402
from deflatedmlmc_schwinger_amd.hierarchy import detect_lattice   # noqa: E402
from oracle import ref_path as rp                                 # noqa: E402

L = 128
T0 = 5
NEV = 32
MOMENTA = (0, 1)
OPERATORS = (('g3', 0), ('g3', 1))


def _digits(values):
    return [[float("%.11e" % v.real), float("%.11e" % v.imag)] for v in np.asarray(values).ravel()]


def main():
    params = gateway.set_params('schwinger128')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    assert A.shape[0] == 2 * L * L
    found = detect_lattice(A)
    assert found is not None and found[0] == L
    V, _ = utils.laplacian_eigenvectors(found[2], L, NEV)
    src = utils.laph_sources(V, L, [T0])                              # (64, n)
    lu = rp.LUSolver(A)
    Z = np.asarray(lu(np.ascontiguousarray(src.T))).T
    tau = utils.perambulators_from_solutions(V, Z, L, nsrc=1)
    M = utils.laph_elementals(V, L, MOMENTA)
    ops = [(g, MOMENTA.index(p)) for g, p in OPERATORS]
    C1, C2 = utils.two_meson_sums(tau, M, [T0], ops, ops)
    C1, C2 = C1[0], C2[0]
    assert C1.shape == (2, 2, L) and C2.shape == (2, 2, 2, 2, L)
    out = {"momenta": list(MOMENTA), "source_timeslice": T0, "distillation_vectors": NEV,
           "operators": [list(op) for op in OPERATORS],
           "C1": _digits(C1), "C1_shape": list(C1.shape), "C2": _digits(C2), "C2_shape": list(C2.shape),
           "note": "C1[k][k'][t] = tr[Q_k S_k'] and C2[k][l][k'][l'][t] = tr[Q_k S_k' Q_l S_l'] of utils.two_meson_sums "
                   "for the sink and source operators (g3, p = 0), (g3, p = 1), 32 eigenvectors of the largest "
                   "eigenvalues of H_t (utils.laplacian_eigenvectors), t0 = 5, schwinger128 at mass -0.1320; 64 exact "
                   "sparse-LU column solves (oracle.ref_path.LUSolver) of utils.laph_sources; flattened in C order, "
                   "entry = [re, im], 12 significant digits"}
    with open(os.path.join(HERE, "two_meson128.json"), "w") as f:
        json.dump(out, f)
    two = utils.two_meson_correlator(C1, C2, 0, 0, 0, 0)
    print("C_pi(t, 0), t = 0..7:", C1[0, 0, :8].real)
    print("isospin-2 pi pi, t = 0..7:", two['isospin2'][:8].real, " max |imag| =", np.max(np.abs(two['isospin2'].imag)))


if __name__ == "__main__":
    main()
