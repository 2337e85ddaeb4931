#!/usr/bin/env python3
"""Distilled three-point functions of schwinger128 at N = 32 Laplacian eigenvectors per timeslice, source timeslice
t0 = 5, sink timeslice tf = 21, Gamma_f = g3, pf = pi = 0, insertion momenta q = 0, 1, all 128 insertion timeslices:

    C3[insertion][Gamma_i][j][t] = utils.distilled_three_point_correlator(G, tau[0, tf], M[0, tf], M[0, t0], 'g3',
                                                                          insertion, Gamma_i)

for the six insertions '1', 'g3', 's1', 's2', 'Jx', 'Jt' and the four source matrices '1', 'g3', 's1', 's2', with G =
utils.generalized_perambulators_from_solutions and tau = utils.perambulators_from_solutions of the 128 sparse-LU solves
of utils.laph_sources(V, L, [t0, tf]), V = utils.laplacian_eigenvectors of the shipped links and M =
utils.laph_elementals(V, L, [0]).  The matrix is rebuilt from the link fixture the package ships.  A one-off CPU job of
a few minutes: python make_golden_distilled_three_point.py; writes tests/golden/distilled_three_point128.json."""
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
T0, TF = 5, 21
NEV = 32
MOMENTA = (0, 1)
SOURCES = ('1', 'g3', 's1', 's2')


def main():
    params = gateway.set_params('schwinger128')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params'])
    assert A.shape[0] == 2 * L * L
    found = detect_lattice(A)
    assert found is not None and found[0] == L
    U1, U2 = found[2], found[3]
    V, lam = utils.laplacian_eigenvectors(U1, L, NEV)
    src = utils.laph_sources(V, L, [T0, TF])                          # (128, n)
    lu = rp.LUSolver(A)
    Z = np.asarray(lu(np.ascontiguousarray(src.T))).T
    tau = utils.perambulators_from_solutions(V, Z, L, nsrc=2)
    G = utils.generalized_perambulators_from_solutions(Z[2 * NEV:], Z[:2 * NEV], U1, U2, L, list(range(L)), MOMENTA)
    M = utils.laph_elementals(V, L, [0])
    C3 = np.stack([np.stack([utils.distilled_three_point_correlator(G, tau[0, TF], M[0, TF], M[0, T0], 'g3', ins, s)
                             for s in SOURCES]) for ins in utils.DISTILLED_INSERTIONS])
    assert C3.shape == (6, 4, len(MOMENTA), L)
    out = {"momenta": list(MOMENTA), "source_timeslice": T0, "sink_timeslice": TF, "sink_gamma": "g3",
           "sink_momentum": 0, "source_momentum": 0, "distillation_vectors": NEV,
           "insertions": list(utils.DISTILLED_INSERTIONS), "source_gammas": list(SOURCES),
           "distilled_three_point128": [float("%.11e" % x) for v in C3.ravel() for x in (v.real, v.imag)],
           "shape": list(C3.shape),
           "note": "C3[insertion][Gamma_i][q][t]: the three-point function of three_point() with box A^-1 box in place "
                   "of the two outer propagators, box(t) the projector onto the 32 eigenvectors of the largest "
                   "eigenvalues of H_t (utils.laplacian_eigenvectors), t0 = 5, tf = 21, Gamma_f = g3, pf = pi = 0, "
                   "q = 0, 1, schwinger128 at mass -0.1320; 128 exact sparse-LU column solves "
                   "(oracle.ref_path.LUSolver) of utils.laph_sources, summed by "
                   "utils.generalized_perambulators_from_solutions and contracted by "
                   "utils.distilled_three_point_correlator; flattened in C order as re, im, re, im, ..., each rounded "
                   "to 12 significant digits (the tests' bar is 2e-10 of an insertion's largest value)"}
    with open(os.path.join(HERE, "distilled_three_point128.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("distilled C3_g3(t, q = 0) with Gamma_i = g3, t = 3..8:", C3[1, 1, 0, 3:9])


if __name__ == "__main__":
    main()
