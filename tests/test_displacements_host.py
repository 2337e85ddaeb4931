"""CPU: the host side of the displaced traces (build-only key x_displacements) -- the golden fixture, the
deflated part tr1_s against a dense inverse, the aggregation of the probe loop and the validation."""
import json
import os

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, matrix, stoch_trace, utils

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    with open(os.path.join(HERE, "golden", "displaced_traces128.json")) as f:
        return np.array([complex(re, im) for re, im in json.load(f)["displaced_traces128"]])


def test_golden_fixture_known_entries():
    g = _golden()
    assert g.shape == (128,)
    assert abs(g[0] - 8326.43205953889) < 1e-9 * abs(g[0])
    ref2 = -8.7482427013797 + 50.215154097995686j
    assert abs(g[2] - ref2) < 1e-9 * abs(ref2)


def test_displaced_tr1_completes_the_projected_trace_on_16():
    """Tr(D_s A^-1 (I - W W^H)) + tr1_s = Tr(A^-1 D_s) for all 16 displacements, dense algebra, k = 8."""
    params = gateway.set_params('schwinger16')
    A = matrix.loadMatrix(params['matrix'], params['matrix_params']).toarray()
    n, L, k = A.shape[0], 16, 8
    g3 = np.ones(n)
    g3[n // 2:] = -1.0
    lam, V = np.linalg.eigh(g3[:, None] * A)
    low = np.argsort(np.abs(lam))[:k]
    Sy, Vx = lam[low], V[:, low]
    W = g3[:, None] * Vx * np.sign(Sy)[None, :]
    Ainv = np.linalg.inv(A)
    AinvPi = Ainv - (Ainv @ W) @ W.conj().T
    shifts = [2 * L * d for d in range(L)]
    tr1 = utils.displaced_tr1(Vx, Sy, g3, n, shifts)
    assert tr1.shape == (L,)
    for j, s in enumerate(shifts):
        D = np.roll(np.eye(n), s, axis=0)              # (D v)[i] = v[(i - s) mod n]
        exact = np.trace(Ainv @ D)
        got = np.trace(D @ AinvPi) + tr1[j]
        assert abs(got - exact) < 1e-10 * max(1.0, abs(exact)), (j, got, exact)
        if s == 0:
            assert abs(exact - 265.8581064657958) < 1e-9 * 265.8581064657958
    # the sparse-matrix form of gamma_3 (as the hierarchy holds it): the same products, summed in another
    # memory order -- n = 512 terms per sum, so a few hundred ulp of the largest entry at the very most
    import scipy.sparse as sp
    other = utils.displaced_tr1(Vx, Sy, sp.diags([g3], [0]), n, shifts)
    assert np.max(np.abs(other - tr1)) < 512 * np.finfo(float).eps * np.max(np.abs(tr1))


def test_displaced_loop_control_column_replays_run_probe_loop(lib_built):
    n, S, control, batch = 64, 4, 2, 16
    rng = np.random.default_rng(5)
    w = rng.standard_normal((n, S)) + 1j * rng.standard_normal((n, S))
    offs = np.array([10.0, -3.0 + 1j, 2.5j, 40.0])

    def fake(probes):
        e = probes.astype(np.float64) @ w / np.sqrt(n) + offs
        z = np.zeros(probes.shape[0], dtype=np.int64)
        return e, z + 3, z

    tols = np.array([0.05, 0.3, 0.2, 1e-6])
    np.random.seed(99)
    ref = stoch_trace.run_probe_loop(lambda p: (fake(p)[0][:, control],) + fake(p)[1:], n, tols[control], 4000,
                                     batch)
    state_ref = np.random.get_state()[1].copy()
    np.random.seed(99)
    got = stoch_trace.run_probe_loop(fake, n, tols, 4000, batch, control=control)
    assert got["index"] == ref["index"] and got["index"] >= batch        # more than one round
    assert got["avg"] == ref["avg"] and got["dev"] == ref["dev"]
    assert np.array_equal(got["ests"][:, control], ref["ests"])
    assert np.array_equal(np.random.get_state()[1], state_ref)
    k = got["index"] + 1
    assert got["ests"].shape == (k, S)
    for j in range(S):
        col = got["ests"][:, j]
        assert got["avgs"][j] == np.sum(col) / k
        assert abs(got["devs"][j] - np.std(col)) <= 1e-12 * np.std(col)
        assert bool(got["converged"][j]) == bool(got["devs"][j] / np.sqrt(k) < tols[j])
    assert got["converged"][control] and got["converged"][1] and not got["converged"][3]
    assert got["iters_fine"].sum() == 3 * k


def _tp(example="hutchinson", **extra):
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params.update(extra)
    return utils.trace_params_from_params(params, example)


def test_key_is_copied_only_when_present():
    assert 'x_displacements' not in _tp()
    assert _tp(x_displacements=[0, 2])['x_displacements'] == [0, 2]
    assert utils.displacements_of(_tp()) is None
    disps, shifts, control = utils.displacements_of(_tp(x_displacements=[0, 1, 2, 4, 8]))
    assert disps == [0, 1, 2, 4, 8] and shifts == [0, 256, 512, 1024, 2048] and control == 2
    assert utils.displacements_of(_tp(x_displacements=[3, 0], use_permuted=False))[2] == 1


@pytest.mark.parametrize("bad,msg", [([0, 1, 4], "control displacement 2"),
                                     ([0, 2, 2], "listed twice"),
                                     ([2, 128], "outside"),
                                     ([2, -1], "outside")])
def test_validation_raises_before_any_engine_call(bad, msg):
    tp = _tp(x_displacements=bad)
    with pytest.raises(Exception, match=msg):
        utils.displacements_of(tp)
    with pytest.raises(Exception, match=msg):
        stoch_trace.hutchinson(None, tp)           # no matrix, no engine: the validation comes first


def test_mlmc_rejects_the_key():
    with pytest.raises(Exception, match="x_displacements"):
        stoch_trace.mlmc(None, _tp("mlmc", x_displacements=[0, 2]))
