"""CPU: utils.lma_correlator, the source-averaged correlator of a lma_two_point() result, against a
plain double loop over the source timeslice and the distance, its translation-invariant limit, its refusal of a
two_point() result, and the validation of the build-only key low_mode_contraction."""
import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import gateway, stoch_trace, utils

L = 12
M = 3
T0 = 5


def _random_result(seed):
    rng = np.random.default_rng(seed)

    def c(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    return {'two_point_low': c(M, 2, 2, 2, 2, L, L), 'two_point_rest': c(M, 2, 2, 2, 2, L), 'source_timeslice': T0}


@pytest.mark.parametrize("sink,source", [('g3', 'g3'), ('s1', '1')])
def test_against_the_double_loop(sink, source):
    res = _random_result(11)
    out = utils.lma_correlator(res, sink, source)
    assert out.shape == (M, L) and out.dtype == np.complex128
    rest = utils.meson_correlator(res['two_point_rest'], sink, source)
    ref = np.zeros((M, L), dtype=np.complex128)
    for d in range(L):
        for t0 in range(L):
            ref[:, d] += utils.meson_correlator(res['two_point_low'][..., t0], sink, source)[:, (t0 + d) % L] / L
        ref[:, d] += rest[:, (T0 + d) % L]
    assert np.max(np.abs(out - ref)) <= 1e-13 * np.max(np.abs(ref))


def test_translation_invariant_low_part_gives_the_single_source_correlator():
    """two_point_low[..., t, t0] = f[..., (t - t0) mod L] and no remainder: every source timeslice carries the same
    correlator, so the average is that correlator itself -- the single-source one rolled to t0 = 0 -- exactly when
    the entries are small integers (the mean of L equal exact numbers with L a power of two)."""
    Lp = 8
    rng = np.random.default_rng(12)
    f = (rng.integers(-8, 9, (M, 2, 2, 2, 2, Lp)) + 1j * rng.integers(-8, 9, (M, 2, 2, 2, 2, Lp))).astype(np.complex128)
    t, t0 = np.arange(Lp)[:, None], np.arange(Lp)[None, :]
    low = f[..., (t - t0) % Lp]
    res = {'two_point_low': low, 'two_point_rest': np.zeros((M, 2, 2, 2, 2, Lp), dtype=np.complex128),
           'source_timeslice': 3}
    out = utils.lma_correlator(res, 'g3', 'g3')
    single = utils.meson_correlator(low[..., 3], 'g3', 'g3')
    assert np.array_equal(out, np.roll(single, -3, axis=-1))
    assert np.array_equal(out, utils.meson_correlator(f, 'g3', 'g3'))


def test_raises_on_a_two_point_result():
    res = _random_result(13)
    plain = {'two_point': res['two_point_rest'], 'source_timeslice': T0}
    with pytest.raises(Exception, match="two_point_low"):
        utils.lma_correlator(plain, 'g3', 'g3')
    bad = dict(res, two_point_low=res['two_point_low'][..., :-1])
    with pytest.raises(Exception, match="expected"):
        utils.lma_correlator(bad, 'g3', 'g3')
    with pytest.raises(Exception, match="unknown spin matrix"):
        utils.lma_correlator(res, 'g5', 'g3')


def test_low_mode_contraction_key():
    assert utils.LOW_MODE_CONTRACTIONS == ("host", "device")
    assert utils.low_mode_contraction_of({}) == "host"
    assert utils.low_mode_contraction_of({'low_mode_contraction': "device"}) == "device"
    with pytest.raises(Exception, match="low_mode_contraction"):
        utils.low_mode_contraction_of({'low_mode_contraction': "gpu"})
    params = gateway.set_params('schwinger128')
    params['function_tol'] = 1e-12
    params['low_mode_contraction'] = "device"
    tp = utils.trace_params_from_params(params, "hutchinson")
    assert tp['low_mode_contraction'] == "device"                      # the whitelist lets the key through
    tp['source_timeslice'] = 5
    tp['low_mode_contraction'] = "numpy"
    with pytest.raises(Exception, match="low_mode_contraction"):       # before any set-up: no operator is needed
        stoch_trace.lma_two_point(None, tp)
