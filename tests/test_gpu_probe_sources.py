"""GPU: a batch the engines generate from the stream (utils.probe_batch_generated) against the same probes drawn
on the host and uploaded (utils.probe_batch), for every resolved method -- the results and both iteration arrays,
bit for bit.  Hierarchy and registrations are those of test_gpu_mlmc_loops.py on schwinger16."""
import os

import numpy as np
import pytest

import test_gpu_mlmc_loops as base

pytestmark = pytest.mark.gpu

from deflatedmlmc_schwinger_amd import utils  # noqa: E402
from deflatedmlmc_schwinger_amd.engine import ProbeStream  # noqa: E402

SEED = 4242
NB = 6


@pytest.fixture(scope="module")
def p16():
    tv = np.load(os.path.join(base.HERE, "golden", "schwinger16_testvectors.npz"))
    p = base.Problem('schwinger16', [tv["tv0"], tv["tv1"]], {'accuracy_mg_eigvs': 'high'})
    assert [l.A.shape[0] for l in p.levels] == [512, 256, 64]
    p.mg.skip_level = False
    utils.register_shifts(p.mg, [2 * p.L * d for d in (0, 1, 5, 15)])
    utils.register_loop_momenta(p.mg, [0, 1, 15])
    utils.register_two_point(p.mg, 5, [0, 1])
    return p


CASES = [("shifts", 0, False, (4,)),
         ("loops", 0, False, (3, 2, 2, 16)),
         ("two_point", 0, False, (2, 2, 2, 2, 2, 16)),
         ("mlmc_loops", 0, False, (3, 2, 2, 16)),
         ("mlmc_loops", 1, False, (3, 2, 2, 16)),
         ("mlmc_loops", 1, True, (3, 2, 2, 16))]


@pytest.mark.parametrize("method,level,deflated,tail", CASES,
                         ids=["shifts", "loops", "two_point", "mlmc_loops-l0", "mlmc_loops-l1", "mlmc_loops-l1-defl"])
def test_generated_batch_equals_uploaded_batch_16(p16, method, level, deflated, tail):
    """Six probes of the stream seeded with 4242, once generated on the device at stream position 0, once drawn by
    draw_probes and uploaded: np.array_equal on the resolved result and on both iteration arrays.  The commit before
    this test gave bitwise equality in all six cases (relative difference 0.0), and two runs of either form agreed
    bit for bit (run-to-run spread 0.0), so no tolerance is needed."""
    p = p16
    n = p.levels[level].A.shape[0]
    if deflated:
        p.eng.set_level_deflation(level, np.linalg.qr(base._rand((n, 4), 77))[0])
    try:
        np.random.seed(SEED)
        window = ProbeStream.from_numpy_state().window()
        for eng in utils._engines(p.mg):
            eng.stream_set(window)
        gen = utils.probe_batch_generated(p.mg, p.tp, method, level, 0, NB, "z2", deflated=deflated)
        up = utils.probe_batch(p.mg, p.tp, method, utils.draw_probes(NB, n, "z2"), level, deflated=deflated)
    finally:
        if deflated:
            p.eng.set_level_deflation(level, None)
    assert gen[3] is None
    assert gen[0].shape == up[0].shape == (NB,) + tail
    assert np.max(np.abs(up[0])) > 0 and up[1].min() >= 1
    for g, u, what in zip(gen[:3], up, ("result", "iters_fine", "iters_coarse")):
        assert np.array_equal(g, u), what
