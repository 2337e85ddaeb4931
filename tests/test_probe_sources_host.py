"""CPU: the engine call trace of the probe sources -- which engine handle generates, selects, runs and fetches what,
in which order, for every estimator method: the share of a batch per handle, the prefetch into the other slot, the
resolved fetch per mode and the round stride the probe loop hands its source.  Fake engines record their calls (one
list per engine: the engines of a batch run on threads); no GPU and no engine library is needed."""
from types import SimpleNamespace

import numpy as np
import pytest

from deflatedmlmc_schwinger_amd import stoch_trace, utils
from deflatedmlmc_schwinger_amd.engine import Engine

TOL = 1e-7
PARAMS = {'function_params': {'tol': TOL}}
LEVEL_N = [2048, 512, 128]                    # maxiter = n below 1000, otherwise 1000
TAILS = {"hutch_fetch_shifts": (3,), "hutch_fetch_loops": (2, 2, 2, 4), "hutch_fetch_mlmc_loops": (2, 2, 2, 4),
         "hutch_fetch_two_point": (2, 2, 2, 2, 2, 4)}


class FakeEngine:
    """Records every call; probe k of the stream evaluates to k (iterations k and 2 k), in every entry of a resolved
    result."""
    hutch_fetch_resolved = Engine.hutch_fetch_resolved

    def __init__(self):
        self.calls = []
        self._slots = {}
        self._first = None

    def stream_set(self, window):
        self.calls.append(("stream_set", int(window[0])))

    def probes_generate(self, slot, level, nb, pos, kind="z2"):
        self.calls.append(("probes_generate", slot, level, nb, pos, kind))
        assert pos % LEVEL_N[level] == 0
        self._slots[slot] = np.arange(nb) + pos // LEVEL_N[level]

    def probes_select(self, slot):
        self.calls.append(("probes_select", slot))
        self._first = self._slots[slot]

    def hutch_run(self, mode, level, tol, maxiter=1000):
        self.calls.append(("hutch_run", mode, level, tol, maxiter))

    def hutch_fetch(self):
        self.calls.append(("hutch_fetch",))
        k = self._first
        return k.astype(np.complex128), k.astype(np.int32), (2 * k).astype(np.int32)

    def _resolved(self, name):
        self.calls.append((name,))
        k = self._first.astype(np.complex128)
        return k.reshape((-1,) + (1,) * len(TAILS[name])) * np.ones(TAILS[name])

    def hutch_fetch_shifts(self):
        return self._resolved("hutch_fetch_shifts")

    def hutch_fetch_loops(self):
        return self._resolved("hutch_fetch_loops")

    def hutch_fetch_mlmc_loops(self):
        return self._resolved("hutch_fetch_mlmc_loops")

    def hutch_fetch_two_point(self):
        return self._resolved("hutch_fetch_two_point")


def fake_solver(nr_engines, skip_level=False):
    levels = [SimpleNamespace(A=SimpleNamespace(shape=(n, n))) for n in LEVEL_N]
    return SimpleNamespace(engines=[FakeEngine() for _ in range(nr_engines)], ml=SimpleNamespace(levels=levels),
                           skip_level=skip_level)


def generated(mg, method, level, first, count, deflated=False, prefetch=None, ready=None):
    return utils.probe_batch_generated(mg, PARAMS, method, level, first, count, "z2", prefetch=prefetch, ready=ready,
                                       deflated=deflated)


def device_probes(mg, method, level, columns=None, deflated=False):
    return stoch_trace.DeviceProbes(mg, PARAMS, method, level, "z2", columns=columns, deflated=deflated)


def resolved_loop(evaluate, n, tols, control, max_nr_ests, batch, comm=None):
    return stoch_trace.run_probe_loop(evaluate, n, tols, max_nr_ests, batch, comm=comm, control=control)


# (method, level, mg_solver.skip_level, deflated) -> (engine mode, resolved fetch): the eleven modes
MODES = [("hutchinson", 0, False, False, 0, None),
         ("mlmc", 1, True, False, 1, None),
         ("mlmc", 0, True, False, 2, None),
         ("level", 2, False, False, 3, None),
         ("shifts", 0, False, False, 4, "hutch_fetch_shifts"),
         ("loops", 0, False, False, 5, "hutch_fetch_loops"),
         ("two_point", 0, False, False, 6, "hutch_fetch_two_point"),
         ("mlmc_loops", 1, True, False, 7, "hutch_fetch_mlmc_loops"),
         ("mlmc_loops", 0, True, False, 8, "hutch_fetch_mlmc_loops"),
         ("mlmc_loops", 1, True, True, 9, "hutch_fetch_mlmc_loops"),
         ("mlmc_loops", 0, True, True, 10, "hutch_fetch_mlmc_loops")]


@pytest.mark.parametrize("method,level,skip_level,deflated,mode,fetch", MODES,
                         ids=["mode%d" % m[4] for m in MODES])
def test_one_engine_batch_of_five(method, level, skip_level, deflated, mode, fetch):
    mg = fake_solver(1, skip_level)
    e, f, c, prefetched = generated(mg, method, level, 3, 5, deflated)
    n = LEVEL_N[level]
    maxiter = {2048: 1000, 512: 512, 128: 128}[n]
    expected = [("probes_generate", 0, level, 5, 3 * n, "z2"), ("probes_select", 0),
                ("hutch_run", mode, level, TOL, maxiter), ("hutch_fetch",)]
    if fetch is not None:
        expected.append((fetch,))
    assert mg.engines[0].calls == expected
    assert prefetched is None
    assert e.shape == (5,) + (TAILS[fetch] if fetch else ())
    assert np.array_equal(e.reshape(5, -1)[:, 0], [3, 4, 5, 6, 7])
    assert np.array_equal(f, [3, 4, 5, 6, 7]) and np.array_equal(c, [6, 8, 10, 12, 14])


def test_without_level_skipping_the_mlmc_modes_are_the_plain_ones():
    for method, deflated, mode in [("mlmc", False, 1), ("mlmc_loops", False, 7), ("mlmc_loops", True, 9)]:
        mg = fake_solver(1, False)
        generated(mg, method, 0, 0, 5, deflated)
        assert mg.engines[0].calls[2] == ("hutch_run", mode, 0, TOL, 1000)


def test_unknown_method_raises():
    with pytest.raises(Exception, match="unknown method"):
        generated(fake_solver(1), "other", 0, 0, 5)


@pytest.mark.parametrize("method,fetch", [("hutchinson", None), ("loops", "hutch_fetch_loops")])
def test_127_probes_stay_on_the_first_of_two_engines(method, fetch):
    mg = fake_solver(2)
    e, f, c, _ = generated(mg, method, 0, 10, 127)
    tail = [(fetch,)] if fetch else []
    assert mg.engines[0].calls == [("probes_generate", 0, 0, 127, 10 * 2048, "z2"), ("probes_select", 0),
                                   ("hutch_run", 0 if fetch is None else 5, 0, TOL, 1000), ("hutch_fetch",)] + tail
    assert mg.engines[1].calls == []
    assert np.array_equal(f, np.arange(10, 137))


@pytest.mark.parametrize("method,mode,fetch", [("hutchinson", 0, None), ("shifts", 4, "hutch_fetch_shifts"),
                                               ("two_point", 6, "hutch_fetch_two_point")])
def test_128_probes_are_shared_64_64_by_two_engines(method, mode, fetch):
    mg = fake_solver(2)
    e, f, c, _ = generated(mg, method, 0, 10, 128)
    tail = [(fetch,)] if fetch else []
    rest = [("probes_select", 0), ("hutch_run", mode, 0, TOL, 1000), ("hutch_fetch",)] + tail
    assert mg.engines[0].calls == [("probes_generate", 0, 0, 64, 10 * 2048, "z2")] + rest
    assert mg.engines[1].calls == [("probes_generate", 0, 0, 64, 74 * 2048, "z2")] + rest
    assert np.array_equal(e.reshape(128, -1)[:, -1], np.arange(10, 138))        # gathered in probe order
    assert np.array_equal(f, np.arange(10, 138)) and np.array_equal(c, 2 * np.arange(10, 138))


@pytest.mark.parametrize("method,level,mode,fetch", [("mlmc", 1, 1, None),
                                                     ("mlmc_loops", 1, 7, "hutch_fetch_mlmc_loops")])
def test_130_probes_on_three_engines_split_at_43_and_86(method, level, mode, fetch):
    mg = fake_solver(3)
    e, f, c, _ = generated(mg, method, level, 7, 130)
    tail = [(fetch,)] if fetch else []
    rest = [("probes_select", 0), ("hutch_run", mode, level, TOL, 512), ("hutch_fetch",)] + tail
    assert mg.engines[0].calls == [("probes_generate", 0, level, 43, 7 * 512, "z2")] + rest
    assert mg.engines[1].calls == [("probes_generate", 0, level, 43, 50 * 512, "z2")] + rest
    assert mg.engines[2].calls == [("probes_generate", 0, level, 44, 93 * 512, "z2")] + rest
    assert np.array_equal(f, np.arange(7, 137))


def test_prefetch_generates_into_the_other_slot_and_the_next_call_selects_it():
    mg = fake_solver(1)
    eng = mg.engines[0]
    run = [("hutch_run", 0, 0, TOL, 1000), ("hutch_fetch",)]
    e, f, c, ready = generated(mg, "hutchinson", 0, 20, 5, prefetch=(25, 5))
    assert ready == (25, 5, 1)
    assert eng.calls == [("probes_generate", 0, 0, 5, 20 * 2048, "z2"), ("probes_generate", 1, 0, 5, 25 * 2048, "z2"),
                         ("probes_select", 0)] + run
    assert np.array_equal(f, [20, 21, 22, 23, 24])
    del eng.calls[:]
    e, f, c, ready = generated(mg, "hutchinson", 0, 25, 5, prefetch=(30, 5), ready=ready)
    assert ready == (30, 5, 0)
    assert eng.calls == [("probes_generate", 0, 0, 5, 30 * 2048, "z2"), ("probes_select", 1)] + run
    assert np.array_equal(f, [25, 26, 27, 28, 29])
    del eng.calls[:]
    # a `ready` that is not this batch is not used: the batch generates for itself into slot 0
    e, f, c, ready = generated(mg, "hutchinson", 0, 40, 5, ready=ready)
    assert ready is None
    assert eng.calls == [("probes_generate", 0, 0, 5, 40 * 2048, "z2"), ("probes_select", 0)] + run


def test_prefetch_on_two_engines_uses_the_shares_of_the_next_batch():
    mg = fake_solver(2)
    _, _, _, ready = generated(mg, "hutchinson", 0, 0, 128, prefetch=(128, 130))
    assert ready == (128, 130, 1)
    assert mg.engines[0].calls[:2] == [("probes_generate", 0, 0, 64, 0, "z2"),
                                       ("probes_generate", 1, 0, 65, 128 * 2048, "z2")]
    assert mg.engines[1].calls[:2] == [("probes_generate", 0, 0, 64, 64 * 2048, "z2"),
                                       ("probes_generate", 1, 0, 65, 193 * 2048, "z2")]


def test_prefetch_for_another_number_of_engines_is_not_issued():
    mg = fake_solver(2)
    _, _, _, ready = generated(mg, "hutchinson", 0, 0, 128, prefetch=(128, 100))
    assert ready is None
    for k in range(2):
        assert [c for c in mg.engines[k].calls if c[0] == "probes_generate"] \
            == [("probes_generate", 0, 0, 64, 64 * k * 2048, "z2")]


class FakeStream:
    """ProbeStream without the library: the window's first word names the stream, jumps are recorded."""
    jumps = []

    @classmethod
    def from_numpy_state(cls, state=None):
        return cls()

    def window(self):
        return np.full(624, 77, dtype=np.uint32)

    def jump(self, ndraws):
        FakeStream.jumps.append(ndraws)

    def numpy_state(self):
        return np.random.get_state()


def test_scalar_source_prefetches_the_round_the_loop_expects_next():
    mg = fake_solver(2)
    src = device_probes(mg, "hutchinson", 0)
    src.begin(FakeStream())
    assert [eng.calls for eng in mg.engines] == [[("stream_set", 77)], [("stream_set", 77)]]
    src.round_stride = 5
    e, f, c = src(0, 5)
    src.round_stride = 0
    e2, f2, c2 = src(5, 5)
    assert mg.engines[1].calls == [("stream_set", 77)]
    run = [("hutch_run", 0, 0, TOL, 1000), ("hutch_fetch",)]
    assert mg.engines[0].calls == [("stream_set", 77), ("probes_generate", 0, 0, 5, 0, "z2"),
                                   ("probes_generate", 1, 0, 5, 5 * 2048, "z2"), ("probes_select", 0)] + run \
        + [("probes_select", 1)] + run
    assert np.array_equal(f, [0, 1, 2, 3, 4]) and np.array_equal(f2, [5, 6, 7, 8, 9])
    # begin() forgets what was prefetched
    src.round_stride = 5
    src(10, 5)
    src.begin(FakeStream())
    del mg.engines[0].calls[:]
    src(15, 5)
    assert mg.engines[0].calls[:3] == [("probes_generate", 0, 0, 5, 15 * 2048, "z2"),
                                       ("probes_generate", 1, 0, 5, 20 * 2048, "z2"), ("probes_select", 0)]


RESOLVED_SOURCES = [("shifts", 0, False, None, 4, "hutch_fetch_shifts", 3),
                    ("loops", 0, False, "loops", 5, "hutch_fetch_loops", 33),
                    ("two_point", 0, False, "two_point", 6, "hutch_fetch_two_point", 129),
                    ("mlmc_loops", 1, False, "loops", 7, "hutch_fetch_mlmc_loops", 33),
                    ("mlmc_loops", 1, True, "loops", 9, "hutch_fetch_mlmc_loops", 33)]


@pytest.mark.parametrize("method,level,deflated,cols,mode,fetch,width", RESOLVED_SOURCES,
                         ids=["mode%d" % r[4] for r in RESOLVED_SOURCES])
def test_resolved_sources_never_prefetch(method, level, deflated, cols, mode, fetch, width):
    mg = fake_solver(1)
    columns = {None: None, "loops": lambda e: stoch_trace.loop_columns(e, 1),
               "two_point": lambda e: stoch_trace.two_point_columns(e, 1)}[cols]
    src = device_probes(mg, method, level, columns, deflated)
    src.begin(FakeStream())
    n = LEVEL_N[level]
    rest = [("probes_select", 0), ("hutch_run", mode, level, TOL, min(n, 1000)), ("hutch_fetch",), (fetch,)]
    expected = [("stream_set", 77)]
    for stride, first in [(5, 0), (5, 5), (0, 10), (7, 15)]:
        src.round_stride = stride
        e, f, c = src(first, 5)
        expected += [("probes_generate", 0, level, 5, first * n, "z2")] + rest
        assert e.shape == (5, width)
        assert np.array_equal(f, first + np.arange(5))
    assert mg.engines[0].calls == expected
    # the control column of loop_columns / two_point_columns: 2 L = 8 resp. 4 L = 16 entries of value k
    if cols is not None:
        assert np.array_equal(e[:, -1], (8 if cols == "loops" else 16) * (15 + np.arange(5)))


class RecordingSource:
    def __init__(self, width=None):
        self.round_stride = -1
        self.width = width
        self.calls = []
        self.begun = 0

    def begin(self, entry_stream):
        self.begun += 1

    def __call__(self, first_probe, count):
        self.calls.append((first_probe, count, self.round_stride))
        k = first_probe + np.arange(count)
        e = k.astype(np.complex128) if self.width is None else np.outer(k, np.ones(self.width))
        return e, k, 2 * k


@pytest.fixture
def fake_stream(monkeypatch):
    monkeypatch.setattr(stoch_trace, "ProbeStream", FakeStream)
    FakeStream.jumps = []
    return FakeStream


def test_probe_loop_sets_the_round_stride_while_two_full_rounds_fit(fake_stream):
    src = RecordingSource()
    out = stoch_trace.run_probe_loop(src, 100, 0.0, 48, 16)
    assert src.begun == 1
    assert src.calls == [(0, 16, 16), (16, 16, 16), (32, 16, 0)]
    assert out["index"] == 47 and out["rounds"] == 3 and out["solved"] == 48
    assert np.array_equal(out["ests"], np.arange(48)) and np.array_equal(out["iters_coarse"], 2 * np.arange(48))
    assert fake_stream.jumps == [48 * 100]
    src = RecordingSource()
    stoch_trace.run_probe_loop(src, 100, 0.0, 40, 16)
    assert src.calls == [(0, 16, 16), (16, 16, 0), (32, 8, 0)]


def test_probe_loop_with_a_control_column(fake_stream):
    src = RecordingSource(width=3)
    out = resolved_loop(src, 100, np.array([0.0, 0.0, 0.0]), 1, 40, 16)
    assert [c[:2] for c in src.calls] == [(0, 16), (16, 16), (32, 8)]
    assert out["index"] == 39 and out["ests"].shape == (40, 3) and out["avgs"].shape == (3,)
    assert out["avg"] == out["avgs"][1] == 19.5 and out["dev"] == out["devs"][1]
    assert not out["converged"].any()
    assert fake_stream.jumps == [40 * 100]
    with pytest.raises(Exception, match=r"displaced probe batch of shape \(16, 3\), expected \(16, 4\)"):
        resolved_loop(RecordingSource(width=3), 100, np.zeros(4), 1, 40, 16)
    with pytest.raises(Exception, match=r"displaced traces \(x_displacements\) run on one rank; got 2"):
        resolved_loop(RecordingSource(width=3), 100, np.zeros(3), 1, 40, 16, comm=SimpleNamespace(world=2))
