"""bench.py's command line, on CPU: a plain run is the lean one (``--full`` and ``--dump-outputs``
are off by default), ``--steps`` must time at least one step, and the sampler that keeps
``--dump-outputs`` under its size budget is fixed from run to run."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    b = bench.parse(["--full", "--dump-outputs", "some/dir", "--no-cpu-baseline"])
    assert b.full is True and b.dump_outputs == "some/dir" and b.no_cpu_baseline


def test_steps_below_one_are_refused():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_fixed_sample_is_seeded_and_within_budget():
    a = np.arange(10_000, dtype=np.float32).reshape(100, 100)
    assert bench._fixed_sample(a, a.nbytes) is a  # fits: unchanged, shape kept
    s1, s2 = bench._fixed_sample(a, 4000), bench._fixed_sample(a.copy(), 4000)
    assert s1.nbytes == 4000 and s1.dtype == np.float32
    assert np.array_equal(s1, s2)  # the same elements every run
    assert np.all(np.diff(s1) > 0)  # distinct elements, in index order
    assert bench.DUMP_BUDGET_BYTES <= 64 * 1000 * 1000
