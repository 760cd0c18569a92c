"""CPU: ``bench.py --dump-outputs`` writes float32 / float64 .npy files of at most 64 MB in all; beyond that a fixed, seeded
sample of every array, the same from run to run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    st = np.arange(-3, 9, dtype=np.int32).reshape(3, 4)
    nm = np.linspace(-5, 5, 24, dtype=np.float32).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path), {"status": st, "norm": nm})
    got = _load(str(tmp_path))
    assert got["status"].dtype == np.float64 and np.array_equal(got["status"], st)
    assert got["norm"].dtype == np.float32 and np.array_equal(got["norm"], nm)


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    cap = 2 * 10 ** 6
    big = {"a": np.arange(600000, dtype=np.float32).reshape(6, 100000), "b": np.arange(300000, dtype=np.int32)}
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), big, max_bytes=cap)
    one, two = _load(str(tmp_path / "one")), _load(str(tmp_path / "two"))
    assert sum(os.path.getsize(str(tmp_path / "one" / (k + ".npy"))) for k in one) <= cap
    for k in one:
        assert np.array_equal(one[k], two[k]) and one[k].ndim == 1 and 0 < one[k].size < big[k].size, k
        # a sample of the values, in their order (sorted flat indices of an arange are increasing values)
        assert np.all(np.diff(one[k]) > 0) and np.isin(one[k], big[k].ravel()).all(), k
    assert one["a"].dtype == np.float32 and one["b"].dtype == np.float64
