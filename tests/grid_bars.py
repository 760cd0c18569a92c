"""The criteria by which a grid run (interp_grid, daily=True) is compared with the oracle's grid, shared by
tests/test_gpu_kernel_matrix.py and tests/test_gpu_gwr_matrix.py."""
import numpy as np

FAST_BAR, F64_BAR = 1e-5, 1e-10                              # degC (the fp64 builds measure ~7e-14)


def assert_f4_oracle(got, want, what):
    """An fp64 build (TWX_FLAG_UK_F64_ALL): the oracle's status, ninvalid, f4 normals / SE bits and daily values."""
    assert np.array_equal(got["status"], want["status"]) and np.all(got["status"] == 0), what
    assert np.array_equal(got["ninvalid"], want["ninvalid"]), what
    for k in ("norm_tmin", "norm_tmax", "se_tmin", "se_tmax"):
        n = int((got[k] != want[k].astype(np.float32)).sum())
        assert n == 0, (what, k, n)                                             # the same f4 bits
    for k in ("daily_tmin", "daily_tmax"):
        assert (got[k] != want[k]).mean() < 2e-6, (what, k, int((got[k] != want[k]).sum()))


def assert_fast_oracle(got, want):
    """The default (fast) build: the oracle's status and ninvalid, normals / SE within 1e-5 degC, daily values within 1."""
    assert np.array_equal(got["status"], want["status"]) and np.all(got["status"] == 0)
    assert np.array_equal(got["ninvalid"], want["ninvalid"])
    for k in ("norm_tmin", "norm_tmax", "se_tmin", "se_tmax"):
        err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
        assert err <= FAST_BAR, (k, err)
    for k in ("daily_tmin", "daily_tmax"):
        assert np.abs(got[k].astype(int) - want[k].astype(int)).max() <= 1, k
