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


def assert_fast_oracle_where(got, want, what=""):
    """assert_fast_oracle for grids with failing cells: the oracle's status on EVERY cell; where it is 0, the oracle's ninvalid
    (two-variable daily runs), normals / SE within 1e-5 degC and daily values within 1; fill values elsewhere.  Returns the
    worst normals / SE error and the number of daily values off by one."""
    assert np.array_equal(got["status"], want["status"]), (what, got["status"].tolist(), want["status"].tolist())
    ok = want["status"] == 0
    worst, off = 0.0, 0
    for k in sorted(got):
        if k == "status":
            continue
        assert np.array_equal(got[k][..., ~ok], want[k][..., ~ok].astype(got[k].dtype)), (what, k, "fill values")
        if not ok.any():
            continue
        if k == "ninvalid":
            assert np.array_equal(got[k][ok], want[k][ok]), (what, k)
        elif k.startswith("daily_"):
            d = np.abs(got[k][:, ok].astype(int) - want[k][:, ok].astype(int))
            assert d.max() <= 1, (what, k, int(d.max()))
            off += int((d != 0).sum())
        else:
            err = float(np.abs(got[k][:, ok].astype(np.float64) - want[k][:, ok]).max())
            assert err <= FAST_BAR, (what, k, err)
            worst = max(worst, err)
    return worst, off


def assert_fast_oracle(got, want):
    """The default (fast) build: the oracle's status and ninvalid, normals / SE within 1e-5 degC, daily values within 1."""
    assert np.array_equal(got["status"], want["status"]) and np.all(got["status"] == 0)
    assert np.array_equal(got["ninvalid"], want["ninvalid"])
    for k in ("norm_tmin", "norm_tmax", "se_tmin", "se_tmax"):
        err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
        assert err <= FAST_BAR, (k, err)
    for k in ("daily_tmin", "daily_tmax"):
        assert np.abs(got[k].astype(int) - want[k].astype(int)).max() <= 1, k
