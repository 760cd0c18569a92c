"""CPU: step15's cross-validation of the infill without a GPU -- the closed form of the hold-out against the literal lines
of the reference (twx/infill/xval_infill.py:78-86) in numpy, the rounding of ``ntrain_yrs``, the eligibility groups under
appended rows, the argument rules of the Python layer, header / binding / build naming, the resource table of a build,
the call-level failures of the three ``twxxv_`` entries (they come before any device work), and the executed-reference
golden (tests/golden/make_golden_xvalinfill.py): its held masks against the closed form, and the numpy restatement of
the matrix builder on a pool copy with the target's column masked against its lists of both stages (stations, nnghs,
max_dist exactly; ioa to the 1e-10 of DESIGN.md section 16)."""
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

from topowx_amd.dates import YMD, get_days_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import xvalinfill_cases as XC  # noqa: E402

NEW_KERNELS = ("k_xv_holdout", "k_xv_score")


def test_closed_form_equals_the_literal_lines():
    from topowx_amd import _qalib
    rs = np.random.RandomState(15)
    for yrs in (0, 0.25, 2, 5, 6, 40 / 365.25):                     # the binding's nkeep is the literal line 73
        assert _qalib.xval_nkeep(yrs) == XC.nmask_of(yrs)
    for nd in XC.HOLD_NDAYS + (2191,):
        rows = np.concatenate([XC.holdout_rows(nd), np.where(rs.rand(6, nd) < 0.4, np.nan, rs.randn(6, nd)).astype(np.float32)])
        for nkeep in XC.holdout_nkeeps(rows) + [_qalib.xval_nkeep(2), _qalib.xval_nkeep(0.25)]:
            for r in rows:
                want = XC.literal_holdout(r, nkeep)
                assert np.array_equal(XC.closed_form(r, nkeep), want), (nd, nkeep)
                nf = int(np.isfinite(r).sum())
                assert want.sum() == (max(nf - nkeep, 0) if nkeep > 0 else 0)     # nkeep 0 holds nothing: [-0:] is everything
                assert not (want & ~np.isfinite(r)).any()


def test_nkeep_rounds_half_to_even():
    from topowx_amd import _qalib
    assert 2 * 365.25 == 730.5 and 6 * 365.25 == 2191.5
    assert XC.nmask_of(2) == _qalib.xval_nkeep(2) == 730            # not 731
    assert XC.nmask_of(6) == _qalib.xval_nkeep(6) == 2192
    assert _qalib.xval_nkeep(5) == 1826 and _qalib.xval_nkeep(0) == 0 and _qalib.xval_nkeep(40 / 365.25) == 40
    assert isinstance(_qalib.xval_nkeep(2), int)


def _pool(n=6, nd=400, seed=3):
    from topowx_amd.qa import StationObsPool
    rs = np.random.RandomState(seed)
    tmin = np.round(rs.randn(nd)[:, None] * 5 + rs.randn(nd, n), 1).astype(np.float32)
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2001, 1, 1) + dt.timedelta(days=nd - 1))
    ids = np.array(["S%03d" % i for i in range(n)])
    return StationObsPool(ids, -110.0 + 0.1 * np.arange(n), np.full(n, 45.0), tmin, tmin + 10, days)


def test_month_groups_ignore_the_appended_rows():
    """The appended rows' own estimates (finite in some months, NaN in others) must not split the months into more calls."""
    from topowx_amd.infill.infill_daily import month_mask_groups
    mean, vari = np.ones((8, 12)), np.ones((8, 12))
    mean[2, :6] = np.nan                                             # a station of the table: two groups of months
    base = month_mask_groups(mean[:6], vari[:6])
    assert [m for _, m in base] == [list(range(6)), list(range(6, 12))]
    mean[6, ::2] = np.nan                                            # appended rows
    vari[7, 5] = np.nan
    assert len(month_mask_groups(mean, vari)) > 2
    never = np.zeros(8, bool)
    never[6:] = True
    got = month_mask_groups(mean, vari, never)
    assert [m for _, m in got] == [m for _, m in base]
    for (a, _), (b, _) in zip(got, base):
        assert np.array_equal(a[:6], b) and not a[6:].any()
    assert np.array_equal(month_mask_groups(mean, vari)[0][0], np.isfinite(mean[:, 0]) & np.isfinite(vari[:, 0]))


def test_argument_validation_of_the_python_layer():
    from topowx_amd.infill import XvalInfill, XvalInfillParams, build_infill_matrices, infill_daily_obs, infill_mean_variance
    pool = _pool()
    ok = np.ones((6, 12))
    p = XvalInfillParams(None, 3, 4, 0.99, True, 0, 0.5, 0.99, False)
    assert (p.min_daily_nnghs, p.nnghs_nnr, p.max_nnr_var, p.chk_perf, p.npcs, p.frac_obs_initnpcs, p.ppca_varyexplain,
            p.verbose, p.nnr_ds) == (3, 4, 0.99, True, 0, 0.5, 0.99, False, None)
    with pytest.raises(ValueError, match="xval_stnids"):
        XvalInfill(pool, "tmin", p, ok, ok)
    with pytest.raises(KeyError, match="not in the pool"):
        XvalInfill(pool, "tmin", p, ok, ok, ["S000", "nobody"])
    for kw in (dict(var_tair="prcp"), dict(mean=np.ones((5, 12))), dict(vari=np.ones((6, 11))), dict(xval_stnids=[]),
               dict(xval_stnids=["S001", "S001"])):
        a = dict(dict(pool=pool, var_tair="tmin", infill_params=p, mean=ok, vari=ok, xval_stnids=["S001"]), **kw)
        with pytest.raises(ValueError):
            XvalInfill(**a)
    xv = XvalInfill(pool, "tmax", p, ok, ok, ["S004", "S001"], ntrain_yrs=2)
    assert xv.nkeep == 730 and xv.stn_ids.tolist() == ["S004", "S001"] and xv.mths.tolist() == list(range(1, 13))
    assert xv.cols.tolist() == [4, 1] and xv.ngh_stn_mask.all()
    for kw in (dict(exclude_cols=np.array([6])), dict(exclude_cols=np.array([-2])), dict(exclude_cols=np.array([0, 1])),
               dict(exclude_cols=np.array([1.0])), dict(never_neighbour=np.zeros(5, bool)),
               dict(never_neighbour=np.zeros(6, int))):
        with pytest.raises(ValueError):
            build_infill_matrices(pool, "tmin", ["S000"], **kw)
    # the single-target facades keep refusing the reference's tair_mask
    with pytest.raises(NotImplementedError, match="belongs to step15"):
        infill_mean_variance("S000", pool, np.ones(6, bool), "tmin", tair_mask=np.zeros(400, bool))
    with pytest.raises(NotImplementedError, match="belongs to step15"):
        infill_daily_obs("S000", pool, "tmin", None, ok, ok, tair_mask=np.zeros(400, bool))


def test_header_binding_and_build():
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxxv_\w+)\s*\(", h))) == sorted(_qalib.XV_EXPORTS) == \
        ["twxxv_holdout", "twxxv_infill_matrix", "twxxv_score"]
    for macro, val in (("TWXXV_NGROUPS", _qalib.XV_NGROUPS), ("TWXXV_NSCORES", _qalib.XV_NSCORES)):
        m = re.search(r"#define %s (\d+)" % macro, h)
        assert m and int(m.group(1)) == val, macro
    assert _qalib.XV_NSCORES == _qalib.XV_NGROUPS + 1 == 13
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_xvalinfill.hip" in build
    assert os.path.exists(os.path.join(ROOT, "topowx_amd", "qa", "twx_xvalinfill.hip"))
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_infillmat.hip")).read()
    assert 'extern "C" int twxxv_infill_matrix' in src and src.count("static int if_matrix(") == 1
    assert src.count("j != self && j != excl && elig[j]") == 2     # both passes of k_if_ring, nothing else


def test_resource_table_lists_the_new_kernels():
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.XV_EXPORTS:
        assert hasattr(lib, name), name
    table = isa_resources.parse(res)
    for k in NEW_KERNELS + ("k_if_ring", "k_if_pair", "k_if_item"):
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    assert table["k_if_ring"]["lds"] == 12 * _qalib.MAX_RADIUS_NGH
    assert table["k_xv_holdout"]["lds"] == 0 and table["k_xv_score"]["lds"] == 256 * (8 + 8 + 4)


def test_entries_reject_bad_arguments_before_any_device_work():
    """Call-level failures (the library is needed, a GPU is not)."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    rows = XC.holdout_rows(65)
    with pytest.raises(_qalib.QaError, match="nkeep >= 0"):
        _qalib.holdout(rows, [0], -1)
    for bad in ([7], [-1]):
        with pytest.raises(_qalib.QaError, match="target index"):
            _qalib.holdout(rows, bad, 3)
    with pytest.raises(_qalib.QaError, match="ntarget >= 1"):
        _qalib.holdout(rows, [], 3)
    with pytest.raises(ValueError):
        _qalib.holdout(rows[0], [0], 3)
    with pytest.raises(ValueError):
        _qalib.holdout(rows, [0], 3.0)
    infill, obs, held, group = XC.score_series(64)
    for g in (12, -2):
        bad = group.copy()
        bad[5] = g
        with pytest.raises(_qalib.QaError, match="group"):
            _qalib.xval_score(infill, obs, held, bad)
    with pytest.raises(ValueError):
        _qalib.xval_score(infill, obs[:, :60], held, group)
    with pytest.raises(ValueError):
        _qalib.xval_score(infill, obs, held, group[:60])
    # the exclusion of twxxv_infill_matrix
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2001, 2, 9))
    rs = np.random.RandomState(3)
    ok = dict(lon=-110.0 + 0.1 * np.arange(6), lat=np.full(6, 45.0), obs=rs.randn(6, 40).astype(np.float32),
              ymd=np.array(days[YMD]), eligible=np.ones(6, bool), target_idx=np.array([0]), group=np.zeros(40, np.int8),
              nthres_all=np.array([27]), nthres_target_por=np.array([[27]]))
    for bad in (6, -2):
        with pytest.raises(_qalib.QaError, match="twxxv_infill_matrix: exclude index"):
            _qalib.infill_matrix(exclude_idx=np.array([bad]), **ok)
    with pytest.raises(_qalib.QaError, match="twxxv_infill_matrix: target index"):
        _qalib.infill_matrix(exclude_idx=np.array([1]), **dict(ok, target_idx=np.array([6])))
    with pytest.raises(ValueError, match="exclude_idx"):
        _qalib.infill_matrix(exclude_idx=np.array([1, 2]), **ok)


# ---- the golden of tests/golden/make_golden_xvalinfill.py (the executed reference) ----
IOA_TOL = 1e-10                    # a d1 sum re-ordered moves by about n 2^-53; the maker asserted 1e-9 margins


@pytest.fixture(scope="module")
def gold():
    return XC.load_gold()


@pytest.fixture(scope="module")
def gcase(gold):
    return XC.gold_case(gold)


def test_golden_content(gold, gcase):
    ids, lon, lat, tmin, days = gcase
    path = os.path.join(ROOT, "tests", "golden", "golden_xvalinfill_v1.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_ppca_v1.npz"))
    xval = gold["xval"].tolist()
    assert tmin.shape == (1461, 18) and xval == [0, 1, 6, 15] and int(gold["nkeep"]) == 730 == XC.nmask_of(float(gold["ntrain_yrs"]))
    assert (lon[6], lat[6]) == (lon[7], lat[7])                      # the co-located pair
    held = XC.gold_held(gold)
    nfin = np.isfinite(tmin[:, xval]).sum(axis=0)
    assert nfin[3] <= 730 and not held[3].any()                      # at most nkeep finite days: nothing is held
    assert ((held[:3].sum(axis=1) / nfin[:3] > 0.35) & (held[:3].sum(axis=1) / nfin[:3] < 0.6)).all()
    assert float(gold["ioa_gap"]) > 1e-9 and float(gold["cand_margin"]) > 1e-9 and float(gold["ring_margin"]) > 1e-6
    for t, s in enumerate(xval):
        # two cross-validation stations rank each other, from their FULL records; the twin at distance 0
        for stage in (1, 2):
            off, idx, ioa, dist, nnghs, maxd = XC.gold_lists(gold, stage, t)
            assert off.size == 13 and (np.diff(off) >= nnghs).all() and (nnghs >= 3).all() and s not in idx
        # the station table: the estimate while infill_daily_obs runs, the original after run_xval (the restore)
        assert np.array_equal(gold["after_mean_%d" % t], gold["mean"][s]) and np.array_equal(gold["after_vari_%d" % t], gold["vari"][s])
        assert np.isfinite(gold["entered_mean_%d" % t]).all() and (gold["entered_vari_%d" % t] > 0).all()
        if held[t].any():
            assert (gold["entered_mean_%d" % t] != gold["mean"][s]).all()
        for k in ("obs_nan", "infill_nan"):                          # NaN exactly off the held days
            assert np.array_equal(np.unpackbits(gold["%s_%d" % (k, t)])[:1461].astype(bool), ~held[t]), (k, t)
    assert 1 in gold["s1_idx_0"] and 0 in gold["s1_idx_1"] and 1 in gold["s2_idx_0"] and 0 in gold["s2_idx_1"]
    first = gold["s1_idx_2"][:gold["s1_off_2"][1]]
    assert 7 in first and gold["s1_dist_2"][:first.size][first == 7][0] == 0.0


def test_held_masks_equal_the_golden(gold, gcase):
    ids, lon, lat, tmin, days = gcase
    held = XC.gold_held(gold)
    for t, s in enumerate(gold["xval"]):
        assert np.array_equal(XC.closed_form(tmin[:, s], int(gold["nkeep"])), held[t]), int(s)
        assert np.array_equal(XC.literal_holdout(tmin[:, s], int(gold["nkeep"])), held[t]), int(s)


def test_restated_matrix_builder_under_masking_equals_the_golden(gold, gcase):
    """tests/restate_infillmat.py on a pool copy with the target's column masked, both stages: the ranked stations, nnghs
    and max_dist exactly, ioa within 1e-10."""
    import restate_infillmat as RI
    from topowx_amd.dates import MONTH
    ids, lon, lat, tmin, days = gcase
    held = XC.gold_held(gold)
    grp = (np.asarray(days[MONTH]) - 1).astype(np.int8)
    worst = 0.0
    for t, s in enumerate(gold["xval"]):
        cp = tmin.copy()
        cp[held[t], s] = np.nan
        m2, v2 = gold["mean"].copy(), gold["vari"].copy()
        m2[s], v2[s] = gold["entered_mean_%d" % t], gold["entered_vari_%d" % t]
        for stage in (1, 2):
            off, idx, ioa, dist, nnghs, maxd = XC.gold_lists(gold, stage, t)
            for g in range(12):
                elig = np.isfinite(gold["mean"][:, 0]) if stage == 1 else np.isfinite(m2[:, g]) & np.isfinite(v2[:, g])
                w = RI.run(lon, lat, cp, elig, [s], np.where(grp == g, 0, -1).astype(np.int8))
                a = slice(off[g], off[g + 1])
                assert w["status"][0, 0] == RI.OK and not RI.knife(w).any()
                assert np.array_equal(w["idx"], idx[a]), (stage, int(s), g)
                assert w["nnghs"][0, 0] == nnghs[g] and w["max_dist"][0, 0] == maxd[g]
                worst = max(worst, float(np.abs(w["ioa"] - ioa[a]).max()))
    print("max |ioa - golden| %.3g" % worst)
    assert worst <= IOA_TOL
