"""Generate tests/golden/golden_nnr_v1.npz by EXECUTING the reference's reanalysis reader, its PCA and the cut of the infill
on the seeded case of tests/nnr_cases.py.  Needs the reference checkout (``make_golden.REF``); the tests only read the
fixture.

    python tests/golden/make_golden_nnr.py

Executed (read at run time, nothing of the text is stored):
  * twx/utils/util_geo.py:19-40 (``grt_circle_dist``);
  * twx/db/reanalysis.py:314-321 (the class constants) and :372-432 (``get_nngh_matrix``) under a class header of ours, on
    in-memory stand-ins of the datasets (``dimensions``, ``variables[name][day_mask, :, lat, lon]``); the attributes that
    ``__init__`` sets are set by hand, since :353 is Python 2 only;
  * twx/utils/pca.py:24-76 (``pca_svd``);
  * twx/infill/infill_normals.py:347-356, the reader call, ``np.take``, ``pca_svd`` and the cut, placed under a function
    header of ours; run at ``max_nnr_var`` 0.99 and 0.90.

The fixture holds: the checksum of the inputs; per station and variable (tmin, tmax) the time slot, the cell order, the
column order and the sha256 of the returned matrix; per distinct Tmax matrix and calendar month ``ncomp`` at 0.99 and 0.90,
``var_explain``, the measured error of the executed scores and ``var_explain`` against the longdouble evaluation of
tests/restate_nnr.py (``e_ref``, ``e_ref_ve``) and that of the restated float64 Gram route (``e_gram``, ``e_gram_ve``); and the
executed scores at the 0.99 cut for the months of ``SCORE_MONTHS`` (every month's would outgrow the fixtures committed so
far; the error figures cover all months).  The maker refuses a case whose retained eigenvalues are closer than 1e-2
(relative), whose cumulative variance comes within 1e-6 of a cut, or on which the restated Gram route misses its own
bound.
"""
import hashlib
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nnr_cases as NC  # noqa: E402
import restate_nnr as RN  # noqa: E402

OUT = os.path.join(HERE, "golden_nnr_v1.npz")
SCORE_MONTHS = (0, 1, 5)                 # January (279 rows), February (254), June (270)
KMAX = 8                                 # columns of the per-component error tables


class _Var(object):
    def __init__(self, a):
        self.a = a

    def __getitem__(self, key):
        return self.a[key]


class _Ds(object):
    def __init__(self, name, a, has_level):
        self.variables = {name: _Var(a)}
        self.dimensions = {"time": None, "lat": None, "lon": None}
        if has_level:
            self.dimensions["level"] = None


def load_reference():
    import make_golden as mg
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    geo = {}
    exec(compile("\n" * 18 + mg._slice("twx/utils/util_geo.py", 19, 40), "util_geo.py", "exec"), geo)
    rd = dict(np=np, grt_circle_dist=geo["grt_circle_dist"])
    src = "class NNRNghData(object):\n" + mg._slice("twx/db/reanalysis.py", 314, 321) + "\n" + \
        mg._slice("twx/db/reanalysis.py", 372, 432)
    exec(compile(src, "reanalysis.py", "exec"), rd)
    pca = {}
    exec(compile("\n" * 23 + mg._slice("twx/utils/pca.py", 24, 76), "pca.py", "exec"), pca)
    inf = dict(np=np, pca_svd=pca["pca_svd"], LON="longitude", LAT="latitude", UTC_OFFSET="utc_offset")
    head = "def _cut(self, nnghs_nnr, max_nnr_var):\n    if True:\n"
    tail = "        return nnr_tair, var_explain, i\n"
    exec(compile(head + mg._slice("twx/infill/infill_normals.py", 347, 356) + tail, "infill_normals.py", "exec"), inf)
    return rd["NNRNghData"], inf["_cut"]


class _Self(object):
    pass


def reader(cls, case):
    r = cls.__new__(cls)
    r.ds_nnr = {var + slot: _Ds(var, case.data[(var, slot)], NC.LEVELS[var] is not None)
                for var in NC.NNR_VARS for slot in NC.NNR_TIMES}
    r.nnr_vars = cls.NNR_VARS
    r.day_mask = np.arange(case.days.size)
    r.days = case.days
    r.nnr_lons, r.nnr_lats = NC.LONS, NC.LATS
    llgrid = np.meshgrid(r.nnr_lons, r.nnr_lats)
    r.grid_lons, r.grid_lats = llgrid[0].ravel(), llgrid[1].ravel()
    return r


def main():
    cls, cut = load_reference()
    case = NC.case()
    r = reader(cls, case)
    ns = case.ids.size
    out = dict(input_sha=np.array(case.checksum()), ids=case.ids, cuts=np.array(NC.CUTS),
               score_months=np.array(SCORE_MONTHS))
    geo_dist = __import__("topowx_amd.reanalysis", fromlist=["grt_circle_dist"]).grt_circle_dist
    mats = {}
    for var in ("tmin", "tmax"):
        sha, cells, slots = [], np.zeros((ns, NC.NNGH), np.int32), []
        for s in range(ns):
            m = r.get_nngh_matrix(case.lon[s], case.lat[s], var, int(case.utc[s]), nngh=NC.NNGH)
            assert m.dtype == np.float32 and m.shape == (case.days.size, 32)
            d = geo_dist(case.lon[s], case.lat[s], r.grid_lons, r.grid_lats)
            assert np.unique(np.sort(d)[:NC.NNGH + 1]).size == NC.NNGH + 1, "a station is equidistant from two cells"
            cells[s] = np.argsort(d, kind="stable")[:NC.NNGH]
            slots.append(cls.UTC_OFFSET_TIMES[var][int(case.utc[s])])
            sha.append(hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest())
            mats[(var, s)] = m
        out["%s_matrix_sha" % var], out["%s_cells" % var], out["%s_slot" % var] = np.array(sha), cells, np.array(slots)
    # the column order of a returned matrix: per cell the variables in NNR_VARS order, each with its levels
    out["column_var"] = np.array([v for _ in range(NC.NNGH) for v in NC.NNR_VARS
                                  for _lev in range(1 if NC.LEVELS[v] is None else len(NC.LEVELS[v]))])
    # one decomposition per distinct Tmax matrix and month
    first = {}
    for s in range(ns):
        first.setdefault(str(out["tmax_matrix_sha"][s]), s)
    stn_set = np.array([list(first).index(str(out["tmax_matrix_sha"][s])) for s in range(ns)], np.int32)
    reps = np.array(list(first.values()), np.int32)
    nset = reps.size
    assert nset < ns, "no two stations share their cells and slot"
    ncomp = np.zeros((nset, 12, 2), np.int32)
    ve = np.zeros((nset, 12, 32))
    e_ref, e_gram = np.zeros((nset, 12, KMAX)), np.zeros((nset, 12, KMAX))
    e_ref_ve, e_gram_ve = np.zeros((nset, 12)), np.zeros((nset, 12))
    for x, s in enumerate(reps):
        for g in range(12):
            me = _Self()
            me.nnr_ds, me.tair_var, me.day_idx = r, "tmax", case.day_idx[g]
            me.stn = {"longitude": case.lon[s], "latitude": case.lat[s], "utc_offset": int(case.utc[s])}
            sc99, vx, i99 = cut(me, NC.NNGH, NC.CUTS[0])
            sc90, _, i90 = cut(me, NC.NNGH, NC.CUTS[1])
            ncomp[x, g] = i99 + 1, i90 + 1
            assert np.array_equal(sc90, sc99[:, :i90 + 1]) and sc99.shape[1] == i99 + 1 <= KMAX
            ve[x, g] = vx
            NC.check_separation(vx, ncomp[x, g])
            a = mats[("tmax", int(s))][case.day_idx[g]]
            ld_ve, ld_lam, ld_sc = RN.components_longdouble(a)
            re = RN.components(a, NC.CUTS)
            assert re["status"] == RN.OK and list(re["ncomp"]) == list(ncomp[x, g])
            k = i99 + 1
            e_ref[x, g, :k] = RN.column_error(sc99, ld_sc[:, :k])
            e_gram[x, g, :k] = RN.column_error(re["scores"][:, :k], ld_sc[:, :k])
            e_ref_ve[x, g] = np.abs(vx.astype(np.longdouble) - ld_ve).max()
            e_gram_ve[x, g] = np.abs(re["var_explain"].astype(np.longdouble) - ld_ve).max()
            bound = RN.score_bound(re["eigval"], re["scores"], e_ref[x, g], k)
            assert (e_gram[x, g, :k] <= bound).all(), ("the Gram route misses its own bound", x, g, e_gram[x, g, :k], bound)
            assert e_gram_ve[x, g] <= RN.var_explain_bound(re["var_explain"], e_ref_ve[x, g])
            if g in SCORE_MONTHS:
                out["scores_%d_%d" % (x, g)] = sc99
    out.update(stn_set=stn_set, set_rep=reps, ncomp=ncomp, var_explain=ve, e_ref=e_ref, e_gram=e_gram, e_ref_ve=e_ref_ve,
               e_gram_ve=e_gram_ve)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes, %d sets, ncomp99 %d..%d, ncomp90 %d..%d" % (OUT, os.path.getsize(OUT), nset, ncomp[..., 0].min(),
                                                                         ncomp[..., 0].max(), ncomp[..., 1].min(), ncomp[..., 1].max()))
    print("e_ref max %.3g  e_gram max %.3g  e_ref_ve max %.3g  e_gram_ve max %.3g" % (e_ref.max(), e_gram.max(), e_ref_ve.max(),
                                                                                   e_gram_ve.max()))


if __name__ == "__main__":
    main()
