"""CPU: the reanalysis columns without a GPU -- the reader ``NNRNghData`` on files written by ``ncio`` in both containers
against the executed-reference golden (tests/golden/make_golden_nnr.py): matrices bit for bit, cell and column order, the
error paths; the numpy restatement of the kernels' route (tests/restate_nnr.py) against the same golden within the bound
DESIGN.md section 22 states; header / binding / build naming; the resource table of a build; the call-level failures of
``twxnr_components`` (they come before any device work) and ``--nnr-dir`` on the three parsers."""
import ctypes
import hashlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nnr_cases as NC  # noqa: E402
import restate_nnr as RN  # noqa: E402

from topowx_amd import _qalib, ncio  # noqa: E402
from topowx_amd.reanalysis import NNRNghData, grt_circle_dist  # noqa: E402

NEW_KERNELS = ("k_nr_gram", "k_nr_eig", "k_nr_scores")
GOLD = os.path.join(ROOT, "tests", "golden", "golden_nnr_v1.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def case():
    return NC.case()


@pytest.fixture(scope="module", params=["NETCDF3_64BIT", None])
def reader(request, case, tmp_path_factory):
    path = case.write(str(tmp_path_factory.mktemp("nnr")), request.param)
    r = NNRNghData(path, (19810101, 19891231))
    yield r
    r.close()


def test_golden_content(gold, case):
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_spatial_v1.npz"))
    assert str(gold["input_sha"]) == case.checksum()
    assert gold["cuts"].tolist() == [0.99, 0.90] and gold["ncomp"].shape[1:] == (12, 2)
    assert (gold["ncomp"][..., 0] > gold["ncomp"][..., 1]).all() and gold["ncomp"].min() >= 1
    assert gold["stn_set"][0] == gold["stn_set"][1] and np.unique(gold["stn_set"]).size == gold["set_rep"].size == 11
    assert str(gold["tmax_slot"][2]) == "24z" and str(gold["tmax_slot"][0]) == "18z" and set(gold["tmin_slot"]) == {"12z"}
    assert max(len(d) for d in case.day_idx) == 279 >= 257 and min(len(d) for d in case.day_idx) == 254
    assert gold["column_var"].tolist() == ["tair", "hgt", "hgt", "thick", "rhum", "uwnd", "vwnd", "slp"] * 4


def test_reader_returns_the_reference_matrices_bit_for_bit(reader, gold, case):
    assert reader.days.size == case.days.size and reader.grid_lons.size == 30
    assert NNRNghData.NNR_VARS.tolist() == list(NC.NNR_VARS) and NNRNghData.NNR_TIMES.tolist() == list(NC.NNR_TIMES)
    for var in ("tmin", "tmax"):
        for s in range(case.ids.size):
            m = reader.get_nngh_matrix(case.lon[s], case.lat[s], var, int(case.utc[s]), nngh=NC.NNGH)
            assert m.dtype == np.float32 and m.shape == (case.days.size, 32)
            assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() == str(gold["%s_matrix_sha" % var][s]), (var, s)
            assert reader.nearest_cells(case.lon[s], case.lat[s], NC.NNGH).tolist() == gold["%s_cells" % var][s].tolist()
    # column order: cell after cell, the variables in NNR_VARS order, hgt with its two levels
    s = 4
    m = reader.get_nngh_matrix(case.lon[s], case.lat[s], "tmax", int(case.utc[s]))
    cells = gold["tmax_cells"][s]
    slot = str(gold["tmax_slot"][s])
    y, x = divmod(int(cells[1]), NC.LONS.size)
    assert np.array_equal(m[:, 8 + 1], case.data[("hgt", slot)][:, 0, y, x])
    assert np.array_equal(m[:, 8 + 2], case.data[("hgt", slot)][:, 1, y, x])
    assert np.array_equal(m[:, 8 + 7], case.data[("slp", slot)][:, y, x])
    # a shorter period
    short = NNRNghData(os.path.dirname(reader.ds_nnr["tair12z"].path), (19830101, 19831231))
    try:
        assert short.days.size == 365 and short.day_mask[0] == 730
        assert np.array_equal(short.get_nngh_matrix(case.lon[s], case.lat[s], "tmax", int(case.utc[s])), m[730:1095])
    finally:
        short.close()


def test_reader_error_paths(case, tmp_path):
    with pytest.raises(KeyError):
        NNRNghData.UTC_OFFSET_TIMES["tmax"][-3]
    bad = NC.NnrCase()
    bad.data = dict(bad.data)
    a = bad.data[("rhum", "18z")].copy()
    a[100, 0, 1, 1] = np.nan
    bad.data[("rhum", "18z")] = a
    b = bad.data[("slp", "24z")].copy()
    b[17, 3, 2] = ncio.FILL_F4
    bad.data[("slp", "24z")] = b
    r = NNRNghData(bad.write(str(tmp_path / "bad"), "NETCDF3_64BIT"), (19810101, 19891231))
    try:
        with pytest.raises(KeyError):
            r.get_nngh_matrix(case.lon[0], case.lat[0], "tmax", -3)
        with pytest.raises(KeyError):
            r.batched_components(case.lon[:1], case.lat[:1], "tmax", [-3], case.day_idx)
        with pytest.raises(ValueError, match="rhum18z.*lon -112.5, lat 45"):
            r.get_nngh_matrix(-112.4, 44.9, "tmax", -6)
        with pytest.raises(ValueError, match="slp24z.*lon -110, lat 40"):
            r.get_nngh_matrix(-110.1, 40.1, "tmax", -7)
        r.get_nngh_matrix(-110.1, 40.1, "tmax", -6)                     # the other slot is clean
    finally:
        r.close()
    assert abs(float(grt_circle_dist(-110.0, 45.0, -109.0, 46.0)) - 135.78628245) < 1e-6


def test_restatement_against_the_golden(gold, case):
    """``ncomp`` equal; ``var_explain`` and the sign-aligned scores within the bound, which is the larger of 100 x e_ref (the
    executed reference against the longdouble evaluation: up to 1.0e-13 for a score, 1.1e-15 for var_explain on this case)
    and 100 x eps x (lambda_1 / gap_k) x max |score_k|.  The restated float64 Gram route itself is up to 4.8e-14 from the
    longdouble evaluation."""
    assert gold["e_ref"].max() < 1e-12 and gold["e_gram"].max() < 1e-12
    for x, s in enumerate(gold["set_rep"]):
        for g in range(12):
            key = "scores_%d_%d" % (x, g)
            if key not in gold:
                continue
            m = _matrix(case, int(s), gold)[case.day_idx[g]]
            re = RN.components(m, NC.CUTS)
            assert re["status"] == RN.OK and list(re["ncomp"]) == gold["ncomp"][x, g].tolist()
            k = int(gold["ncomp"][x, g, 0])
            assert np.abs(re["var_explain"] - gold["var_explain"][x, g]).max() <= \
                RN.var_explain_bound(re["var_explain"], gold["e_ref_ve"][x, g])
            err = RN.column_error(gold[key], re["scores"][:, :k])
            assert (err <= RN.score_bound(re["eigval"], re["scores"], gold["e_ref"][x, g], k)).all(), (x, g, err)


def _matrix(case, s, gold):
    """The Tmax matrix of station s from the case's arrays (the reader's bytes, see above)."""
    slot = str(gold["tmax_slot"][s])
    cols = []
    for cell in gold["tmax_cells"][s]:
        y, x = divmod(int(cell), NC.LONS.size)
        for var in NC.NNR_VARS:
            a = case.data[(var, slot)]
            cols.append(a[:, :, y, x] if a.ndim == 4 else a[:, y, x][:, None])
    return np.hstack(cols)


def test_restatement_statuses():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((40, 5)).astype(np.float32)
    assert RN.components(a[:1])["status"] == RN.FEW_ROWS
    b = a.copy()
    b[3, 2] = np.inf
    assert (RN.components(b)["status"], RN.components(b)["bad_col"]) == (RN.NONFINITE, 2)
    b = a.copy()
    b[:, 4] = 7.0
    assert (RN.components(b)["status"], RN.components(b)["bad_col"]) == (RN.CONSTANT, 4)
    r = RN.components(a, (0.5, 0.999))
    assert r["ncomp"][0] < r["ncomp"][1] <= 5 and (r["loadings"][np.arange(5), np.abs(r["loadings"]).argmax(axis=1)] > 0).all()
    assert (RN.OK, RN.NOCONV, RN.NONFINITE, RN.CONSTANT, RN.FEW_ROWS) == \
        (_qalib.NR_OK, _qalib.NR_NOCONV, _qalib.NR_NONFINITE, _qalib.NR_CONSTANT, _qalib.NR_FEW_ROWS)


def test_header_binding_and_build():
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxnr_\w+)\s*\(", h))) == sorted(_qalib.NR_EXPORTS) == ["twxnr_components"]
    for macro, val in (("TWXNR_MAX_COLS", _qalib.NR_MAX_COLS), ("TWXNR_MAX_CUTS", _qalib.NR_MAX_CUTS),
                       ("TWXNR_MAX_SWEEPS", _qalib.NR_MAX_SWEEPS), ("TWXNR_NKERNELS", len(_qalib.NR_KERNELS)),
                       ("TWXNR_NTIMES", len(_qalib.NR_KERNELS) + len(_qalib.NR_HOST_TIMES)),
                       ("TWXNR_NOCONV", _qalib.NR_NOCONV), ("TWXNR_NONFINITE", _qalib.NR_NONFINITE),
                       ("TWXNR_CONSTANT", _qalib.NR_CONSTANT), ("TWXNR_FEW_ROWS", _qalib.NR_FEW_ROWS)):
        assert re.search(r"#define %s %d\b" % (macro, val), h), macro
    assert "#define TWXNR_OK TWX_CELL_OK" in h and (_qalib.NR_MAX_COLS, _qalib.NR_MAX_SWEEPS) == (64, 30)
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_nnr.hip" in build and os.path.exists(os.path.join(ROOT, "topowx_amd", "qa", "twx_nnr.hip"))
    import topowx_amd
    import twx.db
    assert topowx_amd.NNRNghData is NNRNghData is twx.db.NNRNghData and "NNRNghData" in twx.db.__all__


def test_resource_table_lists_the_new_kernels():
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.NR_EXPORTS:
        assert hasattr(lib, name), name
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    # the header's arithmetic; k_nr_eig's LDS is dynamic (2 P^2 x 8 B of the call's largest P), none static
    assert table["k_nr_gram"]["lds"] == 64 * 65 * 8 + 2 * 64 * 8 + 64 * 4 == 34560
    assert table["k_nr_scores"]["lds"] == 64 * 64 * 8 + 2 * 64 * 8 == 33792
    assert table["k_nr_eig"]["lds"] == 0 and 2 * _qalib.NR_MAX_COLS ** 2 * 8 == 65536


def test_entry_rejects_bad_arguments_before_any_device_work():
    """Call-level failures (the library is needed, a GPU is not)."""
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    cols = np.ones((3, 20), np.float32)
    grp = np.zeros(20, np.int8)
    ok = dict(cols=cols, set_off=[0, 2], set_col=[0, 1], group=grp, max_var=(0.99,))
    for kw, text in ((dict(max_var=(1.0,)), "max_var[0] must lie in (0, 1)"), (dict(max_var=(0.5, 0.0)), "max_var[1]"),
                     (dict(max_var=(0.9, np.nan)), "max_var[1]"), (dict(max_var=(0.1, 0.2, 0.3, 0.4, 0.5)), "TWXNR_MAX_CUTS"),
                     (dict(set_off=[0, 0], set_col=[]), "has 0 columns"),
                     (dict(set_off=[0, 65], set_col=[0] * 65), "TWXNR_MAX_COLS"),
                     (dict(set_col=[0, 3]), "outside 0 .. ncol - 1"), (dict(set_col=[-1, 0]), "outside 0 .. ncol - 1"),
                     (dict(group=np.full(20, 3, np.int8), ngroups=2), "outside -1 .. ngroups - 1"),
                     (dict(group=np.full(20, -2, np.int8), ngroups=1), "outside -1 .. ngroups - 1"),
                     (dict(ngroups=13), "TWXIF_MAX_GROUPS"), (dict(ngroups=0), "TWXIF_MAX_GROUPS")):
        with pytest.raises(_qalib.QaError) as e:
            _qalib.nnr_components_batched(**dict(ok, **kw))
        assert text in str(e.value), (text, str(e.value))
    for kw in (dict(cols=cols[0]), dict(group=grp[:5]), dict(set_off=[0])):
        with pytest.raises(ValueError):
            _qalib.nnr_components_batched(**dict(ok, **kw))
    L = _qalib.load()
    buf = ctypes.create_string_buffer(512)
    assert L.twxnr_components(0, 20, 3, cols.ctypes.data, 1, None, None, 1, grp.ctypes.data, 1, None, None, None, None, None,
                              None, None, None, None, None, None, 0, None, None, buf, 512) != 0
    assert b"null buffer" in buf.value


def test_parsers_accept_nnr_dir(tmp_path, capsys):
    from topowx_amd import step14, step15, step16
    none = str(tmp_path / "none.nc")
    for mod, argv in ((step14, ["--db", none, "--var", "tmin", "--out", "x.npz", "--estimate"]),
                      (step16, ["--db", none, "--var", "tmin", "--normals", "n.npz", "--out", "x.npz"]),
                      (step15, ["--db", none, "--normals", "n.npz", "--xval-stnids", "i.txt", "--out", "x.nc"])):
        assert mod.main(argv + ["--nnr-dir", str(tmp_path)]) == 1      # parsed; the database does not exist
        assert "cannot open" in capsys.readouterr().err
        assert "--nnr-dir" in mod.__doc__


def test_nnr_dir_needs_utc_offset(tmp_path, capsys, case):
    """With --nnr-dir a database without the station variable utc_offset ends the command with a message saying so."""
    from topowx_amd import stationdb as sdb, step14
    from topowx_amd._cli import BadNnrDir, NoUtcOffset, open_nnr
    from topowx_amd.qa import StationObsPool
    stns = np.empty(3, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = case.ids[:3], case.lon[:3], case.lat[:3], 100.0
    db = str(tmp_path / "all.nc")
    ncio.create_quick_db(db, stns, case.days, [("tmin", "f4", ncio.FILL_F4, "tmin", "C"), ("tmax", "f4", ncio.FILL_F4, "tmax", "C")],
                         format="NETCDF3_64BIT")
    assert step14.main(["--db", db, "--var", "tmin", "--out", str(tmp_path / "x.npz"), "--estimate", "--nnr-dir", str(tmp_path)]) == 1
    assert "no station variable utc_offset" in capsys.readouterr().err
    ds = ncio.open_dataset(db, "a")
    try:
        ds.createVariable("utc_offset", "i2", (sdb.STN_ID,), fill_value=ncio.FILL_I2)[:] = case.utc[:3]
    finally:
        ds.close()
    nnr_dir = case.write(str(tmp_path / "nnr"), "NETCDF3_64BIT")
    pool = StationObsPool.from_netcdf(db, qflags=False)
    # subsets that are missing or cover other days: a message of their own, not "cannot open <db>"
    assert step14.main(["--db", db, "--var", "tmin", "--out", str(tmp_path / "x.npz"), "--estimate", "--nnr-dir", str(tmp_path)]) == 1
    assert "cannot open the reanalysis subsets" in capsys.readouterr().err
    other = NC.NnrCase(case.start.replace(year=1982), NC.END).write(str(tmp_path / "other"), "NETCDF3_64BIT")
    with pytest.raises(BadNnrDir, match="do not cover the days"):
        open_nnr(other, db, pool)
    with pytest.raises(SystemExit) as e:                             # without --estimate there is nothing to add columns to
        step14.main(["--db", db, "--var", "tmin", "--out", str(tmp_path / "x.npz"), "--nnr-dir", nnr_dir])
    assert e.value.code == 2
    capsys.readouterr()
    nnr, utc = open_nnr(nnr_dir, db, pool)
    try:
        assert utc.tolist() == case.utc[:3].tolist() and nnr.days.size == case.days.size
    finally:
        nnr.close()
    with pytest.raises(NoUtcOffset):
        ds = ncio.open_dataset(db, "a")
        try:
            ds.variables["utc_offset"][1] = ncio.FILL_I2
        finally:
            ds.close()
        open_nnr(nnr_dir, db, pool)
