"""CPU: step16's host side -- the column assembly against the executed-reference golden, the numpy restatement of the
estimator (tests/restate_ppca.py) pinned by known answers, the component search on hand-made R2cum sequences, and the
resource table of a build.  The GPU kernels are checked against the restatement in tests/test_gpu_ppca.py.

Measured here (printed): two starts C0 (seeds 4324 and 1) at threshold 1e-5 give fits that differ by 6.0e-3 target
standard deviations on the 200 x 8 case below, by 1.4e-5 at 1e-9 and by 5.9e-8 at 1e-13: the size of what R's random stream
could move.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ppca_cases as PC  # noqa: E402
import restate_ppca as RP  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return PC.load_gold()


def test_golden_file(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_ppca_v1.npz")) < 1024 * 1024
    assert min(gold["rel_margin"].min(), gold["r2_margin"].min()) >= 1e-6
    assert set(gold["pool"].tolist()) == {"A", "B"} and (gold["ncomp"][gold["pool"] == "B"] > 0).all()
    assert np.isin(gold["status"], (0, 20)).all() and (gold["nfits"] >= 1).all() and gold["nfits"].max() > 1
    print("golden: %d items, widths %d .. %d, npcs %d .. %d, largest d_ref %.3g" % (
        gold["status"].size, gold["width"].min(), gold["width"].max(), gold["npcs"].min(), gold["npcs"].max(), gold["d_ref"].max()))


def test_assembly_reproduces_the_golden(gold):
    """Column lists, norms / stds (1e-12 relative), widths and score columns (up to sign) of every golden item from the host
    assembly on the neighbour lists of the numpy restatement of the matrix builder."""
    import make_golden_infillmat as mk
    from topowx_amd.infill import assemble_daily_columns, nnr_components
    from topowx_amd.infill.infill_daily import month_mask_groups
    pool, mean, vari = PC.gold_pool(gold)
    n = pool.ids.size
    key = {(str(p), int(t), int(g)): i for i, (p, t, g) in enumerate(zip(gold["pool"], gold["target"], gold["month"]))}
    nnr = mk._Nnr(pool.days.size).m
    seen = 0
    for mask, months in month_mask_groups(mean, vari):
        m = PC.host_matrices(pool, mask, np.arange(n), months)
        for t in range(n):
            for k, g in enumerate(months):
                for p in ("A", "B"):
                    i = key.get((p, t, g))
                    if i is None:
                        continue
                    sc = nnr_components(nnr[m.day_idx(k)], 0.99) if p == "B" else None
                    cols, extra, norms, stds = assemble_daily_columns(m, t, k, mean[:, g], vari[:, g], sc)
                    want = gold["cols"][gold["col_off"][i]:gold["col_off"][i + 1]]
                    assert np.array_equal(np.concatenate([[t], cols]), want), (p, t, g)
                    sl = slice(gold["par_off"][i], gold["par_off"][i + 1])
                    assert 1 + cols.size + extra.shape[1] == gold["width"][i] and extra.shape[1] == gold["ncomp"][i]
                    assert np.allclose(norms, gold["norms"][sl], rtol=1e-12, atol=1e-12 * np.abs(gold["stds"][sl]))
                    assert np.allclose(stds, gold["stds"][sl], rtol=1e-12, atol=0)
                    assert m.max_dist[t, k] == gold["max_dist"][i]
                    name = "scores_%d_%d" % (t, g)
                    if p == "B" and name in gold.files:
                        ref = gold[name]
                        sign = np.sign((ref * extra).sum(axis=0))
                        assert np.abs(ref - extra * sign).max() <= 1e-9 * np.abs(ref).max()
                    seen += 1
    assert seen == gold["status"].size                                # no item left out


# ---- the restatement pinned by known answers ----
@pytest.fixture(scope="module")
def complete():
    rs = np.random.RandomState(3)
    return rs.randn(200, 8) @ rs.randn(8, 8)


def test_complete_data_reaches_the_closed_form(complete):
    r = RP.fit(complete, 3, threshold=1e-14, maxits=100000)
    ss, f = RP.closed_form(complete, 3)
    print("complete data: %d iterations, ss %.12g against %.12g, fit deviation %.3g" % (r["iters"], r["ss"], ss, np.abs(r["fit"] - f).max()))
    assert r["status"] == RP.OK and np.abs(r["fit"] - f).max() < 1e-8
    assert abs(r["ss"] / ss - 1) < 1e-6                               # ss converges more slowly than the subspace


def test_at_least_five_iterations_and_a_falling_objective(complete):
    y = complete.copy()
    y[np.random.RandomState(4).rand(*y.shape) < 0.15] = np.nan
    r = RP.fit(y, 3, threshold=0.5)
    assert r["status"] == RP.OK and r["iters"] == 5                   # rel < threshold long before, count > 5 only now
    r = RP.fit(y, 3)
    obj = np.array(r["objectives"])
    assert r["iters"] > 5 and np.all(np.diff(obj) <= 1e-9 * np.abs(obj[:-1]))
    assert np.all(np.diff(r["r2cum"]) >= -1e-12)                      # R2cum is non-decreasing in i
    r6 = RP.fit(y, 3, maxits=6)
    assert r6["status"] == RP.MAXITS and r6["iters"] == 6 and np.isfinite(r6["fit"]).all()


def test_two_starts_agree_to_the_order_of_the_threshold(complete):
    y = complete.copy()
    y[np.random.RandomState(4).rand(*y.shape) < 0.15] = np.nan
    last = None
    for thr in (1e-5, 1e-9, 1e-13):
        a = RP.fit(y, 3, RP.default_c0(8, 3, 4324), thr, 100000)
        b = RP.fit(y, 3, RP.default_c0(8, 3, 1), thr, 100000)
        dev = np.abs(a["fit"] - b["fit"]).max()
        print("threshold %.0e: two starts differ by %.3g target standard deviations (%d / %d iterations)" % (
            thr, dev, a["iters"], b["iters"]))
        assert last is None or dev < last
        last = dev
    assert last < 1e-6


def test_degenerate_inputs():
    rs = np.random.RandomState(2)
    y = rs.randn(40, 5)
    dup = np.repeat(rs.randn(5, 1), 2, axis=1)
    assert RP.fit(y, 2, dup)["status"] == RP.NUMERIC                  # CtC is singular: the second pivot is exactly 0
    y[:, 3] = np.nan
    assert RP.fit(y, 2)["status"] == RP.EMPTY_COLUMN
    with pytest.raises(ValueError):
        RP.fit(rs.randn(3, 5), 3)
    with pytest.raises(ValueError):
        RP.fit(rs.randn(30, 5), 6)


# ---- the search rules on hand-made R2cum sequences ----
def drive(search, table):
    """Feeds ``table[d]`` (an R2cum list) for every request; returns the requests made."""
    asked = []
    while search.request is not None:
        d = search.request
        asked.append(d)
        search.feed(0, np.array(table[d]), ("fit", d))
    return asked


def test_search_first_index_and_refit():
    from topowx_amd.infill import PcSearch, add_npcs, first_npcs
    assert first_npcs(12, 0.5, 11) == 6 and first_npcs(6, 0.5, 5) == 2 and first_npcs(4, 0.5, 3) == 2     # 5.5 -> 6, 2.5 -> 2
    assert first_npcs(2, 0.5, 1) == 1 and first_npcs(10, 0.6, 9) == 5
    s = PcSearch(12)
    asked = drive(s, {6: [.5, .8, .95, .991, .995, .999], 4: [.5, .8, .95, .9905]})
    assert asked == [6, 4] and s.npcs == 4 and s.nfits == 2 and s.payload == ("fit", 4) and not s.r2_not_reached
    s = PcSearch(12)
    assert drive(s, {6: [.5, .8, .95, .97, .98, .992]}) == [6] and s.npcs == 6 and s.nfits == 1
    # the refit is accepted even if it misses max_r2cum, and a cached count is not fitted again
    s = PcSearch(12)
    asked = drive(s, {6: [.5, .6, .7, .8, .85, .9], 8: [.5, .6, .7, .8, .85, .9, .9901, .995], 7: [.5, .6, .7, .8, .85, .9, .98]})
    assert asked == [6, 8, 7] and s.npcs == 7 and s.nfits == 3
    s = PcSearch(12)
    asked = drive(s, {6: [.5, .6, .7, .8, .9, .95], 7: [.5, .6, .7, .8, .85, .992, .995]})
    assert asked == [6, 7] and s.npcs == 6 and s.payload == ("fit", 6) and s.nfits == 2
    assert add_npcs([.5, .8, .9], .99) == 1 and add_npcs([.5, .6, .6001], .99) == 10 and add_npcs([.9, .93], .99) == 2
    assert add_npcs([.9, .9], .99) == 10 and add_npcs([.9, .89], .99) == 1 and add_npcs([.5], .99) == 1
    assert add_npcs([.90, .925], .99) == 3 and add_npcs([.9, .94], .99) == 1      # 2.6 -> 3, 1.25 -> 1
    s = PcSearch(12, npcs=3)
    assert drive(s, {3: [.1, .2, .3]}) == [3] and s.npcs == 3 and s.nfits == 1


def test_search_cap_rule():
    from topowx_amd.infill import PcSearch
    s = PcSearch(6)                                                   # bound 5
    asked = drive(s, {2: [.5, .6], 5: [.5, .6, .7, .8, .9]})
    assert asked == [2, 5] and s.npcs == 5 and s.r2_not_reached and s.nfits == 2
    s = PcSearch(6)
    assert drive(s, {2: [.5, .6], 5: [.5, .6, .7, .8, .995]}) == [2, 5] and s.npcs == 5 and not s.r2_not_reached
    s = PcSearch(80)                                                  # bound TWXPP_MAX_PCS
    asked = drive(s, {d: list(np.linspace(.1, .5, d)) for d in range(1, 33)})
    assert asked[0] == 32 and s.npcs == 32 and s.r2_not_reached       # round(79 / 2) = 40 is cut to 32
    s = PcSearch(2)                                                   # one neighbour: bound 1
    assert drive(s, {1: [.7]}) == [1] and s.npcs == 1 and s.r2_not_reached
    s = PcSearch(6)
    s.feed(4, np.full(2, np.nan), None)                               # a fit that fails ends the search with its status
    assert s.request is None and s.status == 4 and s.nfits == 1


def test_search_bogus_pc1_rule():
    from topowx_amd.infill import PcSearch
    s = PcSearch(8)                                                   # starts at 4
    asked = drive(s, {4: [.5, .6, .7, .8], 6: [.995, .996, .997, .998, .999, .9995], 1: [.995]})
    assert asked == [4, 6, 1] and s.npcs == 4 and s.payload == ("fit", 4) and s.nfits == 3
    s = PcSearch(8)
    assert drive(s, {4: [.995, .996, .997, .998], 1: [.995]}) == [4, 1] and s.npcs == 1      # nothing cached: PC1 stays


def test_step16_refuses_bad_normals(tmp_path, capsys):
    """A normals file that is unreadable, lacks a field, has the wrong shape or misses stations gives exit 1 and names the
    file (all before any GPU call)."""
    import corrob_cases
    import make_golden_ppca as mg
    from topowx_amd import step16
    ids, lon, lat, tmin, days = mg.case_inputs()
    db = corrob_cases.write_db(str(tmp_path / "all.nc"), ids, lon, lat, tmin, tmin + 10, days, "NETCDF3_64BIT")
    bad = str(tmp_path / "n.npz")
    cases = []
    (tmp_path / "junk.npz").write_text("not a zip file")
    cases.append((str(tmp_path / "junk.npz"), "cannot read the normals"))
    np.savez(bad, ids=ids, mean=np.zeros((ids.size, 12)))
    cases.append((bad, "no ids / mean / variance"))
    np.savez(str(tmp_path / "shape.npz"), ids=ids, mean=np.zeros((ids.size, 11)), variance=np.zeros((ids.size, 11)))
    cases.append((str(tmp_path / "shape.npz"), "must be [%d, 12]" % ids.size))
    np.savez(str(tmp_path / "few.npz"), ids=ids[:3], mean=np.zeros((3, 12)), variance=np.ones((3, 12)))
    cases.append((str(tmp_path / "few.npz"), "have no normals"))
    cases.append((str(tmp_path / "missing.npz"), "cannot read the normals"))
    for path, text in cases:
        assert step16.main(["--db", db, "--var", "tmin", "--normals", path, "--out", str(tmp_path / "o.npz")]) == 1
        err = capsys.readouterr().err
        assert text in err and os.path.basename(path) in err, (path, err)


NEW_KERNELS = ("k_pp_prep", "k_pp_iter")


def test_resource_table_lists_the_new_kernels():
    """No scratch, no spills, LDS at most 80 KiB and what the header's arithmetic says (no build in this checkout: skipped,
    as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    assert hasattr(ctypes.CDLL(_qalib.LIB_PATH), "twxpp_ppca_fit")
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
        assert table[k]["lds"] <= 80 * 1024, (k, table[k])
    it = 2 * 64 * 33 * 8 + 4 * 32 * 32 * 8 + 4 * (64 + 3 * 32) * 8 + 4 * 33 * 8
    assert it <= table["k_pp_iter"]["lds"] <= it + 256
