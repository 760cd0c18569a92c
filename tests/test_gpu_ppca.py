"""GPU: step16's estimator (``twxpp_ppca_fit``; ``topowx_amd.infill.infill_daily``) against the numpy restatement
(tests/restate_ppca.py): on the executed-reference golden (every item, one search), on a random pool, on the smallest
shapes that can still go wrong, for byte equality, and through the facade and the command line.

Statuses, iterations, the final number of components and the number of fits are compared exactly.  The fit is compared per
item within 100 x ``d_ref`` with a floor of 1e-12, in target standard deviations; ``d_ref`` is the distance of the float64
restatement from the ``np.longdouble`` one.  On the random pool an item is left out only if its ``d_ref`` is above 1e-12 or
a ``rel`` / R2cum lies within 1e-6 of its bound, at most 5 %.  Every comparison prints its largest deviation next to ``d_ref``.

Measured (MI355X): see DESIGN.md section 18.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ppca_cases as PC  # noqa: E402
import restate_ppca as RP  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 100.0, 1e-12
NORM, STD = 0.5, 2.0                  # the norms / stds of the station columns of a Batch item


def tol_of(d_ref):
    return max(FACTOR * d_ref, FLOOR)


class Batch(object):
    """Items of ONE library call, each with station rows of its own; equal row counts share a day group."""

    def __init__(self):
        self.items, self.nrows = [], []

    def add(self, x, d, c0=None, extra=None, mstatus=0, share=None):
        x = np.asarray(x, np.float32)
        if x.shape[0] not in self.nrows:
            self.nrows.append(x.shape[0])
        self.items.append(dict(x=x, d=int(d), c0=c0, extra=extra, mstatus=mstatus, share=share))
        return len(self.items) - 1

    def matrix(self, i):
        """The standardised matrix the restatement gets."""
        it = self.items[i]
        y = (it["x"].astype(np.float64) - NORM) / STD
        if it["extra"] is not None:
            e = np.asarray(it["extra"], np.float64)
            y = np.hstack([y, (e - e.mean(axis=0)) / e.std(axis=0, ddof=1)])
        return y

    def c0(self, i):
        it = self.items[i]
        D = self.matrix(i).shape[1]
        return RP.default_c0(D, it["d"]) if it["c0"] is None else np.asarray(it["c0"], np.float64)

    def run(self, **kw):
        from topowx_amd import _qalib
        starts = np.concatenate([[0], np.cumsum(self.nrows)])
        group = np.concatenate([np.full(n, g, np.int8) for g, n in enumerate(self.nrows)])
        nst = sum(it["x"].shape[1] for it in self.items)
        obs = np.full((nst, group.size), np.nan, np.float32)
        row, tg, gr, off, cols, norms, stds, c0, sets, iset, shared = 0, [], [], [0], [], [], [], [], [], [], {}
        for i, it in enumerate(self.items):
            n, p = it["x"].shape
            g = self.nrows.index(n)
            obs[row:row + p, starts[g]:starts[g] + n] = it["x"].T
            tg.append(row); gr.append(g)
            cols += list(range(row + 1, row + p)); off.append(len(cols))
            norms += [NORM] * p; stds += [STD] * p
            s = -1
            if it["extra"] is not None:
                e = np.asarray(it["extra"], np.float64)
                if it["share"] is not None and it["share"] in shared:
                    s = shared[it["share"]]
                else:
                    s = len(sets)
                    sets.append((g, e))
                    if it["share"] is not None:
                        shared[it["share"]] = s
                norms += list(e.mean(axis=0)); stds += list(e.std(axis=0, ddof=1))
            iset.append(s)
            if it["mstatus"] == 0:
                c0.append(self.c0(i).ravel(order="F"))
            row += p
        res = _qalib.ppca_fit(obs, group, tg, gr, [it["d"] for it in self.items], off, cols, norms, stds,
                              np.concatenate(c0) if c0 else np.zeros(0), sets, iset, [it["mstatus"] for it in self.items],
                              full=True, **kw)
        res["fits"] = [(res["fit"][res["fit_off"][i]:res["fit_off"][i + 1]] - NORM) / STD for i in range(len(self.items))]
        return res


def want_fit(y, d, c0, threshold=1e-5, maxits=1000, longdouble=True):
    """The restatement's record of a fit with ``d_ref`` (inf if the longdouble run stops elsewhere) and ``rel_ref``, the same
    distance of the last ``rel``."""
    with np.errstate(all="ignore"):
        a = RP.fit(y, d, c0, threshold, maxits)
        a["d_ref"] = 0.0
        if longdouble and a["status"] in (RP.OK, RP.MAXITS):
            b = RP.fit(y, d, c0, threshold, maxits, dtype=np.longdouble)
            a["d_ref"] = np.inf
            if (b["status"], b["iters"]) == (a["status"], a["iters"]):
                a["d_ref"] = float(np.abs(a["fit"] - np.asarray(b["fit_ld"], np.float64)).max())
                a["rel_ref"] = abs(a["rel"] - b["rels"][-1])
    return a


def compare(res, i, want, what):
    """Item ``i`` of a Batch result against a restatement record: (deviation, d_ref)."""
    assert res["status"][i] == want["status"], (what, res["status"][i], want["status"])
    assert res["iters"][i] == want["iters"], (what, res["iters"][i], want["iters"])
    if want["status"] not in (RP.OK, RP.MAXITS):
        assert np.isnan(res["fits"][i]).all() and np.isnan(res["r2cum"][i]).all(), what
        return 0.0, 0.0
    assert np.isfinite(want["d_ref"]), (what, "float64 and longdouble stop at different iterations")
    dev = float(np.abs(res["fits"][i] - want["fit"]).max())
    d = want["r2cum"].size
    r2dev = float(np.abs(res["r2cum"][i, :d] - want["r2cum"]).max())
    assert dev <= tol_of(want["d_ref"]), (what, dev, want["d_ref"])
    assert r2dev <= max(tol_of(want["d_ref"]), 1e-10) and np.isnan(res["r2cum"][i, d:]).all(), (what, r2dev, want["d_ref"])
    # rel = |1 - objective / old| cancels: where the fit is exact (d = D) ss is rounding noise and so is rel, in the
    # restatement itself; its bound is the restatement's own float64-against-longdouble distance, with the fit's factor
    rel_tol = max(FACTOR * want.get("rel_ref", 0.0), 1e-6 * want["rel"] + 1e-15)
    assert abs(res["rel"][i] - want["rel"]) <= rel_tol, (what, res["rel"][i], want["rel"], want.get("rel_ref"))
    return dev, float(want["d_ref"])


def report(name, devs, nleft=0):
    ratio = max(d[0] / max(d[1], 1e-16) for d in devs)
    worst = max(devs)
    print("%s: largest deviation %.3g (d_ref there %.3g); largest d_ref %.3g; largest deviation / d_ref %.3g over %d items, "
          "%d left out" % (name, worst[0], worst[1], max(d[1] for d in devs), ratio, len(devs), nleft))


def random_matrix(rs, n, p, miss=0.12):
    f = rs.randn(n, 3) @ rs.randn(3, p) * 2.0 + rs.randn(n, p) * (0.3 + 1.2 * rs.rand(p)) + 1.0
    x = np.round(f, 1).astype(np.float32)
    x[rs.rand(n, p) < miss] = np.nan
    return x


# ---- the pools: the golden and a random one, each searched ONCE ----
def searched(pool, mean, vari, targets, nnr=None):
    from topowx_amd.dates import MONTH
    from topowx_amd.infill.infill_daily import daily_items, run_search
    items, obs = daily_items(pool, "tmin", pool.ids[list(targets)], mean, vari, nnr)
    group = (np.asarray(pool.days[MONTH], np.int64) - 1).astype(np.int8)
    search, calls = run_search(obs, group, items)
    return items, obs, group, search, calls


@pytest.fixture(scope="module")
def gold():
    return PC.load_gold()


def test_golden_every_item_in_one_search(gold):
    import make_golden_infillmat as mk
    import make_golden_ppca as mg
    pool, mean, vari = PC.gold_pool(gold)
    key = {(str(p), int(t), int(g)): i for i, (p, t, g) in enumerate(zip(gold["pool"], gold["target"], gold["month"]))}
    devs, seen = [], 0
    for p, targets, nnr in (("A", range(pool.ids.size), None), ("B", range(mg.NNR_TARGETS), mk._Nnr(pool.days.size))):
        items, obs, group, search, calls = searched(pool, mean, vari, targets, nnr)
        for it, s in zip(items, search):
            i = key.get((p, it["t"], it["g"]))
            if i is None:                                            # a target without normals that month
                assert s.status == RP.EMPTY_COLUMN, (p, it["t"], it["g"], s.status)
                continue
            what = "golden %s target %d month %d" % (p, it["t"], it["g"] + 1)
            assert np.array_equal(np.concatenate([[it["col"]], it["cols"]]), gold["cols"][gold["col_off"][i]:gold["col_off"][i + 1]]), what
            assert it["ncomp"] == gold["ncomp"][i] and it["max_dist"] == gold["max_dist"][i], what
            assert (s.status, s.npcs, s.nfits, s.payload[1]) == (gold["status"][i], gold["npcs"][i], gold["nfits"][i], gold["iters"][i]), \
                (what, s.status, s.npcs, s.nfits, s.payload[1], gold["npcs"][i], gold["nfits"][i], gold["iters"][i])
            assert s.r2_not_reached == bool(gold["r2_not_reached"][i]), what
            fit = (s.payload[0] - it["norms"][0]) / it["stds"][0]
            dev = float(np.abs(fit - gold["fit"][gold["fit_off"][i]:gold["fit_off"][i + 1]]).max())
            assert dev <= tol_of(gold["d_ref"][i]), (what, dev, gold["d_ref"][i])
            devs.append((dev, float(gold["d_ref"][i])))
            seen += 1
        print("golden pool %s: %d items in %d library calls" % (p, len(items), calls))
    assert seen == gold["status"].size                                # none left out
    report("golden", devs)


@pytest.fixture(scope="module")
def random_case():
    pool, mean, vari = PC.random_pool()
    items, obs, group, search, calls = searched(pool, mean, vari, PC.RANDOM_TARGETS)
    from topowx_amd.infill import item_matrix
    wants = [PC.want_search(item_matrix(obs, np.nonzero(group == it["g"])[0], it)) for it in items]
    return pool, mean, vari, items, obs, group, search, wants


def test_random_pool(random_case):
    pool, mean, vari, items, obs, group, search, wants = random_case
    devs, nleft = [], 0
    for it, s, w in zip(items, search, wants):
        what = "random target %d month %d" % (it["t"], it["g"] + 1)
        if PC.left_out(w):
            nleft += 1
            print("%s left out: d_ref %.3g, margins %.3g / %.3g" % (what, w["d_ref"], w["rel_margin"], w["r2_margin"]))
            continue
        assert (s.status, s.npcs, s.nfits, s.payload[1], s.r2_not_reached) == (w["status"], w["npcs"], w["nfits"], w["iters"], w["r2_not_reached"]), what
        fit = (s.payload[0] - it["norms"][0]) / it["stds"][0]
        dev = float(np.abs(fit - w["fit"]).max())
        assert dev <= tol_of(w["d_ref"]), (what, dev, w["d_ref"])
        devs.append((dev, w["d_ref"]))
    assert len(items) == 12 * len(PC.RANDOM_TARGETS) and nleft <= 0.05 * len(items), nleft
    report("random pool", devs, nleft)


def test_facade_against_the_restatement(random_case):
    """``infill_daily`` against the restatement driven by the same assembly: fnl_tair, mask_infill, mae, bias."""
    from topowx_amd.infill import infill_daily
    pool, mean, vari, items, obs, group, search, wants = random_case
    tm = {}
    r = infill_daily(pool, "tmin", pool.ids[list(PC.RANDOM_TARGETS)], mean, vari, timing=tm)
    nt = len(PC.RANDOM_TARGETS)
    fnl, infl = np.full((nt, group.size), np.nan), np.full((nt, group.size), np.nan)
    tol = np.zeros((nt, group.size))
    for it, w in zip(items, wants):
        days = np.nonzero(group == it["g"])[0]
        o = obs[it["col"], days].astype(np.float64)
        f = w["fit"] * it["stds"][0] + it["norms"][0]
        fnl[it["t"], days], infl[it["t"], days] = np.where(np.isnan(o), f, o), f
        tol[it["t"], days] = tol_of(w["d_ref"] if np.isfinite(w["d_ref"]) else 1.0) * it["stds"][0]
        assert r.npcs[it["t"], it["g"]] == w["npcs"] or PC.left_out(w)
        assert r.ncols[it["t"], it["g"]] == 1 + len(it["cols"]) and r.matrix_status[it["t"], it["g"]] == 0
    tobs = obs[[pool.idxs[str(s)] for s in r.target_ids]]
    assert np.array_equal(r.mask_infill, np.isnan(tobs))
    assert np.all(np.abs(r.fnl_tair - fnl) <= tol) and np.all(np.abs(r.infill_tair - infl) <= tol)
    assert np.array_equal(r.fnl_tair[~r.mask_infill], tobs[~r.mask_infill].astype(np.float64))
    for t in range(nt):
        om = ~r.mask_infill[t]
        difs = infl[t, om] - fnl[t, om]
        assert abs(r.mae[t] - np.mean(np.abs(difs))) <= tol[t].max() and abs(r.bias[t] - np.mean(difs)) <= tol[t].max()
    assert (r.status == 0).all() and (r.item_r2 > 0.5).all() and (r.item_impossible == 0).all() and r.calls >= 2
    assert tm["pp_calls"] == r.calls and tm["pp_iter_kernel_ms"] > 0 and tm["pp_fits"] == r.nfits.sum()
    print("facade: %d items, %d fits in %d calls, item MAE %.3f .. %.3f" % (r.nfits.size, r.nfits.sum(), r.calls, r.item_mae.min(), r.item_mae.max()))


def test_infill_daily_obs_and_what_is_not_implemented(random_case):
    from topowx_amd.dates import MONTH
    from topowx_amd.infill import infill_daily, infill_daily_obs
    pool, mean, vari = random_case[:3]
    sid = pool.ids[PC.RANDOM_TARGETS[0]]
    masks = [pool.days[MONTH] == m for m in range(1, 13)]
    fnl, mask, infl = infill_daily_obs(sid, pool, "tmin", None, mean, vari, day_masks=masks)
    r = infill_daily(pool, "tmin", [sid], mean, vari)
    assert fnl.tobytes() == r.fnl_tair[0].tobytes() and infl.tobytes() == r.infill_tair[0].tobytes() and np.array_equal(mask, r.mask_infill[0])
    with pytest.raises(NotImplementedError):
        infill_daily_obs(sid, pool, "tmin", None, mean, vari, tair_mask=np.zeros(pool.days.size, bool), day_masks=masks)
    with pytest.raises(NotImplementedError):
        infill_daily_obs(sid, pool, "tmin", None, mean, vari, day_masks=masks, chk_perf=True)


def test_failed_months_are_left_out_of_mae_and_bias(random_case):
    """Station 5 has no normals in the first four months: those items end EMPTY_COLUMN, their days keep NaN where the
    record is missing, and mae / bias come from the eight fitted months."""
    from topowx_amd.infill import infill_daily
    pool, mean, vari, items, obs, group = random_case[:6]
    r = infill_daily(pool, "tmin", [pool.ids[5]], mean, vari)
    assert (r.status[0, :4] == RP.EMPTY_COLUMN).all() and (r.status[0, 4:] == 0).all()
    failed = group < 4
    assert np.isnan(r.infill_tair[0, failed]).all() and np.isfinite(r.infill_tair[0, ~failed]).all()
    assert np.array_equal(np.isnan(r.fnl_tair[0]), failed & r.mask_infill[0])
    om = ~r.mask_infill[0] & ~failed
    difs = r.infill_tair[0, om] - r.fnl_tair[0, om]
    assert np.isfinite(r.mae[0]) and r.mae[0] == np.mean(np.abs(difs)) and r.bias[0] == np.mean(difs)


def test_step16_command_line(tmp_path, capsys, random_case):
    import corrob_cases
    from topowx_amd import step16
    from topowx_amd.infill import infill_daily
    pool, mean, vari = random_case[:3]
    db = corrob_cases.write_db(str(tmp_path / "all.nc"), pool.ids, pool.lon, pool.lat, pool.tmin, pool.tmax, pool.days,
                               "NETCDF3_64BIT")
    targets = pool.ids[[PC.RANDOM_TARGETS[1]]]
    (tmp_path / "t.txt").write_text("\n".join(targets) + "\n")
    np.savez(str(tmp_path / "normals.npz"), ids=pool.ids[::-1], mean=mean[::-1], variance=vari[::-1])
    out = str(tmp_path / "infilled.npz")
    assert step16.main(["--db", db, "--var", "tmin", "--normals", str(tmp_path / "normals.npz"), "--out", out, "--targets",
                        str(tmp_path / "t.txt")]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = infill_daily(pool, "tmin", targets, mean, vari)
    got = np.load(out)
    for k in ("fnl_tair", "mask_infill", "infill_tair", "mae", "bias", "status", "npcs", "nfits", "iters"):
        assert got[k].tobytes() == getattr(want, k).tobytes(), k
    assert rep["items"] == 12 and rep["status"] == {"ok": 12} and rep["fits"] == int(want.nfits.sum()) and "pp_iter_kernel_ms" in rep
    np.savez(str(tmp_path / "short.npz"), ids=pool.ids[:5], mean=mean[:5], variance=vari[:5])
    assert step16.main(["--db", db, "--var", "tmin", "--normals", str(tmp_path / "short.npz"), "--out", out]) == 1


# ---- the smallest shapes ----
def shape_grid():
    """The Batch of the grid and the names of its items.  The N = d + 1 items are complete (with gaps a column of so few
    rows is empty and nothing of the fit is checked); the others have 12 % missing."""
    rs = np.random.RandomState(31)
    b, names = Batch(), []
    for D in (2, 3, 4, 64):
        for d in sorted({k for k in (1, 2, D - 1, 32) if 1 <= k <= min(D, 32)}):
            for n in (d + 1, 63, 64, 65, 255, 256, 257):
                b.add(random_matrix(rs, n, D, 0.0 if n == d + 1 else 0.12), d)
                names.append("D %d d %d N %d" % (D, d, n))
    return b, names


def test_shape_grid():
    """D = 2 / 3 / 4 / TWXPP_MAX_COLS by d = 1 / 2 / D - 1 / TWXPP_MAX_PCS by N = d + 1 / 63 / 64 / 65 / 255 / 256 / 257 in
    one call of 8 iterations: every item ends MAXITS and is compared, none is left out."""
    b, names = shape_grid()
    res = b.run(maxits=8)
    devs = []
    for i, name in enumerate(names):
        w = want_fit(b.matrix(i), b.items[i]["d"], b.c0(i), maxits=8)
        assert w["status"] == RP.MAXITS and w["iters"] == 8, name
        devs.append(compare(res, i, w, name))
    assert len(devs) == len(names) == 70
    report("shape grid (%d items)" % len(names), devs)


def test_shape_grid_stops_on_the_count_rule():
    """The same grid at threshold 0.5: ``rel`` is below it from the first iterations on, so the ``count > 5`` half of the stop
    rule decides and an item ends OK after 5 iterations.  Items with d = D are not taken: their fit is exact, ss and with
    it ``rel`` are rounding noise (see ``compare``), so the iteration they stop at is not defined."""
    b, names = shape_grid()
    res = b.run(maxits=8, threshold=0.5)
    devs, five = [], 0
    for i, name in enumerate(names):
        if b.items[i]["d"] == b.items[i]["x"].shape[1]:
            continue
        w = want_fit(b.matrix(i), b.items[i]["d"], b.c0(i), threshold=0.5, maxits=8)
        assert RP.margin(w["rels"], 0.5) >= 1e-6, name                # a property of the inputs, checked on the CPU
        devs.append(compare(res, i, w, name))
        five += w["status"] == RP.OK and w["iters"] == 5
    assert len(devs) == 63 and five >= 60, (len(devs), five)
    report("shape grid, count rule (%d items)" % len(devs), devs)


def test_caps():
    from topowx_amd import _qalib
    rs = np.random.RandomState(32)
    b = Batch()
    over_cols = b.add(random_matrix(rs, 70, 65), 3)
    at_cols = b.add(random_matrix(rs, 70, 64), 3)
    over_pcs = b.add(random_matrix(rs, 70, 40), 33)
    at_rows = b.add(random_matrix(rs, _qalib.PP_MAX_ROWS, 3), 1)
    over_rows = b.add(random_matrix(rs, _qalib.PP_MAX_ROWS + 1, 3), 1)
    res = b.run(maxits=6)
    for i, st in ((over_cols, RP.COL_CAP), (over_pcs, RP.PCS_CAP), (over_rows, RP.ROW_CAP)):
        assert res["status"][i] == st and np.isnan(res["fits"][i]).all() and np.isnan(res["r2cum"][i]).all() and res["iters"][i] == 0
    devs = [compare(res, i, want_fit(b.matrix(i), b.items[i]["d"], b.c0(i), maxits=6, longdouble=i == at_cols), "cap %d" % i)
            for i in (at_cols, at_rows)]
    report("at the caps", [(d[0], max(d[1], 1e-14)) for d in devs])


def test_complete_data_against_the_closed_form():
    rs = np.random.RandomState(3)
    x = np.round(rs.randn(200, 8) @ rs.randn(8, 8), 1).astype(np.float32)
    b = Batch()
    b.add(x, 3)
    res = b.run(threshold=1e-14, maxits=100000)
    ss, f = RP.closed_form(b.matrix(0), 3)
    dev = np.abs(res["fits"][0] - f).max()
    print("complete data: %d iterations, deviation from the closed form %.3g" % (res["iters"][0], dev))
    assert res["status"][0] == 0 and dev < 1e-8
    assert np.abs(res["M"][0, :8] - b.matrix(0).mean(axis=0)).max() < 1e-14 and np.isnan(res["M"][0, 8:]).all()
    c = res["C"][0, :8, :3]
    assert np.abs(c.T @ c - np.eye(3)).max() < 1e-12 and np.isnan(res["C"][0, 8:]).all() and np.isnan(res["C"][0, :, 3:]).all()


def test_patterns_and_degenerate_items():
    rs = np.random.RandomState(33)
    b, want_status = Batch(), {}
    full = np.round(rs.randn(90, 7) @ rs.randn(7, 7), 1).astype(np.float32)
    one = full.copy(); one[17, 2] = np.nan
    i_one = b.add(one, 3)
    row = random_matrix(rs, 90, 7); row[40, :] = np.nan
    i_row = b.add(row, 3)
    own = full[:64, :7].copy()                                       # every row its own pattern: 64 of the 126 non-empty masks
    for r in range(64):
        bits = r + 1
        own[r, [c for c in range(7) if (bits >> c) & 1 and c < 6]] = np.nan
    i_own = b.add(own, 2)
    empty = random_matrix(rs, 90, 5); empty[:, 3] = np.nan
    want_status[b.add(empty, 2)] = RP.EMPTY_COLUMN
    const = random_matrix(rs, 90, 5, 0.0); const[:, 2] = 1.5
    i_const = b.add(const, 2)
    dup = np.repeat(rs.randn(5, 1), 2, axis=1)
    want_status[b.add(random_matrix(rs, 90, 5), 2, c0=dup)] = RP.NUMERIC
    i_six = b.add(random_matrix(rs, 90, 6), 2)
    want_status[b.add(random_matrix(rs, 90, 4), 2, mstatus=19)] = RP.NO_MATRIX
    extra = rs.randn(90, 2) * 3.0 + 270.0
    i_sh1 = b.add(random_matrix(rs, 90, 4), 3, extra=extra, share="nnr")
    i_sh2 = b.add(random_matrix(rs, 90, 5), 3, extra=extra, share="nnr")
    res = b.run()
    devs = []
    for i in range(len(b.items)):
        if i in want_status:
            assert res["status"][i] == want_status[i] and np.isnan(res["fits"][i]).all(), (i, res["status"][i])
            if want_status[i] != RP.NO_MATRIX:
                assert RP.fit(b.matrix(i), b.items[i]["d"], b.c0(i))["status"] == want_status[i]
        else:
            devs.append(compare(res, i, want_fit(b.matrix(i), b.items[i]["d"], b.c0(i)), "pattern item %d" % i))
    assert b.matrix(i_sh1).shape[1] == 6 and b.matrix(i_sh2).shape[1] == 7
    report("patterns", devs)
    res6 = b.run(maxits=6)
    w6 = want_fit(b.matrix(i_six), 2, b.c0(i_six), maxits=6)
    assert w6["status"] == RP.MAXITS and w6["iters"] == 6
    devs = [compare(res6, i, want_fit(b.matrix(i), b.items[i]["d"], b.c0(i), maxits=6), "maxits 6 item %d" % i)
            for i in (i_one, i_row, i_own, i_const, i_six)]
    report("maxits 6", devs)


def test_call_level_failures():
    """d > D, N <= d and d < 1 are refused by the library (each with a C0 of the size the binding expects for that d, so
    that the binding's own argument check is not what answers); so are a non-positive threshold or maxits."""
    from topowx_amd._qalib import QaError
    rs = np.random.RandomState(34)
    for x, d in ((random_matrix(rs, 30, 4), 5), (random_matrix(rs, 3, 4), 3), (random_matrix(rs, 30, 4), 0)):
        b = Batch()
        b.items.append(dict(x=x, d=d, c0=np.zeros((4, d)), extra=None, mstatus=0, share=None))
        b.nrows.append(x.shape[0])
        with pytest.raises(QaError, match="need 1 <= d <= D and N > d"):
            b.run()
    b = Batch()
    b.add(random_matrix(rs, 30, 4), 2)
    for kw in (dict(threshold=0.0), dict(maxits=0), dict(threshold=float("nan"))):
        with pytest.raises(QaError, match="threshold and maxits must be positive"):
            b.run(**kw)


def test_byte_equality():
    rs = np.random.RandomState(35)
    b = Batch()
    for n, p, d in ((70, 6, 2), (70, 9, 4), (130, 40, 7), (70, 5, 4), (130, 12, 3), (64, 3, 1)):
        b.add(random_matrix(rs, n, p), d)
    keys = ("fit", "r2cum", "iters", "rel", "status", "C", "M")
    a = b.run()
    again, single, small = b.run(), b.run(iters_per_launch=1), b.run(workspace_bytes=60000)
    assert small["batches"] == 3 and single["rounds"] == a["iters"].max() and a["batches"] == 1, (small["batches"], single["rounds"])
    for other in (again, single, small):
        for k in keys:
            assert a[k].tobytes() == other[k].tobytes(), k
    assert (a["status"] == 0).all()
