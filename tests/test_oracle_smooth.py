"""The smoothing of the station parameters (kriging bandwidth, GWR bandwidth, variogram; interp_tair.py:821-835, :245-259,
:837-851) on tables whose fields are NaN raggedly -- CPU side of tests/test_gpu_smooth.py (tests/smooth_cases.py):

* the numpy restatement equals the oracle on every cell of the 24 x 24 window, for every pattern and both variables: each
  month's bandwidths, statuses and variogram (orc_smooth_nnghs / orc_smooth_vario on orc_select's lists), the month-ordered
  walk with and without the GWR steps, and on the 48 point cells orc.krig / orc.gwr_mth (nnghs = 0) and orc.interp themselves;
* every pattern keeps its promise (which ranks the months' finite masks differ in, which months fail and with what status);
* POWER: every mutant a pattern is meant to catch (smooth_cases.MUTANTS) changes a bandwidth -- for the variogram's mutant
  the oracle's kriging mean or variance by more than 10 x the GPU test's bar -- in at least 20 (cell, month) items, the
  previous month's sum of weights on the independent patterns in at least half of them.  Without that the exact
  comparisons of tests/test_gpu_smooth.py could pass on a kernel that takes its sums from the wrong mask.

Measured (Tmin table, the 576 cells of the window; kk / ka items that a mutant changes, of 6912, M1: of the 6336 with month
>= 2; M3: kriged (point, month) items of the 48 points that move by more than 1e-4):
indep05 M1 5685 (89.7 %) / 6055 (95.6 %), M2 ka 5670, M3 576 of 576; indep50 M1 6094 (96.2 %) / 6252 (98.7 %), M2 ka 6791, M3
574 of 576; runs M1 1152 / 1152 (the two changes of mask x 576 cells, every one); runs_shift M1 1728 / 1638 (three changes);
slot1 M1 3166 / 2531 (the 36 chosen cells alone, whose masks differ in the ranks 64 .. 99 only: 91 / 53 of 396); beyond M4
6632 / 5703; one M5 198 / 198 (the 36 chosen cells alone: 68 / 68 of 72 tie items; the quotient x w / w is the tie itself in
142 of 144 (cell, variable, family) triples -- not for every w); families M2 ka 6912, M3 576 of 576."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

import smooth_cases as sc  # noqa: E402
from grid_bars import FAST_BAR  # noqa: E402

MIN_ITEMS = 20
VARS = ("tmin", "tmax")


@pytest.fixture(scope="module", params=sc.PATTERNS)
def cs(request, golden_case):
    return sc.case(request.param, golden_case)


def test_restatement_equals_the_oracle(cs, orc):
    cells, pts = sc.window_cells(), sc.point_cells()
    for var in VARS:
        mine, theirs = cs.numpy(var, cells), cs.oracle(orc, var, cells)
        for a, b, (r, c) in zip(mine, theirs, cells):
            assert np.array_equal(a["rk"], b["rk"]) and np.array_equal(a["ra"], b["ra"]), (var, r, c, a["rk"], b["rk"], a["ra"], b["ra"])
            assert np.array_equal(a["k"], b["k"]) and np.array_equal(a["ka"], b["ka"]), (var, r, c, a["k"], b["k"], a["ka"], b["ka"])
            ok = a["rk"] == 0
            assert np.allclose(a["vario"][ok], b["vario"][ok], rtol=1e-13, atol=0), (var, r, c)
        # the entries a caller sees: a month alone (krig, gwr_mth with nnghs = 0) and the whole walk (interp)
        db, prm = cs.db(orc, var), orc.params()
        for p, (r, c) in zip(cs.numpy(var, pts), pts):
            pt = cs.oracle_pt(orc, var, r, c)
            for m in range(12):
                rc, _, _, used, _ = orc.krig(db, prm, pt, m + 1)
                assert rc == p["rk"][m] and (rc or used == p["k"][m]), (var, r, c, m, rc, used, p["rk"][m], p["k"][m])
                rc, _, used, _, _ = orc.gwr_mth(db, prm, pt, 0.0, m + 1)
                assert rc == p["ra"][m] and (rc or used == p["ka"][m]), (var, r, c, m, rc, used, p["ra"][m], p["ka"][m])
            for daily in (False, True):
                assert orc.interp(db, prm, pt, daily=daily)[0] == sc.walk(p, daily)[2], (var, r, c, daily)


def test_slot_edges_restatement_equals_the_oracle(golden_case, orc):
    """init_nnghs on both sides of the 64-rank slots (path (d) of the GPU test), the independent pattern at p = 0.5."""
    cs, pts = sc.case("indep50", golden_case), sc.point_cells()
    for init in sc.K_EDGES:
        for var in VARS:
            for a, b in zip(cs.numpy(var, pts, init=init), cs.oracle(orc, var, pts, init=init)):
                for key in ("rk", "k", "ra", "ka"):
                    assert np.array_equal(a[key], b[key]), (init, var, key, a[key], b[key])
        assert len({tuple(p["k"]) for p in cs.numpy("tmin", pts, init=init)}) > 1


def test_patterns_keep_their_promises(cs, orc):
    name, block = cs.name, sc.window_cells(sc.WIN, sc.BLOCK_A)
    fin = {v: {k: np.isfinite(cs.cols[v][k]) for k in ("optim", "anom", "nug")} for v in VARS}
    for v in VARS:                                           # the mask is the nugget's: psill and range come and go with it
        assert np.array_equal(fin[v]["nug"], np.isfinite(cs.cols[v]["psill"]))
        assert np.array_equal(fin[v]["nug"], np.isfinite(cs.cols[v]["rng"]))
    if name in ("indep05", "indep50"):
        for v in VARS:
            for k in fin[v]:
                assert all(not np.array_equal(fin[v][k][m], fin[v][k][m - 1]) for m in range(1, 12))
            assert not np.array_equal(fin[v]["optim"], fin[v]["anom"]) and not np.array_equal(fin[v]["optim"], fin[v]["nug"])
    if name in ("runs", "runs_shift"):
        edges = (4, 8) if name == "runs" else (1, 5, 9)      # the first month (0-based) of a new mask
        for v in VARS:
            for k in fin[v]:
                assert [m for m in range(1, 12) if not np.array_equal(fin[v][k][m], fin[v][k][m - 1])] == list(edges)
        assert all(e % sc.GA == 0 for e in (4, 8)) and all(e % sc.GA for e in (1, 5, 9))
    if name in ("slot1", "beyond"):
        for v in VARS:
            for k, d in sc.mask_facts(cs, v, block).items():
                want = (False, True, False) if name == "slot1" else (False, False, True)
                assert np.all(d == want), (v, k)
    if name == "beyond":                                     # the bandwidths do not move; the variogram may (k_m > 100)
        for v in VARS:
            kk, ka, st = sc.walked(cs.numpy(v, block), True)
            assert np.all(st == 0) and np.all(kk == kk[:, :1]) and np.all(ka == ka[:, :1])
        vario = np.array([p["vario"] for p in cs.numpy("tmin", block)])
        assert (np.abs(vario - vario[:, :1]).max(axis=(1, 2)) > 0).any() == (sc.walked(cs.numpy("tmin", block), True)[0].max() > sc.INIT)
    if name == "dead":
        kk, _, st = sc.walked(cs.numpy("tmin", block), False)
        assert len(block) >= MIN_ITEMS and np.all(st == sc.ERR_NNGHS)
        assert np.all(kk[:, :sc.DEAD_OPTIM] > 0) and np.all(kk[:, sc.DEAD_OPTIM:] == 0)
        kk, ka, st = sc.walked(cs.numpy("tmin", block), True)
        e = sc.DEAD_ANOM[0]                                  # the GWR of that month fails: its kriging was reached
        assert np.all(st == sc.ERR_NNGHS) and np.all(kk[:, :e + 1] > 0) and np.all(kk[:, e + 1:] == 0)
        assert np.all(ka[:, :e] > 0) and np.all(ka[:, e:] == 0)
        assert all(p["ra"][sc.DEAD_ANOM[1]] == sc.ERR_NNGHS and p["rk"][sc.DEAD_OPTIM + 1] == 0 for p in cs.numpy("tmin", block))
        blk_c = sc.window_cells(sc.WIN, sc.BLOCK_C)
        kk, _, st = sc.walked(cs.numpy("tmax", blk_c), False)
        assert len(blk_c) >= MIN_ITEMS and np.all(st == sc.ERR_VARIO)
        assert np.all(kk[:, :sc.DEAD_NUG] > 0) and np.all(kk[:, sc.DEAD_NUG:] == 0)
        assert np.all(np.isfinite(cs.cols["tmax"]["optim"]))
        assert np.all(sc.walked(cs.numpy("tmin", blk_c), True)[2] == 0), "Tmin must not hide Tmax's status in a grid run"
    if name == "one":
        exact = 0
        for v in VARS:
            for p, (r, c) in zip(cs.numpy(v, block), block):
                order = cs.rk[v](r, c)[0][:sc.INIT]
                for m in sc.ONE_MONTHS:
                    assert fin[v]["optim"][m, order].sum() == 1 and fin[v]["anom"][m, order].sum() == 1
                # fl(fl(x w) / w) is x for most w, not for all: where it is, the tie goes to the even side (36, 38, 80); where
                # the quotient lands an ulp off the tie, the oracle's rounding of THAT quotient is what the GPU must give
                exact += (p["k"][list(sc.ONE_MONTHS)].tolist() == [36, 38, 80]) + (p["ka"][list(sc.ONE_MONTHS)].tolist() == [38, 80, 36])
                assert np.all(np.abs(p["k"][list(sc.ONE_MONTHS)] - sc.ONE_VALUES) <= 0.5)
                assert np.all(np.abs(p["ka"][list(sc.ONE_MONTHS)] - np.roll(sc.ONE_VALUES, -1)) <= 0.5)
                assert not p["rk"].any() and not p["ra"].any()
        print("one: (cell, family) items of %d whose three quotients are the ties themselves: %d" % (4 * len(block), exact))
        assert exact >= MIN_ITEMS
    if name == "families":
        for v in VARS:
            assert fin[v]["optim"].all() and not fin[v]["anom"].all() and not np.array_equal(fin[v]["anom"], fin[v]["nug"])


def _changed(true, mut, rkey, kkey, months):
    """(cell, month) items whose status or bandwidth the mutant changes."""
    return sum(int(((a[rkey] != b[rkey]) | (a[kkey] != b[kkey]))[months].sum()) for a, b in zip(true, mut))


def test_power_of_the_patterns(cs, orc):
    """Conditions on the INPUTS: see the module's docstring.  A pattern that misses one is enlarged, never the count lowered."""
    cells, pts = sc.window_cells(), sc.point_cells()
    true = cs.numpy("tmin", cells)
    for mut in sc.CATCHES[cs.name]:
        if mut == "M3":
            db, prm = cs.db(orc, "tmin"), orc.params()
            n = tot = 0
            for a, b, (r, c) in zip(cs.numpy("tmin", pts), cs.numpy("tmin", pts, mutant=mut), pts):
                pt = cs.oracle_pt(orc, "tmin", r, c)
                for m in np.nonzero(a["rk"] == 0)[0]:
                    _, m0, v0, _, _ = orc.krig(db, prm, pt, int(m) + 1, nnghs=int(a["k"][m]), vario=a["vario"][m])
                    _, m1, v1, _, _ = orc.krig(db, prm, pt, int(m) + 1, nnghs=int(a["k"][m]), vario=b["vario"][m])
                    n += max(abs(m1 - m0), abs(v1 - v0)) > 10 * FAST_BAR
                    tot += 1
            print("%s %s: %d of %d kriged (point, month) items move by more than %.0e" % (cs.name, mut, n, tot, 10 * FAST_BAR))
            assert n >= MIN_ITEMS, (cs.name, mut, n)
            continue
        months = np.arange(1, 12) if mut == "M1" else np.arange(12)
        mutd = cs.numpy("tmin", cells, mutant=mut)
        nk, na, tot = _changed(true, mutd, "rk", "k", months), _changed(true, mutd, "ra", "ka", months), len(cells) * months.size
        print("%s %s (%s): kk changes in %d of %d items (%.1f %%), ka in %d (%.1f %%)"
              % (cs.name, mut, sc.MUTANTS[mut], nk, tot, 100.0 * nk / tot, na, 100.0 * na / tot))
        if cs.name in ("slot1", "one"):                      # what the chosen cells alone contribute
            blk = sc.window_cells(sc.WIN, sc.BLOCK_A)
            tb, mb = cs.numpy("tmin", blk), cs.numpy("tmin", blk, mutant=mut)
            bk, ba = _changed(tb, mb, "rk", "k", months), _changed(tb, mb, "ra", "ka", months)
            print("%s %s: the %d chosen cells alone: kk %d, ka %d" % (cs.name, mut, len(blk), bk, ba))
            assert bk >= MIN_ITEMS and ba >= MIN_ITEMS, (cs.name, mut, bk, ba)
        if mut != "M2":
            assert nk >= MIN_ITEMS, (cs.name, mut, nk)
        assert na >= MIN_ITEMS, (cs.name, mut, na)
        if mut == "M1" and cs.name.startswith("indep"):
            assert 2 * nk >= tot and 2 * na >= tot, (cs.name, nk, na, tot)
