"""Generate tests/golden/golden_stnrast_v1.npz by EXECUTING the reference's step19 / step20-front lines on scripted inputs.
Needs the reference checkout (``make_golden.REF``); the tests only read the fixture.

    python tests/golden/make_golden_stnrast.py

Executed (read at run time, ``np.int`` / ``np.float`` aliased, nothing of the text is stored):
  * twx/utils/util_geo.py:19-40 (``grt_circle_dist``);
  * twx/raster/raster_dataset.py:68-75 (the extent lines of ``__init__``), :108-202 (``get_coord_grid_1d``, ``get_coord``,
    ``get_row_col``), :229-242 (``read_as_array``) and :329-339 (``is_inbounds``, ``_check_cellxy_valid``), placed under a class
    header and a constructor of ours that takes an array and ``geo_t`` in place of GDAL and an identity in place of osr;
  * twx/infill/post_infill.py:443-510 (``_find_nn_data``);
  * twx/infill/post_infill.py:286-352, the body of ``add_stn_raster_values``, under a function header of ours;
  * twx/infill/post_infill.py:193-246 (``find_dup_stns``) on a stand-in ``stnda`` whose ``flag_infilled`` lives in memory and
    masks its fill value on reading as netCDF4 does.
``bm.interp`` IS NOT EXECUTED REFERENCE: mpl_toolkits.basemap is not installed; ``bm`` is a namespace whose ``interp`` is the
restatement tests/restate_stnrast.py (the precedent: statsmodels stood in by ``lstsq``).  The calls the executed lines make
to it are logged, so the fixture records per station how its value was decided.

The maker refuses a fixture in which a ring winner and a runner-up with a different value lie within a relative 1e-6, in
which a station of an order-0 call has |fractional index - k - 0.5| < 1e-9, in which a forced station has no data cell in
any ring (the reference would loop for ever), or in which the restatement differs from what was executed.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_stnrast as RR  # noqa: E402

OUT = os.path.join(HERE, "golden_stnrast_v1.npz")
STN_ID, LON, LAT = "station_id", "longitude", "latitude"
# the option combinations of scripts/step19_add_raster_predictors.py: (extract_method, revert_nn, force_data_value)
COMBOS = {"lst": (1, True, True), "tdi": (1, True, False), "cell": (0, False, False)}
DUP_NDAYS = 50
FILL_I1 = np.int8(-127)


class _StatusCheck(object):
    def __init__(self, *a):
        pass

    def increment(self, *a):
        pass


class _Band(object):
    def __init__(self, a, ndata):
        self.a, self.ndata = a, ndata

    def ReadAsArray(self):
        return self.a

    def GetNoDataValue(self):
        return self.ndata


class _GdalDs(object):
    def __init__(self, a, ndata):
        self.RasterYSize, self.RasterXSize = a.shape
        self.band = _Band(a, ndata)

    def GetRasterBand(self, k):
        return self.band


class _Identity(object):
    def TransformPoint(self, lon, lat):
        return lon, lat, 0.0


def load_reference():
    import make_golden as mg
    for name, val in (("bool", bool), ("int", int), ("float", float), ("object", object), ("str", str)):
        if name not in vars(np):
            setattr(np, name, val)
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    geo = {}
    exec(compile("\n" * 18 + mg._slice("twx/utils/util_geo.py", 19, 40), "util_geo.py", "exec"), geo)
    head = ("class RasterDataset(object):\n"
            "    def __init__(self, gdal_ds, geo_t, identity):\n"
            "        self.gdal_ds = gdal_ds\n"
            "        self.geo_t = np.array(geo_t)\n"
            "        self.coordTrans_wgs84_to_src = identity\n")
    src = head + "".join(mg._slice("twx/raster/raster_dataset.py", a, b) + "\n" for a, b in ((68, 75), (108, 202), (229, 242),
                                                                                               (329, 339)))
    rast = dict(np=np)
    exec(compile(src, "raster_dataset.py", "exec"), rast)
    post = dict(np=np, grt_circle_dist=geo["grt_circle_dist"], STN_ID=STN_ID, LON=LON, LAT=LAT, StatusCheck=_StatusCheck)
    exec(compile("\n" * 442 + mg._slice("twx/infill/post_infill.py", 443, 510), "post_infill.py", "exec"), post)
    exec(compile("\n" * 192 + mg._slice("twx/infill/post_infill.py", 193, 246), "post_infill.py", "exec"), post)
    head = ("def add_stn_raster_values(stnda, var_name, long_name, units, a_rast, extract_method=1, revert_nn=False, "
            "force_data_value=False):\n")
    exec(compile(head + mg._slice("twx/infill/post_infill.py", 286, 352), "post_infill.py", "exec"), post)
    return geo["grt_circle_dist"], rast["RasterDataset"], post


# ---- the rasters ----------------------------------------------------------------------------------------------------------
def big_raster(rows, cols, dtype, ndata, seed):
    """Data with: a data-bearing row 0 and column 0 (upper half only) that ``_find_nn_data`` never admits; a no-data coast band
    ``band`` cells wide inside them; holes one cell high and two wide, three by four, and 21 by 31 (first data at rings 1, 2
    and 9 from the stations placed in them); scattered single no-data cells on the right-hand side."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if np.dtype(dtype).kind == "f":
        a = (280.0 + 0.05 * yy - 0.03 * xx + rs.randn(rows, cols)).astype(dtype)
    else:
        a = (1 + (yy // 9) * 7 + xx // 11).astype(dtype)
    band = 7 if cols > 100 else 3
    a[1:, 1:band + 1] = ndata                                         # the coast band; column 0 keeps data ...
    a[rows // 2:, 0] = ndata                                          # ... in the upper half only
    a[1:4, band + 1:] = ndata                                         # a band under row 0, which keeps data
    holes = {}
    if cols > 100:
        a[40, 50:52] = ndata
        a[50:53, 60:64] = ndata
        a[60:81, 100:131] = ndata
        holes = {"ring1": (40, 51), "ring2": (51, 62), "ring9": (72, 115)}
    else:
        a[20, 30:32] = ndata
        a[30:33, 40:44] = ndata
        a[38:59, 10:29] = ndata
        holes = {"ring1": (20, 31), "ring2": (31, 42), "ring9": (50, 19)}
    k = rs.permutation((rows - 10) * 20)[:25]
    a[5 + k // 20, cols - 25 + k % 20] = ndata
    return a, band, holes


def stations(grid, band, holes, seed):
    """(lon, lat, edge): ``edge`` marks the stations on cell edges, which only the bilinear combinations use."""
    rs = np.random.RandomState(seed)
    g, rows, cols = grid.geo_t, grid.rows, grid.cols
    pts = []

    def add(r, c, edge=False):                                        # fractional (row, col) of the cell-edge frame
        pts.append((g[0] + c * g[1], g[3] + r * g[5], edge))

    lo = band + 2 if band else 0
    for _ in range(24 if rows > 8 else 6):                            # anywhere inside
        add(rs.uniform(0.6, rows - 0.6), rs.uniform(0.6, cols - 0.6))
    for _ in range(8 if rows > 8 else 3):                             # on cell centres
        add(rs.randint(0, rows) + 0.5, rs.randint(0, cols) + 0.5)
    if rows > 8:
        for _ in range(6):                                            # on edges and corners, where all four cells have data
            add(float(rs.randint(8, rows // 3)), float(rs.randint(lo + 2, cols // 3)) + (0.0 if _ % 2 else 0.37), True)
    for f in (0.2, 0.45):                                             # the half-cell rim between centre and edge bounds
        add(f, rs.uniform(1.1, cols - 1.1)); add(rows - f, rs.uniform(1.1, cols - 1.1))
        add(rs.uniform(1.1, rows - 1.1), f); add(rs.uniform(1.1, rows - 1.1), cols - f)
    add(0.3, 0.3); add(rows - 0.3, cols - 0.3)
    for d in (0.7, 3.3, 1000.2):                                      # outside on each side: mirrored by abs(int()), clipped
        add(-d, rs.uniform(1.1, cols - 1.1)); add(rows + d, rs.uniform(1.1, cols - 1.1))
        add(rs.uniform(1.1, rows - 1.1), -d); add(rs.uniform(1.1, rows - 1.1), cols + d)
        add(rows * 0.75 + 0.27, -d)                                         # west of the lower half, where column 0 has no data
    add(-2.2, -1.4); add(rows + 2.2, cols + 1.4)
    if band:
        for c in range(1, band + 1):                                  # across the coast band: first data at ring band + 1 - c
            add(rows // 3 + 0.31 + c, c + 0.37)
            add(3 * rows // 4 + 0.31 + c, c + 0.37)
        for r in (1, 2, 3):                                           # under row 0
            add(r + 0.41, cols // 2 + 0.29 + r)
    for name, (r, c) in sorted(holes.items()):
        add(r + 0.43, c + 0.61)
        add(r + 0.58, c + 0.36)
    a = np.array(pts)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].astype(bool)


class _Stnda(object):
    """What ``add_stn_raster_values`` and ``find_dup_stns`` touch of a ``StationSerialDataDb``."""

    def __init__(self, ids, lon, lat, flag=None):
        self.stns = np.empty(len(ids), dtype=[(STN_ID, "U16"), (LON, np.float64), (LAT, np.float64)])
        self.stns[STN_ID], self.stns[LON], self.stns[LAT] = ids, lon, lat
        self.stn_ids = self.stns[STN_ID].copy()
        self.ds = self
        self.newvar = None
        if flag is not None:
            self.variables = {"flag_infilled": _MaskedVar(flag, FILL_I1)}

    def add_stn_variable(self, varname, long_name, units, dtype, fill_value=None):
        self.newvar = np.full(self.stns.size, np.nan)
        return self.newvar

    def sync(self):
        pass


class _MaskedVar(object):
    def __init__(self, a, fill):
        self.a, self.fill = a, fill

    def __getitem__(self, key):
        return np.ma.masked_equal(self.a[key], self.fill)


def run_combo(post, Raster, grt, data, geo_t, band_ndata, ndata, lon, lat, combo):
    """Execute ``add_stn_raster_values`` on one raster and one option combination; the fixture entries of the run."""
    method, revert, force = combo
    a_rast = Raster(_GdalDs(data, band_ndata), geo_t, _Identity())
    a_rast.ndata = ndata
    grid = RR.Grid(data, geo_t, band_ndata)
    grid.ndata = ndata
    mine = RR.add_stn_raster_values(grid, lon, lat, method, revert, force)
    if (mine["status"] == RR.NO_DATA_ANYWHERE).any():
        raise SystemExit("refused: a forced station has no data cell in any ring (the reference would not return)")
    log, rings = [], []

    def interp(datain, xin, yin, xout, yout, checkbounds=False, masked=False, order=1):
        try:
            v = RR.interp(datain, xin, yin, xout, yout, checkbounds=checkbounds, masked=masked, order=order)
        except ValueError:
            log.append((checkbounds, order, True))
            raise
        log.append((checkbounds, order, bool(np.ma.is_masked(v))))
        if order == 0:
            for n, cin, out in ((len(xin), xin, xout), (len(yin), yin, yout)):
                f = float(np.clip((n - 1) * (out - cin[0]) / (cin[-1] - cin[0]), 0, n - 1))
                if abs(f - np.floor(f) - 0.5) < 1e-9:
                    raise SystemExit("refused: an order-0 station sits on a rounding boundary (fractional index %r)" % f)
        return v

    find = post["_find_nn_data"]

    def find_nn(a_data, rast, x, y):
        val, dist = find(a_data, rast, x, y)
        rings.append((y, x, float(val), float(dist)))
        return val, dist

    ns = dict(post, bm=types.SimpleNamespace(interp=interp), _find_nn_data=find_nn)
    fn = types.FunctionType(post["add_stn_raster_values"].__code__, ns, "add_stn_raster_values",
                            post["add_stn_raster_values"].__defaults__)
    stnda = _Stnda(["S%04d" % i for i in range(lon.size)], lon, lat)
    ids_ndata = fn(stnda, "v", "", "", a_rast, extract_method=method, revert_nn=revert, force_data_value=force)
    values = np.asarray(stnda.newvar, np.float64)
    # how each station was decided, from the logged calls: one with checkbounds=True per station, in station order, and
    # the checkbounds=False call that may follow it
    status, k = np.empty(lon.size, np.int32), 0
    for i in range(lon.size):
        if not log[k][0]:
            raise SystemExit("refused: the logged interp calls are out of step")
        masked = log[k][2]
        k += 1
        st = RR.OK
        if k < len(log) and not log[k][0]:
            masked = log[k][2]
            k += 1
            if not masked:
                st = RR.NEAREST
        if masked:
            st = RR.NEEDS_FORCE if force else RR.NODATA
        status[i] = st
    if k != len(log):
        raise SystemExit("refused: the logged interp calls do not add up (%d of %d)" % (k, len(log)))
    forced = np.nonzero(status == RR.NEEDS_FORCE)[0]
    if forced.size != len(rings):
        raise SystemExit("refused: %d forced stations but %d ring searches" % (forced.size, len(rings)))
    ring = np.array(rings, np.float64).reshape(-1, 4)
    rowcol = np.array([a_rast.get_row_col(lon[i], lat[i], check_bounds=False) for i in range(lon.size)], np.int32)
    # the restatement against what was executed
    for name, a, b in (("status", status, mine["status"]), ("row", rowcol[:, 0], mine["row"]), ("col", rowcol[:, 1], mine["col"]),
                       ("value", values.view(np.uint64), mine["value"].view(np.uint64)), ("forced", forced, mine["forced"])):
        if not np.array_equal(a, b):
            raise SystemExit("refused: the restatement's %s differs from the executed reference" % name)
    for (y, x, val, dist), nn, i in zip(rings, mine["rings"], forced):
        if (y, x) != (rowcol[i, 0], rowcol[i, 1]) or val != nn["value"] or dist != nn["dist"]:
            raise SystemExit("refused: the restatement's ring search differs from the executed one at station %d" % i)
        if np.isfinite(nn["runner_up"]) and nn["runner_up"] - nn["dist"] <= 1e-6 * nn["runner_up"]:
            raise SystemExit("refused: station %d has a ring winner and a runner-up within a relative 1e-6" % i)
    ids = np.array(["S%04d" % i for i in range(lon.size)])
    if not np.array_equal(np.asarray(ids_ndata), ids[values == ndata]):
        raise SystemExit("refused: the returned ids are not the stations left at ndata")
    info = dict(value=values, status=status, row=rowcol[:, 0], col=rowcol[:, 1], forced=forced.astype(np.int32),
                ring_value=ring[:, 2], ring_dist=ring[:, 3], ring_r=np.array([nn["ring"] for nn in mine["rings"]], np.int32),
                ring_winner=np.array([nn["winner"] for nn in mine["rings"]], np.int32),
                ring_runner_up=np.array([nn["runner_up"] for nn in mine["rings"]], np.float64),
                ndata_ids=(values == ndata))
    return info


def dup_table(grt):
    """A sorted station table with classes of 2, 3 and 5 stations, pairs one ulp apart whose products agree and differ, a
    class whose counts of infilled days tie at the minimum, NaN-free; and its flag_infilled [DUP_NDAYS, nstn]."""
    rs = np.random.RandomState(2019)
    F = RR.RADIAN

    def ulp_pair(same):
        while True:
            v = rs.uniform(25.0, 50.0)
            w = np.nextafter(v, 100.0)
            if (v * F == w * F) == same:
                return v, w

    lon = list(rs.uniform(-120, -70, 24))
    lat = list(rs.uniform(25, 50, 24))

    def put(i, src=None, lo=None, la=None):
        lon[i] = lon[src] if lo is None else lo
        lat[i] = lat[src] if la is None else la

    put(9, 2)                                                         # class of 2: {2, 9}
    put(11, 5); put(20, 5)                                            # class of 3: {5, 11, 20}
    for i in (3, 7, 13, 17):
        put(i, 0)                                                     # class of 5 with the first station: {0, 3, 7, 13, 17}
    put(23, 14)                                                       # the last station in a class: {14, 23}
    v, w = ulp_pair(True)                                             # one ulp apart, equal products: a class {15, 16}
    put(15, lo=-100.25, la=v); put(16, lo=-100.25, la=w)
    v, w = ulp_pair(False)                                            # one ulp apart, different products: no class
    put(18, lo=-101.5, la=v); put(19, lo=-101.5, la=w)
    put(22, 21)                                                       # {21, 22}: tied counts, both kept
    lon, lat = np.array(lon), np.array(lat)
    n = lon.size
    flag = (rs.rand(DUP_NDAYS, n) < 0.4).astype(np.int8)
    flag[:, 22] = flag[:, 21]
    flag[:, 11] = 0; flag[:4, 11] = 1; flag[:, 20] = 0; flag[10:14, 20] = 1; flag[:, 5] = 1      # {5, 11, 20}: 11 and 20 tie
    flag[:5, 3] = FILL_I1                                             # masked days add nothing to the reference's sum
    ids = np.array(["US%05d" % (7 * i + 3) for i in range(n)])
    return ids, lon, lat, flag


def main():
    grt, Raster, post = load_reference()
    rec = {}
    cases = []
    a, band, holes = big_raster(130, 257, np.float32, -9999.0, 11)
    cases.append(("lst", a, (-111.0, 1.0 / 120, 0.0, 46.0, 0.0, -1.0 / 120), -9999.0, -9999.0, band, holes))
    a, band, holes = big_raster(64, 65, np.int16, -32768, 12)
    cases.append(("div", a, (-105.3, 0.05, 0.0, 41.7, 0.0, -0.04), -32768.0, -32768.0, band, holes))
    a, band, holes = big_raster(64, 65, np.uint8, 255, 13)
    a[a != 255] = 1
    cases.append(("mask", a, (-105.3, 0.05, 0.0, 41.7, 0.0, -0.04), 255.0, 0.0, band, holes))     # step19: a_rast.ndata = 0
    a = np.array([[1.5, 2.5, -1.0, 4.5, 5.5], [6.5, -1.0, 8.5, 9.5, 10.5], [-1.0, 12.5, 13.5, 14.5, 15.5]], np.float64)
    cases.append(("small", a, (10.0, 0.5, 0.0, -20.0, 0.0, -0.25), -1.0, -1.0, 0, {}))
    a = np.array([[1.5, -9999.0], [3.25, 4.0]], np.float32)
    cases.append(("two", a, (-0.75, 1.0, 0.0, 0.5, 0.0, -1.0), -9999.0, -9999.0, 0, {}))
    rec["cases"] = np.array([c[0] for c in cases])
    rec["combos"] = np.array(sorted(COMBOS))
    total = 0
    for k, (name, data, geo_t, band_ndata, ndata, band, holes) in enumerate(cases):
        a_rast = Raster(_GdalDs(data, band_ndata), geo_t, _Identity())
        grid = RR.Grid(data, geo_t, band_ndata)
        lon, lat, edge = stations(grid, band, holes, 100 + k)
        # a forced station from whose start no ring holds an admissible data cell cannot be executed (the reference never
        # returns): such a placement is not made.  Only the 2 x 2 raster, whose one admissible cell is (1, 1), has any
        never = RR.add_stn_raster_values(grid, lon, lat, *COMBOS["lst"])["status"] == RR.NO_DATA_ANYWHERE
        if never.any():
            print("%s: %d placements without an admissible data cell in any ring are not made" % (name, never.sum()))
            lon, lat, edge = lon[~never], lat[~never], edge[~never]
        if name == "mask":
            ndata_runs = {"cell": 0.0}                                # the mask raster is only read with extract_method 0
        else:
            ndata_runs = {c: ndata for c in COMBOS}
        rec.update({name + "_data": data, name + "_geo_t": np.array(geo_t), name + "_band_ndata": np.float64(band_ndata),
                    name + "_ndata": np.float64(ndata), name + "_lon": lon, name + "_lat": lat, name + "_edge": edge})
        # the executed methods of RasterDataset
        yg, xg = a_rast.get_coord_grid_1d()
        rr, cc = np.arange(data.shape[0]), np.arange(data.shape[1])
        ycell, xcell = a_rast.get_coord(rr[:, None], cc[None, :])
        masked = a_rast.read_as_array()
        rec.update({name + "_ygrid": yg, name + "_xgrid": xg, name + "_ycell": ycell + 0 * xcell, name + "_xcell": xcell + 0 * ycell,
                    name + "_extent": np.array([a_rast.min_x, a_rast.max_x, a_rast.min_y, a_rast.max_y]),
                    name + "_inbounds": np.array([bool(a_rast.is_inbounds(lon[i], lat[i])) for i in range(lon.size)]),
                    name + "_mask": np.ma.getmaskarray(masked)})
        for combo, nd in sorted(ndata_runs.items()):
            sel = np.ones(lon.size, bool) if COMBOS[combo][0] == 1 else ~edge
            info = run_combo(post, Raster, grt, data, geo_t, band_ndata, nd, lon[sel], lat[sel], COMBOS[combo])
            rec[name + "_" + combo + "_sel"] = sel
            for key, v in info.items():
                rec["%s_%s_%s" % (name, combo, key)] = v
            st = info["status"]
            total += int(sel.sum())
            print("%-5s %-4s %3d stations: %3d by the method, %3d nearest, %3d forced (rings %s), %3d no data" % (
                name, combo, sel.sum(), (st == RR.OK).sum(), (st == RR.NEAREST).sum(), (st == RR.NEEDS_FORCE).sum(),
                sorted(set(info["ring_r"].tolist())), (st == RR.NODATA).sum()))
    print("%d station decisions" % total)
    # ---- grt_circle_dist, the zero-distance criterion on the table, find_dup_stns ----
    ids, lon, lat, flag = dup_table(grt)
    stnda = _Stnda(ids, lon, lat, flag)
    rm = post["find_dup_stns"](stnda)
    mine = RR.find_dup_stns(ids, lon, lat, np.where(flag == FILL_I1, 0, flag))
    if not np.array_equal(np.asarray(rm, dtype=str), np.asarray(mine, dtype=str)):
        raise SystemExit("refused: the restatement's duplicate stations differ from the executed reference")
    zero = np.array([[grt(lon[i], lat[i], lon[j], lat[j]) == 0 for j in range(lon.size)] for i in range(lon.size)])
    cls, size = RR.dup_classes(lon, lat)
    if not np.array_equal(zero, cls[:, None] == cls[None, :]):
        raise SystemExit("refused: the key criterion differs from grt_circle_dist == 0 on the table")
    rs = np.random.RandomState(77)
    plon, plat = rs.uniform(-180, 180, (2, 200)), rs.uniform(-90, 90, (2, 200))
    rec.update(dup_ids=ids, dup_lon=lon, dup_lat=lat, dup_flag=flag, dup_rm=np.asarray(rm, dtype=str), dup_zero=zero,
               dist_lon=plon, dist_lat=plat, dist_km=grt(plon[0], plat[0], plon[1], plat[1]))
    print("duplicates: classes %s, removed %s" % (sorted(set(size[size > 1].tolist())), list(rm)))
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
