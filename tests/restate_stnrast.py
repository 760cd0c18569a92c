"""numpy restatements of step19 and of the front of step20, one station at a time as the reference runs them.

* ``interp``: mpl_toolkits.basemap.interp on a regular grid, orders 0 and 1, ``checkbounds`` and the propagation of a masked
  ``datain`` (the published algorithm restated, as for ``k_sample``: basemap is not vendored and is not executed);
* ``Grid``: the methods of ``RasterDataset`` (twx/raster/raster_dataset.py) that step19 uses, under a constructor that takes
  an array and ``geo_t`` in place of GDAL; the osr transformation is the identity;
* ``sample``: the decision of ``add_stn_raster_values`` (twx/infill/post_infill.py:305-339) up to the ring search;
* ``find_nn_data``: ``_find_nn_data`` (:443-510) with the ring, the slot and the runner-up that ``twxrv_nearest_data`` returns;
* ``add_stn_raster_values``: the two together, per station;
* ``dup_classes`` / ``find_dup_stns``: the location classes by key and the reference's removal rule (:193-246);
* ``col_count``: the two column counts.
"""
import numpy as np

RADIAN = 0.017453292519943295
EARTH_KM = 6371.009
OK, NEAREST, NODATA, NEEDS_FORCE, NO_DATA_ANYWHERE = 0, 35, 36, 37, 38
TIE_REL = 1e-9


def grt_circle_dist(lon1, lat1, lon2, lat2):
    lat1rad, lat2rad = lat1 * RADIAN, lat2 * RADIAN
    lon1rad, lon2rad = lon1 * RADIAN, lon2 * RADIAN
    dlat, dlon = lat1rad - lat2rad, lon1rad - lon2rad
    ca = 2 * np.arcsin(np.sqrt((np.sin(dlat / 2)) ** 2 + np.cos(lat1rad) * np.cos(lat2rad) * (np.sin(dlon / 2)) ** 2))
    return EARTH_KM * ca


def interp(datain, xin, yin, xout, yout, checkbounds=False, masked=False, order=1):
    """basemap.interp for a regular grid (``masked`` must be False, as step19 calls it).  ``datain`` may be a masked array:
    a masked cell masks the result."""
    if masked:
        raise NotImplementedError("masked=True is not what step19 uses")
    if xin[-1] - xin[0] < 0 or yin[-1] - yin[0] < 0:
        raise ValueError("xin and yin must be increasing!")
    if checkbounds:
        if xout.min() < xin.min() or xout.max() > xin.max() or yout.min() < yin.min() or yout.max() > yin.max():
            raise ValueError("yout or xout outside range of yin or xin")
    delx = xin[1:] - xin[0:-1]
    dely = yin[1:] - yin[0:-1]
    if not (max(delx) - min(delx) < 1.e-4 and max(dely) - min(dely) < 1.e-4):
        raise NotImplementedError("irregular grid")
    xcoords = (len(xin) - 1) * (xout - xin[0]) / (xin[-1] - xin[0])
    ycoords = (len(yin) - 1) * (yout - yin[0]) / (yin[-1] - yin[0])
    xcoords = np.clip(xcoords, 0, len(xin) - 1)
    ycoords = np.clip(ycoords, 0, len(yin) - 1)
    if order == 1:
        xi = xcoords.astype(np.int32)
        yi = ycoords.astype(np.int32)
        xip1 = np.clip(xi + 1, 0, len(xin) - 1)
        yip1 = np.clip(yi + 1, 0, len(yin) - 1)
        delx = xcoords - xi.astype(np.float32)
        dely = ycoords - yi.astype(np.float32)
        return (1. - delx) * (1. - dely) * datain[yi, xi] + delx * dely * datain[yip1, xip1] + \
            (1. - delx) * dely * datain[yip1, xi] + delx * (1. - dely) * datain[yi, xip1]
    if order == 0:
        xcoordsi = np.around(xcoords).astype(np.int32)
        ycoordsi = np.around(ycoords).astype(np.int32)
        return datain[ycoordsi, xcoordsi]
    raise ValueError("order keyword must be 0 or 1 here")


class Grid(object):
    """``RasterDataset`` without GDAL.  ``band_ndata``: the band's no-data value (what ``read_as_array`` masks);
    ``ndata``: the attribute step19 may reassign."""

    def __init__(self, data, geo_t, band_ndata):
        self.data = np.asarray(data)
        self.geo_t = np.array(geo_t, dtype=np.float64)
        self.rows, self.cols = self.data.shape
        self.band_ndata = band_ndata
        self.ndata = band_ndata
        self.min_x = self.geo_t[0]
        self.max_x = self.min_x + (self.cols * self.geo_t[1])
        self.max_y = self.geo_t[3]
        self.min_y = self.max_y - (-self.rows * self.geo_t[5])

    def get_coord(self, row, col):
        x = (self.geo_t[0] + col * self.geo_t[1] + row * self.geo_t[2]) + self.geo_t[1] / 2.0
        y = (self.geo_t[3] + col * self.geo_t[4] + row * self.geo_t[5]) + self.geo_t[5] / 2.0
        return y, x

    def get_coord_grid_1d(self):
        ulx = self.geo_t[0] + (self.geo_t[1] / 2.0)
        urx = self.get_coord(0, self.cols - 1)[1]
        uly = self.geo_t[3] + (self.geo_t[5] / 2.0)
        lly = self.get_coord(self.rows - 1, 0)[0]
        return np.linspace(uly, lly, self.rows), np.linspace(ulx, urx, self.cols)

    def is_inbounds(self, x_geo, y_geo):
        return x_geo >= self.min_x and x_geo <= self.max_x and y_geo >= self.min_y and y_geo <= self.max_y

    def get_row_col(self, lon, lat, check_bounds=True):
        if check_bounds and not self.is_inbounds(lon, lat):
            raise ValueError("lat/lon outside raster bounds: " + str(lat) + "," + str(lon))
        xoff = abs(int((lon - self.geo_t[0]) / self.geo_t[1]))
        yoff = abs(int((lat - self.geo_t[3]) / self.geo_t[5]))
        return min(max(yoff, 0), self.rows - 1), min(max(xoff, 0), self.cols - 1)

    def read_as_array(self):
        return np.ma.masked_equal(self.data, self.band_ndata)


def ring_slots(rows, cols, y, x, r):
    """(slot, row, col) of the cells of ring ``r`` that the reference's tests admit, in its order; slots count the whole
    ring: top row, left column, bottom row without its last cell, right column without its last cell."""
    lcol, rcol, trow, brow = x - r, x + r, y - r, y + r
    out, s = [], 0
    for i in range(lcol, rcol + 1):
        if 0 < trow < rows and 0 < i < cols:
            out.append((s, trow, i))
        s += 1
    for i in range(trow, brow + 1):
        if 0 < lcol < cols and 0 < i < rows:
            out.append((s, i, lcol))
        s += 1
    for i in range(rcol, lcol, -1):
        if 0 < brow < rows and 0 < i < cols:
            out.append((s, brow, i))
        s += 1
    for i in range(brow, trow, -1):
        if 0 < rcol < cols and 0 < i < rows:
            out.append((s, i, rcol))
        s += 1
    assert s == 8 * r + 2
    return out


def find_nn_data(a_data, grid, x, y):
    """``_find_nn_data(a_data, a_rast, x, y)``: dict of value, dist, ring, winner (slot), runner_up (the nearest candidate of
    the ring in another cell, +Inf if none) and status.  The ring is capped at max(rows, cols)."""
    for r in range(1, max(grid.rows, grid.cols) + 1):
        nn = [(s, rr, cc) for s, rr, cc in ring_slots(grid.rows, grid.cols, y, x, r) if float(a_data[rr, cc]) != grid.ndata]
        if nn:
            break
    else:
        return dict(value=float(grid.ndata), dist=np.inf, ring=0, winner=-1, runner_up=np.inf, status=NO_DATA_ANYWHERE)
    slot = np.array([n[0] for n in nn])
    rr, cc = np.array([n[1] for n in nn]), np.array([n[2] for n in nn])
    lats, lons = grid.get_coord(rr, cc)
    pt_lat, pt_lon = grid.get_coord(y, x)
    d = grt_circle_dist(pt_lon, pt_lat, lons, lats)
    j = int(np.argsort(d, kind="stable")[0])
    other = (rr != rr[j]) | (cc != cc[j])
    return dict(value=float(a_data[rr[j], cc[j]]), dist=float(d[j]), ring=r, winner=int(slot[j]),
                runner_up=float(d[other].min()) if other.any() else np.inf, status=OK)


def sample(grid, lon, lat, extract_method=1, revert_nn=False, force_data_value=False):
    """post_infill.py:286-339 without the ring search, per station: value, status, row, col arrays."""
    a = grid.read_as_array()
    aflip = np.flipud(a).astype(float)
    ygrid, xgrid = grid.get_coord_grid_1d()
    ygrid = np.sort(ygrid)
    n = len(lon)
    val, status = np.empty(n), np.empty(n, np.int32)
    row, col = np.empty(n, np.int32), np.empty(n, np.int32)
    for x in range(n):
        st = OK
        try:
            rval = interp(aflip, xgrid, ygrid, np.array(lon[x]), np.array(lat[x]), checkbounds=True, masked=False,
                          order=extract_method)
        except ValueError:
            rval = np.ma.masked
        if (np.ma.is_masked(rval) and ((grid.is_inbounds(lon[x], lat[x]) and (extract_method == 0 or revert_nn))
                                       or force_data_value)):
            rval = interp(aflip, xgrid, ygrid, np.array(lon[x]), np.array(lat[x]), checkbounds=False, masked=False, order=0)
            if not np.ma.is_masked(rval):
                st = NEAREST
        if np.ma.is_masked(rval):
            st = NEEDS_FORCE if force_data_value else NODATA
            rval = grid.ndata
        val[x], status[x] = rval, st
        row[x], col[x] = grid.get_row_col(lon[x], lat[x], check_bounds=False)
    return dict(value=val, status=status, row=row, col=col)


def add_stn_raster_values(grid, lon, lat, extract_method=1, revert_nn=False, force_data_value=False):
    """The whole decision: the values written (``ndata`` where none), the per-station status (a forced station keeps
    ``NEEDS_FORCE``; one the ring search could not serve has ``NO_DATA_ANYWHERE``) and the ring results of the forced ones."""
    out = sample(grid, lon, lat, extract_method, revert_nn, force_data_value)
    forced = np.nonzero(out["status"] == NEEDS_FORCE)[0]
    rings = []
    for i in forced:
        nn = find_nn_data(grid.data, grid, int(out["col"][i]), int(out["row"][i]))
        rings.append(nn)
        out["value"][i] = nn["value"]
        if nn["status"] != OK:
            out["status"][i] = NO_DATA_ANYWHERE
    out["forced"], out["rings"] = forced, rings
    return out


def dup_classes(lon, lat):
    """(cls, size): the smallest index with the same keys lat * F, lon * F, and the number of such stations."""
    klon, klat = np.asarray(lon, np.float64) * RADIAN, np.asarray(lat, np.float64) * RADIAN
    n = klon.size
    cls, size = np.arange(n, dtype=np.int32), np.ones(n, np.int32)
    for i in range(n):
        eq = np.nonzero((klat == klat[i]) & (klon == klon[i]))[0]
        if eq.size:
            cls[i], size[i] = eq[0], eq.size
    return cls, size


def find_dup_stns(stn_ids, lon, lat, flag_infilled):
    """``find_dup_stns`` from the classes, for a table sorted by id: classes in order of their first member, members sorted
    by id, every member whose count of infilled days is not the class minimum is removed."""
    stn_ids = np.asarray(stn_ids)
    cls, size = dup_classes(lon, lat)
    rm = []
    for first in np.nonzero((cls == np.arange(cls.size)) & (size > 1))[0]:
        members = np.nonzero(cls == first)[0]
        members = members[np.argsort(stn_ids[members], kind="stable")]
        sums = np.sum(np.asarray(flag_infilled)[:, members], axis=0)
        rm.extend(stn_ids[members][sums != np.min(sums)])
    return np.array(rm)


def col_count(data, cols=None, fill=None):
    data = np.asarray(data)
    cols = np.arange(data.shape[1]) if cols is None else np.asarray(cols, np.int64)
    if data.dtype == np.int8:
        sel = data[:, cols].astype(np.int32)
        if fill is not None:
            sel = np.where(sel == int(fill), 0, sel)
        return sel.sum(axis=0).astype(np.int32).reshape(cols.size)
    sel = data[:, cols]
    return (~np.isfinite(sel) | (sel == np.float32(fill))).sum(axis=0).astype(np.int32).reshape(cols.size)
