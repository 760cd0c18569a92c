"""``twx/infill/post_infill.py`` and the scripts around it, from step16's result to the serially-complete station
databases the interpolation reads:

* ``write_infill_db``: the infilled database of step16's writer (``proc_write``, step16_mpi_infill_stn_daily.py:141-169);
* ``get_bad_infill_stnids`` / ``suspect_infill_stnids`` / ``find_bad_infill_stns`` / ``write_bad_stns_csv``: step17
  (step17_find_bad_infill_stns.py), the whole series of every suspect station through ONE ``twxsc_series_check`` call per
  variable;
* ``create_serially_complete_db`` / ``add_monthly_normals``: step18 (post_infill.py:79-156, 354-402), every station through
  one batched ``twxsc_serial_complete`` call instead of a loop over stations through netCDF;
* ``add_stn_raster_values``: step19 (post_infill.py:248-352 with ``_find_nn_data``, :443-510), one ``twxrv_sample`` call per
  raster over all stations and one ``twxrv_nearest_data`` call over those that need a forced value;
* ``find_dup_stns``: the front of step20 (post_infill.py:193-246), ``twxrv_dup_classes`` and ``twxrv_col_count`` instead of
  the n x n loop.

The kernels are ``topowx_amd/qa/twx_serial.hip`` and ``topowx_amd/qa/twx_stnrast.hip`` (include/twx_qa.h).  There is no CPU
fallback.
"""
import os

import numpy as np

from .. import _qalib, ncio
from ..dates import DAY, MONTH, YEAR
from ..stationdb import LAT, LON, STN_ID, get_norm_varname

__all__ = ["SERIAL_DB_VARIABLES", "USE_ALL_INFILL_THRESHOLD", "write_infill_db", "get_bad_infill_stnids", "suspect_infill_stnids",
           "find_bad_infill_stns", "write_bad_stns_csv", "create_serially_complete_db", "add_monthly_normals", "SerialComplete", "add_stn_raster_values", "find_dup_stns"]

FILL_I1 = -127                                   # netCDF4.default_fillvals['i1']
_LONG = {"tmin": "minimum air temperature", "tmax": "maximum air temperature"}
SERIAL_DB_VARIABLES = {v: [(v, "f4", float(ncio.FILL_F4), _LONG[v], "C"), ("flag_infilled", "i1", FILL_I1, "infilled flag", "")]
                       for v in ("tmin", "tmax")}
USE_ALL_INFILL_THRESHOLD = _qalib.run_threshold(5.0)          # 5 years of data (post_infill.py:39)
NONOPTIM_IMPOSS_VAL, NONOPTIM_VARI_CHGPT = "impossible infill values", "variance change point"      # infill_daily.py:50-51
RECORD_TMAX, RECORD_TMIN = 57.7, -89.4           # world records of daily Tmax and Tmin, degrees C (step17:35-36)
BAD_REASON = "infill issue"


def _field(result, name, *alt):
    for k in (name,) + alt:
        if isinstance(result, dict) or hasattr(result, "files"):
            if k in (result.files if hasattr(result, "files") else result):
                return np.asarray(result[k])
        elif hasattr(result, k):
            return np.asarray(getattr(result, k))
    raise KeyError("the infill result has no %r" % name)


def write_infill_db(path, stns, days, tair_var, result, format=None, deflate=None, device=0, timing=None):
    """The infilled station database of step16's writer (``proc_write``:141-169): ``<var>`` f4, ``flag_infilled`` i1 and
    ``<var>_infilled`` f4 on ``(time, station_id)`` through ``ncio.create_quick_db``, and the station variables ``mae`` and
    ``bias`` f8.  ``result``: what ``infill_daily`` returned, or a loaded step16 report (``ids``, ``fnl_tair``,
    ``mask_infill``, ``infill_tair``, ``mae``, ``bias``); ``stns``: a station table (sorted by id) that holds its stations.
    The database has the result's stations in the table's order.  NaN in the series is written as the fill value.
    ``deflate`` = ``"gpu"``: the three series go station-major, as the result has them, through
    ``ncio.write_series_chunks`` -- their chunks are shuffled and deflated on the GPU, nothing is transposed (``"host"``:
    the same call, libhdf5 deflates); ``None``: the assignment of the transposed arrays, the file as it always was.
    Refuses to overwrite an existing file."""
    if deflate not in (None, "gpu", "host"):
        raise ValueError("deflate must be None, 'gpu' or 'host', not %r" % (deflate,))
    if tair_var not in SERIAL_DB_VARIABLES:
        raise ValueError("tair_var must be 'tmin' or 'tmax'")
    path = os.fspath(path)
    if os.path.exists(path):
        raise FileExistsError("%s exists: the infilled database is not overwritten" % path)
    ids = [str(s) for s in _field(result, "target_ids", "ids")]
    fnl, mask, model = _field(result, "fnl_tair"), _field(result, "mask_infill"), _field(result, "infill_tair")
    mae, bias = _field(result, "mae"), _field(result, "bias")
    nd = int(days.size)
    if fnl.shape != (len(ids), nd) or mask.shape != fnl.shape or model.shape != fnl.shape or mae.shape != (len(ids),) or \
            bias.shape != mae.shape:
        raise ValueError("the infill result must be [nstations, %d days] over its ids" % nd)
    stns = np.asarray(stns)
    pos = {s: i for i, s in enumerate(ids)}
    if len(pos) != len(ids):
        raise ValueError("the infill result names a station twice")
    table = [str(s) for s in stns[STN_ID]]
    missing = [s for s in ids if s not in set(table)]
    if missing:
        raise KeyError("%d stations of the infill result are not in the station table (first: %s)" % (len(missing), missing[0]))
    keep = np.array([s in pos for s in table], bool)
    sub = stns[keep]
    order = np.array([pos[str(s)] for s in sub[STN_ID]], np.int64)
    fill = float(ncio.FILL_F4)
    variables = [SERIAL_DB_VARIABLES[tair_var][0], SERIAL_DB_VARIABLES[tair_var][1],
                 (tair_var + "_infilled", "f4", fill, "infilled " + _LONG[tair_var], "C")]
    ncio.create_quick_db(path, sub, days, variables, format=format)
    ds = ncio.open_dataset(path, "a")
    try:
        def f4(a, rows=False):
            a = np.asarray(a[order], np.float32)
            a = a if rows else a.T
            return np.ascontiguousarray(np.where(np.isnan(a), np.float32(fill), a))
        if deflate is None:
            ds.variables[tair_var][:] = f4(fnl)
            ds.variables[tair_var + "_infilled"][:] = f4(model)
            ds.variables["flag_infilled"][:] = np.ascontiguousarray((mask[order] != 0).astype(np.int8).T)
        else:
            kw = dict(deflate=deflate, device=device, timing=timing)
            ncio.write_series_chunks(ds.variables[tair_var], f4(fnl, rows=True), **kw)
            ncio.write_series_chunks(ds.variables[tair_var + "_infilled"], f4(model, rows=True), **kw)
            ncio.write_series_chunks(ds.variables["flag_infilled"], np.ascontiguousarray((mask[order] != 0).astype(np.int8)), **kw)
        for name, long_name, a in (("mae", "mean absolute error", mae), ("bias", "bias", bias)):
            v = ds.createVariable(name, "f8", (STN_ID,), fill_value=ncio.FILL_F8)
            v.long_name, v.units = long_name, "C"
            a = np.asarray(a[order], np.float64)
            v[:] = np.where(np.isnan(a), ncio.FILL_F8, a)
    finally:
        ds.close()
    return path


def get_bad_infill_stnids(fpath_log):
    """The reference's parser of its step16 log (post_infill.py:404-441), for users who have such logs: the stations of
    the ``Could not infill`` lines and of the ``ERROR|`` lines that name an impossible value or a variance change point.
    Sorted unique ids (an empty array where the reference would fail on a log without such lines)."""
    with open(fpath_log) as fh:
        lines = fh.readlines()
    ids = set()
    for ln in lines:
        if "Could not infill" in ln:
            ids.add(ln.split("|")[0].split(" ")[-1])
        if ln.startswith("ERROR") and (NONOPTIM_IMPOSS_VAL in ln or NONOPTIM_VARI_CHGPT in ln):
            ids.add(ln.split("|")[1].split(" ")[0])
    return np.array(sorted(ids)) if ids else np.array([], "U1")


def suspect_infill_stnids(report):
    """The question of ``get_bad_infill_stnids`` asked of a step16 report (or an ``infill_daily`` result): a station is
    suspect if any month's ``status`` is not ``PP_OK`` (the reference's ``Could not infill``; -1, a month without a day, is
    no item) or, in a ``--chk-perf`` report, if any month is ``nonoptimal`` and the kept attempt's ``reasons`` carry
    ``CK_IMPOSSIBLE`` or ``CK_VAR_CHGPT`` (its ``ERROR|`` lines).  Sorted unique ids."""
    ids = np.array([str(s) for s in _field(report, "target_ids", "ids")])
    status = _field(report, "status")
    bad = ((status != _qalib.PP_OK) & (status != -1)).any(axis=1)
    try:
        nonopt, attempt, reasons = _field(report, "nonoptimal"), _field(report, "attempt"), _field(report, "reasons")
    except KeyError:
        nonopt = None
    if nonopt is not None:
        kept = np.take_along_axis(reasons, np.maximum(attempt, 0)[..., None], axis=2)[..., 0]
        hit = (nonopt != 0) & (attempt >= 0) & (kept >= 0) & ((kept & (_qalib.CK_IMPOSSIBLE | _qalib.CK_VAR_CHGPT)) != 0)
        bad |= hit.any(axis=1)
    return np.unique(ids[bad])


def _read_rows(path, tair_var, stnids, names):
    """The rows of ``stnids`` that the database has, station-major: (present [n] bool, dict of name -> [npresent, ndays])."""
    ds = ncio.open_dataset(path, "r")
    try:
        if tair_var not in ds.variables:
            raise KeyError("%s has no variable %r" % (path, tair_var))
        ids = ncio._read_ids(ds.variables[STN_ID])
        pos = {str(s): i for i, s in enumerate(ids)}
        present = np.array([str(s) in pos for s in stnids], bool)
        cols = np.array([pos[str(s)] for s, p in zip(stnids, present) if p], np.int64)
        out = {}
        for name in names:
            a = np.asarray(ds.variables[name][:])
            out[name] = np.ascontiguousarray(a[:, cols].T)
    finally:
        ds.close()
    return present, out


def find_bad_infill_stns(fpath_infill_tmin, fpath_infill_tmax, stnids, sig=_qalib.CK_SIG, device=0, timing=None):
    """step17 (step17_find_bad_infill_stns.py:40-82): the ``<var>`` series of the stations ``stnids`` from each infilled
    database, ONE ``twxsc_series_check`` call per variable.  A station is bad if either variable has a variance change point
    over its whole series, a value beyond the world records (57.7 / -89.4) or a missing value; an id that a database does
    not have is not bad for that variable (the reference's ``KeyError`` branch).  Returns (bad ids in the order of
    ``stnids``, details): details[var] is a dict of ``present`` [n] and, for the present stations scattered back to [n],
    ``nimpossible``, ``nmissing``, ``cpt_stat``, ``cpt_tau``, ``reasons``, ``status`` (0 / NaN where absent), ``bad`` and
    ``pen``."""
    stnids = [str(s) for s in stnids]
    n = len(stnids)
    bad = np.zeros(n, bool)
    details = {}
    for var, path in (("tmin", fpath_infill_tmin), ("tmax", fpath_infill_tmax)):
        present, rows = _read_rows(path, var, stnids, (var,))
        d = dict(present=present, nimpossible=np.zeros(n, np.int32), nmissing=np.zeros(n, np.int32), cpt_stat=np.full(n, np.nan),
                 cpt_tau=np.zeros(n, np.int32), reasons=np.zeros(n, np.int32), status=np.zeros(n, np.int32),
                 bad=np.zeros(n, bool), pen=np.nan)
        if present.any():
            r = _qalib.series_check(rows[var], sig=sig, fill=float(ncio.FILL_F4), impossible_high=RECORD_TMAX,
                                    impossible_low=RECORD_TMIN, device=device, timing=timing)
            for k in ("nimpossible", "nmissing", "cpt_stat", "cpt_tau", "reasons", "status"):
                d[k][present] = r[k]
            d["pen"] = r["pen"]
            d["bad"][present] = (r["reasons"] & (_qalib.CK_IMPOSSIBLE | _qalib.CK_VAR_CHGPT | _qalib.CK_UNFITTED)) != 0
        bad |= d["bad"]
        details[var] = d
    return [s for s, b in zip(stnids, bad) if b], details


def write_bad_stns_csv(path, ids):
    """``station_id,reason`` rows with the reason ``infill issue`` (step17:80-82)."""
    with open(path, "w") as fh:
        fh.write("%s,reason\n" % STN_ID)
        for s in ids:
            fh.write("%s,%s\n" % (s, BAD_REASON))
    return path


class SerialComplete(object):
    """What ``create_serially_complete_db`` returns: ``stn_ids``, ``all_infill`` [nstn] bool, ``max_run``, ``nmissing``
    [nstn], and ``norm`` [nstn, 12] / ``norm_nmths`` if normals were asked for (else None)."""

    def __init__(self, stn_ids, r):
        self.stn_ids = stn_ids
        self.all_infill, self.max_run, self.nmissing = r["all_infill"], r["max_run"], r["nmissing"]
        self.norm, self.norm_nmths = r.get("norm"), r.get("norm_nmths")


def create_serially_complete_db(fpath_infill_db, tair_var, fpath_out_serial_db, device=0, format=None, timing=None,
                                norm_yrs=None, max_miss=_qalib.SC_MAX_MISS, deflate=None):
    """``create_serially_complete_db`` (post_infill.py:79-156): the serial database with ``SERIAL_DB_VARIABLES`` over the
    infilled database's station table and day axis; per station "observations + infill", or "all model" if its longest run
    of infilled days reaches ``USE_ALL_INFILL_THRESHOLD``; values still missing become the fill value.  One
    ``twxsc_serial_complete`` call over all stations.  ``norm_yrs`` = (start, end): the same call also computes the monthly
    normals, returned in the record (they are written by ``add_monthly_normals``).  Prints the reference's warning per
    station with missing values and its "% of stns with all infilled values" line.  ``deflate`` = ``"gpu"``: the kernel's
    station-major rows go through ``ncio.write_series_chunks``, their chunks shuffled and deflated on the GPU and nothing
    transposed (``"host"``: libhdf5 deflates); ``None``: the assignment of the transposed arrays, the file as it always was."""
    if deflate not in (None, "gpu", "host"):
        raise ValueError("deflate must be None, 'gpu' or 'host', not %r" % (deflate,))
    if tair_var not in SERIAL_DB_VARIABLES:
        raise ValueError("tair_var must be 'tmin' or 'tmax'")
    stns, _, days, _ = ncio.read_station_db_arrays(fpath_infill_db, tair_var)
    ds = ncio.open_dataset(fpath_infill_db, "r")
    try:
        for name in (tair_var, tair_var + "_infilled", "flag_infilled"):
            if name not in ds.variables:
                raise KeyError("%s has no variable %r: not an infilled database" % (fpath_infill_db, name))
        tair = np.ascontiguousarray(np.asarray(ds.variables[tair_var][:], np.float32).T)
        model = np.ascontiguousarray(np.asarray(ds.variables[tair_var + "_infilled"][:], np.float32).T)
        flag = np.ascontiguousarray(np.asarray(ds.variables["flag_infilled"][:]).astype(np.int8).T)
    finally:
        ds.close()
    gf = gn = None
    if norm_yrs is not None:
        gf, gn = _qalib.norm_groups(days[YEAR], days[MONTH], norm_yrs[0], norm_yrs[1], day=days[DAY])
    if os.path.exists(fpath_out_serial_db):
        raise FileExistsError("%s exists: the serial database is not overwritten" % fpath_out_serial_db)
    ncio.create_quick_db(fpath_out_serial_db, stns, days, SERIAL_DB_VARIABLES[tair_var], format=format)
    r = _qalib.serial_complete(tair, model, flag, run_threshold=USE_ALL_INFILL_THRESHOLD, fill=float(ncio.FILL_F4),
                               group_first=gf, group_ndays=gn, max_miss=max_miss, device=device, timing=timing)
    out = ncio.open_dataset(fpath_out_serial_db, "a")
    try:
        if deflate is None:
            out.variables[tair_var][:] = np.ascontiguousarray(r["serial"].T)
            out.variables["flag_infilled"][:] = np.ascontiguousarray(r["flag_infilled"].T)
        else:
            kw = dict(deflate=deflate, device=device, timing=timing)
            ncio.write_series_chunks(out.variables[tair_var], np.ascontiguousarray(r["serial"], np.float32), **kw)
            ncio.write_series_chunks(out.variables["flag_infilled"], np.ascontiguousarray(r["flag_infilled"], np.int8), **kw)
    finally:
        out.close()
    for x in np.nonzero(r["nmissing"] > 0)[0]:
        print("Warning: Station %s has missing values even after infill. Ensure station is flagged as bad." % stns[STN_ID][x])
    print("% of stns with all infilled values: " + str((np.sum(r["all_infill"]) / float(r["all_infill"].size)) * 100.))
    return SerialComplete(np.array(stns[STN_ID]), r)


def add_monthly_normals(stnda, start_norm_yr=1981, end_norm_yr=2010, device=0, max_miss=_qalib.SC_MAX_MISS, timing=None):
    """``add_monthly_normals`` (post_infill.py:354-402): ``norm01 .. norm12`` of a ``StationSerialDataDb``, f8 with the f8
    fill value, from the monthly means with at most ``max_miss`` missing days (``TairAggregate.daily_to_mthly_norms``), in
    ONE ``twxsc_serial_complete`` call in its normals-only form.  Raises ``ValueError`` for a day axis that is not ascending
    and gap-free.  Returns (norm [nstn, 12], norm_nmths [nstn, 12])."""
    if stnda.var is None:
        raise ValueError("database holds no observations")
    gf, gn = _qalib.norm_groups(stnda.days[YEAR], stnda.days[MONTH], start_norm_yr, end_norm_yr, day=stnda.days[DAY])
    norm_vars = {}
    for mth in range(1, 13):
        norm_vars[mth] = stnda.add_stn_variable(get_norm_varname(mth), "%d - %d Monthly Normal" % (start_norm_yr, end_norm_yr),
                                                units="C", dtype="f8", fill_value=ncio.FILL_F8)
    if stnda.stns.size == 0:
        return np.zeros((0, 12)), np.zeros((0, 12), np.int32)
    # a NaN (what a masked entry reads back as) and the fill value are both missing
    r = _qalib.serial_complete(np.ascontiguousarray(np.asarray(stnda.var, np.float32).T), fill=float(ncio.FILL_F4),
                               group_first=gf, group_ndays=gn, max_miss=max_miss, device=device, timing=timing)
    for mth in range(1, 13):
        norm_vars[mth][:] = r["norm"][:, mth - 1]
    if stnda.ds is not None and getattr(stnda.ds, "mode", "r") != "r":
        stnda.ds.sync()
    return r["norm"], r["norm_nmths"]


def add_stn_raster_values(stnda, var_name, long_name, units, a_rast, extract_method=1, revert_nn=False, force_data_value=False,
                          device=0, timing=None, report=None):
    """``add_stn_raster_values`` (post_infill.py:248-352): the raster's value at every station as the ``f8`` station
    variable ``var_name`` with ``fill_value=a_rast.ndata``.  ``a_rast`` is a ``topowx_amd.raster.RasterGrid`` in the
    stations' own geographic coordinates.  ``extract_method`` 0 (nearest) or 1 (bilinear); ``revert_nn`` and
    ``force_data_value`` as in the reference, whose ring search (``_find_nn_data``) runs for all forced stations in one
    ``twxrv_nearest_data`` call.  Returns the ids of the stations left at ``a_rast.ndata``; with ``force_data_value`` such a
    station raises the reference's exception (also where the reference would search for ever: no data cell in any ring).
    ``report`` (a dict) receives the counts of bilinear / nearest / forced / no-data stations and ``redecided``, the
    forced stations whose ring was decided again on the host because winner and runner-up lay within a relative 1e-9."""
    if a_rast.ndata is None:
        raise ValueError("the raster has no no-data value (a_rast.ndata): there is nothing to write for 'no value'")
    lon, lat = np.asarray(stnda.stns[LON], np.float64), np.asarray(stnda.stns[LAT], np.float64)
    newvar = stnda.add_stn_variable(var_name, long_name, units, "f8", fill_value=a_rast.ndata)
    counts = dict(stations=int(lon.size), bilinear=0, nearest=0, forced=0, nodata=0, redecided=0)
    if lon.size:
        r = _qalib.raster_sample(a_rast.data, a_rast.geo_t, a_rast.ndata, lon, lat, band_ndata=a_rast.band_ndata,
                                 extract_method=extract_method, revert_nn=revert_nn, force_data_value=force_data_value,
                                 device=device, timing=timing)
        rvals, status = r["value"], r["status"]
        forced = np.nonzero(status == _qalib.RV_NEEDS_FORCE)[0]
        if forced.size:
            nn = _qalib.raster_nearest_data(a_rast.data, a_rast.geo_t, a_rast.ndata, r["row"][forced], r["col"][forced],
                                            device=device, timing=timing)
            rvals[forced] = nn["value"]                          # ndata where no ring holds a data cell
            counts["redecided"] = nn["redecided"]
        by_method = int((status == _qalib.RV_OK).sum())
        counts.update(bilinear=by_method if extract_method == 1 else 0,
                      nearest=int((status == _qalib.RV_NEAREST).sum()) + (by_method if extract_method == 0 else 0),
                      forced=int(forced.size), nodata=int((status == _qalib.RV_NODATA).sum()))
        newvar[:] = rvals
        if stnda.ds is not None and getattr(stnda.ds, "mode", "r") != "r":
            stnda.ds.sync()
        stnids_ndata = stnda.stn_ids[rvals == a_rast.ndata]
    else:
        stnids_ndata = stnda.stn_ids[:0]
    if report is not None:
        report.update(counts)
    if force_data_value and stnids_ndata.size > 0:
        raise Exception("force_data_value turned on, but station points still had no data values.")
    return stnids_ndata


def find_dup_stns(stnda, device=0, workspace_bytes=0, timing=None):
    """``find_dup_stns`` (post_infill.py:193-246) of an INFILLED database (its ``flag_infilled`` [ndays, nstn] is read
    through ``stnda.ds``): of the stations at one location -- ``grt_circle_dist`` == 0, decided by ``twxrv_dup_classes`` --
    those whose count of infilled days (``twxrv_col_count`` on the file's layout) is not the smallest are returned; stations
    tied at the minimum are ALL kept, as in the reference.  Classes come in the order of their first member, members sorted
    by id.  The reference pairs id-sorted ids with sums in database order, which is right only for a table sorted by id:
    an unsorted table is refused."""
    ids = np.asarray(stnda.stn_ids)
    if ids.size > 1 and not np.all(ids[1:] > ids[:-1]):
        raise ValueError("station table must be sorted by station_id and unique")
    if ids.size < 2:
        return np.array([], dtype=ids.dtype)
    cls, size = _qalib.dup_classes(stnda.stns[LON], stnda.stns[LAT], device=device, timing=timing)
    firsts = np.nonzero((cls == np.arange(cls.size)) & (size > 1))[0]
    if firsts.size == 0:
        return np.array([], dtype=ids.dtype)
    members = [np.nonzero(cls == f)[0] for f in firsts]          # ascending index = ascending id
    if stnda.ds is None or "flag_infilled" not in stnda.ds.variables:
        raise KeyError("find_dup_stns needs the infilled database's flag_infilled variable (open the database from its file)")
    fvar = stnda.ds.variables["flag_infilled"]
    fill = fvar.getncattr("_FillValue") if "_FillValue" in fvar.ncattrs() else FILL_I1
    flag = np.asarray(np.ma.filled(fvar[:], fill)).astype(np.int8)   # a masked day adds nothing to numpy's sum: the kernel skips it
    sums = _qalib.col_count(flag, np.concatenate(members), fill=int(fill), workspace_bytes=workspace_bytes, device=device,
                            timing=timing)
    rm, at = [], 0
    for m in members:
        s = sums[at:at + m.size]
        at += m.size
        rm.extend(ids[m][s != s.min()])
    return np.array(rm, dtype=ids.dtype)
