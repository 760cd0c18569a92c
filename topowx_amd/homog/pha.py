"""step11: the boundary with the external Pairwise Homogenization Algorithm (PHA v52i; Menne and Williams 2009) and what
follows it (twx/homog/pha.py).  Before PHA: its input tree -- the station list, one GHCN-format file of monthly means per
station, the metadata file -- in plain Python text I/O.  After PHA: its adjustment log and its homogenised monthly files
are parsed and every station's daily series is homogenised in ONE ``twxhm_homog_daily`` call (``HomogDaily``), where the
reference loops over the year-months of a station at a time; ``create_homog_db`` is ``InsertHomog``.

Unpacking and building PHA's tar (``setup_pha``'s first half) and running it (``run_pha``) are not ported.
"""
import csv
import os

import numpy as np

from .. import _qalib, ncio
from .. import stationdb as sdb
from ..obs_por import month_axis, read_rows
from .tobs import write_tair_db

__all__ = ["format_stnid", "write_stn_list", "write_stn_obs_files", "write_metadata_file", "write_input_station_data",
           "parse_pha_adj", "read_pha_monthly", "load_input_not_stnlist", "get_pha_adj_csv", "HomogDaily", "create_homog_db",
           "pha_paths", "DTYPE_PHA_ADJ"]

DTYPE_PHA_ADJ = [(sdb.STN_ID, "U50"), ("ymd_start", np.int32), ("ymd_end", np.int32), ("adj", np.float64)]


def pha_paths(path_pha_run, varname):
    """The files of a PHA run directory this package writes and reads."""
    world = os.path.join(path_pha_run, "data", "benchmark", "world1")
    return dict(stnlist=os.path.join(world, "meta", "world1_stnlist.%s" % varname),
                metadata=os.path.join(world, "meta", "world1_metadata_file.txt"),
                raw=os.path.join(world, "monthly", "raw"), fls=os.path.join(world, "monthly", "FLs.r00"),
                adj_log=os.path.join(world, "output", "pha_adj_%s.log" % varname), corr=os.path.join(world, "corr"))


def format_stnid(stnid):
    """The 11-character id PHA takes: GHCN-D ids as they are, SNOTEL and RAWS ids padded behind ``SNT`` / ``WRC``."""
    stnid = str(stnid)
    if stnid.startswith("GHCND_"):
        outid = stnid.split("_")[1]
    elif stnid.startswith("NRCS_"):
        outid = stnid.split("_")[1]
        if ":" in outid:                                             # a triplet id
            outid = outid.replace(":", "")[0:8]
        outid = "SNT" + "{0:0>8}".format(outid)
    elif stnid.startswith("RAWS_"):
        outid = "WRC" + "{0:0>8}".format(stnid.split("_")[1])
    elif stnid.startswith("USH"):
        outid = stnid
    else:
        raise ValueError("Do not recognize stn id prefix for stnid: " + stnid)
    if len(outid) != 11:
        raise ValueError("Formatted station id for PHA was not 11 characters: %s" % outid)
    return outid


def write_stn_list(stns, fpath_out):
    """The GHCN-format station list: id, latitude to 5 decimals, longitude to 5 (4 from -100 on)."""
    with open(fpath_out, "w") as fout:
        for stn in stns:
            lat, lon = float(stn[sdb.LAT]), float(stn[sdb.LON])
            if lat < 0 or lon >= 0:
                raise ValueError("Only handles formating of positive Lats and negative Lons.")
            fmt_lon = "{0:0<9.5F}" if abs(lon) < 100 else "{0:0<9.4F}"
            fout.write(" ".join([format_stnid(stn[sdb.STN_ID]), "{0:0<8.5F}".format(lat), fmt_lon.format(lon), "\n"]))


def write_stn_obs_files(stns, data, yrs, varname, path_out):
    """One ``<id>.raw.<var>`` per station: a line per year of twelve monthly means in hundredths (the float32 product, as
    the reference scales the database's values), -9999 where ``data`` [nmth, nstn] is masked or NaN."""
    data = np.ma.masked_invalid(np.ma.asarray(data, np.float32))
    vals = np.where(np.ma.getmaskarray(data), np.float32(-9999), np.ma.getdata(data) * np.float32(100.0))
    for x, stn in enumerate(stns):
        out_id = format_stnid(stn[sdb.STN_ID])
        with open(os.path.join(path_out, "".join([out_id, ".raw.", varname])), "w") as fout:
            for k, yr in enumerate(yrs):
                fout.write(" ".join([out_id, str(int(yr))]) +
                           "".join(" {0:>5.0f}".format(v) + "   " for v in vals[12 * k:12 * k + 12, x]) + "\n")


def write_metadata_file(fpath, stnhist=()):
    """PHA's station-history file: a line per (station id, ``yyyymm`` of a documented change); empty without history."""
    with open(fpath, "w") as f:
        for stn_id, yyyymm in stnhist:
            f.write("  %s %s 1\n" % (format_stnid(stn_id), str(yyyymm)))


def write_input_station_data(path_pha_run, varname, stns, tair, yrs, stnhist=()):
    """``_write_input_station_data``: the station list, the metadata file and the monthly files under ``path_pha_run``
    (the directories are made if PHA's tar has not made them; its ``tavg`` example files are removed)."""
    p = pha_paths(path_pha_run, varname)
    for d in (os.path.dirname(p["stnlist"]), p["raw"]):
        os.makedirs(d, exist_ok=True)
    write_stn_list(stns, p["stnlist"])
    tavg = os.path.join(os.path.dirname(p["stnlist"]), "world1_stnlist.tavg")
    for f in [tavg] + [os.path.join(p["raw"], n) for n in os.listdir(p["raw"]) if n.endswith(".tavg")]:
        if os.path.exists(f):
            os.remove(f)
    write_metadata_file(p["metadata"], stnhist)
    write_stn_obs_files(stns, tair, yrs, varname, p["raw"])


def parse_pha_adj(path_adj_log):
    """``_parse_pha_adj``: the ``Adj write`` lines of PHA's log by their fixed columns -- id 10-20, ``yyyymm`` of the
    first and last month 25-30 and 45-50, the adjustment 75-80 -- as a structured array of ``DTYPE_PHA_ADJ``."""
    vals = []
    with open(path_adj_log) as f:
        for aline in f:
            if not aline.strip():
                continue
            start, end = aline[25:31], aline[45:51]
            vals.append((aline[10:21], int(start[0:4]) * 10000 + int(start[-2:]) * 100 + 1,
                         int(end[0:4]) * 10000 + int(end[-2:]) * 100 + 1, float(aline[75:81])))
    return np.array(vals, dtype=DTYPE_PHA_ADJ)


def read_pha_monthly(path_fls, fmt_ids, varname, yrs):
    """PHA's homogenised monthly values ``FLs.r00/<id>.FLs.r00.<var>`` as int32 hundredths [nstn, 12 * nyears], -9999 =
    missing: the year in columns 12-16, the values 5 wide every 9 columns from column 17 (pha.py:225-236)."""
    yrs = [int(y) for y in yrs]
    col = dict((y, k) for k, y in enumerate(yrs))
    out = np.full((len(fmt_ids), 12 * len(yrs)), _qalib.HM_PHA_MISSING, np.int32)
    for s, fid in enumerate(fmt_ids):
        with open(os.path.join(path_fls, "%s.FLs.r00.%s" % (fid, varname))) as f:
            for aline in f:
                if not aline.strip():
                    continue
                yr = int(aline[12:17])
                if yr not in col:
                    raise ValueError("%s: year %d is not on the database's axis" % (f.name, yr))
                out[s, 12 * col[yr]:12 * col[yr] + 12] = [int(float(aline[17 + 9 * m:22 + 9 * m])) for m in range(12)]
    return out


def load_input_not_stnlist(path_pha_run):
    """The formatted ids PHA could not homogenise: the first column of every ``corr/*input_not_stnlist``, sorted."""
    corr = pha_paths(path_pha_run, "")["corr"]
    ids = []
    if os.path.isdir(corr):
        for name in sorted(os.listdir(corr)):
            if name.endswith("input_not_stnlist"):
                with open(os.path.join(corr, name)) as f:
                    ids.extend(line.split()[0] for line in f if line.strip())
    return np.sort(np.array(ids, "U11"))


def get_pha_adj_csv(fpath_pha_adj_log, stns, elem, fpath_out):
    """step28's table of the non-zero adjustments (``get_pha_adj_df``): sign flipped, the months moved on by one as the
    reference does, with the station's name and place.  Returns the rows written."""
    meta = dict((format_stnid(s[sdb.STN_ID]), s) for s in stns)
    rows = []
    for a in parse_pha_adj(fpath_pha_adj_log):
        if a[sdb.STN_ID] not in meta or not abs(a["adj"]) > 0:
            continue
        s = meta[a[sdb.STN_ID]]
        nxt = []
        for v in (int(a["ymd_start"]), int(a["ymd_end"])):           # the month after, as the reference's relativedelta
            q, r = divmod((v // 10000) * 12 + v // 100 % 100, 12)
            nxt.append("%d%02d" % (q, r + 1))
        name = s["station_name"] if "station_name" in s.dtype.names else ""
        rows.append([s[sdb.STN_ID], nxt[0], nxt[1], repr(float(-a["adj"])), elem, name, repr(float(s[sdb.LON])),
                     repr(float(s[sdb.LAT])), int(np.round(s[sdb.ELEV]))])
    with open(fpath_out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["STN_ID", "YEAR_MONTH_START", "YEAR_MONTH_END", "ADJ(C)", "VARIABLE", "NAME", "LON", "LAT", "ELEV(m)"])
        w.writerows(rows)
    return rows


class _Pool(object):
    """What ``HomogDaily`` reads of the database PHA's input came from."""

    def __init__(self, ids, days, rows, mth_mean, mth_miss):
        self.ids, self.days, self.rows, self.mth_mean, self.mth_miss = np.asarray(ids).astype(str), days, rows, mth_mean, mth_miss

    @classmethod
    def from_netcdf(cls, path, varname):
        with ncio.open_dataset(path, "r") as ds:
            for name in (varname, varname + "_mth", varname + "_mthmiss"):
                if name not in ds.variables:
                    raise KeyError("%s has no variable %s (python -m topowx_amd.step10 writes the monthly means)" % (path, name))
            days = ncio.days_of(ds)
            ids = ncio._read_ids(ds.variables[sdb.STN_ID])
            rows = read_rows(ds, varname, qflags=True)
            mean = read_rows(ds, varname + "_mth")
            miss = np.ascontiguousarray(np.asarray(np.ma.filled(ds.variables[varname + "_mthmiss"][:], -32767), np.int16).T)
        return cls(ids, days, rows, mean, miss)


class HomogDaily(object):
    """``HomogDaily(stnda, path_pha_run, varname)``: the homogenised daily series of every station of the database that
    was PHA's input.  ``pool_or_path`` is that database's path, or an object with ``ids``, ``days``, ``rows`` [nstn, ndays],
    ``mth_mean`` and ``mth_miss`` [nstn, nmth].  ``homog_all`` runs all stations in one ``twxhm_homog_daily`` call and
    raises ``ValueError`` naming the first station whose adjustment list is missing or overlaps; ``homog_stn(stn_id)`` is
    the reference's call, one row of that batch."""

    def __init__(self, pool_or_path, path_pha_run, varname, device=0):
        pool = pool_or_path if hasattr(pool_or_path, "rows") else _Pool.from_netcdf(pool_or_path, varname)
        self.pool, self.varname, self.device = pool, varname, device
        self.paths = pha_paths(path_pha_run, varname)
        self.fmt_ids = np.array([format_stnid(s) for s in pool.ids])
        self.idxs = dict((s, i) for i, s in enumerate(pool.ids))
        self.pha_adjs = parse_pha_adj(self.paths["adj_log"])
        self.mth_first, self.mth_ndays, self.mth_ymd = month_axis(pool.days)
        self.result = None

    def adj_csr(self, rows=None):
        """The adjustment table as CSR over the stations ``rows`` (default: all), each list sorted by its first month."""
        rows = np.arange(self.fmt_ids.size) if rows is None else np.asarray(rows)
        order = np.argsort(self.pha_adjs["ymd_start"], kind="stable")
        adjs = self.pha_adjs[order]
        by_id = {}
        for k, fid in enumerate(adjs[sdb.STN_ID]):
            by_id.setdefault(fid, []).append(k)
        off, take = [0], []
        for fid in self.fmt_ids[rows]:
            take.extend(by_id.get(fid, ()))
            off.append(len(take))
        take = np.array(take, np.int64)
        return np.array(off, np.int64), adjs["ymd_start"][take], adjs["ymd_end"][take], adjs["adj"][take]

    def homog_all(self, stn_ids=None, timing=None):
        """Homogenise the stations ``stn_ids`` (default: all).  Returns a dict of ``ids``, ``out`` [n, ndays] float32 (NaN =
        none), ``delta`` [n, nmth], ``nchanged``."""
        p = self.pool
        rows = np.arange(p.ids.size) if stn_ids is None else np.array([self.idxs[str(s)] for s in stn_ids], np.int64)
        if rows.size == 0:
            return dict(ids=p.ids[rows], out=np.zeros((0, p.rows.shape[1]), np.float32),
                        delta=np.zeros((0, self.mth_first.size)), nchanged=np.zeros(0, np.int32))
        yrs = np.unique(np.asarray(self.mth_ymd) // 10000)
        pha = read_pha_monthly(self.paths["fls"], self.fmt_ids[rows], self.varname, yrs)
        off, st, en, ad = self.adj_csr(rows)
        r = _qalib.homog_daily(p.rows[rows], p.mth_mean[rows], p.mth_miss[rows], pha, self.mth_ymd, self.mth_first,
                               self.mth_ndays, off, st, en, ad, device=self.device, timing=timing)
        bad = np.nonzero(r["status"] != _qalib.HM_OK)[0]
        if bad.size:
            why = {_qalib.HM_NO_ADJ: "needs PHA's adjustment list and has none",
                   _qalib.HM_OVERLAP: "has a month that falls within more than one change point"}
            raise ValueError("station %s (%s) %s; %d station(s) in all" % (
                p.ids[rows[bad[0]]], self.fmt_ids[rows[bad[0]]], why[int(r["status"][bad[0]])], bad.size))
        return dict(ids=p.ids[rows], out=r["out"], delta=r["delta"], nchanged=r["nchanged"])

    def homog_stn(self, stn_id):
        if self.result is None:
            self.result = self.homog_all()
        return self.result["out"][self.idxs[str(stn_id)]]


def create_homog_db(path_in, path_out, path_pha_run_tmin, path_pha_run_tmax, format=None, device=0, timing=None):
    """``InsertHomog``: the homogenised database.  Per variable the stations PHA lists in ``corr/*input_not_stnlist`` are
    left out (their days are ``MISSING``); the database holds the stations that remain for Tmin or for Tmax, in the
    input's order, with empty quality flags.  Returns a dict of ``ids`` and per variable ``nchanged`` and ``used``."""
    stns, _, days, _ = ncio.read_station_db_arrays(path_in, "")
    fmt = np.array([format_stnid(s) for s in stns[sdb.STN_ID]])
    used, homog = {}, {}
    for var, run in (("tmin", path_pha_run_tmin), ("tmax", path_pha_run_tmax)):
        used[var] = ~np.isin(fmt, load_input_not_stnlist(run))
        homog[var] = HomogDaily(path_in, run, var, device=device).homog_all(stns[sdb.STN_ID][used[var]], timing=timing)
    keep = np.nonzero(used["tmin"] | used["tmax"])[0]
    out = {}
    for var in ("tmin", "tmax"):
        a = np.full((stns.size, days.size), np.nan, np.float32)
        a[used[var]] = homog[var]["out"]
        out[var] = a[keep]
    write_tair_db(path_out, stns[keep], days, out["tmin"], out["tmax"], format=format)
    return dict(ids=stns[sdb.STN_ID][keep], used=used, nchanged=dict((v, homog[v]["nchanged"]) for v in homog))
