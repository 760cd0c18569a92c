"""``scripts/step17_find_bad_infill_stns.py``: the stations whose infilled series are suspect get a variance change-point
test and a world-record test over their WHOLE series (``topowx_amd.infill.find_bad_infill_stns``: one
``twxsc_series_check`` call per variable, no cap of 8192 rows), and the bad ones are written as ``station_id,reason`` rows.

    python -m topowx_amd.step17 --infill-tmin A.nc --infill-tmax B.nc --out flagged_bad.csv
                                (--stnids ids.txt | --log infill.log | --db all.nc --report-tmin R.npz --report-tmax R.npz)
                                [--cpt-sig X] [--device N] [--deflate gpu|host]

The suspects come from a text file of ids (``--stnids``, one per line), from a log of the reference's step16 (``--log``:
its ``Could not infill`` and ``ERROR|`` lines, ``get_bad_infill_stnids``), or from two step16 reports (``--report-*``:
``suspect_infill_stnids``).  With ``--report-*`` the two infilled databases are first WRITTEN from the reports at the
``--infill-*`` paths (``write_infill_db`` over the station table of ``--db``; an existing file is not overwritten).

A station is bad if either variable has a change point at the level ``--cpt-sig`` (default 1e-10), a value above 57.7 or
below -89.4, or a value that is still missing.  An id that neither database has is an error; one that a single database
lacks is not bad for that variable.  The change-point test is the restated one (DESIGN.md sections 19 and 21), not R's
``changepoint`` executed.

Prints one JSON line (suspects, bad, per variable the stations checked, with a change point, an impossible or a missing
value, the penalty, seconds, kernel milliseconds).  Exits with 1 if a file cannot be opened or a station id is unknown.
"""
import argparse
import json
import sys
import time
import zipfile

import numpy as np

from . import _qalib, ncio
from .infill import find_bad_infill_stns, get_bad_infill_stnids, suspect_infill_stnids, write_bad_stns_csv, write_infill_db

__all__ = ["main"]


class _Unknown(Exception):
    pass


def _load_report(path):
    with np.load(path) as z:
        need = ("ids", "fnl_tair", "mask_infill", "infill_tair", "mae", "bias", "status")
        if not all(k in z.files for k in need):
            raise ValueError("%s is not a step16 report (no %s)" % (path, " / ".join(k for k in need if k not in z.files)))
        return {k: z[k] for k in z.files}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step17", description=__doc__.split("\n\n")[0])
    ap.add_argument("--infill-tmin", required=True, help="infilled Tmin database (netCDF); written first with --report-*")
    ap.add_argument("--infill-tmax", required=True, help="infilled Tmax database (netCDF); written first with --report-*")
    ap.add_argument("--out", required=True, help="csv of the bad stations to write")
    ap.add_argument("--stnids", help="text file of suspect station ids, one per line")
    ap.add_argument("--log", help="log of the reference's step16")
    ap.add_argument("--db", help="all-stations database (netCDF): the station table of the databases to write (with --report-*)")
    ap.add_argument("--report-tmin", help="step16 report of Tmin (.npz)")
    ap.add_argument("--report-tmax", help="step16 report of Tmax (.npz)")
    ap.add_argument("--cpt-sig", type=float, default=_qalib.CK_SIG, help="level of the variance change-point check")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--deflate", choices=("gpu", "host"),
                    help="with --report-*: write the databases' series station-major, their chunks deflated on the GPU (gpu) or by "
                         "libhdf5 (host); default: the transposed assignment")
    a = ap.parse_args(argv)
    reports = bool(a.report_tmin or a.report_tmax or a.db)
    if sum([bool(a.stnids), bool(a.log), reports]) != 1 or (reports and not (a.report_tmin and a.report_tmax and a.db)):
        ap.error("give exactly one of --stnids, --log, or --db with --report-tmin and --report-tmax")
    cur = a.stnids or a.log or a.db
    try:
        if a.stnids:
            with open(a.stnids) as fh:
                ids = [ln.strip() for ln in fh if ln.strip()]
        elif a.log:
            ids = [str(s) for s in get_bad_infill_stnids(a.log)]
        else:
            stns, _, days, _ = ncio.read_station_db_arrays(a.db, "tmin")
            ids = set()
            for var, rpath, opath in (("tmin", a.report_tmin, a.infill_tmin), ("tmax", a.report_tmax, a.infill_tmax)):
                cur = rpath
                rep = _load_report(rpath)
                if rep["fnl_tair"].shape[1:] != (days.size,):
                    raise ValueError("%s has %d days, %s has %d" % (rpath, rep["fnl_tair"].shape[1], a.db, days.size))
                ids.update(str(s) for s in suspect_infill_stnids(rep))
                cur = opath
                try:
                    write_infill_db(opath, stns, days, var, rep, deflate=a.deflate, device=a.device)
                except KeyError as e:
                    raise _Unknown(str(e.args[0]))
            ids = sorted(ids)
        known = set()
        for cur in (a.infill_tmin, a.infill_tmax):
            ds = ncio.open_dataset(cur, "r")
            try:
                known.update(str(s) for s in ncio._read_ids(ds.variables["station_id"]))
            finally:
                ds.close()
        missing = [s for s in ids if s not in known]
        if missing:
            raise _Unknown("%d suspect ids are in neither infilled database (first: %s)" % (len(missing), missing[0]))
        tm = {}
        t0 = time.perf_counter()
        cur = a.infill_tmin
        bad, det = find_bad_infill_stns(a.infill_tmin, a.infill_tmax, ids, sig=a.cpt_sig, device=a.device, timing=tm) \
            if ids else ([], {})
        sec = time.perf_counter() - t0
        cur = a.out
        write_bad_stns_csv(a.out, bad)
    except _Unknown as e:
        print("step17: %s" % e, file=sys.stderr)
        return 1
    except (IOError, OSError, ValueError, KeyError, zipfile.BadZipFile) as e:
        print("step17: cannot open %s: %s" % (getattr(e, "filename", None) or cur, e), file=sys.stderr)
        return 1
    line = {"suspects": len(ids), "bad": len(bad), "seconds": round(sec, 3)}
    for var, d in det.items():
        p = d["present"]
        line[var] = {"checked": int(p.sum()), "chgpt": int(((d["reasons"] & _qalib.CK_VAR_CHGPT) != 0).sum()),
                     "impossible": int((d["nimpossible"] > 0).sum()), "missing": int((d["nmissing"] > 0).sum()),
                     "pen": None if np.isnan(d["pen"]) else round(float(d["pen"]), 6)}
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
