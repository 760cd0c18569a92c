#!/usr/bin/env python3
"""Timing of the GHCN-Daily ingest (step04's .dly parse) on a generated corpus; not a test.

    python tests/tools/gpu_ghcn_timing.py [--gb 1.0] [--distinct 96] [--repeats 5] [--out profiles/ghcn_ingest_timing.json]

The corpus: ``--distinct`` station files of canonical text (1900-2016, four elements, made with numpy), each copied under
new names until the directory holds at least ``--gb`` GB; its size is stated in the output.  After one warm-up pass, medians
of ``--repeats`` passes of: reading the files into the page-locked buffer (page cache warm: a memory copy rate, not a disk
rate), the device call (upload, kernels, download of the result), the kernels alone (HIP events), the upload alone (a copy
of the same bytes from page-locked memory, timed on its own), and writing the NetCDF-4 file.  The kernel rate is set
against a device-to-device copy rate measured in the same run.  The per-station Python restatement runs on a subset and
is scaled; the executed reference's rate is the figure ``tests/golden/make_golden_ghcn.py`` prints where the reference
exists, passed in with ``--reference-mb-per-s`` (this tool never reads the reference).
"""
import argparse
import datetime as dt
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def station_text(seed, stn):
    """A station's .dly text, 1900-2016 x 12 months x TMAX / TMIN / PRCP / SNOW, all fields canonical."""
    r = np.random.RandomState(seed)
    ym = [(y, m) for y in range(1900, 2017) for m in range(1, 13)]
    n = len(ym) * 4
    vals = r.randint(-400, 450, (n, 31))
    vals[r.rand(n, 31) < 0.05] = -9999
    body = np.char.add(np.char.mod("%5d", vals), "  0")                  # value, mflag, qflag, sflag
    head = np.array(["%s%04d%02d%s" % (stn, y, m, e) for (y, m) in ym for e in ("TMAX", "TMIN", "PRCP", "SNOW")])
    lines = np.char.add(head, np.array(["".join(row) for row in body]))
    return ("\n".join(lines) + "\n").encode()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--distinct", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-stations", type=int, default=2)
    ap.add_argument("--reference-mb-per-s", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ghcn_ingest_timing.json"))
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import restate_ghcn as RG
    from topowx_amd import _qalib, ghcn
    from topowx_amd.dates import get_days_metadata

    start, end = 19480101, 20161231
    tmp = tempfile.mkdtemp(prefix="ghcn_timing_")
    try:
        texts = [station_text(k, "USC%08d" % k) for k in range(a.distinct)]
        paths, total, k = [], 0, 0
        while total < a.gb * 1e9:
            p = os.path.join(tmp, "USC%08d.dly" % k)
            with open(p, "wb") as fh:
                fh.write(texts[k % a.distinct])
            paths.append(p)
            total += len(texts[k % a.distinct])
            k += 1
        nstn = len(paths)
        _, _, d0, ndays = ghcn._period(start, end)
        sizes = [os.path.getsize(p) for p in paths]
        runs = ghcn._batches(sizes, ghcn.BATCH_BYTES)
        buf = _qalib.PinnedBuffer(max(sum(sizes[i:j]) for i, j in runs))
        from concurrent.futures import ThreadPoolExecutor
        rec = []
        lines = values = 0
        with ThreadPoolExecutor(max_workers=ghcn.MAX_READERS) as pool:
            for rep in range(a.repeats + 1):
                t = dict(read_ms=0.0, call_ms=0.0, kernels_ms=0.0)
                tm = {}
                lines = values = 0
                for i0, i1 in runs:
                    off = np.zeros(i1 - i0 + 1, np.int64)
                    off[1:] = np.cumsum(sizes[i0:i1])
                    t0 = time.perf_counter()
                    list(pool.map(lambda j: ghcn._read_into(paths[i0 + j], buf.view[off[j]:off[j + 1]]), range(i1 - i0)))
                    t1 = time.perf_counter()
                    val, flag, bad, fb, counts = _qalib.ghcn_parse_dly(buf.view, off, np.arange(i1 - i0, dtype=np.int32), i1 - i0,
                                                                       start, end, ndays, timing=tm)
                    t2 = time.perf_counter()
                    assert counts[2] == 0 and (bad == _qalib.GH_NO_BAD_HEADER).all()
                    lines, values = lines + int(counts[0]), values + int(counts[1])
                    t["read_ms"] += (t1 - t0) * 1e3
                    t["call_ms"] += (t2 - t1) * 1e3
                for name in _qalib.GH_KERNELS:
                    t[name + "_kernel_ms"] = tm[name + "_kernel_ms"]
                    t["kernels_ms"] += tm[name + "_kernel_ms"]
                if rep:
                    rec.append(t)
        med = {k_: round(float(np.median([r[k_] for r in rec])), 3) for k_ in rec[0]}
        # the upload alone and the device's copy rate, this run
        nb = sum(sizes[runs[0][0]:runs[0][1]])
        host = torch.frombuffer(buf.view, dtype=torch.uint8, count=nb)
        dev = torch.empty(nb, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(dev)
        up, cp = [], []
        for _ in range(6):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            dev.copy_(host, non_blocking=True)
            e1.record()
            dst.copy_(dev)
            e2.record()
            e2.synchronize()
            up.append(nb / (e0.elapsed_time(e1) * 1e-3))
            cp.append(2 * nb / (e1.elapsed_time(e2) * 1e-3))
        upload_rate, copy_rate = float(np.median(up[1:])), float(np.median(cp[1:]))
        del host, dev, dst
        buf.close()
        # the write: the last batch's rows, as chunks of a NetCDF-4 file
        stns = np.zeros(val.shape[1], ghcn.STN_DTYPE)
        stns["station_id"] = ["GHCN_USC%08d" % j for j in range(val.shape[1])]
        days = get_days_metadata(d0, d0 + dt.timedelta(ndays - 1))
        t0 = time.perf_counter()
        ghcn.write_all_stations_db(os.path.join(tmp, "all.nc"), stns, days, [(0, val.shape[1], val, flag)])
        write_ms_batch = (time.perf_counter() - t0) * 1e3
        written = os.path.getsize(os.path.join(tmp, "all.nc"))
        # the restatement on a subset, scaled by bytes
        t0 = time.perf_counter()
        hb = 0
        for j in range(a.host_stations):                             # rows of the last batch: the same bytes, too
            text = texts[(runs[-1][0] + j) % a.distinct]
            r = RG.parse_dly(text, start, end)
            assert r["val"].tobytes() == val[:, j].tobytes() and r["flag"].tobytes() == flag[:, j].tobytes()
            hb += len(text)
        restate_s = time.perf_counter() - t0
        both = med["gh_claim_kernel_ms"] + med["gh_write_kernel_ms"]
        stages = {"read": med["read_ms"], "upload": total / upload_rate * 1e3, "kernels": med["kernels_ms"],
                  "write": write_ms_batch * nstn / val.shape[1]}
        out = {"tool": "gpu_ghcn_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
               "corpus_bytes": int(total), "corpus_files": nstn, "corpus_distinct_files": a.distinct, "period": [start, end],
               "days": ndays, "batches": len(runs), "batch_bytes": ghcn.BATCH_BYTES, "lines": lines, "values": values,
               "repeats": a.repeats,
               "note": "one run on one machine; medians of the repeats after one warm-up pass; files read from a warm page "
                       "cache; the write is one batch's rows measured once and scaled to the corpus; upload is the corpus "
                       "size over the measured page-locked copy rate",
               "median_ms": med, "stage_ms": {k_: round(v, 1) for k_, v in stages.items()},
               "limiting_stage": max(stages, key=stages.get),
               "parse_kernels_bytes_per_s": round(2 * total / (both * 1e-3), 0),
               "copy_rate_measured_bytes_per_s": round(copy_rate, 0),
               "parse_kernels_share_of_measured_copy_rate": round(2 * total / (both * 1e-3) / copy_rate, 4),
               "upload_rate_measured_bytes_per_s": round(upload_rate, 0),
               "corpus_mb_per_s_whole": round(total / 1e6 / (sum(stages.values()) * 1e-3), 1),
               "written_bytes_batch": int(written), "write_ms_batch": round(write_ms_batch, 1),
               "restatement_mb_per_s": round(hb / 1e6 / restate_s, 2), "restatement_stations": a.host_stations,
               "restatement_corpus_s_scaled": round(total / (hb / restate_s), 1),
               "reference_mb_per_s_one_core": a.reference_mb_per_s,
               "reference_corpus_s_scaled": round(total / 1e6 / a.reference_mb_per_s, 1) if a.reference_mb_per_s else None}
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
