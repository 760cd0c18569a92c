#!/usr/bin/env python3
"""Timing of the RAWS ingest (step04's daily-listing parse) on a GENERATED corpus; not a test.

    python tests/tools/gpu_raws_timing.py [--gb 1.0] [--distinct 48] [--repeats 5] [--out profiles/raws_ingest_timing.json]

The corpus is generated, because no real RAWS listing is at hand: ``--distinct`` station files in the listing's layout (7
heading lines, a line a day 1996-2015 of 17 tokens in plain decimals, a ``Copyright`` line), each copied under new names
until the directory holds at least ``--gb`` GB; its size is stated in the output.  After one warm-up pass, medians of
``--repeats`` passes of: reading the files into the page-locked buffer (page cache warm: a memory copy rate, not a disk
rate), the device call (upload, kernels, download of the result), each kernel group (HIP events) and the host settlement.
Measured once in the same run: the upload alone (a copy of a batch's bytes from page-locked memory), the download alone (a
copy of a batch's result to the host), a device-to-device copy rate to set the kernels against, and the writing of one
batch's rows as NetCDF-4 chunks, scaled to the corpus.  The per-file Python restatement runs on a subset and is scaled; the
executed reference's rate is the figure ``tests/golden/make_golden_raws.py`` stores in the golden fixture, measured where
the reference exists (this tool never reads the reference).
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
START, END = 19960101, 20151231


def station_text(seed):
    """A station's listing: 1996-2015, a line a day, plain decimals only."""
    r = np.random.RandomState(seed)
    d0 = dt.date(1996, 1, 1)
    n = (dt.date(2015, 12, 31) - d0).days + 1
    days = [d0 + dt.timedelta(k) for k in range(n)]
    t = 12.0 + 14.0 * np.sin(np.arange(n) / 58.1) + r.randn(n) * 3
    cols = [np.array([d.strftime("%m/%d/%Y") for d in days]), np.array(["%d" % d.year for d in days]),
            np.array(["%d" % d.timetuple().tm_yday for d in days]), np.char.mod("%d", np.arange(1, n + 1)),
            np.char.mod("%.1f", r.rand(n) * 700), np.char.mod("%.2f", r.rand(n) * 9), np.char.mod("%d", r.randint(0, 360, n)),
            np.char.mod("%.1f", r.rand(n) * 25), np.char.mod("%.1f", t), np.char.mod("%.1f", t + 5 + r.rand(n) * 5),
            np.char.mod("%.1f", t - 5 - r.rand(n) * 5), np.char.mod("%d", r.randint(5, 100, n)), np.char.mod("%d", r.randint(50, 101, n)),
            np.char.mod("%d", r.randint(1, 50, n)), np.char.mod("%.1f", np.where(r.rand(n) < 0.7, 0.0, r.gamma(1.0, 40.0, n))),
            np.char.mod("%.2f", r.rand(n) * 30), np.char.mod("%d", r.randint(0, 100, n))]
    line = cols[0]
    for c in cols[1:]:
        line = np.char.add(np.char.add(line, "    "), np.char.rjust(c, 8))
    head = " Generated Site Nevada\n\n: Daily Summary\n: generated corpus\n: Date Year Day Run ...\n:----\n: mm/dd/yyyy\n"
    return (head + "\n".join(line) + "\nCopyright: generated\n").encode()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--distinct", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-stations", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raws_ingest_timing.json"))
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import restate_raws as RR
    from topowx_amd import _qalib, ghcn, raws
    from topowx_amd.dates import get_days_metadata
    from concurrent.futures import ThreadPoolExecutor

    if not torch.cuda.is_available():
        raise SystemExit("gpu_raws_timing: no GPU; a time measured without one says nothing")
    gold = os.path.join(ROOT, "tests", "golden", "golden_raws_v1.npz")
    ref_rate = float(np.load(gold)["reference_mb_per_s"])
    tmp = tempfile.mkdtemp(prefix="raws_timing_")
    try:
        texts = [station_text(k) for k in range(a.distinct)]
        paths, total, k = [], 0, 0
        while total < a.gb * 1e9:
            p = os.path.join(tmp, "G%05d.txt" % k)
            with open(p, "wb") as fh:
                fh.write(texts[k % a.distinct])
            paths.append(p)
            total += len(texts[k % a.distinct])
            k += 1
        nstn = len(paths)
        min_ymd, max_ymd, d0, ndays = ghcn._period(START, END)
        sizes = [os.path.getsize(p) for p in paths]
        runs = ghcn._batches(sizes, ghcn.BATCH_BYTES, max(1, ghcn.MAX_BATCH_CELLS // (3 * ndays)))
        buf = _qalib.PinnedBuffer(max(sum(sizes[i:j]) for i, j in runs))
        rec, counts_all = [], None
        with ThreadPoolExecutor(max_workers=ghcn.MAX_READERS) as pool:
            for rep in range(a.repeats + 1):
                t = dict(read_ms=0.0, call_ms=0.0, settle_ms=0.0, kernels_ms=0.0)
                tm, counts_all = {}, np.zeros(len(raws.RW_COUNTS), np.int64)
                for i0, i1 in runs:
                    off = np.zeros(i1 - i0 + 1, np.int64)
                    off[1:] = np.cumsum(sizes[i0:i1])
                    t0 = time.perf_counter()
                    list(pool.map(lambda j: ghcn._read_into(paths[i0 + j], buf.view[off[j]:off[j + 1]]), range(i1 - i0)))
                    t1 = time.perf_counter()
                    val, win, unc, rse, counts = raws.raws_parse(buf.view, off, min_ymd, max_ymd, ndays, timing=tm)
                    t2 = time.perf_counter()
                    raws._settle(buf.view, off, paths[i0:i1], val, win, unc, rse, min_ymd, max_ymd, d0)
                    t3 = time.perf_counter()
                    assert counts[5] == 0 and counts[6] == 0           # plain decimals: everything is the device's
                    counts_all += counts
                    t["read_ms"] += (t1 - t0) * 1e3
                    t["call_ms"] += (t2 - t1) * 1e3
                    t["settle_ms"] += (t3 - t2) * 1e3
                for name in raws.RW_KERNELS:
                    t[name + "_kernel_ms"] = tm[name + "_kernel_ms"]
                    t["kernels_ms"] += tm[name + "_kernel_ms"]
                if rep:
                    rec.append(t)
        med = {k_: round(float(np.median([r[k_] for r in rec])), 3) for k_ in rec[0]}
        # the upload and the download alone, and the device's copy rate, this run
        nb = sum(sizes[runs[0][0]:runs[0][1]])
        host = torch.frombuffer(buf.view, dtype=torch.uint8, count=nb)
        dev = torch.empty(nb, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(dev)
        res = torch.empty(val.size, dtype=torch.float32, device="cuda")
        back = torch.empty(val.size, dtype=torch.float32)
        up, cp, down = [], [], []
        for _ in range(6):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            dev.copy_(host, non_blocking=True)
            e[1].record()
            dst.copy_(dev)
            e[2].record()
            back.copy_(res)
            e[3].record()
            e[3].synchronize()
            up.append(nb / (e[0].elapsed_time(e[1]) * 1e-3))
            cp.append(2 * nb / (e[1].elapsed_time(e[2]) * 1e-3))
            down.append(val.nbytes / (e[2].elapsed_time(e[3]) * 1e-3))
        upload_rate, copy_rate, down_rate = (float(np.median(x[1:])) for x in (up, cp, down))
        del host, dev, dst, res, back
        buf.close()
        # the write: the last batch's rows, as chunks of a NetCDF-4 file
        stns = np.zeros(val.shape[1], ghcn.STN_DTYPE)
        stns["station_id"] = ["RAWS_G%05d" % j for j in range(val.shape[1])]
        days = get_days_metadata(d0, d0 + dt.timedelta(ndays - 1))
        t0 = time.perf_counter()
        ghcn.write_all_stations_db(os.path.join(tmp, "all.nc"), stns, days, [(0, val.shape[1], val, np.zeros(val.shape, np.uint8))])
        write_ms_batch = (time.perf_counter() - t0) * 1e3
        # the restatement on a subset, scaled by bytes
        t0 = time.perf_counter()
        hb = 0
        for j in range(a.host_stations):                             # rows of the last batch: the same bytes, too
            text = texts[(runs[-1][0] + j) % a.distinct]
            r = RR.parse_raws(text, START, END)
            assert r["val"].tobytes() == val[:, j].tobytes()
            hb += len(text)
        restate_s = time.perf_counter() - t0
        parse = med["rw_body_kernel_ms"] + med["rw_claim_kernel_ms"] + med["rw_write_kernel_ms"]
        stages = {"read": med["read_ms"], "upload": total / upload_rate * 1e3, "kernels": med["kernels_ms"],
                  "download": 12.0 * nstn * ndays / down_rate * 1e3, "settle": med["settle_ms"],
                  "write": write_ms_batch * nstn / val.shape[1]}
        out = {"tool": "gpu_raws_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
               "corpus": "generated in the daily listing's layout, plain decimals only; no real RAWS listing was at hand",
               "corpus_bytes": int(total), "corpus_files": nstn, "corpus_distinct_files": a.distinct, "period": [START, END],
               "days": ndays, "batches": len(runs), "batch_bytes": ghcn.BATCH_BYTES,
               "counts": {n: int(c) for n, c in zip(raws.RW_COUNTS, counts_all)}, "repeats": a.repeats,
               "note": "one run on one machine; medians of the repeats after one warm-up pass; files read from a warm page "
                       "cache; upload, download and the device copy rate are measured on one batch and scaled by bytes; the "
                       "write is one batch's rows measured once and scaled; call_ms holds allocation, upload, kernels and "
                       "download of a call",
               "median_ms": med, "stage_ms": {k_: round(v, 1) for k_, v in stages.items()},
               "limiting_stage": max(stages, key=stages.get),
               "parse_kernels_bytes_per_s": round(3 * total / (parse * 1e-3), 0),
               "parse_kernels_note": "body + claim + write groups: each reads the text once",
               "copy_rate_measured_bytes_per_s": round(copy_rate, 0),
               "parse_kernels_share_of_measured_copy_rate": round(3 * total / (parse * 1e-3) / copy_rate, 4),
               "upload_rate_measured_bytes_per_s": round(upload_rate, 0),
               "download_rate_measured_bytes_per_s": round(down_rate, 0),
               "corpus_mb_per_s_whole": round(total / 1e6 / (sum(stages.values()) * 1e-3), 1),
               "write_ms_batch": round(write_ms_batch, 1),
               "restatement_mb_per_s": round(hb / 1e6 / restate_s, 2), "restatement_stations": a.host_stations,
               "restatement_corpus_s_scaled": round(total / (hb / restate_s), 1),
               "reference_mb_per_s_one_core": round(ref_rate, 2),
               "reference_corpus_s_scaled": round(total / 1e6 / ref_rate, 1)}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
