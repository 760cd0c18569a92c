"""GPU: the measurements of the step26 / step27 mosaic route (profiles/mosaic_timing.json).

    python tests/tools/gpu_mosaic_timing.py [--out FILE] [--work DIR] [--rows 4] [--cols 6] [--days 365]

Corpus: one year of generated tile files (a smooth field in 1/100 degC plus noise, tests/mosaic_cases.py's recipe made cheaper)
for a rectangle of ``rows x cols`` tiles of 325 x 350 cells in chunks of 65 x 70, i.e. a mosaic of whole (1, 325, 700) chunks; one
variable; the page cache is warm (the files were just written).  GPU route: medians of five calls after a warm-up, per stage.
Host route: ONE call over the same files (libhdf5 deflates on one core).  Coder: int16 GB/s through hist .. compact against a
device-to-device copy of the same bytes.  Size: stream bytes / int16 bytes, and zlib level 1 / level 4 on a sample of the same
shuffled chunks.  Memory: the whole-year object at 3250 x 7000."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def corpus(fm, path_tiles, days, seed=1):
    from topowx_amd import ncio
    info = fm.tinfo
    ty, tx = info.tile_size_y, info.tile_size_x
    Y, X = len(info.lats), len(info.lons)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Y, 0:X]
    base = (1500.0 + 900.0 * np.sin(yy / 137.0) * np.cos(xx / 253.0) - 0.9 * yy + 0.4 * xx).astype(np.float32)
    noise = rng.normal(0.0, 20.0, (Y + 64, X + 64)).astype(np.float32)
    w = ncio.TileWriter(info, path_tiles, format="NETCDF4")
    z = np.zeros((12, ty, tx), np.float32)
    names = sorted(info.tile_rc)
    for name in names:
        r, c = info.tile_rc[name]
        slab = np.empty((days.size, ty, tx), np.int16)
        for d in range(days.size):
            o = (d * 7) % 64
            slab[d] = np.rint(base[r:r + ty, c:c + tx] + 800.0 * np.sin(d / 58.0) + noise[r + o:r + o + ty, c + o:c + o + tx])
        w.write_tile_chunk(name, "tmin", days, 0, 0, slab, z, z, np.zeros((ty, tx), np.int32))
    return names


def med(xs):
    return float(np.median(xs))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mosaic_timing.json"))
    ap.add_argument("--work")
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--cols", type=int, default=6)
    ap.add_argument("--days", type=int, default=365)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.init()                                       # (before the project's libraries open the device)
    import mosaic_cases as MC
    from topowx_amd import _qalib, h5nc
    from topowx_amd.interp import TileMosaic
    work = a.work or tempfile.mkdtemp(prefix="mosaic_timing_")
    os.makedirs(work, exist_ok=True)
    Y, X = a.rows * 325, a.cols * 350
    fm = TileMosaic(MC.write_mask(os.path.join(work, "mask.nc"), Y, X), 325, 350, 65, 70)
    days = MC.days_between((2001, 1, 1), (2001, 12, 31))[:a.days] if a.days < 365 else MC.days_between((2001, 1, 1), (2001, 12, 31))
    t0 = time.perf_counter()
    names = corpus(fm, os.path.join(work, "tiles"), days)
    res = {"corpus": {"tiles": len(names), "tile": [325, 350], "tile_chunk": [65, 70], "mosaic": [Y, X], "days": int(days.size),
                      "int16_bytes": int(days.size) * Y * X * 2, "variable": "tmin", "page_cache": "warm",
                      "generate_s": round(time.perf_counter() - t0, 2)}}
    print(json.dumps(res["corpus"]), flush=True)
    tdir = os.path.join(work, "tiles")
    # ---- the GPU route: warm-up, then five calls ----
    runs = []
    for k in range(6):
        tm = []
        out = os.path.join(work, "gpu")
        shutil.rmtree(out, ignore_errors=True)
        shutil.rmtree(out + "_m", ignore_errors=True)
        fm.create_dly_ann_mosaics(names, "tmin", tdir, out, 2001, 2001, "1.0", deflate="gpu", path_out_mthly=out + "_m", timings=tm)
        if k:
            runs.append(tm[0])
        print(json.dumps({kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in tm[0].items()}), flush=True)
    keys = [k for k in runs[0] if isinstance(runs[0][k], float)]
    g = {k: round(med([r[k] for r in runs]), 4) for k in keys}
    g.update(runs=runs[0]["runs"], bytes_out=runs[0]["bytes_out"], device_bytes=runs[0]["device_bytes"], pinned_bytes=runs[0]["pinned_bytes"])
    stages = {k: g[k] for k in ("read_s", "place_s", "deflate_s", "write_s", "monthly_s")}
    g["limiting_stage"] = max(stages, key=stages.get)
    res["gpu_route"] = g
    nbytes = res["corpus"]["int16_bytes"]
    coder_ms = g["hist_table_ms"] + g["count_scan_ms"] + g["emit_ms"] + g["compact_ms"]
    x = torch.empty(nbytes // 2, dtype=torch.int16, device="cuda")
    y = torch.empty_like(x)
    cp = []
    for k in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        if k:
            cp.append(e0.elapsed_time(e1))
    del x, y
    copy_gbs = nbytes / (med(cp) * 1e-3) / 1e9                      # bytes copied per second (each read once and written once)
    res["coder"] = {"kernel_ms": round(coder_ms, 3), "int16_gb_per_s": round(nbytes / (coder_ms * 1e-3) / 1e9, 2),
                    "copy_gb_per_s": round(copy_gbs, 2), "share_of_copy_rate": round(nbytes / (coder_ms * 1e-3) / 1e9 / copy_gbs, 4)}
    # ---- size: the streams, zlib level 1 and level 4 on a sample of the same chunks ----
    with h5nc.Dataset(os.path.join(work, "gpu", "tmin_2001.nc")) as ds:
        v = ds.variables["tmin"]
        info = v.chunk_info()
        stored = sum(s for _, s, _ in info.values())
        keys_ = list(info)
        pick = keys_[::max(1, len(keys_) // 120)][:120]
        z1 = z4 = raw = mine = 0
        for (d, r0, c0) in pick:
            chunk = np.ascontiguousarray(v[d:d + 1, r0:r0 + 325, c0:c0 + 700], "<i2")
            b = chunk.reshape(-1).view(np.uint8).reshape(-1, 2)
            sh = np.ascontiguousarray(b.T).tobytes()
            raw += len(sh)
            z1 += len(zlib.compress(sh, 1))
            z4 += len(zlib.compress(sh, 4))
            mine += info[(d, r0, c0)][1]
    slot = _qalib.mosaic_sizes(1, Y, X, 325, 700)["slot_bytes"]
    res["size"] = {"stream_bytes": int(stored), "ratio": round(stored / nbytes, 4), "sample_chunks": len(pick),
                   "sample_ratio_gpu": round(mine / raw, 4), "sample_ratio_zlib1": round(z1 / raw, 4),
                   "sample_ratio_zlib4": round(z4 / raw, 4), "longest_stream": int(max(s for _, s, _ in info.values())),
                   "slot_bytes": slot}
    assert res["size"]["longest_stream"] <= slot
    # ---- the host route over the same files: one call ----
    t0 = time.perf_counter()
    out = os.path.join(work, "host")
    paths = fm.create_dly_ann_mosaics(names, "tmin", tdir, out, 2001, 2001, "1.0")
    t1 = time.perf_counter()
    from topowx_amd import ncio
    from topowx_amd.interp import write_ds_mthly
    with ncio.open_dataset(paths[0]) as ds:
        write_ds_mthly(ds, os.path.join(work, "host_mthly.nc"), "tmin", 2001, "1.0")
    t2 = time.perf_counter()
    res["host_route"] = {"daily_s": round(t1 - t0, 3), "monthly_s": round(t2 - t1, 3), "total_s": round(t2 - t0, 3), "calls": 1,
                         "mb_per_s_daily": round(nbytes / (t1 - t0) / 1e6, 1)}
    res["speedup_end_to_end"] = round((t2 - t0) / g["total_s"], 2)
    MC.assert_same_files(os.path.join(work, "gpu", "tmin_2001.nc"), paths[0], "tmin")
    MC.assert_same_files(os.path.join(work, "gpu_m", "tmin_2001.nc"), os.path.join(work, "host_mthly.nc"), "tmin")
    res["files_equal"] = True
    # ---- memory: the whole-year object at 3250 x 7000 ----
    free = _qalib.device_free_bytes(0)
    s = _qalib.mosaic_sizes(366, 3250, 7000, 325, 700)
    with _qalib.Mosaic(366, 3250, 7000, 325, 700) as mo:
        t = mo.timing()
    res["memory_3250x7000"] = {"formula_device_bytes": s["device_bytes"], "measured_device_bytes": t["device_bytes"],
                               "measured_pinned_bytes_at_create": t["pinned_bytes"], "free_bytes_before": free,
                               "largest_max_days_admitted": _qalib.mosaic_max_days(3250, 7000, 325, 700, free, 100000)}
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True), flush=True)
    if not a.work:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
