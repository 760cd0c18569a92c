"""Timing of ``twxpc_spatial_corrob`` on synthetic rows (needs an MI355X and a build): 12 000 stations x 25 203 days
(1948-2016), every station a target.

    python tests/tools/gpu_prcpcorrob_timing.py [--out profiles/prcpcorrob_timing.json] [--stations 12000] [--repeats 5]
                                                [--host-targets 2]

One warm-up call, then the MEDIAN of ``--repeats`` calls of the check after the missing check (the spatial-only chain): HIP-event
milliseconds per kernel group and host-clock milliseconds of the whole call (copies included; the host share is what is
left after the kernels).  The walk's rate: the bytes it is ESTIMATED to move -- targets x days x mean neighbours x 4 B, one
read of every neighbour value, the reads of the days x - 1 and x + 1 taken as cache hits; an estimate, not a measured
traffic figure -- over its time, as a share of the rate a device-to-device copy of the pool reaches in the same run (read +
write bytes over HIP-event time, median of five).  Next to it the host time of the numpy restatement
(tests/restate_prcpcorrob.py) on the first ``--host-targets`` targets against their neighbours, named, not scaled up.  The
rows are those of gpu_prcp_timing.py (a block of 400 random series repeated: 30 % wet days, hundredths of a centimetre, 5 %
missing, a few large values); the stations stand on a lattice of 0.3 x 0.225 degrees between 30 and 52 degrees north, which
gives every station some 25 to 40 neighbours within 75 km.
"""
import argparse
import datetime as dt
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prcpcorrob_timing.json"))
    ap.add_argument("--stations", type=int, default=12000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-targets", type=int, default=2)
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import restate_prcpcorrob as RC
    from topowx_amd import _qalib
    from topowx_amd.dates import YMD, get_days_metadata
    days = get_days_metadata(dt.date(1948, 1, 1), dt.date(2016, 12, 31))
    nd = days.size
    ymd = np.ascontiguousarray(days[YMD], np.int32)
    rs = np.random.RandomState(912)
    blk = 400
    base = np.where(rs.rand(blk, nd) < 0.30, np.round(rs.gamma(0.8, 0.9, (blk, nd)) + 0.01, 2), 0.0).astype(np.float32)
    base[rs.rand(blk, nd) < 0.05] = np.nan
    for s in range(blk):
        base[s, rs.randint(0, nd, 5)] = np.round(rs.uniform(20.0, 70.0, 5), 2)
    reps = -(-a.stations // blk)
    prcp = np.ascontiguousarray(np.tile(base, (reps, 1))[:a.stations])
    ns = prcp.shape[0]
    k = np.arange(ns)
    lon, lat = -120.0 + 0.3 * (k % 120), 30.0 + 0.225 * (k // 120)
    flags0 = np.where(np.isnan(prcp), 2, 1).astype(np.uint8)
    tgt = np.arange(ns)

    def call(tm):
        t0 = time.perf_counter()
        f, st = _qalib.prcp_spatial_corrob(lon, lat, prcp, ymd, tgt, flags0, timing=tm)
        tm["host_ms"] = (time.perf_counter() - t0) * 1e3
        return f, st

    flags, status = call({})                                         # warm-up: code objects, allocator, page faults
    runs = []
    for _ in range(a.repeats):
        tm = {}
        f, _ = call(tm)
        assert f.tobytes() == flags.tobytes()
        runs.append(tm)
        print(json.dumps({k_: round(v, 3) for k_, v in tm.items()}), flush=True)
    med = {k_: round(float(np.median([r[k_] for r in runs])), 3) for k_ in runs[0]}
    # the copy rate of this device, this run: a device-to-device copy of the pool
    src = torch.empty(ns * nd, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    rates = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        rates.append(2 * src.numel() * 4 / (e0.elapsed_time(e1) * 1e-3))
    copy_rate = float(np.median(rates))
    del src, dst
    # neighbour counts of the lattice, from the restatement's distances (a row of the lattice at a time would do; all is cheap)
    nngh = np.array([RC.neighbours(lon, lat, int(s))[0].size for s in range(0, ns, max(1, ns // 600))])
    mean_ngh = float(nngh.mean())
    walk_bytes = ns * nd * mean_ngh * 4.0
    walk_rate = walk_bytes / (med["pc_walk_kernel_ms"] * 1e-3)
    # the restatement on a few targets against their neighbours (the same neighbour sets as in the whole pool)
    h = min(a.host_targets, ns)
    sub = sorted(set(range(h)) | set(int(j) for s in range(h) for j in RC.neighbours(lon, lat, s)[0]))
    pos = {s: i for i, s in enumerate(sub)}
    t0 = time.perf_counter()
    want = RC.run(lon[sub], lat[sub], prcp[sub].T, ymd, [pos[s] for s in range(h)], flags0[:h].T)
    host_ms = (time.perf_counter() - t0) * 1e3
    knife = want["margin"] < 1e-5
    assert np.array_equal(want["flags"].T[~knife.T], flags[:h][~knife.T]), "the timed call and the restatement differ on the host slice"
    kernels = sum(med[k_ + "_kernel_ms"] for k_ in _qalib.PC_KERNELS)
    slowest = max(_qalib.PC_KERNELS, key=lambda k_: med[k_ + "_kernel_ms"])
    out = {"tool": "gpu_prcpcorrob_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
           "stations": int(ns), "targets": int(ns), "days": int(nd), "years": 69, "repeats": a.repeats,
           "note": "one run on one machine; medians of the repeats after one warm-up call; spatial-only chain; "
                   "the walk's bytes are an estimate (targets x days x mean neighbours x 4 B), not a measured traffic figure",
           "median_ms": med, "kernels_ms": round(kernels, 3), "host_share_ms": round(med["host_ms"] - kernels, 3),
           "slowest_kernel_group": slowest,
           "flags": {str(k_): int((flags == k_).sum()) for k_ in (1, 2, 17)},
           "status": {str(int(k_)): int((status == k_).sum()) for k_ in np.unique(status)},
           "mean_neighbours_sampled": round(mean_ngh, 2), "max_neighbours_sampled": int(nngh.max()),
           "copy_rate_measured_bytes_per_s": round(copy_rate, 0), "walk_bytes_estimated": int(walk_bytes),
           "walk_bytes_per_s_estimated": round(walk_rate, 0), "walk_share_of_measured_copy_rate": round(walk_rate / copy_rate, 4),
           "station_years_per_s_whole_call": round(ns * 69 / (med["host_ms"] * 1e-3), 0),
           "station_years_per_s_kernels": round(ns * 69 / (kernels * 1e-3), 0),
           "restatement_host_ms": round(host_ms, 1), "restatement_targets": int(h), "restatement_pool": len(sub)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
