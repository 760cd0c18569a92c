#!/usr/bin/env python3
"""Timing of step13's time-zone lookup on generated polygons; not a test.

    python tests/tools/gpu_tz_timing.py [--points 30000] [--repeats 5] [--out profiles/tz_lookup_timing.json]

The polygons: ``tzpoly_cases.fractal_zones()`` -- a lattice of cells over a North America box whose shared sides are
midpoint-displacement polylines, about 3.0e3 parts of 512 edges in about 400 zones, a tenth of the cells left out (water).
No real ``tz_world.json`` / ``combined.json`` is used: the row is measured on generated polygons only.  The points:
``--points`` uniform in the same box, seeded.  After one warm-up call, medians of ``--repeats`` calls of
``UtcOffset.get_utc_offsets``, by phase: upload, candidates, containment, forced, download (HIP events inside the one library
call) and the host settlement (wall time).  The containment kernel's edge bytes (32 per edge of every candidate pair) per
second are set against the float4 copy rate measured on this part, 6.29 TB/s.

The baseline is a per-point numpy restatement of the same rule (bbox candidates, a vectorised even-odd test per candidate,
the nearest edge over all edges for a point nothing contains), timed on ``--baseline-points`` of the points and scaled; it
is float64 without the exact settlement, and it is not the reference's tzwhere + shapely, which is not available here.
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

COPY_RATE = 6.29e12                      # bytes/s, the float4 copy of DESIGN section 21
BOX = (-170.0, 10.0, -50.0, 85.0)


def numpy_point(tz, px, py, max_force2):
    """One point the per-point way, in float64: (poly, forced)."""
    b = tz.bbox
    for p in np.nonzero((b[:, 0] <= px) & (px <= b[:, 2]) & (b[:, 1] <= py) & (py <= b[:, 3]))[0]:
        e = tz.edges[tz.edge_off[p]:tz.edge_off[p + 1]]
        st = (e[:, 1] > py) != (e[:, 3] > py)
        dy = e[:, 3] - e[:, 1]
        det = (e[:, 2] - e[:, 0]) * (py - e[:, 1]) - (px - e[:, 0]) * dy
        if np.count_nonzero(st & (det * dy > 0.0)) & 1:
            return int(p), False
    e = tz.edges
    dx, dy, wx, wy = e[:, 2] - e[:, 0], e[:, 3] - e[:, 1], px - e[:, 0], py - e[:, 1]
    t = np.clip((wx * dx + wy * dy) / (dx * dx + dy * dy), 0.0, 1.0)
    d2 = (wx - t * dx) ** 2 + (wy - t * dy) ** 2
    k = int(np.argmin(d2))
    return (int(np.searchsorted(tz.edge_off, k, side="right") - 1) if d2[k] <= max_force2 else -1), True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-points", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tz_lookup_timing.json"))
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import tzpoly_cases as TC
    from topowx_amd import _qalib
    from topowx_amd.utc_offsets import UtcOffset

    t0 = time.perf_counter()
    tz = TC.fractal_zones()
    gen_s = time.perf_counter() - t0
    print("generated %d parts, %d edges, %d zones in %.1f s" % (tz.zone.size, len(tz.edges), len(tz.names), gen_s), file=sys.stderr,
          flush=True)
    utc = UtcOffset.__new__(UtcOffset)                               # generated zone names have no offsets: the lookup alone
    utc.tz, utc.ndata, utc.max_force_deg, utc.device, utc.last_report = tz, -32767, 1.0, 0, None
    utc.tz_offsets = {n: float(k % 5 - 8) for k, n in enumerate(tz.names)}
    lon, lat = TC.box_points(a.points, BOX, 2009)
    rec, res = [], None
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        res = utc.get_utc_offsets(lon, lat)
        total = (time.perf_counter() - t0) * 1e3
        r = utc.last_report
        print("call %d: %.1f ms, settled %d" % (rep, total, r["settled"]), file=sys.stderr, flush=True)
        if rep:
            rec.append({"total_ms": total, "upload_ms": r["tz_upload_ms"], "candidates_ms": r["tz_candidates_ms"],
                        "containment_ms": r["tz_contain_ms"], "forced_ms": r["tz_forced_ms"], "download_ms": r["tz_download_ms"],
                        "settle_ms": r["tz_settle_ms"]})
    med = {k: round(float(np.median([x[k] for x in rec])), 3) for k in rec[0]}
    rep = utc.last_report
    # edge bytes of the containment kernel: 32 per edge of every candidate pair
    nedge_poly = np.diff(tz.edge_off)
    pair_edges = 0
    for s in range(0, lon.size, 2000):
        x, y = lon[s:s + 2000, None], lat[s:s + 2000, None]
        hit = (tz.bbox[None, :, 0] <= x) & (x <= tz.bbox[None, :, 2]) & (tz.bbox[None, :, 1] <= y) & (y <= tz.bbox[None, :, 3])
        pair_edges += int((hit * nedge_poly[None, :]).sum())
    edge_bytes = pair_edges * 32
    # the per-point numpy restatement on a subset, scaled
    sub = np.random.default_rng(5).choice(lon.size, min(a.baseline_points, lon.size), replace=False)
    t0 = time.perf_counter()
    got = [numpy_point(tz, float(lon[i]), float(lat[i]), 1.0) for i in sub]
    base_ms = (time.perf_counter() - t0) * 1e3
    agree = sum(int(g[0] == res.poly[i]) for g, i in zip(got, sub))
    phases = {k[:-3]: med[k] for k in ("upload_ms", "candidates_ms", "containment_ms", "forced_ms", "download_ms", "settle_ms")}
    out = {"tool": "gpu_tz_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
           "polygons": "generated (tzpoly_cases.fractal_zones, seed 13): no real tz_world.json / combined.json on the machine",
           "parts": int(tz.zone.size), "zones": len(tz.names), "edges": int(len(tz.edges)), "edge_bytes_uploaded": int(len(tz.edges)) * 32,
           "points": int(lon.size), "box": list(BOX), "max_force_deg": 1.0, "repeats": a.repeats,
           "note": "one run on one machine; medians of the repeats after one warm-up call; the five device phases are HIP-event "
                   "times inside the one library call, settle_ms is the wall time of the host's exact settlement, total_ms the "
                   "wall time of get_utc_offsets (allocation and the Python result arrays included)",
           "median_ms": med, "phase_ms": phases, "limiting_phase": max(phases, key=phases.get),
           "pairs": rep["pairs"], "pairs_per_point": round(rep["pairs"] / lon.size, 3), "items": rep["items"],
           "forced_points": rep["forced_points"], "forced_share": round(rep["forced_points"] / lon.size, 4),
           "inside": rep["inside"], "forced": rep["forced"], "none": rep["none"], "settled": rep["settled"],
           "containment_edge_bytes": int(edge_bytes),
           "containment_bytes_per_s": round(edge_bytes / (med["containment_ms"] * 1e-3), 0),
           "copy_rate_bytes_per_s": COPY_RATE,
           "containment_share_of_copy_rate": round(edge_bytes / (med["containment_ms"] * 1e-3) / COPY_RATE, 5),
           "forced_edge_bytes": int(rep["forced_points"]) * int(len(tz.edges)) * 32,
           "numpy_per_point_baseline": {"points_timed": int(sub.size), "ms": round(base_ms, 1),
                                        "scaled_to_all_points_ms": round(base_ms * lon.size / sub.size, 0),
                                        "same_polygon_as_gpu": agree},
           "gpu_call_ms": med["total_ms"]}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
