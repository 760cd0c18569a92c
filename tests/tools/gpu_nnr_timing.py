#!/usr/bin/env python3
"""Time the reanalysis columns of step14 on a synthetic pool of 2 000 targets x 12 months x 69 years with the reference's
32-column shape (4 cells x 8 variable / level columns), both routes:

* ``host``: the per-target route of ``estimate_mean_variance`` with a reader that exposes only ``get_nngh_matrix`` -- its
  ``assemble_s`` (one matrix, one hash and, per distinct matrix and month, one numpy SVD).  The estimator call that follows
  ``assemble_s`` is replaced by a stub for these calls: nothing of it is inside the figure.
* ``batched``: ``NNRNghData.batched_components`` -- cell selection, upload, the three kernels, download -- and the
  ``assemble_s`` of ``estimate_mean_variance`` that contains it.

The median of ``--calls`` calls each.  Writes one JSON document with the device name as the runtime reports it.

    python tests/tools/gpu_nnr_timing.py --out profiles/nnr_components_timing.json [--targets 2000] [--calls 5]
"""
import argparse
import datetime as dt
import json
import os
import sys
import time

import torch  # noqa: F401  -- first: its bundled HIP runtime must be the one the process loads

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import numpy as np  # noqa: E402

import nnr_cases as NC  # noqa: E402
from gpu_infillmat_timing import make_pool  # noqa: E402
from topowx_amd import _qalib  # noqa: E402
from topowx_amd.infill import build_infill_matrices, estimate_mean_variance  # noqa: E402
from topowx_amd.reanalysis import NNRNghData  # noqa: E402


def make_reader(pool, seed=11):
    """An in-memory reader on the pool's days whose 2.5-degree grid covers the pool; one array serves the three slots."""
    rng = np.random.default_rng(seed)
    lons = np.arange(2.5 * np.floor(pool.lon.min() / 2.5) - 2.5, 2.5 * np.ceil(pool.lon.max() / 2.5) + 3.0, 2.5)
    lats = np.arange(2.5 * np.ceil(pool.lat.max() / 2.5) + 2.5, 2.5 * np.floor(pool.lat.min() / 2.5) - 3.0, -2.5)
    nd = pool.days.size
    lat = (rng.standard_normal((nd, 6)) * 0.5 ** np.arange(6)).astype(np.float32)
    data = {}
    for var in NC.NNR_VARS:
        nlev = 1 if NC.LEVELS[var] is None else len(NC.LEVELS[var])
        w = rng.standard_normal((nlev, lats.size, lons.size, 6)).astype(np.float32)
        a = np.einsum("dl,vyxl->dvyx", lat, w) + 0.03 * rng.standard_normal((nd, nlev, lats.size, lons.size), dtype=np.float32)
        a = (NC.OFFSET[var] + NC.SCALE[var] * a).astype(np.float32)
        a = a if NC.LEVELS[var] is not None else a[:, 0]
        for slot in NC.NNR_TIMES:
            data[(var, slot)] = a
    return NNRNghData.from_arrays(pool.days, lons, lats, data), lons.size * lats.size


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--targets", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    t0 = time.perf_counter()
    pool = make_pool(a.targets, dt.date(1948, 1, 1), dt.date(2016, 12, 31))
    nnr, ncells = make_reader(pool)
    utc = np.where(pool.lon < -100.0, -7, -6).astype(np.int16)
    m = build_infill_matrices(pool, "tmin", None, device=a.device)
    setup_s = time.perf_counter() - t0
    print("setup %.1f s: %d stations x %d days, %d cells" % (setup_s, pool.ids.size, pool.days.size, ncells), flush=True)
    day_idx = [m.day_idx(g) for g in range(m.ngroups)]
    lon, lat = pool.lon[m.target_cols], pool.lat[m.target_cols]
    parts, batched_s, assemble_b = [], [], []
    nnr.batched_components(lon[:4], lat[:4], "tmin", utc[:4], day_idx, (0.99,), device=a.device)      # context, code objects
    for k in range(a.calls):
        nnr._data = {}                                               # every call reads its columns afresh
        tm = {}
        t1 = time.perf_counter()
        b = nnr.batched_components(lon, lat, "tmin", utc, day_idx, (0.99, 0.90), device=a.device, timing=tm)
        batched_s.append(time.perf_counter() - t1)
        parts.append(tm)
        print("batched call %d: %.3f s" % (k, batched_s[-1]), flush=True)
    for k in range(a.calls):
        nnr._data = {}
        tm = {}
        estimate_mean_variance(m, nnr, utc, device=a.device, timing=tm)
        assemble_b.append(tm["assemble_s"])
        print("batched assemble_s %d: %.3f s (em_library_s %.3f)" % (k, tm["assemble_s"], tm["em_library_s"]), flush=True)
    em_s = tm["em_library_s"]
    ncomp = b.res.ncomp

    class Stop(Exception):
        pass

    real = _qalib.em_mean_variance
    host_s = []

    def stub(*args, **kw):
        raise Stop()
    only = NC.OnlyMatrix(nnr)
    for k in range(a.calls):
        nnr._data = {}
        _qalib.em_mean_variance = stub
        t1 = time.perf_counter()
        try:
            estimate_mean_variance(m, only, utc, device=a.device)
        except Stop:
            pass
        finally:
            _qalib.em_mean_variance = real
        host_s.append(time.perf_counter() - t1)
        print("host assemble %d: %.3f s" % (k, host_s[-1]), flush=True)
    med = lambda v: float(np.median(v))      # noqa: E731
    doc = dict(tool="gpu_nnr_timing", device_name=torch.cuda.get_device_name(a.device), targets=int(lon.size),
               days=int(pool.days.size), months=12, columns=32, cells=int(ncells), distinct_sets=int(len(b.sets)),
               items=int(b.res.status.size), calls=a.calls, setup_s=round(setup_s, 1),
               ncomp_099=[int(ncomp[..., 0].min()), int(ncomp[..., 0].max())],
               ncomp_090=[int(ncomp[..., 1].min()), int(ncomp[..., 1].max())],
               sweeps=[int(b.res.sweeps.min()), int(b.res.sweeps.max())],
               host_assemble_s=round(med(host_s), 3), host_assemble_all_s=[round(x, 3) for x in host_s],
               batched_assemble_s=round(med(assemble_b), 3), batched_assemble_all_s=[round(x, 3) for x in assemble_b],
               batched_components_s=round(med(batched_s), 3), batched_components_all_s=[round(x, 3) for x in batched_s],
               batched_parts={k: round(med([p[k] for p in parts]), 3) for k in
                              ("nr_select_s", "nr_library_s", "nr_upload_ms", "nr_gram_kernel_ms", "nr_eig_kernel_ms",
                               "nr_scores_kernel_ms", "nr_download_ms")},
               em_library_s=round(em_s, 3), score_bytes=int(b.res._out["scores"].nbytes),
               note="host_assemble_s is assemble_s of estimate_mean_variance with a get_nngh_matrix-only reader (the "
                    "estimator call after it stubbed); batched_assemble_s is assemble_s with the reader's "
                    "batched_components inside; nr_select_s is cell selection and column gathering on the host")
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
