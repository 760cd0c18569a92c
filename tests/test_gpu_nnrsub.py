"""GPU: step12's reanalysis subsets.  ``twxns_subset`` against the numpy restatement byte for byte over the edge shapes,
both raw types, both layouts and the padding of edge chunks; all 65 536 packed values through the unpack; two calls, the
same bytes; and ``python -m topowx_amd.step12`` end to end on generated yearly files in both containers, against the
hashes of the EXECUTED reference (tests/golden/golden_nnrsub_v1.npz).  No tolerance anywhere: every operation is one
correctly rounded float32 operation."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import nnrsub_cases as NC  # noqa: E402
import restate_nnrsub as RN  # noqa: E402
from topowx_amd import _qalib, h5nc, ncio, reanalysis  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "golden_nnrsub_v1.npz"))
NL = 4
# six products in one call: one level, two levels (not in file order), thickness, each conversion, every slot
PRODUCTS = [dict(slot=0, levels=[2]), dict(slot=1, levels=[3, 0], conv="k_to_c"), dict(slot=2, thick=(3, 0)),
            dict(slot=1, thick=(1, 2), conv="k_to_c"), dict(slot=2, levels=[1, 1]), dict(slot=0, levels=[0, 1], conv="none")]


def make_case(ndays, nlat, nlon, dtype, nmarks, seed):
    """Records in shuffled order: slot 0 misses the first and the last day, slot 1 has every day, slot 2 every other day;
    some records belong to no slot, some to no day.  ``lon_idx`` descends with gaps; ``lat_idx`` is a permutation."""
    rng = np.random.default_rng([seed, ndays, nlat, nlon, nmarks])
    ny, nx = nlat + 3, 2 * nlon + 1
    recs = [(0, d) for d in range(1, ndays - 1)] + [(1, d) for d in range(ndays)] + [(2, d) for d in range(0, ndays, 2)]
    recs += [(-1, d % ndays) for d in range(5)] + [(s % 3, -1) for s in range(4)] + [(-1, -1)]
    recs = [recs[k] for k in rng.permutation(len(recs))]
    slot, day = np.array([r[0] for r in recs], np.int32), np.array([r[1] for r in recs], np.int32)
    shape = (len(recs), NL, ny, nx)
    if dtype == np.int16:
        raw = rng.integers(-32768, 32768, shape, dtype=np.int16)
        marks = [(None, None), (32766, None), (32766, -32767)][nmarks]
        scale, offset = NC.PACKS[seed % len(NC.PACKS)]
    else:
        raw = rng.normal(250.0, 40.0, shape).astype(np.float32)
        raw[rng.random(shape) < 0.01] = np.float32(-0.0)           # (no NaN: IEEE 754 leaves the sign of a NaN result open)
        marks = [(None, None), (None, NC.F4_MARK), (np.float32(1e20), NC.F4_MARK)][nmarks]
        scale, offset = ((1.0, 0.0), (0.5, -3.25))[seed % 2]
    for m in marks:
        if m is not None:
            raw[rng.random(shape) < 0.03] = m
    return dict(raw=raw, scale=scale, offset=offset, marks=marks, rec_slot=slot, rec_day=day, ndays=ndays,
                lat_idx=rng.permutation(ny)[:nlat], lon_idx=np.arange(nx - 1, -1, -2)[:nlon], products=PRODUCTS)


@pytest.mark.parametrize("nlat,nlon", [(1, 1), (4, 4), (5, 3), (6, 7), (21, 33)])
@pytest.mark.parametrize("ndays", [1, 63, 64, 65, 257])
def test_entry_equals_the_restatement_byte_for_byte(ndays, nlat, nlon):
    for k, dtype in enumerate((np.int16, np.float32)):
        case = make_case(ndays, nlat, nlon, dtype, (ndays + nlat + k) % 3, seed=k + nlon)
        want, want_counts = RN.subset(**case)
        assert want_counts[0, 2] == min(ndays, 2) and want_counts[1, 2] == 0          # a first and a last day without a record
        assert case["marks"] != (None, None) or want_counts[:, 1].sum() == 0
        assert ndays * nlat * nlon < 1000 or case["marks"] == (None, None) or want_counts[:, 1].min() > 0
        for layout in (_qalib.NS_TILED, _qalib.NS_PLAIN):
            tm = {}
            outs, counts = _qalib.ns_subset(layout=layout, timing=tm, **case)
            assert all(np.isfinite(tm[k + "_ms"]) and tm[k + "_ms"] >= 0 for k in _qalib.NS_KERNELS), tm
            again, counts2 = _qalib.ns_subset(layout=layout, **case)
            assert np.array_equal(counts, want_counts) and np.array_equal(counts2, counts)
            for p, (a, b, w) in enumerate(zip(outs, again, want)):
                ref = RN.tile(w) if layout == _qalib.NS_TILED else w
                assert a.shape == ref.shape and a.dtype == np.float32
                assert a.tobytes() == ref.tobytes(), (dtype.__name__, layout, p, int((a.view(np.uint32) != ref.view(np.uint32)).sum()))
                assert b.tobytes() == a.tobytes()
                if layout == _qalib.NS_TILED:                      # the padding of edge chunks, spelled out
                    full = a.transpose(2, 3, 0, 4, 1, 5).reshape(ndays, a.shape[3], a.shape[0] * 4, a.shape[1] * 4)
                    assert (full[:, :, nlat:, :] == NC.FILL_F4).all() and (full[:, :, :, nlon:] == NC.FILL_F4).all()
                    assert full[:, :, :nlat, :nlon].tobytes() == w.tobytes()


@pytest.mark.parametrize("pack", NC.PACKS)
def test_every_packed_value_through_the_unpack(pack):
    raw = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16).reshape(1, 1, 256, 256)
    outs, counts = _qalib.ns_subset(raw, pack[0], pack[1], (None, None), [0], [0], 1, np.arange(256), np.arange(256),
                                    [dict(slot=0, levels=[0]), dict(slot=0, levels=[0], conv="k_to_c")], layout=_qalib.NS_PLAIN)
    u = (raw.astype(np.float32) * np.float32(pack[0])).astype(np.float32) + np.float32(pack[1])
    assert outs[0].tobytes() == u.tobytes() and outs[1].tobytes() == (u - np.float32(273.15)).tobytes()
    assert counts.tolist() == [[1, 0, 0], [1, 0, 0]]
    tiled, _ = _qalib.ns_subset(raw, pack[0], pack[1], (None, None), [0], [0], 1, np.arange(256), np.arange(256),
                                [dict(slot=0, levels=[0], conv="k_to_c")], layout=_qalib.NS_TILED)
    assert reanalysis.untile(tiled[0], 256, 256).tobytes() == outs[1].tobytes()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


RUNS = [pytest.param("NETCDF3_64BIT", "NETCDF4", marks=pytest.mark.skipif(not h5nc.available(), reason="libhdf5 not loadable")),
        pytest.param("NETCDF4", "NETCDF3_64BIT", marks=pytest.mark.skipif(not h5nc.available(), reason="libhdf5 not loadable"))]


@pytest.mark.parametrize("raw_fmt,out_fmt", RUNS)
def test_step12_end_to_end_equals_the_executed_reference(tmp_path, raw_fmt, out_fmt):
    raw_dir, out_dir = tmp_path / "raw", tmp_path / "out"
    raw_dir.mkdir()
    NC.write_raw_files(str(raw_dir), raw_fmt)
    res = subprocess.run([sys.executable, "-m", "topowx_amd.step12", "--nnr-raw", str(raw_dir), "--out", str(out_dir),
                          "--start-year", "2000", "--end-year", "2000", "--format", out_fmt], cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["files"] == 21 and line["days"] == 731 and line["years"] == 2
    arrays = {}
    for name in (str(n) for n in GOLD["names"]):
        path = str(out_dir / (name + ".nc"))
        assert ncio.file_format(path) == out_fmt
        with ncio.open_dataset(path) as ds:
            v = ds.variables[name.split("_")[1]]
            a = np.asarray(v[:])
            assert a.dtype == np.float32 and a.shape == tuple(GOLD[name + "/shape"]) and _sha(a) == str(GOLD[name + "/sha"]), name
            assert line["nsub_counts"][name + ".nc"] == GOLD[name + "/counts"].tolist(), name
            if out_fmt == "NETCDF4":
                assert v.chunking() == [731] + ([a.shape[1]] if a.ndim == 4 else []) + [4, 4] and not v.filters()["zlib"]
            arrays[name] = a.reshape(731, -1, 6, 7)
    nn = reanalysis.NNRNghData(str(out_dir), (20000305, 20000314))
    try:
        d0 = int(nn.day_mask[0])
        free = np.ones((6, 7), bool)
        for name in nn.NNR_VARS:
            free &= ~(arrays["nnr_%s_12z" % name][d0:d0 + 10] == NC.FILL_F4).any(axis=(0, 1))
        pts = [(nn.nnr_lons[j] + 5.0, nn.nnr_lats[i] - 4.0) for i in range(5) for j in range(6)]
        pts = [pt for pt in pts if free.ravel()[nn.nearest_cells(*pt)].all()]
        assert pts
        m = nn.get_nngh_matrix(pts[0][0], pts[0][1], "tmin", -6)
        want = np.hstack([arrays["nnr_%s_12z" % name][d0:d0 + 10, :, c // 7, c % 7] for c in nn.nearest_cells(*pts[0])
                          for name in nn.NNR_VARS])
        assert m.tobytes() == want.tobytes() and m.shape == (10, 32)
    finally:
        nn.close()
