"""GPU: step26 / step27 with the mosaics' chunks deflated on the device (libtwxqa's twxmo_*, topowx_amd/qa/twx_mosaic.hip;
``TileMosaic.create_dly_ann_mosaics(..., deflate="gpu")``).  Every comparison demands exact equality.

The expected streams come from oracle/deflate_oracle.py as it is: ONE table from the histograms of every day of the call, every
``(1, cy, cx)`` chunk of the fill-padded image deflated with it (tests/mosaic_cases.py: oracle_streams).  The shapes are the
smallest at which one boundary of the coder is crossed each:
  (130, 510)  N = 66 300 > 65 535: two stored blocks in the low plane, five segments, the last one partial; 3 x 3 chunks with
              the edge chunks padded by 90 rows and 430 columns; two days
  (128, 128)  N = 16 384: exactly one segment; 2 x 2 chunks; three days
  (255, 257)  N = 65 535: exactly one stored block; the odd chunk width takes the one-value gather; 1 x 2 chunks
  (256, 256)  N = 65 536: one byte into the second stored block; one chunk
  (7, 9)      a chunk smaller than one 64-byte piece row; 20 x 20: edges in both directions; five days"""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mosaic_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

#         chunk       mosaic       days
CASES = [((130, 510), (300, 1100), 2),
         ((128, 128), (200, 250), 3),
         ((255, 257), (255, 300), 1),
         ((256, 256), (256, 256), 1),
         ((7, 9), (20, 20), 5)]
_REF = {}


def _case(k):
    """(image, padded image, the oracle's streams, the device's streams, its offsets, its image read back) of CASES[k]: computed
    once, shared by the tests, never changed."""
    if k not in _REF:
        from topowx_amd import _qalib
        (cy, cx), (Y, X), nd = CASES[k]
        img = MC.make_image(nd, Y, X, cy, cx, seed=100 + k)
        img_p = MC.padded(img, cy, cx)
        want = MC.oracle_streams(img_p, cy, cx)
        with _qalib.Mosaic(nd, Y, X, cy, cx) as mo:
            assert (mo.Yp, mo.Xp) == img_p.shape[1:] and mo.sizes["vec"] == (2 if cx % 2 == 0 else 1)
            mo.clear(nd)
            mo.place(img, 0, 0)
            back = mo.download(nd)
            got, off = mo.deflate(nd, with_offset=True)
            got = [bytes(s) for s in got]
            again = [bytes(s) for s in mo.deflate(nd)]
            t = mo.timing()
            slot = mo.sizes["slot_bytes"]
        _REF[k] = dict(img=img, img_p=img_p, want=want, got=got, off=off, back=back, again=again, timing=t, slot=slot)
    return _REF[k]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_streams_equal_the_oracles(k):
    c = _case(k)
    (cy, cx), _, nd = CASES[k]
    assert np.array_equal(c["back"], c["img_p"])                       # the padding holds the fill value
    assert len(c["got"]) == len(c["want"]) == nd * (c["img_p"].shape[1] // cy) * (c["img_p"].shape[2] // cx)
    for i, (g, w) in enumerate(zip(c["got"], c["want"])):
        assert g == w, "stream %d of case %d: %d bytes, the oracle %d" % (i, k, len(g), len(w))
    assert np.array_equal(c["off"], np.concatenate([[0], np.cumsum([len(w) for w in c["want"]])]))
    assert max(len(g) for g in c["got"]) <= c["slot"]
    t = c["timing"]
    assert all(t[g + "_ms"] > 0 for g in ("clear", "place", "hist_table", "count_scan", "emit", "compact")) and t["aggregate_ms"] == 0
    assert t["device_bytes"] > 0 and t["pinned_bytes"] > 0


@pytest.mark.parametrize("k", range(len(CASES)))
def test_any_inflate_reads_the_streams(k):
    c = _case(k)
    (cy, cx), _, nd = CASES[k]
    img_p = c["img_p"]
    i = 0
    for d in range(nd):
        for r0 in range(0, img_p.shape[1], cy):
            for c0 in range(0, img_p.shape[2], cx):
                raw = np.frombuffer(zlib.decompress(c["got"][i]), np.uint8)          # (zlib checks the Adler-32 itself)
                n = cy * cx
                assert raw.size == 2 * n
                chunk = np.stack([raw[:n], raw[n:]], axis=1).reshape(-1).view("<i2").reshape(cy, cx)
                assert np.array_equal(chunk, img_p[d, r0:r0 + cy, c0:c0 + cx]), (d, r0, c0)
                i += 1


@pytest.mark.parametrize("k", range(len(CASES)))
def test_two_calls_give_the_same_bytes(k):
    c = _case(k)
    assert c["again"] == c["got"]


def test_placement_at_every_alignment():
    """Pieces of widths 1, 2, 7, 8, 9, 64 and 250 at odd and even columns of an image whose padded row length is odd, so that
    the rows of one piece meet every combination of source and destination alignment; a later piece wins where two overlap;
    a piece that leaves Y x X -- the padding is outside -- is refused with a message and changes nothing."""
    from topowx_amd import _qalib
    Y, X, cy, cx, nd = 45, 601, 13, 601, 3
    rng = np.random.default_rng(7)
    want = np.full((nd, 52, 601), MC.FILL, np.int16)
    with _qalib.Mosaic(nd, Y, X, cy, cx) as mo:
        assert (mo.Yp, mo.Xp) == (52, 601)
        mo.clear(nd)
        y = 0
        for tx in (1, 2, 7, 8, 9, 64, 250):
            for x0 in (0, 1, 2, 3, 4, 5, 6, 7, 8, 101, 350):
                for pnd, ty in ((nd, 3), (1, 2)):
                    a = rng.integers(-5000, 5000, (pnd, ty, tx)).astype(np.int16)
                    y0 = y % (Y - ty + 1)
                    mo.place(a, y0, x0)
                    want[:pnd, y0:y0 + ty, x0:x0 + tx] = a
                    y += 5
        a = rng.integers(-5000, 5000, (2, 20, 300)).astype(np.int16)       # over many earlier pieces: the later one wins
        mo.place(a, 11, 33)
        want[:2, 11:31, 33:333] = a
        b = mo.staging((nd, 4, 17))                                         # filled in place, no copy on the way
        b[...] = rng.integers(-5000, 5000, b.shape).astype(np.int16)
        keep = b.copy()
        mo.place(b, 40, 500)
        want[:, 40:44, 500:517] = keep
        one = np.zeros((1, 2, 2), np.int16)
        for y0, x0, shape in ((44, 0, (1, 2, 2)), (0, 600, (1, 2, 2)), (-1, 0, (1, 2, 2)), (0, -1, (1, 2, 2)), (0, 0, (nd + 1, 2, 2)),
                              (0, 0, (1, 46, 2)), (0, 0, (1, 2, 602)), (2 ** 31 - 1, 0, (1, 2, 2))):
            with pytest.raises(_qalib.QaError, match="outside the mosaic|more days"):
                mo.place(np.zeros(shape, np.int16) if shape != one.shape else one, y0, x0)
        got = mo.download(nd)
    assert np.array_equal(got, want)


def test_arguments_are_refused_before_the_device():
    from topowx_amd import _qalib
    for args in ((0, 10, 10, 5, 5), (1, 10, 10, 11, 5), (1, 10, 10, 5, 0), (1, 0, 10, 5, 5)):
        with pytest.raises(ValueError, match="twxmo_sizes"):
            _qalib.Mosaic(*args)
    with _qalib.Mosaic(2, 10, 10, 5, 5) as mo:
        for call in (lambda: mo.clear(3), lambda: mo.deflate(3), lambda: mo.deflate(13, monthly=True), lambda: mo.download(0),
                     lambda: mo.monthly(2, [1, 13])):
            with pytest.raises(_qalib.QaError):
                call()


# ---- file level -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def daily_files(tmp_path_factory):
    """Tile files of a 2 x 2 rectangle of 200 x 400 tiles, one of them missing, on a day axis from 30 December 2003 to
    2 January 2005 (2004 is a leap year): the host route's and the GPU route's three yearly files of a 400 x 800 mosaic, whose
    (1, 325, 700) chunks are 2 x 2 with edges."""
    from topowx_amd import h5nc
    from topowx_amd.interp import TileMosaic
    if not h5nc.available():
        pytest.skip("libhdf5 not loadable")
    tmp = tmp_path_factory.mktemp("mosaic_daily")
    fm = TileMosaic(MC.write_mask(str(tmp / "mask.nc"), 400, 800), 200, 400, 50, 50)
    days = MC.days_between((2003, 12, 30), (2005, 1, 2))
    tiles, whole = MC.write_tiles(fm, str(tmp / "tiles"), days, "tmin", seed=5, missing=("h01v01",))
    assert len(tiles) == 4
    host = fm.create_dly_ann_mosaics(tiles, "tmin", str(tmp / "tiles"), str(tmp / "host"), 2003, 2005, "1.2.3")
    timings = []
    gpu = fm.create_dly_ann_mosaics(tiles, "tmin", str(tmp / "tiles"), str(tmp / "gpu"), 2003, 2005, "1.2.3", deflate="gpu",
                                    timings=timings)
    return dict(fm=fm, tmp=tmp, days=days, tiles=tiles, whole=whole, host=host, gpu=gpu, timings=timings)


def test_daily_files_equal_the_host_routes(daily_files):
    f = daily_files
    assert [os.path.basename(p) for p in f["gpu"]] == ["tmin_2003.nc", "tmin_2004.nc", "tmin_2005.nc"]
    assert [os.path.basename(p) for p in f["host"]] == [os.path.basename(p) for p in f["gpu"]]
    yrs = np.asarray(f["days"]["YEAR"])
    r, c = f["fm"].tinfo.tile_rc["h01v01"]
    for ph, pg, yr, nd in zip(f["host"], f["gpu"], (2003, 2004, 2005), (2, 366, 2)):
        vals = MC.assert_same_files(pg, ph, "tmin")
        assert vals.shape == (nd, 400, 800) and np.array_equal(vals, f["whole"][yrs == yr])
        assert np.all(vals[:, r:r + 200, c:c + 400] == MC.FILL)                       # the missing tile
        from topowx_amd import h5nc
        with h5nc.Dataset(pg) as ds:
            v = ds.variables["tmin"]
            assert v.chunking() == [1, 325, 700] and v.filters()["zlib"] and v.filters()["shuffle"]
            assert int(v.getncattr("_FillValue")) == -32767
            assert len(v.chunk_info()) == nd * 4
    try:                                                  # an independent binding, where this interpreter has one
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:
        with h5py.File(f["gpu"][1], "r") as h:
            assert np.array_equal(h["tmin"][:], f["whole"][yrs == 2004])
    t = f["timings"]
    assert [x["year"] for x in t] == [2003, 2004, 2005] and all(x["runs"] == 1 and x["emit_ms"] > 0 for x in t)
    assert all(x["bytes_out"] > 0 and x["bytes_in"] == x["ndays"] * 400 * 800 * 2 for x in t)


def test_daily_files_in_runs_of_two_days(daily_files):
    f = daily_files
    paths = f["fm"].create_dly_ann_mosaics(f["tiles"], "tmin", str(f["tmp"] / "tiles"), str(f["tmp"] / "runs"), 2004, 2005, "1.2.3",
                                           deflate="gpu", batch_days=2)
    assert [os.path.basename(p) for p in paths] == ["tmin_2004.nc", "tmin_2005.nc"]          # start_yr cuts 2003 off
    for p, ph in zip(paths, f["host"][1:]):
        MC.assert_same_files(p, ph, "tmin")


def test_classic_mosaics_are_refused(daily_files):
    f = daily_files
    with pytest.raises(ValueError, match="NETCDF4"):
        f["fm"].create_dly_ann_mosaics(f["tiles"], "tmin", str(f["tmp"] / "tiles"), str(f["tmp"] / "nc3"), 2004, 2004, "1.2.3",
                                       deflate="gpu", format="NETCDF3_64BIT")


def test_monthly_file_equals_write_ds_mthly(tmp_path):
    """One whole non-leap year on a 40 x 60 mosaic (a single chunk per layer): the monthly file written in the same pass equals
    the file write_ds_mthly makes from the host route's daily mosaic, in every variable and attribute."""
    from topowx_amd import h5nc, ncio
    from topowx_amd.interp import TileMosaic, write_ds_mthly
    if not h5nc.available():
        pytest.skip("libhdf5 not loadable")
    fm = TileMosaic(MC.write_mask(str(tmp_path / "mask.nc"), 40, 60), 20, 30, 10, 10)
    days = MC.days_between((2001, 1, 1), (2001, 12, 31))
    tiles, whole = MC.write_tiles(fm, str(tmp_path / "tiles"), days, "tmax", seed=9, missing=("h00v01",))
    host = fm.create_dly_ann_mosaics(tiles, "tmax", str(tmp_path / "tiles"), str(tmp_path / "host"), 2001, 2001, "1.2.3")
    with ncio.open_dataset(host[0]) as ds:
        want = write_ds_mthly(ds, str(tmp_path / "host_mthly.nc"), "tmax", 2001, "1.2.3")
    gpu = fm.create_dly_ann_mosaics(tiles, "tmax", str(tmp_path / "tiles"), str(tmp_path / "gpu"), 2001, 2001, "1.2.3", deflate="gpu",
                                    path_out_mthly=str(tmp_path / "gpu_mthly"))
    MC.assert_same_files(gpu[0], host[0], "tmax")
    m = MC.assert_same_files(str(tmp_path / "gpu_mthly" / "tmax_2001.nc"), want, "tmax")
    assert m.shape == (12, 40, 60) and np.all(m[:, 20:, :30] == MC.FILL) and np.any(m != MC.FILL)


def test_commands_end_to_end(tmp_path):
    """``python -m topowx_amd.step26`` (host and gpu, the latter with --out-monthly) and ``step27`` (host and gpu) on generated
    tile files give the files the library calls give; both print which deflate runs."""
    import subprocess
    from topowx_amd import h5nc, ncio
    from topowx_amd.interp import TileMosaic, write_ds_mthly
    if not h5nc.available():
        pytest.skip("libhdf5 not loadable")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mask = MC.write_mask(str(tmp_path / "mask.nc"), 40, 60)
    fm = TileMosaic(mask, 20, 20, 10, 10)                                   # (the commands take ONE tile edge: 2 x 3 square tiles)
    days = MC.days_between((2001, 1, 1), (2001, 12, 31))
    tiles, _ = MC.write_tiles(fm, str(tmp_path / "tiles"), days, "tmin", seed=11)
    assert len(tiles) == 6
    lib = fm.create_dly_ann_mosaics(tiles, "tmin", str(tmp_path / "tiles"), str(tmp_path / "lib"), 2001, 2001, "4.5.6")
    with ncio.open_dataset(lib[0]) as ds:
        lib_m = write_ds_mthly(ds, str(tmp_path / "lib_mthly.nc"), "tmin", 2001, "4.5.6")
    lib_n = fm.create_normals_mosaic(tiles, "tmin", str(tmp_path / "tiles"), str(tmp_path / "lib_normals.nc"), "4.5.6")

    def run(mod, *args):
        r = subprocess.run([sys.executable, "-m", "topowx_amd." + mod] + list(args), capture_output=True, text=True, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    for how in ("host", "gpu"):
        out = tmp_path / how
        o = run("step26", "--mask", mask, "--tiles", str(tmp_path / "tiles"), "--out-normals", str(out / "n"), "--out-daily", str(out / "d"),
                "--out-monthly", str(out / "m26"), "--start-year", "2001", "--end-year", "2001", "--version", "4.5.6", "--vars", "tmin",
                "--tile", "20", "--chunk", "10", "--deflate", how)
        assert "chunks deflated on the %s" % how in o
        MC.assert_same_files(str(out / "d" / "tmin" / "tmin_2001.nc"), lib[0], "tmin")
        MC.assert_same_files(str(out / "m26" / "tmin" / "tmin_2001.nc"), lib_m, "tmin")
        MC.assert_same_files(str(out / "n" / "normals_tmin.nc"), lib_n, "tmin_normal")
        o = run("step27", "--daily", str(out / "d"), "--out", str(out / "m27"), "--start-year", "2001", "--end-year", "2001",
                "--version", "4.5.6", "--vars", "tmin", "--deflate", how)
        assert "chunks deflated on the %s" % how in o
        MC.assert_same_files(str(out / "m27" / "tmin" / "tmin_2001.nc"), lib_m, "tmin")
