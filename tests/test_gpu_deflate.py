"""GPU: the daily outputs of a streamed tile as HDF5 shuffle + deflate chunk bytes formed on the device (twx_stream_deflate,
csrc/twx_deflate.h).  The reference reaches that storage form through netCDF4-python's ``zlib=True`` (tiling.py:720,894,913,
1035).  Checks: (1) zlib -- the decoder inside libhdf5 -- inflates every stream to the shuffled chunk of what the synchronous
entry computes; (2) the GPU's bytes equal the CPU restatement's (oracle/deflate_oracle.py), byte for byte; (3) a NetCDF-4 tile
file whose chunks were appended with H5Dwrite_chunk reads back through libhdf5 as the same int16 arrays.  Through the same entry,
what the kernel probe (tests/test_gpu_deflate_kernels.py) cannot see -- df_launch's own carving and launch order -- at the sizes
temperature tiles of 1 096 days never reach: day axes of 1 and 3 days, an all-masked tile, the 25 203-day production axis."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _tile_chunks(daily, cy, cx):
    return [np.ascontiguousarray(daily[:, r0:r0 + cy, c0:c0 + cx]) for r0 in range(0, daily.shape[1], cy)
            for c0 in range(0, daily.shape[2], cx)]


@pytest.mark.parametrize("rows,cols,cy,cx", [(slice(20, 60), slice(30, 80), 10, 10),      # 20 chunks of 109 600 values: 7 blocks each
                                             (slice(0, 30), slice(60, 100), 30, 40),      # one chunk: 21 stored blocks, 81 segments (6 of them counted for the code)
                                             (slice(40, 52), slice(8, 22), 4, 7)])        # odd shapes: rows of 7 cells
def test_deflated_chunks_equal_the_restatement_and_inflate_to_the_daily_values(golden_case, rows, cols, cy, cx):
    from oracle import deflate_oracle as dorc
    from topowx_amd import _lib
    grid, tmin, tmax = golden_case
    grid = dict(grid)
    mask = np.array(grid["mask"], copy=True)
    mask[45:50, 10:40] = 0                                    # fill values inside some chunks
    grid["mask"] = mask
    ctx = _lib.Context()
    ctx.set_stations(_lib.TMIN, tmin)
    ctx.set_stations(_lib.TMAX, tmax)
    want = ctx.interp_grid(grid, daily=True, rows=rows, cols=cols)
    Y, X = want["status"].shape
    st = ctx.stream(Y, X, daily=True, nslots=2, deflate_chunks=(cy, cx))
    st.submit(0, grid, rows, cols)
    st.submit(1, grid, rows, cols)                            # (the same tile in the other device image)
    outs = []
    for slot in (0, 1):
        o = st.wait(slot)
        outs.append({k: ([bytes(b) for b in v] if k.startswith("deflated_") else (np.array(v) if hasattr(v, "shape") else v))
                     for k, v in o.items()})
    dev_ms, copy_ms = st.times(1)
    timing = ctx.timing()
    st.close()
    ctx.close()
    assert dev_ms > 0 and copy_ms > 0 and timing["deflate_ms"] > 0
    nd = tmin.days.size
    for o in outs:
        assert "daily_tmin" not in o and o["deflate_chunks"] == (cy, cx)
        for k in ("norm_tmin", "se_tmin", "norm_tmax", "se_tmax", "ninvalid", "status"):
            assert np.array_equal(o[k], want[k]), k
        for var in ("tmin", "tmax"):
            chunks = _tile_chunks(want["daily_" + var], cy, cx)
            blobs = o["deflated_" + var]
            assert len(blobs) == len(chunks)
            for c, (blob, chunk) in enumerate(zip(blobs, chunks)):
                raw = np.frombuffer(zlib.decompress(blob), np.uint8)          # zlib checks the Adler-32 itself
                lo, hi = dorc.shuffled(chunk)
                assert raw.size == 2 * lo.size and np.array_equal(raw[:lo.size], lo) and np.array_equal(raw[lo.size:], hi), (var, c)
                assert np.array_equal(dorc.inflate_chunk(blob, nd, cy, cx), chunk)
    # byte for byte against the restatement (pure Python: a few chunks, whatever their size)
    o = outs[0]
    for var in ("tmin", "tmax"):
        chunks = _tile_chunks(want["daily_" + var], cy, cx)
        table = dorc.tile_table(want["daily_" + var], cy, cx)         # the variable's Huffman code, from every 16th segment of every chunk
        for c in sorted({0, len(chunks) // 2, len(chunks) - 1}):
            assert o["deflated_" + var][c] == dorc.deflate_chunk(chunks[c], table), (var, c)
    sizes = [len(b) for b in o["deflated_tmin"]]
    assert max(sizes) <= 2 * nd * cy * cx + 5 * (nd * cy * cx // dorc.SEG + nd * cy * cx // 65535 + 2) + 11       # never longer than stored


def _stream_one_tile(ctx, grid, rows, cols, cy, cx):
    """one tile through ctx.stream(..., deflate_chunks=(cy, cx)) -- the library's own carving and launch order (df_launch) --
    -> {variable: [chunk streams]}"""
    Y, X = rows.stop - rows.start, cols.stop - cols.start
    st = ctx.stream(Y, X, daily=True, nslots=2, deflate_chunks=(cy, cx))
    st.submit(0, grid, rows, cols)
    o = st.wait(0)
    got = {var: [bytes(b) for b in o["deflated_" + var]] for var in ("tmin", "tmax")}
    st.close()
    return got


def _assert_streams(got, want, cy, cx, compared):
    """every stream inflates (zlib) to its shuffled chunk; the chunks `compared(number of chunks)` names equal the restatement"""
    from oracle import deflate_oracle as dorc
    for var in ("tmin", "tmax"):
        daily = want["daily_" + var]
        chunks = _tile_chunks(daily, cy, cx)
        assert len(got[var]) == len(chunks)
        n = chunks[0].size
        for c, (blob, chunk) in enumerate(zip(got[var], chunks)):
            lo, hi = dorc.shuffled(chunk)
            assert zlib.decompress(blob) == lo.tobytes() + hi.tobytes(), (var, c)
            assert len(blob) <= 2 + n + 5 * -(-n // 65535) + n + 5 * -(-n // dorc.SEG) + 9, (var, c)
        table = dorc.tile_table(daily, cy, cx)
        for c in compared(len(chunks)):
            assert got[var][c] == dorc.deflate_chunk(chunks[c], table), (var, c)


def _synthetic(first, last, nstns, nrows=None, ncols=None):
    import datetime as dt
    from topowx_amd import _lib, synth
    from topowx_amd.dates import get_days_metadata
    days = get_days_metadata(dt.date(*first), dt.date(*last))
    grid = synth.make_grid("C2", nrows=nrows, ncols=ncols) if nrows else synth.make_grid("C1")
    ctx = _lib.Context()
    for var, which in (("tmin", _lib.TMIN), ("tmax", _lib.TMAX)):
        ctx.set_stations(which, synth.make_stations(grid["bbox"], nstns, 1, var, days, with_obs=True))
    return days, grid, ctx


@pytest.mark.parametrize("ndays", [1, 3])
def test_a_short_day_axis_through_the_stream(ndays):
    """Chunks shorter than a piece (N = ndays cy cx of 3 .. 12 < 64) through the library's own launch path: one segment of a
    partial piece, most threads without a byte, every high-plane block stored (the code's description alone is longer)."""
    days, grid, ctx = _synthetic((1981, 1, 1), (1981, 1, ndays), 300)
    assert days.size == ndays
    rows, cols = slice(10, 14), slice(20, 26)
    want = ctx.interp_grid(grid, daily=True, rows=rows, cols=cols)
    assert np.all(want["status"] == 0) and want["daily_tmin"].shape == (ndays, 4, 6)
    for cy, cx in ((2, 2), (1, 3)):
        assert ndays * cy * cx < 64
        got = _stream_one_tile(ctx, grid, rows, cols, cy, cx)
        _assert_streams(got, want, cy, cx, lambda n: range(n))
        for var in ("tmin", "tmax"):
            assert all(len(b) == 2 + (ndays * cy * cx + 5) * 2 + 9 for b in got[var])          # both planes stored
    ctx.close()


def test_an_all_masked_tile_through_the_stream(golden_case):
    """A tile without one unmasked cell is not short-cut: its chunks are the constant fill value (-32767: high byte 0x80, one
    64-byte match per piece) and are deflated like any other."""
    from topowx_amd import _lib
    grid, tmin, tmax = golden_case
    grid = dict(grid)
    grid["mask"] = np.zeros_like(grid["mask"])
    ctx = _lib.Context()
    ctx.set_stations(_lib.TMIN, tmin)
    ctx.set_stations(_lib.TMAX, tmax)
    rows, cols = slice(20, 40), slice(30, 50)
    want = ctx.interp_grid(grid, daily=True, rows=rows, cols=cols)
    assert np.all(want["daily_tmin"] == _lib.FILL_I2) and np.all(want["daily_tmax"] == _lib.FILL_I2) and _lib.FILL_I2 == -32767
    got = _stream_one_tile(ctx, grid, rows, cols, 10, 10)
    ctx.close()
    _assert_streams(got, want, 10, 10, lambda n: range(n))
    n = tmin.days.size * 100
    assert all(len(b) < 0.52 * 2 * n for b in got["tmin"])              # the high plane is next to nothing


def test_the_full_day_axis_through_the_stream():
    """The production day axis (1948-01-01 .. 2016-12-31, 25 203 days; construction of test_gpu_fullsize.py's
    test_full_day_axis_1948_2016 with fewer stations: the kriging is not under test) on a 20 x 20 tile: chunks of 10 x 10 give
    154 segments (the Adler scan of k_deflate_scan takes two passes), chunks of 10 x 20 give 308 (both scans do) -- what every
    production chunk (50 x 50: 3 846 segments) goes through.  Every stream inflated by zlib; the first and the last chunk of
    both variables byte for byte against the restatement."""
    from oracle import deflate_oracle as dorc
    days, grid, ctx = _synthetic((1948, 1, 1), (2016, 12, 31), 300, 64, 64)
    assert days.size == 25203
    rows, cols = slice(22, 42), slice(8, 28)
    want = ctx.interp_grid(grid, daily=True, rows=rows, cols=cols)
    assert np.all(want["status"] == 0)
    for (cy, cx), nseg in (((10, 10), 154), ((10, 20), 308)):
        assert -(-25203 * cy * cx // dorc.SEG) == nseg
        got = _stream_one_tile(ctx, grid, rows, cols, cy, cx)
        _assert_streams(got, want, cy, cx, lambda n: (0, n - 1))
    ctx.close()


def test_streamed_deflated_tiles_into_netcdf4(golden_case, tmp_path):
    """driver.interp_tiles_streamed(deflate_chunks=...) -> ncio.TileSink(zlib=True): the sink appends the GPU's chunk bytes with
    H5Dwrite_chunk; the files read back through libhdf5 (shuffle + deflate filters) as what the synchronous path computes."""
    from topowx_amd import _lib, driver, h5nc, ncio
    from topowx_amd.interp import Tiler
    if not h5nc.available():
        pytest.skip("libhdf5 not loadable")
    grid, tmin, tmax = golden_case
    ctx = _lib.Context()
    ctx.set_stations(_lib.TMIN, tmin)
    ctx.set_stations(_lib.TMAX, tmax)
    tiles = driver.tile_list(grid["mask"], 50, 50)
    want = driver.interp_tiles(grid, driver.gpu_compute(ctx, daily=True), tiles, 50, 50)
    info = Tiler(grid, 50, 50, 10, 10, process_tiles=()).build_tile_grid_info()
    sink = ncio.TileSink(info, str(tmp_path), tmin.days, threads=4, zlib=True, verify=(tiles[2][0],))
    log = {}
    driver.interp_tiles_streamed(ctx, grid, tiles, 50, 50, daily=True, sink=sink, precision="fast", deflate_chunks=(10, 10), log=log)
    sink.close()
    assert sink.stats["tiles"] == 4 and sink.stats["verified"] == 1 and log["tiles_fast"] == 4
    assert sink.stats["int16_bytes"] == 4 * 2 * want[0]["daily_tmin"].nbytes and sink.stats["disk_bytes"] < sink.stats["int16_bytes"]
    for k, i, j, _ in tiles:
        for var in ("tmin", "tmax"):
            t = ncio.read_tile(sink.writer.fpath(info.get_tile_id(k), var), var)
            assert np.array_equal(t["daily"], want[k]["daily_" + var]) and np.array_equal(t["norm"], want[k]["norm_" + var])
            assert np.array_equal(t["ninvalid"], want[k]["ninvalid"])
    ds = ncio.open_dataset(sink.writer.fpath(info.get_tile_id(0), "tmax"))
    f = ds.variables["tmax"].filters()
    assert ds.variables["tmax"].chunking() == [tmin.days.size, 10, 10] and f["zlib"] and f["shuffle"]
    ds.close()
    # the default sink collects the streams; a sink without zlib refuses them
    got, _, _ = driver.interp_tiles_streamed(ctx, grid, tiles[:1], 50, 50, daily=True, precision="fast", deflate_chunks=(25, 50))
    k = tiles[0][0]
    assert len(got[k]["deflated_tmin"]) == 2 and "daily_tmin" not in got[k]
    assert np.array_equal(ncio.TileSink._inflate_tile(got[k]["deflated_tmax"], want[k]["daily_tmax"].shape, 25, 50), want[k]["daily_tmax"])
    plain = ncio.TileSink(info, str(tmp_path / "plain"), tmin.days, threads=2)
    with pytest.raises(IOError, match="zlib=True"):
        driver.interp_tiles_streamed(ctx, grid, tiles[:1], 50, 50, daily=True, sink=plain, precision="fast", deflate_chunks=(10, 10))
    plain.close()
    ctx.close()


def test_deflate_stream_argument_checks(golden_case):
    from topowx_amd import _lib
    grid, tmin, tmax = golden_case
    ctx = _lib.Context()
    ctx.set_stations(_lib.TMIN, tmin)
    ctx.set_stations(_lib.TMAX, tmax)
    with pytest.raises(_lib.TwxError, match="divide"):
        ctx.stream(20, 20, daily=True, deflate_chunks=(8, 10))
    with pytest.raises(_lib.TwxError, match="daily"):
        ctx.stream(20, 20, daily=False, deflate_chunks=(10, 10))
    st = ctx.stream(20, 20, daily=True, nslots=3, deflate_chunks=(10, 20), variables=("tmax",))
    # three tiles submitted before anything is waited for: the third needs the first one's device image -> the library copies
    # the first one out itself
    for slot, r0 in enumerate((0, 20, 40)):
        st.submit(slot, grid, slice(r0, r0 + 20), slice(10, 30))
    for slot, r0 in enumerate((0, 20, 40)):
        o = st.wait(slot)
        assert "deflated_tmin" not in o and len(o["deflated_tmax"]) == 2
        want = ctx_sync(tmin, tmax, grid, slice(r0, r0 + 20), slice(10, 30))
        got = np.concatenate([np.frombuffer(zlib.decompress(bytes(b)), np.uint8) for b in o["deflated_tmax"]])
        n = tmin.days.size * 10 * 20
        for c in range(2):
            raw = got[c * 2 * n:(c + 1) * 2 * n]
            chunk = np.stack([raw[:n], raw[n:]], axis=1).reshape(-1).view("<i2").reshape(-1, 10, 20)
            assert np.array_equal(chunk, want["daily_tmax"][:, c * 10:(c + 1) * 10, :])
    st.close()
    ctx.close()


def ctx_sync(tmin, tmax, grid, rows, cols):
    from topowx_amd import _lib
    c = _lib.Context()
    c.set_stations(_lib.TMIN, tmin)
    c.set_stations(_lib.TMAX, tmax)
    out = c.interp_grid(grid, daily=True, rows=rows, cols=cols)
    c.close()
    return out
