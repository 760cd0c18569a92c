"""The five deflate kernels of csrc/twx_deflate.h on int16 images chosen against them, run by tests/tools/deflate_probe.hip (a
child process with df_launch's kernel sequence, sizes and load-width rule) and compared, exactly, with

* zlib -- the decoder inside libhdf5: every chunk's stream inflates to the shuffled chunk (zlib verifies the Adler-32);
* the CPU restatement oracle/deflate_oracle.py: sampled token counts, the Huffman table (lengths, codes, header bits), the
  stream bytes.

Through the library the kernels only ever see kriged temperature fields (smooth high bytes, 1 096 days, <= 81 segments a
chunk).  The cases below reach what those never do: stored high-plane segments beside Huffman ones, the depth-limit halving
loop of k_deflate_table, the second pass of both scans of k_deflate_scan, both load widths across 65 535-byte stored-block
boundaries, chunks shorter than a piece, constant images, runs cut at every kind of boundary.  Every case names its path in
``Case.path``; ``test_cases_reach_their_paths`` (CPU, restatement only) asserts the precondition that makes the case worth
running, so a generator that drifts cannot turn a GPU test into a no-op.

The probe adds two checks of its own: guard bands around every device buffer (the only check there is for piece_bits, seg_off
and adl) and a second run into separate buffers that must be byte-identical (a race between the plain and the atomic LDS
stores of k_deflate_emit would show there).  Its second run launches k_deflate_table with two work-groups, as a two-variable
tile does; work-group 0 then builds the code of an all-zero count array.

All cases go through ONE probe process (the module opens the GPU once); if it fails, every test of the module fails with
the case the probe named and the probe is not run again."""
import functools
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from oracle import deflate_oracle as dorc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "deflate_probe.hip")
PROBE_MAGIC = 0x44464C50524F4231
STEP1 = 256                                                  # elements a work-group stages per step with one value per load
BUFFERS = ("out", "seg_bytes", "seg_off", "adl", "piece_bits", "chunk_bytes", "hist", "table", "daily", "hist0", "table0")


class Case(object):
    def __init__(self, name, image, cy, cx, path, needs=(), compare="all"):
        self.name, self.image, self.cy, self.cx, self.path = name, np.ascontiguousarray(image, "<i2"), cy, cx, path
        self.needs, self.compare = tuple(needs), compare
        self.ndays, self.Y, self.X = self.image.shape
        assert self.Y % cy == 0 and self.X % cx == 0, name
        self.N = self.ndays * cy * cx
        self.nchunk = (self.Y // cy) * (self.X // cx)
        self.nseg = -(-self.N // dorc.SEG)
        self.vec = 2 if cx % 2 == 0 and self.X % 2 == 0 else 1        # df_launch's `pairs` rule

    def chunks(self):
        return dorc._chunks(self.image, self.cy, self.cx)

    def compared(self):
        """indices of the chunks compared byte for byte with the restatement"""
        return list(range(self.nchunk)) if self.compare == "all" else sorted({0, self.nchunk // 2, self.nchunk - 1})


def _bound(n):
    """the longest stream of a chunk of n elements: everything stored"""
    return 2 + n + 5 * -(-n // dorc.STORED) + n + 5 * -(-n // dorc.SEG) + 9


def _planes(lo, hi, shape):
    return ((np.asarray(hi).astype(np.uint16) << 8) | np.asarray(lo).astype(np.uint16)).astype("<u2").view("<i2").reshape(shape)


def _noise(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8)


def _smooth(rng, n, values=range(96, 112), maxrun=150):
    """n bytes in runs of 1 .. maxrun - 1 of the given values"""
    k = 4 * n // maxrun + 16
    out = np.repeat(rng.choice(np.array(list(values)), k), rng.integers(1, maxrun, k)).astype(np.uint8)
    assert out.size >= n
    return out[:n]


def _columns(seqs, cx):
    """a tile [ndays][1][len(seqs) * cx] whose chunk c (1 x cx cells, all days) is, in chunk element order, seqs[c]"""
    ndays = seqs[0].size // cx
    img = np.empty((ndays, 1, len(seqs) * cx), "<i2")
    for c, s in enumerate(seqs):
        img[:, 0, c * cx:(c + 1) * cx] = s.reshape(ndays, cx)
    return img


RUN_LENGTHS = (1, 2, 3, 4, 62, 63, 64, 65, 66, 67, 130, 300)
RUN_OFFSETS = (-2, -1, 0, 1, 2)
RUN_N = 13 * dorc.STORED + 405                               # even; multiples 1 .. 12 of 65 535 carry the twelve lengths


def _run_plan(off):
    """[(start, length)] of the runs of the chunk with offset `off`: length i at multiple i + 1 of 65 535, at a multiple of
    16 384 that is no multiple of 65 536 (those lie beside the former) and at a multiple of 64 below 16 384: all 512 and more
    apart"""
    plan = []
    for i, L in enumerate(RUN_LENGTHS):
        plan += [((i + 1) * dorc.STORED + off, L), ((i + 1 + i // 3) * dorc.SEG + off, L), (dorc.PIECE * (8 + 16 * i) + off, L)]
    return plan


def _run_bytes(off):
    """a high plane without any two equal neighbours, then the planned runs written into it (values the background lacks)"""
    hi = ((np.arange(RUN_N, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)
    for k, (s, L) in enumerate(_run_plan(off)):
        hi[s:s + L] = 252 + k % 4
    return hi


def _runs_of(hi):
    """(starts, lengths) of the maximal runs of equal bytes"""
    starts = np.concatenate([[0], np.flatnonzero(np.diff(hi.astype(np.int16)) != 0) + 1])
    return starts, np.diff(np.concatenate([starts, [hi.size]]))


def _geom_steps(cy, cx, vec):
    step = STEP1 * vec
    return step % cx, step // cx % cy, step // cx // cy


@functools.lru_cache(maxsize=None)
def _cases():
    cases = []
    add = lambda *a, **k: cases.append(Case(*a, **k))

    # noise: 2 segments + 100 elements of uniform bytes in both planes
    rng = np.random.default_rng(101)
    n = 2 * dorc.SEG + 100
    add("noise_vec2", _planes(_noise(rng, n), _noise(rng, n), (n // 4, 2, 2)), 2, 2,
        "every high-plane segment stored (df_seg_stored, the early return of k_deflate_emit); length == the bound", needs=("all_stored",))
    add("noise_vec1", _planes(_noise(rng, n), _noise(rng, n), (n, 1, 1)), 1, 1,
        "the same with one value per load", needs=("all_stored",))

    # mixed: smooth, three noise segments, smooth whose first 5 bytes repeat the last noise byte
    for name, shape, cy, cx in (("mixed_vec2", (1280, 8, 8), 8, 8), ("mixed_vec1", (16384, 1, 5), 1, 5)):
        rng = np.random.default_rng(102)
        mid = _noise(rng, 3 * dorc.SEG)
        last = _smooth(rng, dorc.SEG)
        last[:5] = mid[-1]
        last[5] = mid[-1] ^ 1
        hi = np.concatenate([_smooth(rng, dorc.SEG), mid, last])
        add(name, _planes(_noise(rng, hi.size), hi, shape), cy, cx,
            "Huffman and stored blocks in one chunk; a distance-1 match reaching back into a stored block", needs=("mixed_flags",))

    # deep_code: geometric high-byte frequencies -> a Huffman tree deeper than 15
    rng = np.random.default_rng(103)
    p = 0.5 ** np.arange(1, 21)
    p[-1] *= 2
    hi = rng.choice(10 + 5 * np.arange(20), 4096 * 8 * 16, p=p)
    add("deep_code", _planes(_noise(rng, hi.size), hi, (4096, 8, 16)), 4, 8,
        "the halving loop of k_deflate_table (20 values, probabilities 2^-k)", needs=("halving", "multi_chunk"))
    p2 = p
    p = 1.62 ** -np.arange(30.0)
    hi = rng.choice(3 + 7 * np.arange(30), 4096 * 8 * 16, p=p / p.sum())
    add("deep_code_ratio_1_62", _planes(_noise(rng, hi.size), hi, (4096, 8, 16)), 4, 8,
        "the halving loop of k_deflate_table (30 values, ratio 1.62)", needs=("halving", "multi_chunk"))

    rng = np.random.default_rng(104)
    hi = rng.choice(10 + 5 * np.arange(20), 4096 * 16 * 16, p=p2)
    add("deep_code_64_chunks", _planes(_noise(rng, hi.size), hi, (4096, 16, 16)), 2, 2,
        "the same frequencies counted over 64 one-segment chunks (2^20 sampled bytes): the halving loop goes round five times",
        needs=("halving", "halving_repeats", "multi_chunk"))

    # constant images
    for tag, v in (("fill", -32767), ("zero", 0), ("7f7f", 0x7F7F)):
        add("constant_%s_vec2" % tag, np.full((3000, 4, 6), v, "<i2"), 2, 6,
            "one 64-byte match per piece, a one-symbol-dominated code (value %d), 3 segments" % v, needs=("constant", "multi_chunk"))
        add("constant_%s_vec1" % tag, np.full((700, 6, 9), v, "<i2"), 2, 3,
            "the same in one short segment, one value per load", needs=("constant", "multi_chunk"))

    # tiny chunks
    rng = np.random.default_rng(105)
    some = np.array([-32767, 0, 255, 256, 1234, 1235, -1], "<i2")

    def tiny(shape):
        a = rng.integers(-32768, 32768, shape).astype("<i2")
        b = rng.choice(some, shape)
        return np.where(rng.random(shape) < 0.5, a, b)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 67):
        add("tiny_days_%d" % n, tiny((n, 2, 3)), 1, 1, "N = %d as days x 1 x 1, six chunks: a partial first piece, threads without bytes" % n,
            needs=("tiny", "multi_chunk"))
    for n in (1, 2, 32):
        add("tiny_days_%d_vec2" % n, tiny((n, 2, 4)), 1, 2, "N = %d with two values per load" % (2 * n), needs=("tiny", "multi_chunk"))
    for cy, cx in ((1, 1), (1, 3), (3, 1), (5, 1), (1, 5), (7, 9), (9, 7), (5, 13), (13, 5), (1, 67), (67, 1), (1, 2), (2, 2), (8, 8)):
        add("tiny_cells_%dx%d" % (cy, cx), tiny((1, 2 * cy, 3 * cx)), cy, cx, "N = %d as one day of %d x %d cells, six chunks" % (cy * cx, cy, cx),
            needs=("tiny", "multi_chunk"))

    # segment and stored-block boundaries, both load widths, two chunks a tile
    rng = np.random.default_rng(106)
    for n in (16383, 16384, 16385, 65534, 65535, 65536, 131070, 131071, 196608):
        seqs = [_planes(_noise(rng, n), _smooth(rng, n), (n,)) for _ in range(2)]
        add("edges_%d_vec1" % n, _columns(seqs, 1), 1, 1, "N = %d: segment / stored-block boundaries, one value per load" % n,
            needs=("multi_chunk",) + (("boundary_inside",) if n > dorc.STORED else ()))
        if n % 2 == 0:
            needs = ("multi_chunk",) + (("boundary_inside",) if n > dorc.STORED else ()) + (("second_boundary",) if n > 2 * dorc.STORED else ())
            add("edges_%d_vec2" % n, _columns(seqs, 2), 1, 2,
                "N = %d, two values per load: the pair that straddles byte 65 535 (and 196 605), the exact landing on 131 070" % n, needs=needs)

    # runs cut at piece, segment and stored-block ends
    rng = np.random.default_rng(107)
    seqs = [_planes(_noise(rng, RUN_N), _run_bytes(off), (RUN_N,)) for off in RUN_OFFSETS]
    for vec in (1, 2):
        add("runs_vec%d" % vec, _columns(seqs, vec), 1, vec,
            "df_piece<true>: runs of %s bytes starting -2 .. +2 around multiples of 64, 16 384 and 65 535 (chunk c: offset c - 2)" % (RUN_LENGTHS,),
            needs=("runs", "multi_chunk", "boundary_inside"), compare="all")

    # long chunks: the scans of k_deflate_scan beyond one pass
    rng = np.random.default_rng(108)
    nd = 532000
    level = 100 + np.cumsum(rng.integers(-1, 2, nd) * (rng.random(nd) < 0.02)) % 50
    bias = np.repeat(np.repeat(np.array([[0, 1], [2, 3]]), 2, axis=0), 2, axis=1)
    bias[3, 3] += 1                                           # (one cell of the last chunk apart: shorter runs there)
    hi = (level[:, None, None] + bias[None]).astype(np.uint8)
    add("long_adler", _planes(_noise(rng, hi.size).reshape(hi.shape), hi, hi.shape), 2, 2,
        "130 segments a chunk: the second pass of the Adler scan only; 2 x 2 chunks", needs=("nseg_adler", "multi_chunk"), compare="fml")
    for name, n, cx, nch in (("long_scan_vec1", 300 * dorc.SEG - 37, 1, 1), ("long_scan_vec2", 300 * dorc.SEG - 36, 2, 2)):
        seqs = []
        for _ in range(nch):
            h = _smooth(rng, n)
            for s in (0, 100, 101, 257, 299):                 # some segments of noise: stored blocks before and after seg 256
                h[s * dorc.SEG:(s + 1) * dorc.SEG] = _noise(rng, h[s * dorc.SEG:(s + 1) * dorc.SEG].size)
            seqs.append(_planes(_noise(rng, n), h, (n,)))
        add(name, _columns(seqs, cx), 1, cx, "300 segments: the second pass of both scans%s; 75 stored-block boundaries" %
            ("; chunk-indexed offsets at ch > 0" if nch > 1 else ""),
            needs=("nseg_scan", "boundary_inside") + (("multi_chunk", "second_boundary") if nch > 1 else ()), compare="fml")

    # odd geometries: the carried (x, y, day) counters of stage
    rng = np.random.default_rng(109)
    for cy, cx in ((1, 1), (1, 3), (1, 7), (5, 1), (5, 3), (5, 7), (5, 9), (3, 11)):
        nd = 50000 // (cy * cx) + 7
        Y, X = 2 * cy, 3 * cx
        cell = 100 + rng.integers(0, 3, (Y, X))
        day = np.cumsum(rng.integers(-1, 2, nd) * (rng.random(nd) < 0.05)) % 8
        hi = (cell[None] + day[:, None, None]).astype(np.uint8)
        add("odd_geometry_%dx%d" % (cy, cx), _planes(_noise(rng, hi.size).reshape(hi.shape), hi, hi.shape), cy, cx,
            "rows of %d cells, %d rows: step components %s" % (cx, cy, _geom_steps(cy, cx, 1)),
            needs=("multi_chunk", "x_ne_cx") + (("step_all_nonzero",) if all(_geom_steps(cy, cx, 1)) else ()))

    # property run: uniformly random int16 tiles, random shapes and chunkings (the GPU twin of
    # test_deflate_oracle.py::test_property_any_int16_tile_round_trips)
    for i in range(26):
        rng = np.random.default_rng(1100 + i)
        cy, cx = int(rng.integers(1, 7)), (1 if i % 5 == 0 else int(rng.integers(1, 9)))
        ny, nx = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        nd = int(rng.integers(1, max(2, 40000 // (cy * cx))))
        d = rng.integers(-32768, 32768, (nd, ny * cy, nx * cx)).astype("<i2")
        if i >= 20:
            d = np.repeat(d, 3, axis=0)[:nd]                  # (the last six: runs along the day axis, as in the CPU property test)
        add("random_%02d" % i, d, cy, cx, "random int16 tile %s in chunks of %d x %d" % (d.shape, cy, cx), needs=("random",))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def _case(name):
    return {c.name: c for c in _cases()}[name]


NAMES = [c.name for c in _cases()]


@functools.lru_cache(maxsize=None)
def _hist(name):
    c = _case(name)
    return dorc.tile_hist(c.image, c.cy, c.cx)


@functools.lru_cache(maxsize=None)
def _table(name):
    return dorc.make_table(_hist(name))


def _halvings(hist):
    """how often huff_lengths(hist + 1, 15) halves the counts"""
    cnt, k = [int(h) + 1 for h in hist], 0
    while max(dorc.huff_lengths(cnt, 10 ** 9)) > 15:
        cnt, k = [(v + 1) >> 1 for v in cnt], k + 1
    return k


def _stored_flags(chunk, table):
    """per segment of the chunk's high plane: does the restatement store it?"""
    _, hi = dorc.shuffled(chunk)
    return [len(dorc._huffman_block(hi, s0, min(hi.size, s0 + dorc.SEG), table)) > min(hi.size, s0 + dorc.SEG) - s0 + 5
            for s0 in range(0, hi.size, dorc.SEG)]


def _len_symbol(L):
    return 257 + max(j for j, b in enumerate(dorc._LBASE) if b <= L)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_cases_cover_the_table():
    """every row of the case table is there, nothing is filtered by size"""
    for prefix in ("noise", "mixed", "deep_code", "constant", "tiny_days", "tiny_cells", "edges", "runs", "long_adler", "long_scan", "odd_geometry"):
        assert any(n.startswith(prefix) for n in NAMES), prefix
    rnd = [c for c in _cases() if c.name.startswith("random")]
    assert len(rnd) >= 20 and any(c.cx == 1 for c in rnd) and any(c.nchunk > 1 for c in rnd) and any(c.vec == 2 for c in rnd)
    assert {c.N for c in _cases() if c.name.startswith("tiny_days") and c.vec == 1} == {1, 2, 3, 4, 5, 63, 64, 65, 67}
    assert {1, 3, 5, 63, 65, 67} <= {c.N for c in _cases() if c.name.startswith("tiny_cells")}
    for n in (16383, 16384, 16385, 65534, 65535, 65536, 131070, 131071):
        assert _case("edges_%d_vec1" % n).N == n and (n % 2 or _case("edges_%d_vec2" % n).N == n)
    assert {(c.cy, c.cx) for c in _cases() if c.name.startswith("odd_geometry")} >= {(cy, cx) for cy in (1, 5) for cx in (1, 3, 7)}
    needs = {n for c in _cases() for n in c.needs}
    assert needs == {"all_stored", "mixed_flags", "halving", "halving_repeats", "multi_chunk", "constant", "tiny", "boundary_inside", "second_boundary", "runs",
                     "nseg_adler", "nseg_scan", "x_ne_cx", "step_all_nonzero", "random"}
    for need, vec in (("boundary_inside", 1), ("boundary_inside", 2), ("second_boundary", 2), ("all_stored", 1), ("all_stored", 2),
                      ("mixed_flags", 1), ("mixed_flags", 2), ("nseg_scan", 1), ("nseg_scan", 2), ("runs", 1), ("runs", 2)):
        assert any(need in c.needs and c.vec == vec for c in _cases()), (need, vec)
    assert sum("step_all_nonzero" in c.needs for c in _cases()) >= 3


@pytest.mark.parametrize("name", NAMES)
def test_cases_reach_their_paths(name):
    """CPU, restatement only: the precondition that makes the case worth running on the GPU."""
    c = _case(name)
    assert c.needs, name
    for need in c.needs:
        if need == "all_stored":
            for chunk in c.chunks():
                assert all(_stored_flags(chunk, _table(name)))
                assert len(dorc.deflate_chunk(chunk, _table(name))) == _bound(c.N)
            assert c.N != 2 * dorc.SEG + 100 or _bound(c.N) == 65767
        elif need == "mixed_flags":
            assert c.nchunk == 1 and _stored_flags(c.image, _table(name)) == [False, True, True, True, False]
            _, hi = dorc.shuffled(c.image)
            first = dorc.tokens(hi, 4 * dorc.SEG, 4 * dorc.SEG + dorc.PIECE)[0]
            assert first == (_len_symbol(5), 0, 0), first       # the run of 5 begins with a match: its byte is in the stored block
        elif need == "halving":
            k = _halvings(_hist(name))
            assert k >= 1 and max(dorc.huff_lengths([h + 1 for h in _hist(name)], 10 ** 9)) > 15
            assert max(_table(name)[0]) <= 15
        elif need == "halving_repeats":
            assert _halvings(_hist(name)) >= 2                # the loop's own __syncthreads between two rounds
        elif need == "multi_chunk":
            assert c.nchunk >= 2
        elif need == "constant":
            assert c.image.min() == c.image.max()
            h = _hist(name)
            assert h[_len_symbol(64)] > 0 and sum(1 for v in h if v) <= 3
        elif need == "tiny":
            assert c.nseg == 1 and c.N <= 67
        elif need == "boundary_inside":
            assert c.N > dorc.STORED                          # byte 65 535 of the low plane begins a second stored block
        elif need == "second_boundary":
            assert c.vec == 2 and c.N > 2 * dorc.STORED
        elif need == "runs":
            assert c.nchunk == len(RUN_OFFSETS) and c.N == RUN_N
            for chunk, off in zip(c.chunks(), RUN_OFFSETS):
                starts, lengths = _runs_of(dorc.shuffled(chunk)[1])
                for M in (dorc.PIECE, dorc.SEG, dorc.STORED):
                    for L in RUN_LENGTHS:
                        assert ((starts[lengths == L] - off) % M == 0).any(), (M, L, off)
                for s0, L in _run_plan(off):                  # every planned run is there, whole and alone
                    i = int(np.searchsorted(starts, s0))
                    assert starts[i] == s0 and lengths[i] == L, (s0, L, off)
        elif need == "nseg_adler":
            assert 129 <= c.nseg <= 256                       # 2 nseg > 256 >= nseg
        elif need == "nseg_scan":
            assert c.nseg > 256
            flags = _stored_flags(c.chunks()[-1], _table(name))
            assert any(flags[:256]) and any(flags[256:]) and not all(flags[256:])
        elif need == "x_ne_cx":
            assert c.X != c.cx and c.vec == 1
        elif need == "step_all_nonzero":
            assert all(_geom_steps(c.cy, c.cx, c.vec)) and c.N > STEP1
        elif need == "random":
            pass                                              # (counted in test_cases_cover_the_table)
        else:
            raise AssertionError("unknown precondition %s" % need)


def _compile(out_dir):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = os.path.join(str(out_dir), "deflate_probe")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "topowx_amd", "csrc"), SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_deflate_probe_compiles(tmp_path):
    """CPU: the probe (twx_deflate.h exactly as the library includes it) cross-compiles for gfx950."""
    exe = _compile(tmp_path)
    assert os.path.getsize(exe) > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _read_table(raw, at):
    n = dorc.NSYM
    t = {"len": np.frombuffer(raw, np.uint8, n, at), "code": np.frombuffer(raw, "<u2", n, at + n)}
    at += 3 * n
    t["hdr_bits"] = int(np.frombuffer(raw, "<u4", 1, at)[0])
    t["hdr"] = np.frombuffer(raw, "<u4", 80, at + 4)
    return t, at + 4 + 320


def _parse(path, c):
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, "<i8", 8, 0)
    assert head[0] == PROBE_MAGIC
    r = dict(nchunk=int(head[1]), nseg=int(head[2]), slot=int(head[3]), guard=int(head[4]), repeat=int(head[5]), pairs=int(head[6]), N=int(head[7]))
    at = 64
    r["chunk_bytes"] = np.frombuffer(raw, "<i8", r["nchunk"], at)
    at += 8 * r["nchunk"]
    r["hist"] = np.frombuffer(raw, "<u4", dorc.NSYM, at)
    at += 4 * dorc.NSYM
    r["table"], at = _read_table(raw, at)
    r["table_two_groups"], at = _read_table(raw, at)
    r["table_decoy"], at = _read_table(raw, at)
    r["seg_bytes"] = np.frombuffer(raw, "<u4", r["nchunk"] * r["nseg"], at).reshape(r["nchunk"], r["nseg"])
    at += 4 * r["nchunk"] * r["nseg"]
    r["streams"] = []
    for n in r["chunk_bytes"].tolist():
        n = n if 0 <= n <= r["slot"] else 0
        r["streams"].append(raw[at:at + n])
        at += n
    assert at == len(raw), (c.name, at, len(raw))
    return r


_PROBE = {}


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """{case name: the probe's outputs}: one probe process for all cases, run once whatever comes of it"""
    if "error" not in _PROBE:
        _PROBE["error"] = "the probe was not run"
        d = tmp_path_factory.mktemp("deflate_probe")
        exe = _compile(d)
        lines = []
        for c in _cases():
            img, out = str(d / (c.name + ".i16")), str(d / (c.name + ".out"))
            c.image.tofile(img)
            lines.append("%s %d %d %d %d %d %s %s" % (c.name, c.ndays, c.Y, c.X, c.cy, c.cx, img, out))
        manifest = d / "manifest.txt"
        manifest.write_text("\n".join(lines) + "\n")
        try:
            # sized to the manifest: ~150 MB of images read and ~0.5 GB of buffers copied back, kernels of milliseconds
            r = subprocess.run([exe, str(manifest)], capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired as e:
            so = e.stdout or ""
            done = [ln for ln in (so if isinstance(so, str) else so.decode(errors="replace")).split("\n") if ln.startswith("DONE")]
            _PROBE["error"] = "deflate_probe timed out after %d finished cases (last: %s)" % (len(done), done[-1:] or "none")
        else:
            print(r.stdout[-6000:])
            if r.returncode != 0:
                _PROBE["error"] = "deflate_probe exited with %d: %s" % (r.returncode, r.stderr[-2000:])
            else:
                assert r.stdout.strip().endswith("ALL %d" % len(NAMES)), r.stdout[-500:]
                _PROBE["results"] = {c.name: _parse(str(d / (c.name + ".out")), c) for c in _cases()}
                _PROBE["error"] = None
    if _PROBE["error"]:
        pytest.fail(_PROBE["error"])
    return _PROBE["results"]


def _guard_names(mask):
    """the probe's guard mask: bits 0 .. 7 the buffers of run 0, 8 .. 10 the shared ones, 16 .. 23 the buffers of run 1"""
    return [("run 1: " + BUFFERS[b - 16]) if b >= 16 else ("run 0: " if b < 8 else "") + BUFFERS[b] for b in range(24) if mask >> b & 1 and b % 16 < 11]


def _assert_table(t, want, what):
    lens, codes, hdr = want
    n = dorc.NSYM
    assert t["len"][:n].tolist() == lens, what + ": code lengths"
    assert t["code"][:n].tolist() == [int(format(cd, "0%db" % ln)[::-1], 2) for cd, ln in zip(codes, lens)], what + ": codes"
    assert t["hdr_bits"] == hdr.nbits(), what + ": header bits"
    val = int.from_bytes(bytes(hdr.out), "little") | (hdr.acc << (8 * len(hdr.out)))
    assert sum(int(w) << (32 * i) for i, w in enumerate(t["hdr"])) == val, what + ": header bit string"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_kernels_on_the_device(device, name):
    """One case: guard bands, the repeated run, hist, the table (one and two work-groups, the decoy), seg_bytes, chunk_bytes,
    zlib on every chunk, the restatement's bytes -- in the order that localizes a failure (hist: stage / tokenizer; table:
    k_deflate_table; seg_bytes: k_deflate_count; bytes with all of those right: k_deflate_emit / k_deflate_scan).

    Seen on gfx950: all 92 cases equal the restatement byte for byte, bands intact, second run identical; stored segments
    3 of 3 (noise), 3 of 5 (mixed), 159 of 265 (runs), 9 of 520 (long_adler), 5 of 300 / 10 of 600 (long_scan); the tables of
    deep_code (1 halving), deep_code_64_chunks (5) and long_adler (3) equal make_table's.  No kernel was wrong."""
    c, r = _case(name), device[name]
    assert (r["nchunk"], r["nseg"], r["N"], 2 if r["pairs"] else 1) == (c.nchunk, c.nseg, c.N, c.vec)
    assert r["guard"] == 0, "guard bands overwritten: %s" % _guard_names(r["guard"])
    assert r["repeat"] == 0, "a second run differs in: %s" % [BUFFERS[b] for b in range(8) if r["repeat"] >> b & 1]
    assert r["hist"].tolist() == _hist(name), "hist"
    _assert_table(r["table"], _table(name), "table")
    _assert_table(r["table_two_groups"], _table(name), "table built by work-group 1")
    _assert_table(r["table_decoy"], dorc.make_table([0] * dorc.NSYM), "table of work-group 0 (no counts)")
    lo_bytes = c.N + 5 * -(-c.N // dorc.STORED)
    seg_len = [min(dorc.SEG, c.N - s * dorc.SEG) for s in range(c.nseg)]
    chunks = c.chunks()
    stored = 0
    for ch, chunk in enumerate(chunks):
        stream = r["streams"][ch]
        assert int(r["chunk_bytes"][ch]) == len(stream) == 2 + lo_bytes + int(r["seg_bytes"][ch].sum()) + 9, ("chunk_bytes", ch)
        assert len(stream) <= _bound(c.N), ("bound", ch)
        assert all(int(b) <= n + 5 for b, n in zip(r["seg_bytes"][ch], seg_len)), ("seg_bytes", ch)
        stored += sum(int(b) == n + 5 for b, n in zip(r["seg_bytes"][ch], seg_len))
        lo, hi = dorc.shuffled(chunk)
        assert zlib.decompress(stream) == lo.tobytes() + hi.tobytes(), ("inflate", ch)
    print("%s: %d of %d high-plane segments stored" % (name, stored, c.nchunk * c.nseg))
    if "all_stored" in c.needs:
        assert stored == c.nchunk * c.nseg and all(len(s) == _bound(c.N) for s in r["streams"])
    if "mixed_flags" in c.needs:
        assert [int(b) == n + 5 for b, n in zip(r["seg_bytes"][0], seg_len)] == [False, True, True, True, False]
    for ch in c.compared():
        assert r["streams"][ch] == dorc.deflate_chunk(chunks[ch], _table(name)), ("bytes differ from the restatement", ch)
