"""The seeded cases of the series coder's tests (tests/test_series_deflate_host.py, tests/test_gpu_series_deflate.py), each with
the property it exists for.  ``check(case, restated)`` asserts that property on the restatement
(tests/restate_series_deflate.py), on the CPU: a generator that drifts fails there and cannot empty a GPU test.

A case is a dict: ``name``, ``rows`` [nrows, n] (C-contiguous, itemsize 1, 2 or 4: one ``twxsd_deflate`` call) and ``prop``,
one of the names of ``PROPS``."""
import numpy as np
from scipy.signal import lfilter

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 32769, 25203)     # 25 203: the production axis
FILL_F4 = np.float32(9.96921e36)
MISSING = np.float32(-9999.0)
PROPS = ("roundtrip", "all_fill", "all_stored", "no_equal_neighbours", "one_symbol_plane", "runs", "halving", "mixed", "special")


def tenths(rng, nrows, n, gaps=True):
    """Observations in tenths of a degree, AR(1) around a seasonal cycle, with missing stretches (-9999)."""
    t = np.arange(n)
    out = np.empty((nrows, n), np.float32)
    for r in range(nrows):
        x = lfilter([1.0], [1.0, -0.7], rng.standard_normal(n) * 3.0)          # x[i] = 0.7 x[i - 1] + e[i]
        v = np.round((10.0 + 12.0 * np.sin(2 * np.pi * t / 365.25 + r) + x) * 10.0) / 10.0
        out[r] = v.astype(np.float32)
        if gaps:
            for _ in range(1 + n // 4000):
                a = int(rng.integers(0, n))
                out[r, a:a + int(rng.integers(1, max(2, n // 6)))] = MISSING
    return out


def raw_gaps(rng, nrows, n):
    """Raw series with LONG missing stretches: most of a row is -9999."""
    out = tenths(rng, nrows, n, gaps=False)
    for r in range(nrows):
        a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
        keep = np.zeros(n, bool)
        keep[a:b] = True
        if b - a > n // 2:                                   # at least half of every row is missing
            keep[a + n // 4:b] = False
        out[r, ~keep] = MISSING
    return out


def model(rng, nrows, n):
    """Unrounded model values."""
    t = np.arange(n)
    return (10.0 + 12.0 * np.sin(2 * np.pi * t / 365.25)[None, :] + rng.standard_normal((nrows, n)).cumsum(axis=1) * 0.3 +
            rng.standard_normal((nrows, n))).astype(np.float32)


def flags(rng, nrows, n):
    """GHCN quality flags: mostly empty, a few letters."""
    a = np.zeros((nrows, n), np.uint8)
    hit = rng.random((nrows, n)) < 0.03
    a[hit] = rng.choice(np.frombuffer(b"DGIKLMNORSTWXZ", np.uint8), int(hit.sum()))
    return a


def tobs(rng, nrows, n):
    """Times of observation: -1 = none, else hhmm, constant for years."""
    a = np.full((nrows, n), -1, np.int16)
    for r in range(nrows):
        i = int(rng.integers(0, max(1, n // 3)))
        while i < n:
            j = i + int(rng.integers(1, max(2, n // 2)))
            a[r, i:j] = rng.choice(np.array([700, 800, 1700, 1800, 2400], np.int16))
            i = j
    return a


def pool(kind, nrows=16, n=25203):
    """The seeded pools of the size test."""
    rng = np.random.default_rng(dict(tenths=101, raw=102, model=103)[kind])
    return dict(tenths=tenths, raw=raw_gaps, model=model)[kind](rng, nrows, n)


def no_equal_neighbours(nrows, n, dtype):
    """No two neighbouring bytes are equal in any plane: byte i of plane p is (7 i + 3 p + 11 r) mod 251."""
    es = np.dtype(dtype).itemsize
    i = np.arange(n, dtype=np.int64)
    b = np.stack([np.stack([(7 * i + 3 * p + 11 * r) % 251 for p in range(es)], axis=1) for r in range(nrows)]).astype(np.uint8)
    return np.ascontiguousarray(b).view(dtype).reshape(nrows, n)


RUN_LENGTHS = (1, 2, 3, 66, 67, 300)
RUN_DELTAS = (-2, -1, 0, 1, 2)
RUN_BASES = (640, 16384, 32768)
RUN_N = 33169


def runs_rows():
    """uint8 rows without equal neighbours but for runs of every length of RUN_LENGTHS starting at every delta of RUN_DELTAS
    around a multiple of 64 and two multiples of 16 384: a row per (length, delta), the run's byte 253."""
    rows = []
    for length in RUN_LENGTHS:
        for d in RUN_DELTAS:
            row = no_equal_neighbours(1, RUN_N, np.uint8)[0].copy()
            for base in RUN_BASES:
                row[base + d:base + d + length] = 253
            rows.append(row)
    return np.stack(rows)


def halving_rows():
    """An es = 1 pool whose symbol probabilities fall as 2^-k: byte k with probability 2^-(k + 1), k = 0 .. 23, laid out so
    that no two neighbours are equal (the counts are those of the literals), 65 rows of 16 384."""
    rng = np.random.default_rng(7)
    nrows, n = 65, 16384
    k = np.minimum(rng.geometric(0.5, size=(nrows, n)) - 1, 23).astype(np.int64)
    # a byte equal to its predecessor would become part of a run: alternate two alphabets by position parity
    return (k + 100 * (np.arange(n)[None, :] % 2)).astype(np.uint8)


def cases():
    out = []

    def add(name, rows, prop="roundtrip"):
        assert prop in PROPS
        out.append(dict(name=name, rows=np.ascontiguousarray(rows), prop=prop))

    rng = np.random.default_rng(20240229)
    # every size, every element size, two rows: row 1 starts at n * es bytes -- every alignment (odd n for es = 1; n = 1, 2, 3
    # mod 4 for es = 4)
    for n in SIZES:
        add("tenths_n%d" % n, tenths(rng, 2, n))
        add("flags_n%d" % n, flags(rng, 2, n))
        add("tobs_n%d" % n, tobs(rng, 2, n))
    assert {n % 4 for n in SIZES} == {0, 1, 2, 3} and any(n % 2 for n in SIZES)
    # one row; 65 rows: more than one work-group of the row scan, 17 sampled rows
    add("tenths_1row", tenths(rng, 1, 25203))
    add("tenths_65rows", tenths(rng, 65, 257))
    add("flags_65rows", flags(rng, 65, 255))
    add("tobs_65rows", tobs(rng, 65, 65))
    add("model_3rows", model(rng, 3, 25203))
    add("raw_gaps", raw_gaps(rng, 3, 25203))
    # rows that are all fill: runs across pieces and segments
    add("fill_f4", np.full((2, 25203), FILL_F4, np.float32), "all_fill")
    add("fill_i2", np.full((1, 16385), -9999, np.int16), "all_fill")
    add("fill_7f", np.full((2, 32769), 0x7F7F7F7F, np.uint32), "all_fill")
    add("fill_u1", np.full((65, 257), 0x7F, np.uint8), "all_fill")
    # random bits: every block stored, the stream as long as twxsd_bound
    for n, dt, nr in ((1, np.uint8, 1), (2, np.uint16, 2), (3, np.uint32, 2), (63, np.uint8, 2), (64, np.uint32, 2), (65, np.uint16, 2),
                      (16385, np.uint8, 2), (257, np.uint16, 65), (25203, np.uint32, 2), (32769, np.uint32, 1)):
        add("random_%s_n%d" % (np.dtype(dt).name, n), rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), (nr, n), dtype=np.uint64).astype(dt),
            "all_stored")
    # NaN, -0.0, infinities among ordinary values
    sp = tenths(rng, 2, 257, gaps=False)
    sp[0, ::7], sp[0, 1::11], sp[1, ::5], sp[1, 3::13] = np.nan, -0.0, np.inf, -np.inf
    sp[1, 100:140] = np.float32(-0.0)
    add("nan_negzero", sp, "special")
    for dt in (np.uint8, np.uint16, np.uint32):
        add("no_equal_%s" % np.dtype(dt).name, no_equal_neighbours(2, 16385, dt), "no_equal_neighbours")
    add("one_symbol_plane", rng.integers(0, 256, (2, 16384)).astype(np.int16), "one_symbol_plane")
    add("runs", runs_rows(), "runs")
    add("halving", halving_rows(), "halving")
    # a noise row among compressible ones: stored and Huffman blocks side by side in one plane
    mixed = tenths(rng, 5, 25203)
    mixed[2] = rng.integers(0, 1 << 32, 25203, dtype=np.uint64).astype(np.uint32).view(np.float32)
    add("mixed", mixed, "mixed")
    return out


def check(case, R, restated):
    """The property ``case`` exists for, on the restatement ``restated`` = ``R.deflate_call(case['rows'])``."""
    rows, prop = case["rows"], case["prop"]
    nrows, n = rows.shape
    es = rows.dtype.itemsize
    nseg = (n + R.SEG - 1) // R.SEG
    assert restated["blocks"] == nrows * es * nseg and len(restated["streams"]) == nrows
    planes = [R.shuffled(rows[r]) for r in range(nrows)]
    if prop == "all_fill":
        assert all((pl == pl[:, :1]).all() for pl in planes)
        # a block is stored only where its segment is shorter than a block header (the last element of n = 16 385)
        sm = restated["stored_map"]
        assert all(min(n, (k + 1) * R.SEG) - k * R.SEG < 64 for k in range(nseg) if sm[:, :, k].any())
        assert max(len(s) for s in restated["streams"]) < n * es // 10 + 60 * es * nseg
    elif prop == "all_stored":
        assert restated["stored"] == restated["blocks"]
        assert all(len(s) == R.bound(n, es) for s in restated["streams"])
    elif prop == "no_equal_neighbours":
        for pl in planes:
            assert (pl[:, 1:] != pl[:, :-1]).all()
            for p in range(es):
                assert (R.tokens(pl[p], 0, min(n, R.SEG))[0] < 256).all()
    elif prop == "one_symbol_plane":
        assert all((pl[1] == pl[1][0]).all() and np.unique(pl[0]).size > 100 for pl in planes)
    elif prop == "runs":
        assert nrows == len(RUN_LENGTHS) * len(RUN_DELTAS) and n == RUN_N
        k = 0
        for length in RUN_LENGTHS:
            for d in RUN_DELTAS:
                eq = np.nonzero(rows[k, 1:] == rows[k, :-1])[0] + 1
                want = np.concatenate([np.arange(b + d + 1, b + d + length) for b in RUN_BASES]) if length > 1 else np.zeros(0, int)
                assert np.array_equal(eq, want), (length, d)
                k += 1
    elif prop == "halving":
        assert es == 1 and restated["halvings"][0] >= 1
    elif prop == "mixed":
        sm = restated["stored_map"]
        assert any(sm[:, p, :].any() and not sm[:, p, :].all() for p in range(es))
        assert 0 < restated["stored"] < restated["blocks"]
    elif prop == "special":
        assert np.isnan(rows).any() and np.signbit(rows[rows == 0]).any() and np.isinf(rows).any()
