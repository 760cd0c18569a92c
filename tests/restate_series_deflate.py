"""CPU restatement of topowx_amd/qa/twxsd_serdeflate.hip -- TEST INFRASTRUCTURE ONLY: the stored bytes of the ``(ndays, 1)``
chunks of a station database as the GPU forms them, byte for byte (include/twx_series_deflate.h states the format).

A row of ``n`` elements of ``es`` bytes is shuffled into ``es`` planes.  The stream is ``78 01``; for every plane
``ceil(n / 16384)`` blocks, each a dynamic-Huffman block closed by end-of-block and an empty stored block, or a stored block
when that is shorter (``df_seg_stored``); ``01 00 00 FF FF``; the Adler-32.  Tokens are those of ``oracle/deflate_oracle.py``
(pieces of 64 bytes, literal or match(3 .. 64, distance 1)), with the byte before a plane's first byte counting as "none".
ONE code per (call, plane): ``deflate_oracle.make_table`` over the token counts of segment s of row r for s % 16 == 0 and
r % 4 == 0.  Parity is pinned twice, as for the int16 coder: ``zlib.decompress`` of every stream is the shuffled row (no
restatement involved), and the GPU's bytes equal these.

The tokens and the bit strings are formed with numpy (a pool of the size test holds millions of bytes); a test compares them
with the oracle's plain loops on small rows."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import deflate_oracle as DO  # noqa: E402

PIECE, SEG, NSYM = DO.PIECE, DO.SEG, DO.NSYM
SAMPLE_SEG, SAMPLE_ROW = 16, 4                       # TWXSD_SAMPLE_SEG, TWXSD_SAMPLE_ROW

# the length symbol, extra bits and their number of a match of L bytes (RFC 1951 3.2.5), L = 3 .. 66
_LSYM = np.zeros(67, np.int64)
_LEXT = np.zeros(67, np.int64)
_LNE = np.zeros(67, np.int64)
for _L in range(3, 67):
    _k = max(j for j, b in enumerate(DO._LBASE) if b <= _L)
    _LSYM[_L], _LEXT[_L], _LNE[_L] = 257 + _k, _L - DO._LBASE[_k], DO._LEXTRA[_k]


def bound(n, es):
    """``twxsd_bound``: the longest stream of a row; -1 for a bad argument."""
    if es not in (1, 2, 4) or n < 1 or es * n >= 1 << 31:
        return -1
    return 2 + es * (n + 5 * ((n + SEG - 1) // SEG)) + 9


def shuffled(row):
    """HDF5's shuffle of one row: uint8 [es, n], plane p = byte p of every element."""
    a = np.ascontiguousarray(row).reshape(-1)
    return np.ascontiguousarray(a.view(np.uint8).reshape(a.size, a.dtype.itemsize).T)


def tokens(plane, start, stop):
    """(symbol, extra, number of extra bits) arrays of plane[start:stop] (start a multiple of 64): what
    ``deflate_oracle.tokens`` gives, without the loops."""
    b = plane[start:stop].astype(np.int64)
    n = b.size
    prev = np.empty(n, np.int64)
    prev[0] = int(plane[start - 1]) if start > 0 else 256
    prev[1:] = b[:-1]
    eq = b == prev                                   # the byte extends (or, at the start of a piece, opens) a run
    idx = np.arange(n)
    first = eq & ((idx % PIECE == 0) | ~np.concatenate([[False], eq[:-1]]))
    rid = np.cumsum(first) - 1
    rlen = np.bincount(rid[eq], minlength=max(int(first.sum()), 1))
    runlen = np.where(eq, rlen[np.maximum(rid, 0)], 0)
    match = first & (runlen >= 3)
    keep = ~eq | (runlen < 3) | match                # a run of 1 or 2 is literals; a longer one is ONE match at its first byte
    sym = np.where(match, _LSYM[np.minimum(runlen, 66)], b)[keep]
    rl = np.minimum(runlen, 66)[keep]
    m = match[keep]
    return sym, np.where(m, _LEXT[rl], 0), np.where(m, _LNE[rl], 0)


def sampled(row, seg):
    return row % SAMPLE_ROW == 0 and seg % SAMPLE_SEG == 0


def call_hist(planes):
    """planes: [nrows][es, n] -> token counts [es][NSYM] of the sampled (row, segment) items."""
    es, n = planes[0].shape
    hist = np.zeros((es, NSYM), np.int64)
    for r in range(0, len(planes), SAMPLE_ROW):
        for s0 in range(0, n, SEG * SAMPLE_SEG):
            for p in range(es):
                hist[p] += np.bincount(tokens(planes[r][p], s0, min(n, s0 + SEG))[0], minlength=NSYM)
    return hist


def halvings(hist):
    """How often ``deflate_oracle.huff_lengths`` halves the counts before the code fits 15 bits."""
    count, k = [int(h) + 1 for h in hist], 0
    while max(DO.huff_lengths(count, 1 << 30)) > 15:
        count, k = [(c + 1) >> 1 for c in count], k + 1
    return k


class Table(object):
    """A plane's code: ``deflate_oracle.make_table`` and what the bit strings need of it."""

    def __init__(self, hist):
        self.lens, self.codes, hdr = DO.make_table(hist)
        self.halvings = halvings(hist)
        self.len = np.array(self.lens, np.int64)
        self.rev = np.array([int(format(c, "0%db" % ln)[::-1], 2) for c, ln in zip(self.codes, self.lens)], np.int64)
        self.hdr_nbits = hdr.nbits()
        v = int.from_bytes(bytes(hdr.out), "little") | (hdr.acc << (8 * len(hdr.out)))
        self.hdr_bits = np.array([(v >> i) & 1 for i in range(self.hdr_nbits)], np.uint8)


def _bits(values, nbits, width=24):
    sel = np.arange(width)
    return ((values[:, None] >> sel) & 1).astype(np.uint8)[sel < nbits[:, None]]


def block(plane, start, stop, table):
    """(bytes, stored?) of the block of plane[start:stop]."""
    sym, ext, ne = tokens(plane, start, stop)
    ln = table.len[sym]
    val = table.rev[sym] | (ext << ln)               # code, extra bits, then the distance code (one 0 bit) of a match
    nb = ln + ne + (sym > 256)
    eob = np.array([(int(table.rev[256]) >> i) & 1 for i in range(int(table.len[256]))] + [0, 0, 0], np.uint8)
    bits = np.concatenate([table.hdr_bits, _bits(val, nb), eob])
    huff = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
    m = stop - start
    assert len(huff) == (table.hdr_nbits + int(nb.sum()) + int(table.len[256]) + 3 + 7) // 8 + 4      # df_huff_bytes
    if len(huff) > m + 5:
        return bytes([0, m & 255, m >> 8, ~m & 255, (~m >> 8) & 255]) + plane[start:stop].tobytes(), True
    return huff, False


def deflate_call(rows):
    """What one ``twxsd_deflate`` call gives for ``rows`` [nrows, n]: a dict of ``streams`` (list of bytes), ``blocks``,
    ``stored``, ``halvings`` [4], ``stored_map`` [nrows, es, nseg] bool and ``tables``."""
    rows = np.ascontiguousarray(rows)
    assert rows.ndim == 2 and rows.dtype.itemsize in (1, 2, 4) and rows.shape[1] >= 1
    nrows, n = rows.shape
    es, nseg = rows.dtype.itemsize, (n + SEG - 1) // SEG
    out = dict(streams=[], blocks=nrows * es * nseg, stored=0, halvings=[0, 0, 0, 0], stored_map=np.zeros((nrows, es, nseg), bool),
               tables=[])
    if nrows == 0:
        return out
    planes = [shuffled(rows[r]) for r in range(nrows)]
    tables = [Table(h) for h in call_hist(planes)]
    out["tables"] = tables
    out["halvings"][:es] = [t.halvings for t in tables]
    for r in range(nrows):
        s = bytearray(b"\x78\x01")
        for p in range(es):
            for k in range(nseg):
                blk, st = block(planes[r][p], k * SEG, min(n, (k + 1) * SEG), tables[p])
                s += blk
                out["stored_map"][r, p, k] = st
        s += b"\x01\x00\x00\xff\xff" + zlib.adler32(planes[r].tobytes()).to_bytes(4, "big")
        out["streams"].append(bytes(s))
    out["stored"] = int(out["stored_map"].sum())
    return out


def deflate_batched(rows, batch_rows):
    """The streams of ``rows`` deflated in calls of at most ``batch_rows`` rows (a code per call)."""
    streams = []
    for i0 in range(0, rows.shape[0], batch_rows):
        streams += deflate_call(rows[i0:i0 + batch_rows])["streams"]
    return streams


def inflate_row(stream, dtype, n):
    """The row a reader gets: inflate, unshuffle."""
    dt = np.dtype(dtype)
    raw = np.frombuffer(zlib.decompress(stream), np.uint8)
    assert raw.size == n * dt.itemsize
    return np.ascontiguousarray(raw.reshape(dt.itemsize, n).T).view(dt).reshape(n)
