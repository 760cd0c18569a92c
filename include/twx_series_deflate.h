/* twx_series_deflate.h -- libtwxqa.so: the stored bytes of the (ndays, 1) chunks of a station database, formed on the GPU
 * (topowx_amd/qa/twxsd_serdeflate.hip).  The unit has a header of its own, and topowx_amd/series_deflate.py binds its two
 * entries. */
#ifndef TWX_SERIES_DEFLATE_H
#define TWX_SERIES_DEFLATE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the reference stores every (time, station_id) variable of its station databases with zlib=True, chunksizes=(ndays, 1)
 * (twx/db/create_db_all_stations.py:307-311, 399-435): a chunk is the shuffled and deflated series of one station.  These
 * entries turn station-major rows into those chunk bytes.
 *
 * A row has n elements of es bytes, es = 1, 2 or 4.  Its chunk is the es * n bytes of HDF5's shuffle: plane p is byte p of
 * every element, planes in order 0 .. es - 1.  The stream (RFC 1950 / 1951; any inflate reads it):
 *     78 01
 *     for every plane ceil(n / 16384) blocks of at most 16 384 input bytes, whichever of these is shorter:
 *         a dynamic-Huffman block (header, tokens, end-of-block, then an empty stored block 00 00 00 FF FF: byte-aligned), or
 *         a stored block 00 LEN ~LEN data
 *     01 00 00 FF FF, the Adler-32 of the es * n bytes (big endian)
 * Tokens are those of topowx_amd/csrc/twx_deflate.h (df_piece / df_step_tokens): pieces of 64 bytes, a literal or a match of
 * length 3 .. 64 at distance 1; the byte before a plane's first byte counts as "none".  ONE Huffman code per (call, plane),
 * from the token counts (+ 1 per symbol, integer atomics) of segment s of row r of that plane for every s % 16 == 0 and
 * r % 4 == 0 (rows counted within the call).  No float arithmetic: two calls give the same bytes. ---- */
#define TWXSD_NKERNELS 4                /* kernel groups timed: histogram + tables; count pass; row scan; emit pass */
#define TWXSD_NTIMES 6                  /* kernel_ms: the groups, then upload and download in host-clock milliseconds */
#define TWXSD_OK 0
#define TWXSD_E_CAP 2                   /* the packed streams need more than out_cap bytes: counts[TWXSD_C_BYTES_OUT] is the size needed */
#define TWXSD_C_BLOCKS 0                /* counts: blocks of the call (nrows * es * ceil(n / 16384)) */
#define TWXSD_C_STORED 1                /*   ... of these, stored blocks */
#define TWXSD_C_HALVINGS 2              /*   [2 .. 5]: times the counts of plane 0 .. 3's code were halved (0 for a plane >= es) */
#define TWXSD_C_BYTES_IN 6              /*   nrows * n * es */
#define TWXSD_C_BYTES_OUT 7             /*   bytes of the packed streams = offsets[nrows] */
#define TWXSD_C_N 8

/* The longest stream of a row: 2 + es * (n + 5 * ceil(n / 16384)) + 9.  Pure host.  -1 for a bad argument (es not 1, 2, 4;
 * n < 1; es * n >= 2^31). */
int64_t twxsd_bound(int64_t n, int32_t es);

/*
 * rows: host pointer to [nrows][n] contiguous elements of es bytes.  Row r's stream is out[offsets[r] : offsets[r + 1]];
 * offsets [nrows + 1]; counts [TWXSD_C_N]; kernel_ms (optional) [TWXSD_NTIMES].  The streams are formed and packed on the
 * device and come out in ONE transfer.  Returns TWXSD_OK; TWXSD_E_CAP when the packed size exceeds out_cap -- the message
 * names the size needed, offsets and counts are complete, nothing is written to out; -1 for any other failure.  Every
 * argument is checked before anything touches the device: es, n >= 1, es * n < 2^31, nrows >= 0 (and nrows * ceil(n / 16384)
 * < 2^31), non-null pointers, out_cap >= 0.  nrows = 0 succeeds with offsets[0] = 0.
 */
int twxsd_deflate(int device, const void *rows, int64_t nrows, int64_t n, int32_t es, uint8_t *out, int64_t out_cap,
                  int64_t *offsets, int64_t *counts, float *kernel_ms, char *errbuf, int errlen);

#ifdef __cplusplus
}
#endif
#endif
