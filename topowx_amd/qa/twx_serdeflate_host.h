// twx_serdeflate_host.h -- the host-side arithmetic of the series coder (twxsd_serdeflate.hip, twxsd_* of
// include/twx_series_deflate.h): the longest stream of a row, block counts, the sampling rule of the histogram, workspace sizes,
// the row offsets and the argument checks.  Plain C++ without HIP, so that tests/tools/serdeflate_hostcheck.cpp runs it under
// the address and undefined-behaviour sanitizers as a program of its own.
//
// The coder's constants are those of topowx_amd/csrc/twx_deflate.h, restated here (twxsd_serdeflate.hip pins them to the coder's
// with static_asserts).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TWXSD_HD __host__ __device__
#else
#define TWXSD_HD
#endif

#define TWXSD_SEG 16384                    // TWX_DF_SEG: input bytes of one block = elements of one segment of a row
#define TWXSD_THREADS 256                  // TWX_DF_THREADS
#define TWXSD_NSYM 277                     // TWX_DF_NSYM
#define TWXSD_SAMPLE_SEG 16                // the histogram counts segment s of row r iff s % 16 == 0 and r % 4 == 0
#define TWXSD_SAMPLE_ROW 4
#define TWXSD_MAX_GRID 2147483647LL        // (row, segment) items are the x dimension of the grids

TWXSD_HD inline bool sd_es_ok(int64_t es) { return es == 1 || es == 2 || es == 4; }
TWXSD_HD inline int64_t sd_nseg(int64_t n) { return (n + TWXSD_SEG - 1) / TWXSD_SEG; }
TWXSD_HD inline int64_t sd_seg_len(int64_t n, int64_t seg) { const int64_t l = n - seg * TWXSD_SEG; return l < TWXSD_SEG ? l : TWXSD_SEG; }
TWXSD_HD inline bool sd_sampled(int64_t row, int64_t seg) { return row % TWXSD_SAMPLE_ROW == 0 && seg % TWXSD_SAMPLE_SEG == 0; }
inline int64_t sd_round256(int64_t b) { return (b + 255) / 256 * 256; }

// the longest stream of a row of n elements of es bytes (every block stored); -1 for a bad argument
inline int64_t sd_bound(int64_t n, int64_t es)
{
    if (!sd_es_ok(es) || n < 1 || n > (((int64_t)1 << 31) - 1) / es) return -1;
    return 2 + es * (n + 5 * sd_nseg(n)) + 9;
}

// elements handled one by one before the first 16-byte unit of a segment that starts at byte address `addr` (at most len)
TWXSD_HD inline int sd_head(uint64_t addr, int es, int len)
{
    const int h = (int)(((16u - (unsigned)(addr & 15u)) & 15u) / (unsigned)es);
    return h < len ? h : len;
}

struct SdDims {
    int64_t nrows, n;
    int32_t es;
    int64_t nseg;                          // segments of a row = blocks of one plane
    int64_t nblk;                          // blocks of a row: es * nseg
    int64_t items;                         // (row, segment) work items: nrows * nseg
    int64_t bound;                         // sd_bound
    int64_t in_bytes;
    int64_t work_bytes;                    // the workspace between the passes (table_bytes = sizeof(DfTable) of the coder)
};

// nullptr, or what is wrong with the arguments
inline const char *sd_dims(int64_t nrows, int64_t n, int64_t es, int64_t table_bytes, SdDims *out)
{
    if (!sd_es_ok(es)) return "es must be 1, 2 or 4";
    if (n < 1) return "n must be at least 1";
    if (n > (((int64_t)1 << 31) - 1) / es) return "es * n must be below 2^31";
    if (nrows < 0) return "nrows must not be negative";
    SdDims d{};
    d.nrows = nrows; d.n = n; d.es = (int32_t)es;
    d.nseg = sd_nseg(n); d.nblk = es * d.nseg; d.bound = sd_bound(n, es);
    if (nrows > TWXSD_MAX_GRID / d.nseg) return "more (row, segment) items than 2^31 - 1: deflate in batches";
    if (nrows > ((int64_t)1 << 46) / (n * es)) return "rows of more than 2^46 bytes: deflate in batches";
    d.items = nrows * d.nseg;
    d.in_bytes = nrows * n * es;
    const int64_t per = nrows * d.nblk;
    // seg_bytes, seg_off (u32), adl (2 u32), piece_bits (256 u16) per block; row_bytes, row offsets (i64), row Adler (u32) per row;
    // hist and table per plane; the counters (stored blocks, halvings per plane)
    d.work_bytes = sd_round256(per * 4) * 2 + sd_round256(per * 8) + sd_round256(per * TWXSD_THREADS * 2) + sd_round256(nrows * 8) +
                   sd_round256((nrows + 1) * 8) + sd_round256(nrows * 4) + sd_round256(es * TWXSD_NSYM * 4) +
                   sd_round256(es * table_bytes) + 256;
    *out = d;
    return nullptr;
}

// offsets [nrows + 1] of the packed streams from their sizes (exclusive scan); a size outside 12 .. bound is refused
inline const char *sd_offsets(const int64_t *row_bytes, int64_t nrows, int64_t bound, int64_t *offset)
{
    int64_t o = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        if (row_bytes[r] < 12 || row_bytes[r] > bound) return "a deflated row has an impossible size";
        offset[r] = o;
        o += row_bytes[r];
    }
    offset[nrows] = o;
    return nullptr;
}
