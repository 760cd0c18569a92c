// twx_mosaic_host.h -- the host-side arithmetic of the mosaic unit (twx_mosaic.hip, twxmo_* of include/twx_qa.h): padded sizes,
// slot sizes, the order of the chunks, the offsets of the compaction and the argument checks.  Plain C++ without HIP, so that
// tests/tools/mosaic_hostcheck.cpp runs it under the address and undefined-behaviour sanitizers as a program of its own.
//
// The chunk slots are those of topowx_amd/csrc/twx_deflate.h for a chunk whose time extent is one day; its constants are
// restated here (twx_mosaic.hip pins them to the coder's with static_asserts, and compares the slot size at run time).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TWXMO_HD __host__ __device__
#else
#define TWXMO_HD
#endif

#define TWXMO_DF_SEG 16384                 // TWX_DF_SEG: input bytes of one high-plane block
#define TWXMO_DF_STORED 65535              // TWX_DF_STORED: bytes of one stored block of the low plane
#define TWXMO_DF_THREADS 256               // TWX_DF_THREADS
#define TWXMO_DF_NSYM 277                  // TWX_DF_NSYM
#define TWXMO_MONTHS 12
#define TWXMO_MAX_GRID_X 2147483647LL      // chunks are the x dimension of the coder's grids
#define TWXMO_MAX_GRID_Y 65535LL           // segments of a chunk their y dimension

struct MoDims {
    int64_t max_days;
    int32_t Y, X, cy, cx;
    int32_t Yp, Xp;                        // Y, X rounded up to whole chunks: the image is int16 [layers][Yp][Xp]
    int32_t ncy, ncx, nchunk;              // chunks of one layer, row-major
    int32_t nseg, vec;                     // high-plane blocks per chunk; values per load of the coder's gather (2: cx and Xp even)
    int64_t N;                             // values per chunk
    int64_t lo_bytes, slot_bytes;          // bytes of the low plane's stored blocks; of a chunk's slot (the longest stream, to 256)
    int64_t layers;                        // layers the workspace serves: max(max_days, 12) -- the monthly image has 12
    int64_t image_bytes, mthly_bytes, slots_bytes, small_bytes, table_bytes, device_bytes;
};

inline int64_t mo_lo_bytes(int64_t N) { return N + 5 * ((N + TWXMO_DF_STORED - 1) / TWXMO_DF_STORED); }
inline int64_t mo_nseg(int64_t N) { return (N + TWXMO_DF_SEG - 1) / TWXMO_DF_SEG; }
inline int64_t mo_slot_bytes(int64_t N) { return (2 + mo_lo_bytes(N) + mo_nseg(N) * (TWXMO_DF_SEG + 5) + 9 + 255) / 256 * 256; }
inline int64_t mo_round256(int64_t b) { return (b + 255) / 256 * 256; }

// Sizes of a mosaic object; nullptr, or what is wrong with the arguments.  table_bytes = sizeof(DfTable) of the coder.
inline const char *mo_dims(int64_t max_days, int64_t Y, int64_t X, int64_t cy, int64_t cx, int64_t table_bytes, MoDims *out)
{
    if (max_days < 1 || max_days > 1000000) return "max_days must be 1 .. 1 000 000";
    if (Y < 1 || X < 1 || Y > (1 << 24) || X > (1 << 24)) return "Y and X must be 1 .. 2^24";
    if (cy < 1 || cx < 1 || cy > Y || cx > X) return "the chunk must be at least 1 x 1 and no larger than the mosaic";
    MoDims d{};
    d.max_days = max_days; d.Y = (int32_t)Y; d.X = (int32_t)X; d.cy = (int32_t)cy; d.cx = (int32_t)cx;
    const int64_t ncy = (Y + cy - 1) / cy, ncx = (X + cx - 1) / cx;
    const int64_t Yp = ncy * cy, Xp = ncx * cx;
    d.layers = max_days > TWXMO_MONTHS ? max_days : TWXMO_MONTHS;
    d.N = cy * cx;
    if (mo_slot_bytes(d.N) >= (int64_t)1 << 32) return "a chunk of more than 2^31 values";
    if (mo_nseg(d.N) > TWXMO_MAX_GRID_Y) return "a chunk of more than 65 535 blocks";
    // (products are formed only after a division has shown that they fit: ncy, ncx <= 2^24, Yp, Xp < 2^25)
    if (d.layers > TWXMO_MAX_GRID_X / (ncy * ncx)) return "more chunks than the grid's x dimension holds";
    if (d.layers * Yp > TWXMO_MAX_GRID_X) return "more image rows than 2^31";
    if (d.layers > ((int64_t)1 << 46) / (Yp * Xp)) return "an image of more than 2^46 values";
    if (d.layers * ncy * ncx > ((int64_t)1 << 50) / mo_slot_bytes(d.N)) return "chunk slots of more than 2^50 bytes";
    d.Yp = (int32_t)Yp; d.Xp = (int32_t)Xp; d.ncy = (int32_t)ncy; d.ncx = (int32_t)ncx; d.nchunk = (int32_t)(ncy * ncx);
    d.nseg = (int32_t)mo_nseg(d.N);
    d.vec = (cx % 2 == 0 && Xp % 2 == 0) ? 2 : 1;
    d.lo_bytes = mo_lo_bytes(d.N); d.slot_bytes = mo_slot_bytes(d.N);
    const int64_t nslot = d.layers * d.nchunk, per = nslot * d.nseg;
    d.image_bytes = mo_round256(max_days * Yp * Xp * 2);
    d.mthly_bytes = mo_round256((int64_t)TWXMO_MONTHS * Yp * Xp * 2);
    d.slots_bytes = nslot * d.slot_bytes + 256;                            // (+ 256: the compaction reads whole words)
    // seg_bytes, seg_off (u32), adl (4 u32), piece_bits (256 u16) per block; chunk_bytes, offsets (i64) per chunk; hist; table
    d.small_bytes = mo_round256(per * 4) * 2 + mo_round256(per * 16) + mo_round256(per * TWXMO_DF_THREADS * 2) +
                    mo_round256(nslot * 8) + mo_round256((nslot + 1) * 8) + mo_round256(TWXMO_DF_NSYM * 4) + mo_round256(table_bytes);
    d.table_bytes = table_bytes;
    d.device_bytes = d.image_bytes + d.mthly_bytes + d.slots_bytes + d.small_bytes;
    *out = d;
    return nullptr;
}

// a slab int16 [nd][ty][tx] placed at (y0, x0) of layers 0 .. nd - 1: refused, not clipped, when any of it lies outside
inline const char *mo_check_place(const MoDims &d, int64_t nd, int64_t ty, int64_t tx, int64_t y0, int64_t x0)
{
    if (nd < 1 || ty < 1 || tx < 1) return "an empty slab";
    if (nd > d.max_days) return "more days than the mosaic object holds";
    if (y0 < 0 || x0 < 0 || ty > d.Y || tx > d.X || y0 > d.Y - ty || x0 > d.X - tx) return "the slab lies outside the mosaic";
    return nullptr;
}

// stream k of a call over `layers` layers is (layer, chunk row, chunk column) in row-major order: the order of the file
inline void mo_chunk_origin(const MoDims &d, int64_t k, int64_t *layer, int64_t *r0, int64_t *c0)
{
    *layer = k / d.nchunk;
    const int64_t ch = k % d.nchunk;
    *r0 = ch / d.ncx * d.cy;
    *c0 = ch % d.ncx * d.cx;
}

// offsets [n + 1] of the compacted streams from their sizes (exclusive scan); a size outside 1 .. slot_bytes is refused
inline const char *mo_offsets(const int64_t *chunk_bytes, int64_t n, int64_t slot_bytes, int64_t *offset)
{
    int64_t o = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (chunk_bytes[k] < 1 || chunk_bytes[k] > slot_bytes) return "a deflated chunk has an impossible size";
        offset[k] = o;
        o += chunk_bytes[k];
    }
    offset[n] = o;
    return nullptr;
}

// widest copy unit (int16 values: 8, 4, 2 or 1) at which a row copied from element address sa to element address da can use
// aligned loads AND aligned stores after a scalar head: the two addresses must agree modulo the unit
TWXMO_HD inline int mo_copy_width(uint64_t sa, uint64_t da)
{
    const unsigned diff = (unsigned)((sa - da) & 7u);
    return diff == 0 ? 8 : (diff & 3u) == 0 ? 4 : (diff & 1u) == 0 ? 2 : 1;
}
// scalar values before the first aligned unit of width w at element address da (at most n)
TWXMO_HD inline int mo_copy_head(uint64_t da, int w, int n)
{
    const int h = (int)(((uint64_t)w - da % (uint64_t)w) % (uint64_t)w);
    return h < n ? h : n;
}
