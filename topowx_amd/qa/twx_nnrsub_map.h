// twx_nnrsub_map.h -- the index mapping of twx_nnrsub.hip (step12's reanalysis subsets), shared with a CPU program of the
// tests (tests/tools/nnrsub_hostcheck.cpp): a thread of a product's launch -> (chunk, day, level, row) or (day, level, lat,
// lon), and that tuple -> the offsets into the raw slab and the output.  Plain C++, no device call.
#ifndef TWX_NNRSUB_MAP_H
#define TWX_NNRSUB_MAP_H
#include <stdint.h>

#ifdef __HIPCC__
#define NS_HD __host__ __device__ __forceinline__
#else
#define NS_HD inline
#endif

#define NS_MAX_LEV 32                        // TWXNS_MAX_LEV
#define NS_KIND_LEVELS 0
#define NS_KIND_THICK 1

struct NsShape {
    int64_t nrec, nl, ny, nx;                // the raw slab [nrec][nl][ny][nx]
    int64_t ndays, nlat_out, nlon_out;
};

struct NsProd {
    int32_t kind, conv, nlev;                // nlev: the output's levels (1 for a thickness)
    int32_t lev[NS_MAX_LEV];                 // level indices; a thickness: lev[0] = upper, lev[1] = lower
};

struct NsCell {                              // one float4 of a TILED product: row `row` of chunk (cy, cx) at (day, lev)
    int64_t cy, cx, day;
    int32_t lev, row;
};

NS_HD int64_t ns_nchunk(int64_t n) { return (n + 3) / 4; }

// floats of a product
NS_HD int64_t ns_tiled_size(const NsShape &s, int32_t nlev)
{
    return ns_nchunk(s.nlat_out) * ns_nchunk(s.nlon_out) * s.ndays * (int64_t)nlev * 16;
}

NS_HD int64_t ns_plain_size(const NsShape &s, int32_t nlev) { return s.ndays * (int64_t)nlev * s.nlat_out * s.nlon_out; }

// TILED [cy][cx][day][lev][4][4]: thread t owns the four floats at 4 t .. 4 t + 3; row is the fastest index, so the 64 lanes
// of a wavefront store 1024 contiguous bytes.  False: t is past the product.
NS_HD bool ns_tiled_cell(const NsShape &s, int32_t nlev, int64_t t, NsCell *c)
{
    if (t < 0 || t >= ns_tiled_size(s, nlev) / 4) return false;
    c->row = (int32_t)(t & 3);
    int64_t r = t >> 2;
    c->lev = (int32_t)(r % nlev);
    r /= nlev;
    c->day = r % s.ndays;
    r /= s.ndays;
    const int64_t ncx = ns_nchunk(s.nlon_out);
    c->cx = r % ncx;
    c->cy = r / ncx;
    return true;
}

NS_HD int64_t ns_tiled_offset(const NsShape &s, int32_t nlev, const NsCell &c)
{
    return ((((c.cy * ns_nchunk(s.nlon_out) + c.cx) * s.ndays + c.day) * nlev + c.lev) * 4 + c.row) * 4;
}

// PLAIN [day][lev][lat][lon]: thread t owns element t.  False: t is past the product.
NS_HD bool ns_plain_cell(const NsShape &s, int32_t nlev, int64_t t, int64_t *day, int32_t *lev, int64_t *lat, int64_t *lon)
{
    if (t < 0 || t >= ns_plain_size(s, nlev)) return false;
    *lon = t % s.nlon_out;
    int64_t r = t / s.nlon_out;
    *lat = r % s.nlat_out;
    r /= s.nlat_out;
    *lev = (int32_t)(r % nlev);
    *day = r / nlev;
    return true;
}

// the raw datum of (record, level index, raw row, raw column); the caller has checked every index against the slab
NS_HD int64_t ns_raw_offset(const NsShape &s, int64_t rec, int64_t lev, int64_t y, int64_t x)
{
    return ((rec * s.nl + lev) * s.ny + y) * s.nx + x;
}

#endif
