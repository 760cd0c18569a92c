// nnrsub_hostcheck -- the index mapping of twx_nnrsub.hip (twx_nnrsub_map.h) on the CPU, as a program of its own, built
// by tests/test_nnrsub_host.py with -fsanitize=address,undefined.
//
//   nnrsub_hostcheck NDAYS NLEV NLAT NLON
//
// Walks every thread of a TILED and of a PLAIN launch of one product, and 300 threads past each end, as the kernels do:
// the cell of the thread, its output offset, the raw offsets it gathers from (through descending index lists), reading and
// writing real buffers of exactly the sizes the library allocates, so that an offset outside one is a sanitizer report.
// Checks: every output element is owned exactly once; a TILED thread's offset is 4 t; the padding of edge chunks is where
// the layout says and nowhere else; TILED and PLAIN hold the same datum for the same (day, level, lat, lon).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "twx_nnrsub_map.h"

#define REQUIRE(c)                                                                                   \
    do {                                                                                             \
        if (!(c)) { fprintf(stderr, "nnrsub_hostcheck: %s fails (line %d)\n", #c, __LINE__); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: nnrsub_hostcheck NDAYS NLEV NLAT NLON\n"); return 2; }
    NsShape s;
    const int32_t nlev = atoi(argv[2]);
    s.ndays = atoll(argv[1]), s.nlat_out = atoll(argv[3]), s.nlon_out = atoll(argv[4]);
    s.nrec = s.ndays + 1, s.nl = nlev + 1, s.ny = s.nlat_out + 2, s.nx = s.nlon_out + 3;
    REQUIRE(s.ndays >= 1 && nlev >= 1 && nlev <= NS_MAX_LEV && s.nlat_out >= 1 && s.nlon_out >= 1);
    std::vector<int32_t> raw((size_t)(s.nrec * s.nl * s.ny * s.nx));
    for (size_t i = 0; i < raw.size(); ++i) raw[i] = (int32_t)i;
    std::vector<int32_t> lat_idx((size_t)s.nlat_out), lon_idx((size_t)s.nlon_out), day_rec((size_t)s.ndays), lev((size_t)nlev);
    for (int64_t i = 0; i < s.nlat_out; ++i) lat_idx[(size_t)i] = (int32_t)(s.ny - 1 - i);
    for (int64_t i = 0; i < s.nlon_out; ++i) lon_idx[(size_t)i] = (int32_t)(s.nx - 1 - i - (i & 1));   // falling, with gaps and repeats
    for (int64_t d = 0; d < s.ndays; ++d) day_rec[(size_t)d] = (int32_t)(s.nrec - 1 - d);
    for (int32_t l = 0; l < nlev; ++l) lev[(size_t)l] = nlev - l;
    const int32_t PAD = -1;

    const int64_t ntiled = ns_tiled_size(s, nlev), nplain = ns_plain_size(s, nlev);
    REQUIRE(ntiled % 16 == 0 && ntiled >= nplain);
    std::vector<int32_t> tiled((size_t)ntiled, -7), plain((size_t)nplain, -7);
    std::vector<uint8_t> own_t((size_t)ntiled, 0), own_p((size_t)nplain, 0);
    for (int64_t t = -3; t < ntiled / 4 + 300; ++t) {
        NsCell c;
        if (!ns_tiled_cell(s, nlev, t, &c)) {
            REQUIRE(t < 0 || t >= ntiled / 4);
            continue;
        }
        REQUIRE(t >= 0 && t < ntiled / 4);
        const int64_t off = ns_tiled_offset(s, nlev, c);
        REQUIRE(off == 4 * t && c.row >= 0 && c.row < 4 && c.lev >= 0 && c.lev < nlev && c.day >= 0 && c.day < s.ndays);
        REQUIRE(c.cy >= 0 && c.cy < ns_nchunk(s.nlat_out) && c.cx >= 0 && c.cx < ns_nchunk(s.nlon_out));
        const int64_t lat = c.cy * 4 + c.row;
        for (int k = 0; k < 4; ++k) {
            const int64_t lon = c.cx * 4 + k;
            int32_t v = PAD;
            if (lat < s.nlat_out && lon < s.nlon_out)
                v = raw.at((size_t)ns_raw_offset(s, day_rec[(size_t)c.day], lev[(size_t)c.lev], lat_idx.at((size_t)lat), lon_idx.at((size_t)lon)));
            tiled.at((size_t)(off + k)) = v;
            ++own_t.at((size_t)(off + k));
        }
    }
    for (int64_t t = -3; t < nplain + 300; ++t) {
        int64_t day = 0, lat = 0, lon = 0;
        int32_t l = 0;
        if (!ns_plain_cell(s, nlev, t, &day, &l, &lat, &lon)) {
            REQUIRE(t < 0 || t >= nplain);
            continue;
        }
        REQUIRE(day >= 0 && day < s.ndays && l >= 0 && l < nlev && lat >= 0 && lat < s.nlat_out && lon >= 0 && lon < s.nlon_out);
        REQUIRE(((day * nlev + l) * s.nlat_out + lat) * s.nlon_out + lon == t);
        plain.at((size_t)t) = raw.at((size_t)ns_raw_offset(s, day_rec[(size_t)day], lev[(size_t)l], lat_idx[(size_t)lat], lon_idx[(size_t)lon]));
        ++own_p.at((size_t)t);
    }
    for (size_t i = 0; i < own_t.size(); ++i) REQUIRE(own_t[i] == 1);
    for (size_t i = 0; i < own_p.size(); ++i) REQUIRE(own_p[i] == 1);
    // the two layouts element by element, from the layout's definition: [cy][cx][day][lev][4][4] against [day][lev][lat][lon]
    const int64_t ncy = ns_nchunk(s.nlat_out), ncx = ns_nchunk(s.nlon_out);
    int64_t npad = 0;
    for (int64_t cy = 0; cy < ncy; ++cy)
        for (int64_t cx = 0; cx < ncx; ++cx)
            for (int64_t d = 0; d < s.ndays; ++d)
                for (int32_t l = 0; l < nlev; ++l)
                    for (int r = 0; r < 4; ++r)
                        for (int k = 0; k < 4; ++k) {
                            const int32_t got = tiled[(size_t)((((((cy * ncx + cx) * s.ndays + d) * nlev + l) * 4 + r) * 4) + k)];
                            const int64_t lat = cy * 4 + r, lon = cx * 4 + k;
                            if (lat >= s.nlat_out || lon >= s.nlon_out) {
                                REQUIRE(got == PAD);
                                ++npad;
                            } else {
                                REQUIRE(got == plain[(size_t)(((d * nlev + l) * s.nlat_out + lat) * s.nlon_out + lon)]);
                            }
                        }
    REQUIRE(npad == ntiled - nplain);
    printf("ok %lld tiled %lld plain %lld padding\n", (long long)ntiled, (long long)nplain, (long long)npad);
    return 0;
}
