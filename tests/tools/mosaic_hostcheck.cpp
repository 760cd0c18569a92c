// mosaic_hostcheck.cpp -- the host-side arithmetic of the mosaic unit (topowx_amd/qa/twx_mosaic_host.h) as a program of its
// own, so that the address and undefined-behaviour sanitizers see every index it forms:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itopowx_amd/qa \
//         tests/tools/mosaic_hostcheck.cpp -o mosaic_hostcheck
//     mosaic_hostcheck
//
// Prints one line per case ("dims max_days Y X cy cx -> Yp Xp nchunk nseg vec slot_bytes device_bytes") for the test to compare
// with its own arithmetic, walks every chunk origin and every row of a placement on heap blocks of exactly the image's size
// (a wrong padded size or a placement check that lets a slab through is a write past the block), and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "twx_mosaic_host.h"

namespace {

int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

void dims_case(int64_t max_days, int64_t Y, int64_t X, int64_t cy, int64_t cx)
{
    MoDims d;
    const char *bad = mo_dims(max_days, Y, X, cy, cx, 1300, &d);
    if (bad) { std::printf("dims %lld %lld %lld %lld %lld -> refused: %s\n", (long long)max_days, (long long)Y, (long long)X,
                           (long long)cy, (long long)cx, bad); return; }
    std::printf("dims %lld %lld %lld %lld %lld -> %d %d %d %d %d %lld %lld\n", (long long)max_days, (long long)Y, (long long)X,
                (long long)cy, (long long)cx, d.Yp, d.Xp, d.nchunk, d.nseg, d.vec, (long long)d.slot_bytes, (long long)d.device_bytes);
    EXPECT(d.Yp >= d.Y && d.Yp - d.Y < d.cy && d.Xp >= d.X && d.Xp - d.X < d.cx && d.Yp % d.cy == 0 && d.Xp % d.cx == 0);
    EXPECT(d.slot_bytes % 256 == 0 && d.slot_bytes >= 2 + d.lo_bytes + 9);
    EXPECT(d.device_bytes == d.image_bytes + d.mthly_bytes + d.slots_bytes + d.small_bytes);
    if (d.layers * d.Yp * d.Xp > (1 << 24)) return;                       // the walks below: small images only
    // every chunk of every layer lies inside the padded image, in file order, each cell exactly once
    std::vector<uint8_t> seen((size_t)(d.max_days * d.Yp * d.Xp), 0);
    int64_t pl = -1, pr = -1, pc = -1;
    for (int64_t k = 0; k < d.max_days * d.nchunk; ++k) {
        int64_t l, r0, c0;
        mo_chunk_origin(d, k, &l, &r0, &c0);
        EXPECT(l > pl || (l == pl && (r0 > pr || (r0 == pr && c0 > pc))));
        pl = l; pr = r0; pc = c0;
        for (int64_t r = r0; r < r0 + d.cy; ++r)
            for (int64_t c = c0; c < c0 + d.cx; ++c) seen[(size_t)((l * d.Yp + r) * d.Xp + c)]++;
    }
    for (uint8_t s : seen) EXPECT(s == 1);
}

void place_case(const MoDims &d, int64_t nd, int64_t ty, int64_t tx, int64_t y0, int64_t x0, bool want_ok)
{
    const char *bad = mo_check_place(d, nd, ty, tx, y0, x0);
    EXPECT((bad == nullptr) == want_ok);
    if (bad) return;
    // the kernel's row copy on heap blocks: head, aligned units, tail
    std::vector<int16_t> img((size_t)(d.max_days * d.Yp * d.Xp), (int16_t)-32767), src((size_t)(nd * ty * tx));
    for (size_t i = 0; i < src.size(); ++i) src[i] = (int16_t)(i * 7 + 1);
    for (int64_t row = 0; row < nd * ty; ++row) {
        const int64_t day = row / ty, r = row - day * ty;
        const int16_t *s = src.data() + row * tx;
        int16_t *o = img.data() + (day * d.Yp + y0 + r) * d.Xp + x0;
        const uint64_t sa = (uint64_t)(uintptr_t)s / 2, da = (uint64_t)(uintptr_t)o / 2;
        const int w = mo_copy_width(sa, da);
        const int head = mo_copy_head(da, w, (int)tx);
        EXPECT(w == 1 || w == 2 || w == 4 || w == 8);
        EXPECT(head == tx || ((da + (uint64_t)head) % (uint64_t)w == 0 && (sa + (uint64_t)head) % (uint64_t)w == 0));
        for (int i = 0; i < head; ++i) o[i] = s[i];
        const int nv = ((int)tx - head) / w;
        for (int j = 0; j < nv; ++j) std::memcpy(o + head + j * w, s + head + j * w, (size_t)w * 2);
        for (int i = head + nv * w; i < tx; ++i) o[i] = s[i];
    }
    for (int64_t day = 0; day < nd; ++day)
        for (int64_t r = 0; r < ty; ++r)
            for (int64_t c = 0; c < tx; ++c)
                EXPECT(img[(size_t)((day * d.Yp + y0 + r) * d.Xp + x0 + c)] == src[(size_t)((day * ty + r) * tx + c)]);
}

}  // namespace

int main()
{
    dims_case(2, 300, 1100, 130, 510);
    dims_case(3, 200, 250, 128, 128);
    dims_case(1, 255, 300, 255, 257);
    dims_case(1, 256, 256, 256, 256);
    dims_case(5, 20, 20, 7, 9);
    dims_case(366, 3250, 7000, 325, 700);
    dims_case(0, 10, 10, 5, 5);
    dims_case(1, 10, 10, 11, 5);
    dims_case(1, 10, 10, 5, 0);
    dims_case(1000000, 1 << 24, 1 << 24, 1, 1);                          // more chunks than a grid's x dimension
    dims_case(1, 1 << 24, 1 << 24, 1 << 24, 1 << 24);                    // a slot of 2^32 bytes or more
    MoDims d;
    if (mo_dims(3, 45, 601, 13, 601, 1300, &d)) return 2;
    for (int tx : {1, 2, 7, 8, 9, 64, 250})
        for (int x0 : {0, 1, 2, 3, 5, 8, 101, 350}) place_case(d, 3, 3, tx, 4, x0, true);
    place_case(d, 1, 2, 2, 44, 0, false);                                 // rows 44, 45: row 45 is padding
    place_case(d, 1, 2, 2, 43, 599, true);                                // the last rows and columns
    place_case(d, 1, 2, 2, 0, 600, false);
    place_case(d, 1, 2, 2, -1, 0, false);
    place_case(d, 1, 2, 2, 0, -1, false);
    place_case(d, 4, 2, 2, 0, 0, false);
    place_case(d, 1, 46, 2, 0, 0, false);
    place_case(d, 1, 2, 602, 0, 0, false);
    place_case(d, 1, 2, 2, INT32_MAX, 0, false);
    place_case(d, 1, 2, 2, 0, INT64_MAX, false);
    place_case(d, 0, 2, 2, 0, 0, false);
    // the offsets of the compaction
    const int64_t sizes[5] = {10, 1, 256, 7, 99};
    int64_t off[6];
    EXPECT(mo_offsets(sizes, 5, 256, off) == nullptr);
    EXPECT(off[0] == 0 && off[1] == 10 && off[2] == 11 && off[3] == 267 && off[4] == 274 && off[5] == 373);
    EXPECT(mo_offsets(sizes, 5, 255, off) != nullptr);                    // a stream longer than its slot
    const int64_t zero[2] = {5, 0};
    EXPECT(mo_offsets(zero, 2, 256, off) != nullptr);
    EXPECT(mo_offsets(sizes, 0, 256, off) == nullptr && off[0] == 0);
    if (failures) { std::fprintf(stderr, "%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
