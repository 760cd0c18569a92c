// The series coder without a device, as a program of its own (tests/test_series_deflate_host.py builds it with
// -fsanitize=address,undefined): the host arithmetic of topowx_amd/qa/twx_serdeflate_host.h, and a host-side encoder made of
// the SAME functions the kernels call -- df_piece, df_step_tokens, df_build_table, DfBits, df_huff_bytes, df_seg_stored of
// topowx_amd/csrc/twx_deflate.h -- over the rows of a file.  Its streams must equal tests/restate_series_deflate.py's.
//
//   serdeflate_hostcheck arith                      prints the arithmetic, one "key value" line each
//   serdeflate_hostcheck encode IN OUT              IN: int64 nrows, n, es, then the rows; OUT: int64 counts[8], offsets[nrows + 1], bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "twx_serdeflate_host.h"
#include "twx_deflate.h"

static int arith()
{
    const int64_t ns[] = {0, 1, 2, 16383, 16384, 16385, 25203, 32769, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 29) - 1, (int64_t)1 << 29};
    for (int64_t n : ns)
        for (int es : {0, 1, 2, 3, 4, 8}) printf("bound %lld %d %lld\n", (long long)n, es, (long long)sd_bound(n, es));
    for (int64_t n : {1, 16384, 16385, 25203, 49153})
        printf("nseg %lld %lld last %lld\n", (long long)n, (long long)sd_nseg(n), (long long)sd_seg_len(n, sd_nseg(n) - 1));
    for (unsigned a = 0; a < 32; ++a)
        for (int es : {1, 2, 4})
            if (a % es == 0) printf("head %u %d %d %d\n", a, es, sd_head(a, es, 16384), sd_head(a, es, 2));
    for (int r = 0; r < 9; ++r) printf("sampled %d %d %d %d\n", r, sd_sampled(r, 0) ? 1 : 0, sd_sampled(r, 16) ? 1 : 0, sd_sampled(r, 17) ? 1 : 0);
    SdDims d;
    const struct { int64_t nrows, n, es; } bad[] = {{1, 1, 3}, {1, 0, 4}, {1, (int64_t)1 << 29, 4}, {-1, 5, 1}, {(int64_t)1 << 31, 5, 1},
                                                   {(int64_t)1 << 30, 16385, 1}};
    for (auto &b : bad) { const char *m = sd_dims(b.nrows, b.n, b.es, 1000, &d); printf("dims_bad %s\n", m ? m : "accepted"); }
    const char *ok = sd_dims(12000, 25203, 4, (int64_t)sizeof(DfTable), &d);
    printf("dims_ok %s %lld %lld %lld %lld %lld\n", ok ? ok : "accepted", (long long)d.nseg, (long long)d.nblk, (long long)d.items,
           (long long)d.bound, (long long)d.in_bytes);
    ok = sd_dims(0, 7, 2, (int64_t)sizeof(DfTable), &d);
    printf("dims_empty %s %lld %lld\n", ok ? ok : "accepted", (long long)d.items, (long long)d.in_bytes);
    int64_t sizes[3] = {17, 30, 12}, off[4];
    const char *m = sd_offsets(sizes, 3, 30, off);
    printf("offsets %s %lld %lld %lld %lld\n", m ? m : "ok", (long long)off[0], (long long)off[1], (long long)off[2], (long long)off[3]);
    sizes[1] = 31;
    m = sd_offsets(sizes, 3, 30, off);
    printf("offsets_long %s\n", m ? m : "ok");
    sizes[1] = 11;
    m = sd_offsets(sizes, 3, 30, off);
    printf("offsets_short %s\n", m ? m : "ok");
    return 0;
}

// the tokens of plane[s0 .. s0 + len): tok(symbol, extra, number of extra bits), pieces of TWX_DF_PIECE bytes
template <class Tok>
static void segment_tokens(const uint8_t *plane, int64_t s0, int len, Tok tok)
{
    for (int p0 = 0; p0 < len; p0 += TWX_DF_PIECE) {
        const int plen = len - p0 < TWX_DF_PIECE ? len - p0 : TWX_DF_PIECE;
        const int prev = s0 + p0 > 0 ? (int)plane[s0 + p0 - 1] : 256;
        df_piece<false>(plane + s0 + p0, plen, prev, [&](int run, int pv, int c) { df_step_tokens(run, pv, c, tok); });
    }
}

static int encode(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", in); return 2; }
    int64_t hd[3];
    if (fread(hd, 8, 3, f) != 3) { fclose(f); return 2; }
    const int64_t nrows = hd[0], n = hd[1], es = hd[2];
    SdDims d;
    const char *bad = sd_dims(nrows, n, es, (int64_t)sizeof(DfTable), &d);
    if (bad) { fprintf(stderr, "%s\n", bad); fclose(f); return 2; }
    std::vector<uint8_t> rows((size_t)d.in_bytes);
    if (d.in_bytes && fread(rows.data(), 1, rows.size(), f) != rows.size()) { fclose(f); return 2; }
    fclose(f);
    // the shuffled rows: plane p of row r at (r * es + p) * n
    std::vector<uint8_t> pl(rows.size());
    for (int64_t r = 0; r < nrows; ++r)
        for (int64_t i = 0; i < n; ++i)
            for (int64_t p = 0; p < es; ++p) pl[(size_t)((r * es + p) * n + i)] = rows[(size_t)((r * n + i) * es + p)];
    std::vector<DfTable> table((size_t)es);
    int64_t counts[8] = {0};
    for (int64_t p = 0; p < es; ++p) {
        uint32_t hist[TWX_DF_NSYM] = {0};
        for (int64_t r = 0; r < nrows; ++r)
            for (int64_t s = 0; s < d.nseg; ++s)
                if (sd_sampled(r, s))
                    segment_tokens(&pl[(size_t)((r * es + p) * n)], s * TWXSD_SEG, (int)sd_seg_len(n, s),
                                   [&](int sym, unsigned, unsigned) { hist[sym]++; });
        df_build_table(hist, &table[(size_t)p]);
        // the halvings: df_build_table's loop, counted
        uint32_t cnt[TWX_DF_NSYM], wt[2 * TWX_DF_NSYM];
        uint16_t order[TWX_DF_NSYM], parent[2 * TWX_DF_NSYM], depth[2 * TWX_DF_NSYM];
        uint8_t len[TWX_DF_NSYM + 3];
        for (int i = 0; i < TWX_DF_NSYM; ++i) cnt[i] = hist[i] + 1u;
        for (;;) {
            df_sort_order(cnt, TWX_DF_NSYM, order);
            if (df_huff_sorted(cnt, order, TWX_DF_NSYM, 15, wt, parent, depth, len)) break;
            counts[2 + p]++;
            for (int i = 0; i < TWX_DF_NSYM; ++i) cnt[i] = (cnt[i] + 1u) >> 1;
        }
    }
    std::vector<uint8_t> packed;
    std::vector<int64_t> offsets((size_t)nrows + 1, 0);
    std::vector<uint32_t> words((TWX_DF_SEG + 5 + 3) / 4 + 2);
    for (int64_t r = 0; r < nrows; ++r) {
        packed.push_back(0x78); packed.push_back(0x01);
        uint32_t A = 1, B = 0;
        for (int64_t p = 0; p < es; ++p) {
            const uint8_t *plane = &pl[(size_t)((r * es + p) * n)];
            const DfTable &t = table[(size_t)p];
            for (int64_t i = 0; i < n; ++i) { A = (A + plane[i]) % TWX_ADLER_P; B = (B + A) % TWX_ADLER_P; }
            for (int64_t s = 0; s < d.nseg; ++s) {
                const int len = (int)sd_seg_len(n, s);
                uint32_t bits = 0;
                segment_tokens(plane, s * TWXSD_SEG, len, [&](int sym, unsigned, unsigned ne) { bits += t.len[sym] + ne + (sym > 256 ? 1u : 0u); });
                const uint32_t nbytes = df_huff_bytes(bits, t.hdr_bits, t.len[256]);
                counts[0]++;
                if (df_seg_stored(nbytes, len)) {
                    counts[1]++;
                    const unsigned bl = (unsigned)len;
                    const uint8_t h[5] = {0, (uint8_t)bl, (uint8_t)(bl >> 8), (uint8_t)~bl, (uint8_t)(~bl >> 8)};
                    packed.insert(packed.end(), h, h + 5);
                    packed.insert(packed.end(), plane + s * TWXSD_SEG, plane + s * TWXSD_SEG + len);
                    continue;
                }
                std::fill(words.begin(), words.end(), 0u);
                for (uint32_t i = 0; i < (t.hdr_bits + 31u) / 32u; ++i) words[i] = t.hdr[i];
                DfBits b{words.data(), t.hdr_bits};
                segment_tokens(plane, s * TWXSD_SEG, len, [&](int sym, unsigned ex, unsigned ne) {
                    b.put(t.code[sym], t.len[sym]);
                    b.put(ex, ne);
                    if (sym > 256) b.put(0u, 1);                 // the distance code: one code, one bit
                });
                b.put(t.code[256], t.len[256]);
                if (b.n != t.hdr_bits + bits + t.len[256]) { fprintf(stderr, "bit count\n"); return 3; }
                std::vector<uint8_t> blk(nbytes, 0);
                memcpy(blk.data(), words.data(), (b.n + 7) / 8);
                blk[nbytes - 2] = 0xFF; blk[nbytes - 1] = 0xFF;
                packed.insert(packed.end(), blk.begin(), blk.end());
            }
        }
        const uint8_t tail[9] = {1, 0, 0, 0xFF, 0xFF, (uint8_t)(B >> 8), (uint8_t)B, (uint8_t)(A >> 8), (uint8_t)A};
        packed.insert(packed.end(), tail, tail + 9);
        offsets[(size_t)r + 1] = (int64_t)packed.size();
        if (offsets[(size_t)r + 1] - offsets[(size_t)r] > d.bound) { fprintf(stderr, "a stream beyond sd_bound\n"); return 3; }
    }
    counts[6] = d.in_bytes; counts[7] = (int64_t)packed.size();
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(counts, 8, 8, o);
    fwrite(offsets.data(), 8, offsets.size(), o);
    if (!packed.empty()) fwrite(packed.data(), 1, packed.size(), o);
    fclose(o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "arith")) return arith();
    if (argc == 4 && !strcmp(argv[1], "encode")) return encode(argv[2], argv[3]);
    fprintf(stderr, "usage: serdeflate_hostcheck arith | encode IN OUT\n");
    return 2;
}
