// raws_hostcheck.cpp -- the token and field code of the RAWS ingest (topowx_amd/qa/twx_raws_field.h) on the CPU: a
// stand-alone program for the sanitizers (tests/test_raws_host.py builds it with -fsanitize=address,undefined and runs it).
//
//   raws_hostcheck MANIFEST OUT
//
// MANIFEST: "raws MIN_YMD MAX_YMD NFILES", then NFILES paths, one a line.  Every file is a batch of its own, placed at 0 in a
// buffer padded with zero bytes as the device's is.  The lines are indexed by a plain scan; each body line is tokenised in
// aligned 16-byte steps with the kernel's own helpers (rw_nonspace16, rw_nth_bit: a lane's share of a window, one lane
// after the other) and decided with the kernel's own field functions, in the kernel's order; of several decided lines of a
// day the last one wins.
// OUT: int64 nfiles, ndays; float32 val [nfiles][3][ndays]; int64 counts [nfiles][8] (lines, body, skipped, values,
// duplicates, uncertain, raise, date-uncertain); int64 n, then n entries of 8 int64 (the uncertain list); the same for the
// raise list.  The entries are in file, then line, then field order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "twx_raws_field.h"

namespace {

struct Lists { std::vector<int64_t> unc, rse; };

void put(std::vector<int64_t> &l, int64_t f, int64_t pos, int64_t field, int64_t off, int64_t len, int64_t win, int64_t day, int64_t start)
{
    const int64_t e[8] = {f, pos, field, off, len, win, day, start};
    l.insert(l.end(), e, e + 8);
}

struct Pending { int64_t pos, day; int field[3], nf; int64_t off[3], len[3]; };

void parse_file(int64_t f, const std::string &data, int64_t min_ymd, int64_t max_ymd, int64_t day0, int64_t ndays, float *val,
                int64_t *cnt, Lists &out)
{
    const int64_t n = (int64_t)data.size();
    std::vector<uint8_t> buf((size_t)((n + 15) / 16 * 16 + 16), 0);
    if (n) memcpy(buf.data(), data.data(), (size_t)n);
    std::vector<int64_t> starts;                                  // a newline that ends the file opens no further line
    if (n > 0) starts.push_back(0);
    for (int64_t i = 0; i + 1 < n; ++i)
        if (buf[(size_t)i] == 0x0a) starts.push_back(i + 1);
    cnt[0] = (int64_t)starts.size();
    std::map<int64_t, int64_t> winner;
    std::vector<Pending> pending;
    for (size_t li = 7; li < starts.size(); ++li) {
        const int64_t start = starts[li];
        const int64_t lineend = li + 1 < starts.size() ? starts[li + 1] - 1 : n;   // as the kernel takes it from the index
        bool stop = false;
        for (int64_t q = start; q + 9 <= lineend && !stop; ++q) stop = memcmp(&buf[(size_t)q], "Copyright", 9) == 0;
        if (stop) break;
        ++cnt[1];
        int64_t tpos[RW_NFIELDS] = {0, 0, 0, 0};
        int ntok = 0;
        uint32_t carry = 0;
        for (int64_t p = start & ~(int64_t)15; p < lineend && ntok < RW_NTOKENS; p += 16) {
            uint32_t w[4];
            memcpy(w, &buf[(size_t)p], 16);
            const int lo = (int)(start - p > 16 ? 16 : (start - p < 0 ? 0 : start - p));
            const int hi = (int)(lineend - p > 16 ? 16 : lineend - p);
            const uint32_t m = rw_nonspace16(w[0], w[1], w[2], w[3], lo, hi);
            const uint32_t s = m & ~((m << 1) | carry) & 0xffffu;
            const int c = __builtin_popcount(s);
            for (int q = 0; q < RW_NFIELDS; ++q) {
                const int T = rw_field_token(q);
                if (ntok <= T && T < ntok + c) tpos[q] = p + rw_nth_bit(s, T - ntok);
            }
            ntok += c;
            carry = m >> 15;
        }
        if (ntok == 0) { put(out.rse, f, start, 0, 0, 0, 0, 0xffffffffLL, start); continue; }
        const uint8_t *t0 = &buf[(size_t)tpos[0]];
        const int n0 = rw_token_len(t0, lineend - tpos[0]);
        int64_t didx = 0;
        const int ds = rw_date(t0, n0, min_ymd, max_ymd, day0, &didx);
        if (ds == RW_DATE_UNCERTAIN) {
            put(out.unc, f, start, RW_FIELD_DATE, tpos[0] - start, n0, 0, 0xffffffffLL, start);
            ++cnt[7];
            continue;
        }
        if (ds == RW_DATE_SKIP) { ++cnt[2]; continue; }
        if (ds == RW_DATE_OUTSIDE) continue;
        if (didx < 0 || didx >= ndays) { fprintf(stderr, "day index %lld outside the period\n", (long long)didx); exit(2); }
        if (ntok < RW_NTOKENS) { put(out.rse, f, start, 1, 0, ntok, 0, didx, start); continue; }
        float v[3] = {0, 0, 0};
        Pending pd;
        pd.pos = start, pd.day = didx, pd.nf = 0;
        for (int q = 1; q < RW_NFIELDS; ++q) {
            const uint8_t *t = &buf[(size_t)tpos[q]];
            const int len = rw_token_len(t, lineend - tpos[q]);
            if (rw_value(t, len, q, &v[q - 1]) != RW_OK) {
                pd.field[pd.nf] = q, pd.off[pd.nf] = tpos[q] - start, pd.len[pd.nf] = len;
                ++pd.nf;
            }
        }
        if (pd.nf) { pending.push_back(pd); continue; }
        ++cnt[3];
        if (winner.count(didx)) ++cnt[4];
        winner[didx] = start + 1;
        val[(size_t)rw_field_elem(RW_FIELD_TMAX) * ndays + didx] = v[0];
        val[(size_t)rw_field_elem(RW_FIELD_TMIN) * ndays + didx] = v[1];
        val[(size_t)rw_field_elem(RW_FIELD_PRCP) * ndays + didx] = v[2];
    }
    std::vector<int64_t> late;
    for (const Pending &pd : pending)
        for (int k = 0; k < pd.nf; ++k)
            put(late, f, pd.pos, pd.field[k], pd.off[k], pd.len[k], winner.count(pd.day) ? winner[pd.day] : 0, pd.day, pd.pos);
    // the two kinds of uncertain entries in line order
    std::vector<int64_t> all(out.unc.end() - 8 * cnt[7], out.unc.end());
    out.unc.resize(out.unc.size() - (size_t)(8 * cnt[7]));
    all.insert(all.end(), late.begin(), late.end());
    std::vector<size_t> order(all.size() / 8);
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    for (size_t a = 1; a < order.size(); ++a)                      // insertion sort by (line, field): the lists are short
        for (size_t b = a; b > 0; --b) {
            const int64_t *x = &all[8 * order[b - 1]], *y = &all[8 * order[b]];
            if (x[7] < y[7] || (x[7] == y[7] && x[2] <= y[2])) break;
            std::swap(order[b - 1], order[b]);
        }
    for (size_t k : order) out.unc.insert(out.unc.end(), &all[8 * k], &all[8 * k] + 8);
    cnt[5] = (int64_t)order.size();
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: raws_hostcheck MANIFEST OUT\n"); return 2; }
    std::ifstream man(argv[1]);
    std::string kind;
    long long min_ymd = 0, max_ymd = 0, nfiles = 0;
    man >> kind >> min_ymd >> max_ymd >> nfiles;
    if (!man || kind != "raws" || nfiles < 0) { fprintf(stderr, "bad manifest\n"); return 2; }
    const int64_t day0 = gh_days_from_civil(min_ymd / 10000, min_ymd / 100 % 100, min_ymd % 100);
    const int64_t ndays = gh_days_from_civil(max_ymd / 10000, max_ymd / 100 % 100, max_ymd % 100) - day0 + 1;
    std::vector<float> val((size_t)(nfiles * 3 * ndays), (float)RW_MISSING);
    std::vector<int64_t> cnt((size_t)(nfiles * 8), 0);
    Lists lists;
    std::string path;
    std::getline(man, path);
    for (long long f = 0; f < nfiles; ++f) {
        if (!std::getline(man, path)) { fprintf(stderr, "the manifest ends early\n"); return 2; }
        std::ifstream in(path, std::ios::binary);
        if (!in) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        const std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const size_t before = lists.rse.size();
        parse_file(f, data, min_ymd, max_ymd, day0, ndays, &val[(size_t)(f * 3 * ndays)], &cnt[(size_t)(f * 8)], lists);
        cnt[(size_t)(f * 8 + 6)] = (int64_t)((lists.rse.size() - before) / 8);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const int64_t head[2] = {nfiles, ndays};
    const int64_t nu = (int64_t)lists.unc.size() / 8, nr = (int64_t)lists.rse.size() / 8;
    fwrite(head, 8, 2, out);
    if (nfiles) fwrite(val.data(), 4, val.size(), out);
    if (nfiles) fwrite(cnt.data(), 8, cnt.size(), out);
    fwrite(&nu, 8, 1, out);
    if (nu) fwrite(lists.unc.data(), 8, lists.unc.size(), out);
    fwrite(&nr, 8, 1, out);
    if (nr) fwrite(lists.rse.data(), 8, lists.rse.size(), out);
    fclose(out);
    return 0;
}
