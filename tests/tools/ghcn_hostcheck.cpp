// ghcn_hostcheck.cpp -- the field logic of the GHCN-Daily kernels (topowx_amd/qa/twx_ghcn_field.h) run on the CPU, as a
// program of its own so that the address and undefined-behaviour sanitizers see every byte it reads:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itopowx_amd/qa \
//         tests/tools/ghcn_hostcheck.cpp -o ghcn_hostcheck
//     ghcn_hostcheck MANIFEST OUT
//
// MANIFEST (text): "dly MIN_YMD MAX_YMD NFILES" and NFILES paths, or "tobs MIN_YMD MAX_YMD NFILES NSTN ELEM", NSTN ids
// (sorted, 11 characters) and NFILES paths.  The files are laid end to end in ONE heap block of exactly their size, as
// the kernels see them, so a read past a truncated last line is a read past the block.  The line index and the two passes
// (claim by position, then write) are those of twx_ghcn.hip.  OUT (binary): dly: val [nfiles][3][ndays] float32, flag
// [nfiles][3][ndays] uint8, bad_header [nfiles] uint32, nvalues int64, nfallback int64, fallback [n][3] int64 (file, line
// position in the file, day field); tobs: tobs [nstn][ndays] int16, then values, outside, bad as int64.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "twx_ghcn_field.h"

namespace {

struct Line { int f; int64_t start, fend; };

std::vector<Line> line_index(const uint8_t *buf, const std::vector<int64_t> &off)
{
    std::vector<Line> out;
    const int nfiles = (int)off.size() - 1;
    for (int f = 0; f < nfiles; ++f) {
        if (off[f + 1] > off[f]) out.push_back({f, off[f], off[f + 1]});
        for (int64_t p = off[f]; p + 1 < off[f + 1]; ++p)
            if (buf[p] == 0x0a) out.push_back({f, p + 1, off[f + 1]});
    }
    return out;
}

std::vector<uint8_t> read_file(const std::string &path)
{
    std::ifstream fh(path, std::ios::binary);
    if (!fh) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(fh)), std::istreambuf_iterator<char>());
}

template <class T> void put(std::ofstream &o, const T *p, size_t n) { o.write(reinterpret_cast<const char *>(p), (std::streamsize)(n * sizeof(T))); }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ghcn_hostcheck MANIFEST OUT\n"); return 2; }
    std::ifstream man(argv[1]);
    std::string mode, elem;
    int64_t min_ymd = 0, max_ymd = 0;
    int nfiles = 0, nstn = 0;
    man >> mode >> min_ymd >> max_ymd >> nfiles;
    if (!man || (mode != "dly" && mode != "tobs") || nfiles < 1) { std::fprintf(stderr, "bad manifest\n"); return 2; }
    std::vector<std::string> ids;
    if (mode == "tobs") {
        man >> nstn >> elem;
        ids.resize((size_t)nstn);
        for (auto &s : ids) man >> s;
    }
    std::vector<int64_t> off(1, 0);
    std::vector<std::vector<uint8_t>> files;
    for (int f = 0; f < nfiles; ++f) {
        std::string p;
        man >> p;
        files.push_back(read_file(p));
        off.push_back(off.back() + (int64_t)files.back().size());
    }
    const int64_t nbytes = off.back();
    uint8_t *buf = static_cast<uint8_t *>(std::malloc((size_t)std::max<int64_t>(nbytes, 1)));    // exactly the files' bytes
    for (int f = 0; f < nfiles; ++f)
        if (!files[(size_t)f].empty()) std::memcpy(buf + off[(size_t)f], files[(size_t)f].data(), files[(size_t)f].size());
    const int64_t day0 = gh_days_from_civil(min_ymd / 10000, (min_ymd / 100) % 100, min_ymd % 100);
    const int64_t ndays = gh_days_from_civil(max_ymd / 10000, (max_ymd / 100) % 100, max_ymd % 100) - day0 + 1;
    const std::vector<Line> lines = line_index(buf, off);
    std::ofstream out(argv[2], std::ios::binary);

    if (mode == "dly") {
        const size_t cells = (size_t)nfiles * 3 * (size_t)ndays;
        std::vector<float> val(cells, (float)GH_MISSING);
        std::vector<uint8_t> flag(cells, 0);
        std::vector<uint32_t> win(cells, 0), bad((size_t)nfiles, 0xffffffffu);
        std::vector<int64_t> fb;
        int64_t nvalues = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (const Line &l : lines) {
                const uint8_t *line = buf + l.start;
                const int avail = (int)std::min<int64_t>(l.fend - l.start, GH_LINE_BYTES);
                int len = avail;
                for (int k = 0; k < avail; ++k)
                    if (line[k] == 0x0a) { len = k + 1; break; }
                int64_t year = 0, month = 0;
                if (gh_header(line, len, &year, &month) != GH_NUM_OK) {
                    bad[(size_t)l.f] = std::min(bad[(size_t)l.f], (uint32_t)(l.start - off[(size_t)l.f]));
                    continue;
                }
                const int elem_i = gh_element(line, len);
                if (elem_i == GH_ELEM_NONE) continue;
                for (int d = 0; d < 31; ++d) {
                    float v = 0.0f;
                    uint8_t q = 0;
                    int64_t didx = 0;
                    const int rc = gh_field(line, len, year, month, elem_i, d, min_ymd, max_ymd, day0, &v, &q, &didx);
                    if (rc == GH_FIELD_SKIP) continue;
                    if (didx < 0 || didx >= ndays) { std::fprintf(stderr, "day index out of range\n"); return 3; }
                    const size_t slot = ((size_t)l.f * 3 + (size_t)elem_i) * (size_t)ndays + (size_t)didx;
                    const uint32_t me = (uint32_t)l.start + 1u;
                    if (rc == GH_FIELD_VALUE) {
                        if (pass == 0) { win[slot] = std::max(win[slot], me); ++nvalues; }
                        else if (win[slot] == me) { val[slot] = v; flag[slot] = q; }
                    } else if (pass == 1) {
                        fb.push_back(l.f);
                        fb.push_back(l.start - off[(size_t)l.f]);
                        fb.push_back(d);
                    }
                }
            }
        const int64_t nfb = (int64_t)fb.size() / 3;
        put(out, val.data(), cells);
        put(out, flag.data(), cells);
        put(out, bad.data(), bad.size());
        put(out, &nvalues, 1);
        put(out, &nfb, 1);
        put(out, fb.data(), fb.size());
    } else {
        if (elem.size() != 4) { std::fprintf(stderr, "bad element\n"); return 2; }
        const size_t cells = (size_t)nstn * (size_t)ndays;
        std::vector<int16_t> tobs(cells, -1);
        std::vector<uint32_t> win(cells, 0);
        int64_t counts[3] = {0, 0, 0};
        for (int pass = 0; pass < 2; ++pass)
            for (const Line &l : lines) {
                int64_t e = l.start;
                while (e < l.fend && buf[e] != 0x0a) ++e;
                const int len = (int)(e - l.start);
                const uint8_t *line = buf + l.start;
                if (!gh_tobs_selected(line, len, reinterpret_cast<const uint8_t *>(elem.data()))) continue;
                const std::string id(reinterpret_cast<const char *>(line), 11);
                const auto it = std::lower_bound(ids.begin(), ids.end(), id);
                if (it == ids.end() || *it != id) continue;
                int64_t didx = 0;
                int32_t v = 0;
                const int rc = gh_tobs_fields(line, len, min_ymd, max_ymd, day0, &didx, &v);
                if (rc == GH_TOBS_BAD) { counts[2] += pass; continue; }
                if (rc == GH_TOBS_OUTSIDE) { counts[1] += pass; continue; }
                if (didx < 0 || didx >= ndays) { std::fprintf(stderr, "day index out of range\n"); return 3; }
                const size_t slot = (size_t)(it - ids.begin()) * (size_t)ndays + (size_t)didx;
                const uint32_t me = (uint32_t)l.start + 1u;
                if (pass == 0) { win[slot] = std::max(win[slot], me); ++counts[0]; }
                else if (win[slot] == me) tobs[slot] = (int16_t)v;
            }
        put(out, tobs.data(), cells);
        put(out, counts, 3);
    }
    std::free(buf);
    return out.good() ? 0 : 4;
}
