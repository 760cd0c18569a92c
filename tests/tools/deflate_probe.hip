// deflate_probe.hip -- runs the deflate kernels of twx_deflate.h (included exactly as the library includes it) on int16 images
// read from files, for tests/test_gpu_deflate_kernels.py, which compares every output with zlib and with the CPU restatement
// (oracle/deflate_oracle.py).  The library's ABI only deflates what interp_grid produced; this hands the kernels any image.
//
//   deflate_probe MANIFEST      one case per line:  name ndays Y X cy cx image_file out_file
//                               image_file: int16 little endian [ndays][Y][X]
//
// Per case the kernel sequence of df_launch (twx_hip.hip) with its sizes (df_slot_bytes, df_lo_bytes, df_nseg) and its `pairs`
// rule: memset of hist, k_deflate_hist, k_deflate_table, k_deflate_count, k_deflate_scan, k_deflate_emit.  The sequence runs
// TWICE into separate buffers: run 0 launches k_deflate_table with one work-group (a one-variable tile), run 1 with two
// (blockIdx.x = 1 builds this case's code from hist1 into table1; work-group 0 builds the code of an all-zero count array
// into a decoy table), as a two-variable tile does.
//
// Two checks of its own, reported in the out_file's header:
//   guard bands    every device buffer lies between two bands of PROBE_GUARD sentinel bytes; the trailing band starts at the
//                  buffer's exact last byte + 1.  Mask of damaged bands: bit b of run r at 16 r + b (B_* below).
//   repeatability  the two runs' buffers must be byte-identical (whole slots included; of the table its defined content).
//                  Mask of differing buffers, B_* bits.
//
// out_file (little endian): int64 {magic, nchunk, nseg, slot_bytes, guard_mask, repeat_mask, pairs, N}; int64 chunk_bytes[nchunk];
//   uint32 hist[277]; table of run 0, table of run 1, decoy table, each {uint8 len[277]; uint16 code[277]; uint32 hdr_bits;
//   uint32 hdr[80]}; uint32 seg_bytes[nchunk][nseg]; every chunk's stream (chunk_bytes[c] bytes; none if that is out of range).
//
// Every HIP call is checked: at the first error the case's name and the error go to stderr, the exit status is 3 and nothing
// further is started.  Exit status 0: every case ran and its out_file was written (the masks are the test's to judge).
#include "twx_deflate.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define PROBE_GUARD 4096
#define PROBE_SENTINEL 0xA5
#define PROBE_MAGIC 0x44464C50524F4231ll

static const char *g_case = "(start)";

#define CHK(x)                                                                                                     \
    do {                                                                                                           \
        hipError_t e_ = (x);                                                                                       \
        if (e_ != hipSuccess) {                                                                                    \
            fprintf(stderr, "ERROR case %s: %s:%d: %s: %s\n", g_case, __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            return 3;                                                                                              \
        }                                                                                                          \
    } while (0)

enum { B_OUT, B_SEG_BYTES, B_SEG_OFF, B_ADL, B_PIECE_BITS, B_CHUNK_BYTES, B_HIST, B_TABLE, B_DAILY, B_HIST0, B_TABLE0, B_COUNT };

struct Guarded {
    char *base = nullptr;
    size_t size = 0;
    template <class T> T *as() const { return reinterpret_cast<T *>(base + PROBE_GUARD); }
    hipError_t alloc(size_t n, int fill)
    {
        size = n;
        hipError_t e = hipMalloc((void **)&base, n + 2 * PROBE_GUARD);
        if (e != hipSuccess) return e;
        e = hipMemset(base, PROBE_SENTINEL, n + 2 * PROBE_GUARD);
        if (e != hipSuccess) return e;
        return n ? hipMemset(base + PROBE_GUARD, fill, n) : hipSuccess;
    }
    // 0: both bands intact, 1: damaged, < 0: a HIP error (in *err)
    int damaged(hipError_t *err) const
    {
        std::vector<uint8_t> g(2 * PROBE_GUARD);
        *err = hipMemcpy(g.data(), base, PROBE_GUARD, hipMemcpyDeviceToHost);
        if (*err != hipSuccess) return -1;
        *err = hipMemcpy(g.data() + PROBE_GUARD, base + PROBE_GUARD + size, PROBE_GUARD, hipMemcpyDeviceToHost);
        if (*err != hipSuccess) return -1;
        for (uint8_t b : g) if (b != PROBE_SENTINEL) return 1;
        return 0;
    }
    hipError_t fetch(std::vector<uint8_t> &h) const
    {
        h.resize(size);
        return size ? hipMemcpy(h.data(), base + PROBE_GUARD, size, hipMemcpyDeviceToHost) : hipSuccess;
    }
    void release() { if (base) (void)hipFree(base); base = nullptr; }
};

// the table's defined content: len / code of the TWX_DF_NSYM symbols, hdr_bits, hdr (entries NSYM .. NSYM + 2 and the struct's
// padding are never written by k_deflate_table nor read by anyone: they hold whatever the LDS held)
static void put_table(std::vector<uint8_t> &o, const uint8_t *raw)
{
    DfTable t;
    memcpy(&t, raw, sizeof t);
    const size_t at = o.size();
    o.resize(at + TWX_DF_NSYM * 3 + 4 + sizeof t.hdr);
    uint8_t *p = o.data() + at;
    memcpy(p, t.len, TWX_DF_NSYM); p += TWX_DF_NSYM;
    memcpy(p, t.code, TWX_DF_NSYM * 2); p += TWX_DF_NSYM * 2;
    memcpy(p, &t.hdr_bits, 4); p += 4;
    memcpy(p, t.hdr, sizeof t.hdr);
}

static int run_case(const std::string &name, int64_t ndays, int Y, int X, int cy, int cx, const std::string &image, const std::string &outp)
{
    if (ndays <= 0 || Y <= 0 || X <= 0 || cy <= 0 || cx <= 0 || Y % cy || X % cx) {
        fprintf(stderr, "ERROR case %s: bad geometry\n", g_case);
        return 1;
    }
    const int64_t N = ndays * cy * cx, nval = ndays * Y * X;
    if (df_slot_bytes(N) >= (int64_t)1 << 32) {
        fprintf(stderr, "ERROR case %s: chunk too large\n", g_case);
        return 1;
    }
    std::vector<uint16_t> img((size_t)nval);
    FILE *f = fopen(image.c_str(), "rb");
    if (!f || fread(img.data(), 2, (size_t)nval, f) != (size_t)nval || fgetc(f) != EOF) {
        fprintf(stderr, "ERROR case %s: %s does not hold exactly %lld int16 values\n", g_case, image.c_str(), (long long)nval);
        return 1;
    }
    fclose(f);
    const int nchunk = (Y / cy) * (X / cx), nseg = df_nseg(N);
    const int64_t slot = df_slot_bytes(N);
    const size_t per_var = (size_t)nchunk * nseg;
    const bool pairs = cx % 2 == 0 && X % 2 == 0;          // (df_launch's rule)

    Guarded daily, hist0, table0, buf[2][B_DAILY];
    CHK(daily.alloc((size_t)nval * 2, 0));
    CHK(hipMemcpy(daily.as<void>(), img.data(), (size_t)nval * 2, hipMemcpyHostToDevice));
    CHK(hist0.alloc(TWX_DF_NSYM * 4, 0));
    CHK(table0.alloc(sizeof(DfTable), 0xCD));
    DfArgs args[2];
    for (int r = 0; r < 2; ++r) {
        Guarded *b = buf[r];
        CHK(b[B_OUT].alloc((size_t)nchunk * slot, 0xEE));
        CHK(b[B_SEG_BYTES].alloc(per_var * 4, 0xCD));
        CHK(b[B_SEG_OFF].alloc(per_var * 4, 0xCD));
        CHK(b[B_ADL].alloc(per_var * 4 * 4, 0xCD));
        CHK(b[B_PIECE_BITS].alloc(per_var * TWX_DF_THREADS * 2, 0xCD));
        CHK(b[B_CHUNK_BYTES].alloc((size_t)nchunk * 8, 0xCD));
        CHK(b[B_HIST].alloc(TWX_DF_NSYM * 4, 0xCD));
        CHK(b[B_TABLE].alloc(sizeof(DfTable), 0xCD));
        DfArgs a{};
        a.daily = daily.as<const uint16_t>();
        a.out = b[B_OUT].as<uint8_t>();
        a.seg_bytes = b[B_SEG_BYTES].as<uint32_t>();
        a.seg_off = b[B_SEG_OFF].as<uint32_t>();
        a.adl = b[B_ADL].as<uint32_t>();
        a.piece_bits = b[B_PIECE_BITS].as<uint16_t>();
        a.chunk_bytes = b[B_CHUNK_BYTES].as<int64_t>();
        a.hist = b[B_HIST].as<uint32_t>();
        a.table = b[B_TABLE].as<DfTable>();
        a.N = N; a.slot_bytes = slot; a.lo_bytes = df_lo_bytes(N);
        a.Y = Y; a.X = X; a.cy = cy; a.cx = cx; a.ncx = X / cx; a.nseg = nseg;
        args[r] = a;
    }
    const dim3 grid((unsigned)nchunk, (unsigned)nseg);
    const dim3 sgrid((unsigned)nchunk, (unsigned)((nseg + TWX_DF_SAMPLE - 1) / TWX_DF_SAMPLE));
    const dim3 th(TWX_DF_THREADS);
    for (int r = 0; r < 2; ++r) {
        const DfArgs &a = args[r];
        CHK(hipMemsetAsync(a.hist, 0, TWX_DF_NSYM * 4, nullptr));
        if (pairs) hipLaunchKernelGGL(k_deflate_hist<2>, sgrid, th, 0, nullptr, a);
        else hipLaunchKernelGGL(k_deflate_hist<1>, sgrid, th, 0, nullptr, a);
        if (r == 0) hipLaunchKernelGGL(k_deflate_table, dim3(1), th, 0, nullptr, a.hist, a.table, a.hist, a.table);
        else hipLaunchKernelGGL(k_deflate_table, dim3(2), th, 0, nullptr, hist0.as<const uint32_t>(), table0.as<DfTable>(), a.hist, a.table);
        if (pairs) hipLaunchKernelGGL(k_deflate_count<2>, grid, th, 0, nullptr, a);
        else hipLaunchKernelGGL(k_deflate_count<1>, grid, th, 0, nullptr, a);
        hipLaunchKernelGGL(k_deflate_scan, dim3((unsigned)nchunk), th, 0, nullptr, a);
        if (pairs) hipLaunchKernelGGL(k_deflate_emit<2>, grid, th, 0, nullptr, a);
        else hipLaunchKernelGGL(k_deflate_emit<1>, grid, th, 0, nullptr, a);
        CHK(hipGetLastError());
        CHK(hipDeviceSynchronize());
    }

    int64_t guard_mask = 0, repeat_mask = 0;
    hipError_t err = hipSuccess;
    int d;
    for (int r = 0; r < 2; ++r)
        for (int b = 0; b < B_DAILY; ++b) {
            if ((d = buf[r][b].damaged(&err)) < 0) CHK(err);
            if (d) guard_mask |= (int64_t)1 << (16 * r + b);
        }
    const Guarded *shared[3] = {&daily, &hist0, &table0};
    for (int b = 0; b < 3; ++b) {
        if ((d = shared[b]->damaged(&err)) < 0) CHK(err);
        if (d) guard_mask |= (int64_t)1 << (B_DAILY + b);
    }
    std::vector<uint8_t> h[2][B_DAILY], decoy;
    for (int b = 0; b < B_DAILY; ++b) {
        CHK(buf[0][b].fetch(h[0][b]));
        CHK(buf[1][b].fetch(h[1][b]));
        if (b == B_TABLE) {                                  // (its defined content)
            std::vector<uint8_t> t0, t1;
            put_table(t0, h[0][b].data());
            put_table(t1, h[1][b].data());
            if (t0 != t1) repeat_mask |= (int64_t)1 << b;
        } else if (h[0][b] != h[1][b]) repeat_mask |= (int64_t)1 << b;
    }
    CHK(table0.fetch(decoy));

    std::vector<uint8_t> o;
    auto put = [&](const void *p, size_t n) { const uint8_t *q = static_cast<const uint8_t *>(p); o.insert(o.end(), q, q + n); };
    const int64_t head[8] = {PROBE_MAGIC, nchunk, nseg, slot, guard_mask, repeat_mask, pairs ? 1 : 0, N};
    put(head, sizeof head);
    put(h[0][B_CHUNK_BYTES].data(), h[0][B_CHUNK_BYTES].size());
    put(h[0][B_HIST].data(), h[0][B_HIST].size());
    put_table(o, h[0][B_TABLE].data());
    put_table(o, h[1][B_TABLE].data());
    put_table(o, decoy.data());
    put(h[0][B_SEG_BYTES].data(), h[0][B_SEG_BYTES].size());
    const int64_t *cb = reinterpret_cast<const int64_t *>(h[0][B_CHUNK_BYTES].data());
    for (int c = 0; c < nchunk; ++c)
        if (cb[c] >= 0 && cb[c] <= slot) put(h[0][B_OUT].data() + (size_t)c * slot, (size_t)cb[c]);
    f = fopen(outp.c_str(), "wb");
    if (!f || fwrite(o.data(), 1, o.size(), f) != o.size() || fclose(f) != 0) {
        fprintf(stderr, "ERROR case %s: cannot write %s\n", g_case, outp.c_str());
        return 1;
    }
    for (int r = 0; r < 2; ++r)
        for (int b = 0; b < B_DAILY; ++b) buf[r][b].release();
    daily.release(); hist0.release(); table0.release();
    printf("DONE %s nchunk %d nseg %d vec %d guard %lld repeat %lld\n", name.c_str(), nchunk, nseg, pairs ? 2 : 1, (long long)guard_mask,
           (long long)repeat_mask);
    fflush(stdout);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s MANIFEST\n", argv[0]);
        return 1;
    }
    std::ifstream mf(argv[1]);
    if (!mf) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    std::string line;
    int ncase = 0;
    while (std::getline(mf, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name, image, outp;
        long long ndays;
        int Y, X, cy, cx;
        if (!(ls >> name >> ndays >> Y >> X >> cy >> cx >> image >> outp)) {
            fprintf(stderr, "bad manifest line: %s\n", line.c_str());
            return 1;
        }
        g_case = name.c_str();
        const int rc = run_case(name, ndays, Y, X, cy, cx, image, outp);
        if (rc) return rc;                                   // the first error ends the run: nothing further is started
        ++ncase;
    }
    printf("ALL %d\n", ncase);
    return 0;
}
