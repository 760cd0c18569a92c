// twx_ghcn.hip -- libtwxqa.so: the GHCN-Daily ingest of step04.  InsertGhcn.parse_stn_obs
// (twx/db/create_db_all_stations.py:1042-1103) for a batch of .dly files in one call, and create_tobs_db
// (twx/homog/tobs.py:121-157) for a batch of by-year CSV files.  The sixteenth translation unit of the library
// (include/twx_qa.h, twxgh_*).  The field logic -- calendar, clipping to the line's end, the grammar of a number, the unit
// conversion -- is twx_ghcn_field.h, shared with a CPU program of the tests.
//
// The line index.  Both entries see one byte buffer of files laid end to end (file_off [nfiles + 1]).  A line starts at a
// file's first byte (a non-empty file) or after a newline byte that is not its file's last byte; a last line without a
// newline is a line; lines never span files.
//   k_gh_count   256 threads x 16 bytes (one aligned 128-bit load each): newline bytes per 4 KiB block
//   k_gh_scan    one workgroup: exclusive sums of the block counts
//   k_gh_starts  the same loads; the positions after the newlines, compacted in buffer order
// A newline that ends its file yields a candidate at the file's end: the consumers drop it when they look the file up.
//
// k_gh_dly<pass>  half a wavefront per line, a lane per day field, 8 lines per workgroup.  Lanes 0 .. 17 of the half stage
//                 288 bytes of the line in LDS with aligned 128-bit loads, each bounded by the file's end (which is bounded
//                 by the buffer's); the lanes then read their 8-byte fields from LDS.  31 consecutive days of a station are
//                 124 contiguous bytes of output.  LDS 2.25 KiB.
// k_gh_tobs<pass> a thread per by-year line: the filter, a binary search of the sorted id table, the date, the value.
//
// Duplicates.  The reference keeps the LAST line that gave a (day, element) a value.  Pass 0 takes an integer atomicMax of
// "line position + 1" per (row, day, element); pass 1 parses again and only the line that holds the maximum writes.  A
// position is unique, so no result depends on which wave got there first; there are no floating-point atomics.  Fields only
// Python's float() can decide take no part: pass 1 lists them with the winning position, and the caller settles them in
// position order.  Built with -ffp-contract=off; the one division is fp64, rounded once to float32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_ghcn_field.h"
#include "twx_ghcn_index.h"
#include "twx_qa.h"
#include "twx_qa_common.h"

#define GH_CHUNK 4096                        // bytes per workgroup of k_gh_count / k_gh_starts
#define GH_LINES_PER_WG 8
#define GH_STAGE 288                         // 18 x 16 bytes: 15 bytes of misalignment + GH_LINE_BYTES
#define GH_NONE 0xffffffffu

namespace {

// bit k set: byte k of the 16 is a newline, k < nvalid
__device__ __forceinline__ uint32_t gh_newlines(uint4 w, int nvalid)
{
    const uint32_t v[4] = {w.x, w.y, w.z, w.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (((v[k >> 2] >> (8 * (k & 3))) & 0xffu) == 0x0au) m |= 1u << k;
    return nvalid >= 16 ? m : (nvalid <= 0 ? 0u : (m & ((1u << nvalid) - 1u)));
}

// The newline bytes of this thread's 16 whose successor is still inside the buffer.  The load is aligned and starts below
// nbytes; the buffer is allocated to a multiple of 16.
__device__ __forceinline__ uint32_t gh_thread_newlines(const uint8_t *__restrict__ buf, int64_t nbytes, int64_t p0)
{
    if (p0 >= nbytes - 1) return 0u;
    const uint4 w = *reinterpret_cast<const uint4 *>(buf + p0);
    const int64_t left = nbytes - 1 - p0;
    return gh_newlines(w, left > 16 ? 16 : (int)left);
}

}  // namespace

__global__ __launch_bounds__(256) void k_gh_count(const uint8_t *__restrict__ buf, int64_t nbytes, uint32_t *__restrict__ blk_cnt)
{
    __shared__ uint32_t part[4];
    const int64_t p0 = (int64_t)blockIdx.x * GH_CHUNK + (int64_t)threadIdx.x * 16;
    uint32_t c = (uint32_t)__popc(gh_thread_newlines(buf, nbytes, p0));
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(1024) void k_gh_scan(const uint32_t *__restrict__ blk_cnt, int64_t nblk, uint32_t *__restrict__ blk_off,
                                                  uint32_t *__restrict__ total)
{
    __shared__ uint32_t sums[1024];
    const int t = threadIdx.x;
    const int64_t seg = (nblk + 1023) / 1024;
    const int64_t a = std::min<int64_t>(nblk, t * seg), b = std::min<int64_t>(nblk, a + seg);
    uint32_t s = 0;
    for (int64_t i = a; i < b; ++i) s += blk_cnt[i];
    sums[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                          // inclusive scan of the segment sums
        const uint32_t v = t >= o ? sums[t - o] : 0u;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    uint32_t run = sums[t] - s;
    for (int64_t i = a; i < b; ++i) { blk_off[i] = run; run += blk_cnt[i]; }
    if (t == 1023) *total = sums[1023];
}

__global__ __launch_bounds__(256) void k_gh_starts(const uint8_t *__restrict__ buf, int64_t nbytes,
                                                   const uint32_t *__restrict__ blk_off, uint32_t ncand, uint32_t *__restrict__ cand)
{
    __shared__ uint32_t sc[256];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * GH_CHUNK + (int64_t)t * 16;
    uint32_t m = gh_thread_newlines(buf, nbytes, p0);
    const uint32_t c = (uint32_t)__popc(m);
    sc[t] = c;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t v = t >= o ? sc[t - o] : 0u;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    uint32_t k = blk_off[blockIdx.x] + sc[t] - c;
    while (m) {
        const int bit = __ffs((int)m) - 1;
        m &= m - 1;
        if (k < ncand) cand[k] = (uint32_t)(p0 + bit + 1);
        ++k;
    }
}

__global__ __launch_bounds__(256) void k_gh_fill(float *__restrict__ a, int64_t n, float v)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

// PASS 0 claims the (row, day, element) slots; PASS 1 writes what won and lists the fields left to Python.
template <int PASS>
__global__ __launch_bounds__(256) void k_gh_dly(const uint8_t *__restrict__ buf, int nfiles, const int64_t *__restrict__ file_off,
                                                const int32_t *__restrict__ file_col, const uint32_t *__restrict__ cand,
                                                int64_t nlines, int64_t nrows, int64_t ndays, int64_t min_ymd, int64_t max_ymd,
                                                int64_t day0, uint32_t *__restrict__ win, float *__restrict__ val,
                                                uint8_t *__restrict__ qflag, uint32_t *__restrict__ bad_header,
                                                uint32_t *__restrict__ fb, uint32_t fb_cap, uint32_t *__restrict__ fb_count,
                                                unsigned long long *__restrict__ nwritten)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[GH_LINES_PER_WG][GH_STAGE];
    const int h = threadIdx.x >> 5, sub = threadIdx.x & 31;
    const int64_t i = (int64_t)blockIdx.x * GH_LINES_PER_WG + h;
    int f = 0;
    int64_t start = 0, fend = 0;
    const bool live = gh_line(i, nlines, nfiles, file_off, cand, &f, &start, &fend);
    const int avail = live ? (int)std::min<int64_t>(fend - start, GH_LINE_BYTES) : 0;
    const int mis = (int)(start & 15);
    if (sub < GH_STAGE / 16) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        const int64_t p = start - mis + 16 * sub;                // aligned; loaded only if it starts below the line's end
        if (live && p < start + avail) w =*reinterpret_cast<const uint4 *>(buf + p);
        *reinterpret_cast<uint4 *>(&stage[h][16 * sub]) = w;
    }
    __syncthreads();
    const uint8_t *line = &stage[h][mis];
    int nl = GH_STAGE;                                           // the first newline among the avail bytes
    for (int k = 0; k < 9; ++k) {
        const int idx = sub * 9 + k;
        if (idx < avail && line[idx] == 0x0a) { nl = idx; break; }
    }
    for (int o = 16; o > 0; o >>= 1) nl = min(nl, __shfl_xor(nl, o, 32));
    const int len = nl < avail ? nl + 1 : avail;                 // with its newline, as readline gives it

    bool wrote = false;
    if (live) {
        int64_t year = 0, month = 0;
        if (gh_header(line, len, &year, &month) != GH_NUM_OK) {
            if (PASS == 0 && sub == 0) atomicMin(&bad_header[f], (uint32_t)(start - file_off[f]));
        } else {
            const int elem = gh_element(line, len);
            if (elem != GH_ELEM_NONE && sub < 31) {
                float v = 0.0f;
                uint8_t q = 0;
                int64_t didx = 0;
                const int rc = gh_field(line, len, year, month, elem, sub, min_ymd, max_ymd, day0, &v, &q, &didx);
                if (rc != GH_FIELD_SKIP && didx >= 0 && didx < ndays) {
                    const size_t slot = ((size_t)elem * (size_t)nrows + (size_t)file_col[f]) * (size_t)ndays + (size_t)didx;
                    const uint32_t me = (uint32_t)start + 1u;
                    if (rc == GH_FIELD_VALUE) {
                        if (PASS == 0) {
                            atomicMax(&win[slot], me);
                            wrote = true;
                        } else if (win[slot] == me) {
                            val[slot] = v;
                            qflag[slot] = q;
                        }
                    } else if (PASS == 1) {
                        const uint32_t k = atomicAdd(fb_count, 1u);
                        if (k < fb_cap) {
                            uint32_t *e = fb + (size_t)k * TWXGH_FB_WORDS;
                            e[0] = (uint32_t)f;
                            e[1] = (uint32_t)(start - file_off[f]);
                            e[2] = (uint32_t)len;
                            e[3] = (uint32_t)sub;
                            e[4] = (uint32_t)elem;
                            e[5] = win[slot];
                            e[6] = (uint32_t)didx;
                            e[7] = (uint32_t)start;
                        }
                    }
                }
            }
        }
    }
    if (PASS == 0) {
        const unsigned long long b = __ballot(wrote);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(nwritten, (unsigned long long)__popcll(b));
    }
}

// the row of id[0 .. 11) in the sorted table [nstn][11], or -1
__device__ __forceinline__ int gh_lookup(const uint8_t *__restrict__ ids, int nstn, const uint8_t *id)
{
    int lo = 0, hi = nstn - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const uint8_t *t = ids + (size_t)mid * 11;
        int c = 0;
        for (int k = 0; k < 11 && c == 0; ++k) c = (int)id[k] - (int)t[k];
        if (c == 0) return mid;
        if (c < 0) hi = mid - 1; else lo = mid + 1;
    }
    return -1;
}

template <int PASS>
__global__ __launch_bounds__(256) void k_gh_tobs(const uint8_t *__restrict__ buf, int nfiles, const int64_t *__restrict__ file_off,
                                                 const uint32_t *__restrict__ cand, int64_t nlines, const uint8_t *__restrict__ ids,
                                                 int nstn, uint32_t elem_word, int64_t min_ymd, int64_t max_ymd, int64_t day0,
                                                 int64_t win0, int64_t nwin, uint32_t *__restrict__ win, int16_t *__restrict__ tobs,
                                                 uint32_t *__restrict__ bad, uint32_t bad_cap, uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int f = 0;
    int64_t start = 0, fend = 0;
    if (!gh_line(i, nlines, nfiles, file_off, cand, &f, &start, &fend)) return;
    int64_t e = start;                                           // every byte read lies in [start, fend), fend <= nbytes
    while (e < fend && buf[e] != 0x0a) ++e;
    if (e - start > 4096) return;                                 // (no by-year line: longer than any line the filter keeps)
    const int len = (int)(e - start);
    const uint8_t *line = buf + start;
    const uint8_t elem4[4] = {(uint8_t)elem_word, (uint8_t)(elem_word >> 8), (uint8_t)(elem_word >> 16), (uint8_t)(elem_word >> 24)};
    if (!gh_tobs_selected(line, len, elem4)) return;
    const int row = gh_lookup(ids, nstn, line);
    if (row < 0) return;                                         // the reference's KeyError
    int64_t didx = 0;
    int32_t v = 0;
    const int rc = gh_tobs_fields(line, len, min_ymd, max_ymd, day0, &didx, &v);
    if (rc == GH_TOBS_BAD) {
        if (PASS == 1) {
            const uint32_t k = atomicAdd(&counts[TWXGH_TC_BAD], 1u);
            if (k < bad_cap) { bad[2 * (size_t)k] = (uint32_t)f; bad[2 * (size_t)k + 1] = (uint32_t)(start - file_off[f]); }
        }
        return;
    }
    if (rc == GH_TOBS_OUTSIDE) {
        if (PASS == 0) atomicAdd(&counts[TWXGH_TC_OUTSIDE], 1u);
        return;
    }
    if (didx < win0 || didx >= win0 + nwin) {
        if (PASS == 0) atomicAdd(&counts[TWXGH_TC_OTHER_WINDOW], 1u);
        return;
    }
    const size_t slot = (size_t)row * (size_t)nwin + (size_t)(didx - win0);
    const uint32_t me = (uint32_t)start + 1u;
    if (PASS == 0) {
        atomicMax(&win[slot], me);
        atomicAdd(&counts[TWXGH_TC_VALUES], 1u);
    } else if (win[slot] == me) {
        tobs[slot] = (int16_t)v;
    }
}

// ---------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------
namespace {

// The arguments both entries share, checked before anything touches the device.  *ndays_out: days of the period.
int gh_check(const char *who, int64_t nbytes, int64_t nfiles, const int64_t *file_off, int32_t min_ymd, int32_t max_ymd,
             int64_t *day0, int64_t *ndays_out, char *errbuf, int errlen)
{
    char msg[320];
    if (nfiles < 1 || nfiles > INT32_MAX / 2 || nbytes < 0 || nbytes > TWXGH_MAX_BYTES) {
        snprintf(msg, sizeof msg, "%s: need nfiles >= 1 and 0 <= nbytes <= TWXGH_MAX_BYTES = %lld", who, (long long)TWXGH_MAX_BYTES);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!file_off || file_off[0] != 0 || file_off[nfiles] != nbytes) {
        snprintf(msg, sizeof msg, "%s: file_off must run from 0 to nbytes", who);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t f = 0; f < nfiles; ++f)
        if (file_off[f + 1] < file_off[f]) {
            snprintf(msg, sizeof msg, "%s: file_off[%lld] decreases", who, (long long)(f + 1));
            return qa_fail(errbuf, errlen, msg);
        }
    const int64_t y0 = min_ymd / 10000, m0 = (min_ymd / 100) % 100, d0 = min_ymd % 100;
    const int64_t y1 = max_ymd / 10000, m1 = (max_ymd / 100) % 100, d1 = max_ymd % 100;
    if (min_ymd < 0 || max_ymd < min_ymd || !gh_valid_date(y0, m0, d0) || !gh_valid_date(y1, m1, d1)) {
        snprintf(msg, sizeof msg, "%s: min_ymd = %d, max_ymd = %d is not a period of calendar days", who, (int)min_ymd, (int)max_ymd);
        return qa_fail(errbuf, errlen, msg);
    }
    *day0 = gh_days_from_civil(y0, m0, d0);
    *ndays_out = gh_days_from_civil(y1, m1, d1) - *day0 + 1;
    return 0;
}

// Upload the buffer (padded to 16 bytes, the pad zeroed) and the offsets, build the candidate list.  ms: the three kernels.
int gh_index(const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off, QaBuf &b_buf, QaBuf &b_off,
             QaBuf &b_cand, QaBuf &b_blk, uint32_t *ncand_out, QaTimer &tm, float *ms, char *errbuf, int errlen)
{
    const size_t padded = ((size_t)nbytes + 15) / 16 * 16 + 16;
    QACHK(hipMalloc(&b_buf.p, padded));
    QACHK(hipMemset(static_cast<uint8_t *>(b_buf.p) + (padded - 32), 0, 32));
    if (nbytes > 0) QACHK(hipMemcpy(b_buf.p, buf, (size_t)nbytes, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_off.p, (size_t)(nfiles + 1) * 8));
    QACHK(hipMemcpy(b_off.p, file_off, (size_t)(nfiles + 1) * 8, hipMemcpyHostToDevice));
    const int64_t nblk = std::max<int64_t>(1, (nbytes + GH_CHUNK - 1) / GH_CHUNK);
    QACHK(hipMalloc(&b_blk.p, (size_t)(2 * nblk + 1) * 4));
    uint32_t *d_cnt = static_cast<uint32_t *>(b_blk.p), *d_boff = d_cnt + nblk, *d_total = d_boff + nblk;
    const uint8_t *d_buf = static_cast<const uint8_t *>(b_buf.p);
    float a = 0.0f, b = 0.0f;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_gh_count, dim3((unsigned)nblk), dim3(256), 0, nullptr, d_buf, nbytes, d_cnt);
    QACHK(hipGetLastError());
    hipLaunchKernelGGL(k_gh_scan, dim3(1), dim3(1024), 0, nullptr, (const uint32_t *)d_cnt, nblk, d_boff, d_total);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&a));
    uint32_t ncand = 0;
    QACHK(hipMemcpy(&ncand, d_total, 4, hipMemcpyDeviceToHost));
    QACHK(hipMalloc(&b_cand.p, std::max<size_t>(16, (size_t)ncand * 4)));
    if (ncand > 0) {
        QACHK(tm.start());
        hipLaunchKernelGGL(k_gh_starts, dim3((unsigned)nblk), dim3(256), 0, nullptr, d_buf, nbytes, (const uint32_t *)d_boff, ncand,
                           static_cast<uint32_t *>(b_cand.p));
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&b));
    }
    *ncand_out = ncand;
    *ms = a + b;
    return 0;
}

}  // namespace

// twx_ghcn_index.h: the index for another unit, which owns what comes back in dev
int gh_index_build(const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off, void *dev[4], uint32_t *ncand,
                   float *ms, char *errbuf, int errlen)
{
    QaBuf b[4];
    QaTimer tm;
    dev[0] = dev[1] = dev[2] = dev[3] = nullptr;
    QACHK(tm.init());
    const int rc = gh_index(buf, nbytes, nfiles, file_off, b[0], b[1], b[2], b[3], ncand, tm, ms, errbuf, errlen);
    for (int k = 0; k < 4; ++k) { dev[k] = b[k].p; b[k].p = nullptr; }
    return rc;
}

extern "C" int twxgh_parse_dly(int device, const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off,
                               const int32_t *file_col, int64_t nrows, int32_t min_ymd, int32_t max_ymd, int64_t ndays,
                               float *val, uint8_t *qflag, uint32_t *bad_header, uint32_t *fallback, int64_t fallback_cap,
                               int64_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    int64_t day0 = 0, nd = 0;
    if (gh_check("twxgh_parse_dly", nbytes, nfiles, file_off, min_ymd, max_ymd, &day0, &nd, errbuf, errlen) != 0) return -1;
    if (nd != ndays) return qa_fail(errbuf, errlen, "twxgh_parse_dly: ndays is not the number of days from min_ymd to max_ymd");
    if ((nbytes > 0 && !buf) || !file_col || !val || !qflag || !bad_header || !counts || (fallback_cap > 0 && !fallback))
        return qa_fail(errbuf, errlen, "twxgh_parse_dly: null buffer");
    if (nrows < 1 || nrows > INT32_MAX || fallback_cap < 0 || fallback_cap > INT32_MAX ||
        (double)nrows * (double)ndays * 3.0 > (double)TWXGH_MAX_CELLS)
        return qa_fail(errbuf, errlen, "twxgh_parse_dly: need 1 <= nrows, 3 nrows ndays <= TWXGH_MAX_CELLS, 0 <= fallback_cap");
    {
        std::vector<uint8_t> seen((size_t)nrows, 0);
        for (int64_t f = 0; f < nfiles; ++f) {
            if (file_col[f] < 0 || file_col[f] >= nrows || seen[(size_t)file_col[f]])
                return qa_fail(errbuf, errlen, "twxgh_parse_dly: file_col must be distinct rows in 0 .. nrows - 1");
            seen[(size_t)file_col[f]] = 1;
        }
    }
    const size_t cells = 3 * (size_t)nrows * (size_t)ndays;
    float ms[TWXGH_NKERNELS];
    for (int i = 0; i < TWXGH_NKERNELS; ++i) ms[i] = 0.0f;

    QACHK(hipSetDevice(device));
    QaBuf b_buf, b_off, b_cand, b_blk, b_col, b_win, b_val, b_q, b_bad, b_fb, b_cnt;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_val.p, cells * 4));
    QACHK(hipMalloc(&b_q.p, cells));
    QACHK(hipMemset(b_q.p, 0, cells));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_gh_fill, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, nullptr, static_cast<float *>(b_val.p),
                       (int64_t)cells, (float)GH_MISSING);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[0]));
    QACHK(hipMalloc(&b_bad.p, (size_t)nfiles * 4));
    QACHK(hipMemset(b_bad.p, 0xff, (size_t)nfiles * 4));
    QACHK(hipMalloc(&b_cnt.p, 16));
    QACHK(hipMemset(b_cnt.p, 0, 16));
    unsigned long long *d_nw = static_cast<unsigned long long *>(b_cnt.p);
    uint32_t *d_fbn = reinterpret_cast<uint32_t *>(d_nw + 1);
    uint32_t ncand = 0;
    int64_t nlines = 0;
    if (nbytes > 0) {
        if (gh_index(buf, nbytes, nfiles, file_off, b_buf, b_off, b_cand, b_blk, &ncand, tm, &ms[1], errbuf, errlen) != 0) return -1;
        nlines = nfiles + (int64_t)ncand;
        QACHK(hipMalloc(&b_col.p, (size_t)nfiles * 4));
        QACHK(hipMemcpy(b_col.p, file_col, (size_t)nfiles * 4, hipMemcpyHostToDevice));
        QACHK(hipMalloc(&b_win.p, cells * 4));
        QACHK(hipMemset(b_win.p, 0, cells * 4));
        QACHK(hipMalloc(&b_fb.p, std::max<size_t>(16, (size_t)fallback_cap * TWXGH_FB_WORDS * 4)));
        const unsigned grid = (unsigned)((nlines + GH_LINES_PER_WG - 1) / GH_LINES_PER_WG);
#define GH_DLY_ARGS                                                                                                          \
    static_cast<const uint8_t *>(b_buf.p), (int)nfiles, static_cast<const int64_t *>(b_off.p),                             \
        static_cast<const int32_t *>(b_col.p), static_cast<const uint32_t *>(b_cand.p), nlines, nrows, ndays,              \
        (int64_t)min_ymd, (int64_t)max_ymd, day0, static_cast<uint32_t *>(b_win.p), static_cast<float *>(b_val.p),         \
        static_cast<uint8_t *>(b_q.p), static_cast<uint32_t *>(b_bad.p), static_cast<uint32_t *>(b_fb.p),                  \
        (uint32_t)fallback_cap, d_fbn, d_nw
        QACHK(tm.start());
        hipLaunchKernelGGL(k_gh_dly<0>, dim3(grid), dim3(256), 0, nullptr, GH_DLY_ARGS);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[2]));
        QACHK(tm.start());
        hipLaunchKernelGGL(k_gh_dly<1>, dim3(grid), dim3(256), 0, nullptr, GH_DLY_ARGS);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[3]));
#undef GH_DLY_ARGS
    }
    unsigned long long nw = 0;
    uint32_t nfb = 0;
    QACHK(hipMemcpy(&nw, d_nw, 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(&nfb, d_fbn, 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(val, b_val.p, cells * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(qflag, b_q.p, cells, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(bad_header, b_bad.p, (size_t)nfiles * 4, hipMemcpyDeviceToHost));
    const size_t nget = (size_t)std::min<int64_t>(nfb, fallback_cap);
    if (nget > 0) {
        QACHK(hipMemcpy(fallback, b_fb.p, nget * TWXGH_FB_WORDS * 4, hipMemcpyDeviceToHost));
        struct Row { uint32_t w[TWXGH_FB_WORDS]; };
        Row *r = reinterpret_cast<Row *>(fallback);                // buffer order, then day: the slots the atomics gave are gone
        std::sort(r, r + nget, [](const Row &x, const Row &y) { return x.w[7] != y.w[7] ? x.w[7] < y.w[7] : x.w[3] < y.w[3]; });
    }
    counts[TWXGH_DC_LINES] = nlines;
    counts[TWXGH_DC_VALUES] = (int64_t)nw;
    counts[TWXGH_DC_FALLBACK] = (int64_t)nfb;
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxgh_parse_tobs(int device, const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off,
                                int64_t nstn, const uint8_t *ids, const char *element, int32_t min_ymd, int32_t max_ymd,
                                int64_t win0, int64_t nwin, int16_t *tobs, uint32_t *bad, int64_t bad_cap, int64_t *counts,
                                float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    int64_t day0 = 0, nd = 0;
    if (gh_check("twxgh_parse_tobs", nbytes, nfiles, file_off, min_ymd, max_ymd, &day0, &nd, errbuf, errlen) != 0) return -1;
    if ((nbytes > 0 && !buf) || !ids || !element || !tobs || !counts || (bad_cap > 0 && !bad))
        return qa_fail(errbuf, errlen, "twxgh_parse_tobs: null buffer");
    if (strlen(element) != 4) return qa_fail(errbuf, errlen, "twxgh_parse_tobs: the element is four characters");
    if (nstn < 1 || nstn > INT32_MAX || win0 < 0 || nwin < 1 || win0 + nwin > nd || bad_cap < 0 || bad_cap > INT32_MAX ||
        (double)nstn * (double)nwin > (double)TWXGH_MAX_CELLS)
        return qa_fail(errbuf, errlen, "twxgh_parse_tobs: need nstn >= 1, a window of days inside the period, nstn nwin <= "
                                       "TWXGH_MAX_CELLS and bad_cap >= 0");
    for (int64_t s = 1; s < nstn; ++s)
        if (memcmp(ids + (s - 1) * 11, ids + s * 11, 11) >= 0)
            return qa_fail(errbuf, errlen, "twxgh_parse_tobs: the id table must be sorted and without duplicates");
    const size_t cells = (size_t)nstn * (size_t)nwin;
    float ms[TWXGH_NKERNELS];
    for (int i = 0; i < TWXGH_NKERNELS; ++i) ms[i] = 0.0f;
    uint32_t cnt[TWXGH_TC_N];
    memset(cnt, 0, sizeof cnt);
    int64_t nlines = 0;
    if (nbytes > 0) {
        QACHK(hipSetDevice(device));
        QaBuf b_buf, b_off, b_cand, b_blk, b_ids, b_win, b_out, b_bad, b_cnt;
        QaTimer tm;
        QACHK(tm.init());
        uint32_t ncand = 0;
        if (gh_index(buf, nbytes, nfiles, file_off, b_buf, b_off, b_cand, b_blk, &ncand, tm, &ms[1], errbuf, errlen) != 0) return -1;
        nlines = nfiles + (int64_t)ncand;
        QACHK(hipMalloc(&b_ids.p, (size_t)nstn * 11));
        QACHK(hipMemcpy(b_ids.p, ids, (size_t)nstn * 11, hipMemcpyHostToDevice));
        QACHK(hipMalloc(&b_win.p, cells * 4));
        QACHK(hipMemset(b_win.p, 0, cells * 4));
        QACHK(hipMalloc(&b_out.p, cells * 2));
        QACHK(hipMemcpy(b_out.p, tobs, cells * 2, hipMemcpyHostToDevice));
        QACHK(hipMalloc(&b_bad.p, std::max<size_t>(16, (size_t)bad_cap * 8)));
        QACHK(hipMalloc(&b_cnt.p, sizeof cnt));
        QACHK(hipMemset(b_cnt.p, 0, sizeof cnt));
        uint32_t ew = 0;
        memcpy(&ew, element, 4);
        const unsigned grid = (unsigned)((nlines + 255) / 256);
#define GH_TOBS_ARGS                                                                                                         \
    static_cast<const uint8_t *>(b_buf.p), (int)nfiles, static_cast<const int64_t *>(b_off.p),                             \
        static_cast<const uint32_t *>(b_cand.p), nlines, static_cast<const uint8_t *>(b_ids.p), (int)nstn, ew,             \
        (int64_t)min_ymd, (int64_t)max_ymd, day0, win0, nwin, static_cast<uint32_t *>(b_win.p),                            \
        static_cast<int16_t *>(b_out.p), static_cast<uint32_t *>(b_bad.p), (uint32_t)bad_cap, static_cast<uint32_t *>(b_cnt.p)
        QACHK(tm.start());
        hipLaunchKernelGGL(k_gh_tobs<0>, dim3(grid), dim3(256), 0, nullptr, GH_TOBS_ARGS);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[2]));
        QACHK(tm.start());
        hipLaunchKernelGGL(k_gh_tobs<1>, dim3(grid), dim3(256), 0, nullptr, GH_TOBS_ARGS);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[3]));
#undef GH_TOBS_ARGS
        QACHK(hipMemcpy(cnt, b_cnt.p, sizeof cnt, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(tobs, b_out.p, cells * 2, hipMemcpyDeviceToHost));
        const size_t nget = (size_t)std::min<int64_t>(cnt[TWXGH_TC_BAD], bad_cap);
        if (nget > 0) {
            QACHK(hipMemcpy(bad, b_bad.p, nget * 8, hipMemcpyDeviceToHost));
            struct Row { uint32_t f, pos; };
            Row *r = reinterpret_cast<Row *>(bad);
            std::sort(r, r + nget, [](const Row &x, const Row &y) { return x.f != y.f ? x.f < y.f : x.pos < y.pos; });
        }
    }
    counts[TWXGH_TC_VALUES] = cnt[TWXGH_TC_VALUES];
    counts[TWXGH_TC_OUTSIDE] = cnt[TWXGH_TC_OUTSIDE];
    counts[TWXGH_TC_OTHER_WINDOW] = cnt[TWXGH_TC_OTHER_WINDOW];
    counts[TWXGH_TC_BAD] = cnt[TWXGH_TC_BAD];
    counts[TWXGH_TC_N] = nlines;
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

// Page-locked host memory for the file buffer: the reader threads fill it, the upload is one copy from it.
extern "C" void *twxgh_host_alloc(int64_t nbytes)
{
    void *p = nullptr;
    if (nbytes < 1 || hipHostMalloc(&p, (size_t)nbytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

extern "C" void twxgh_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}
