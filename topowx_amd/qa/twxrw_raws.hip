// twxrw_raws.hip -- libtwxqa.so: the RAWS ingest of step04.  InsertRaws.parse_stn_obs
// (twx/db/create_db_all_stations.py:1177-1233) for a batch of WRCC daily listings in one call.  The twentieth translation
// unit of the library (include/twx_raws.h, twxrw_*).  What a token is and what the device decides of a field is
// twx_raws_field.h, shared with a CPU program of the tests.
//
// The line index is twx_ghcn.hip's (twx_ghcn_index.h): the files laid end to end, the positions after the newlines.
//   k_rw_body   a thread per file: the start of its 8th line (the 7th candidate inside the file), or none
//   k_rw_stop   a thread per 16 bytes (two aligned 128-bit loads, the second for a match that runs over): every "Copyright"
//               at or after its file's 8th line and inside the file takes an integer atomicMin of its position per file
//   k_rw_line<pass>  a wavefront per line, RW_LINES_PER_WAVE consecutive lines per wavefront.  A line's end is the next
//               candidate of the index (or the file's end), so the body test and the stop test come before any byte is read.
//               The line is read in windows of 1 KiB, one aligned 128-bit load per lane, only loads that start below the
//               line's end; every lane marks its bytes that are no whitespace, a token starts where such a byte follows one
//               that is not (the previous lane's last bit by a shuffle, the previous window's by a carried bit); the token
//               counts are scanned over the wavefront and carried from window to window, so tokens 0, 9, 10 and 14 are
//               located wherever they fall in a line of any length.  No LDS.  The date is decided by every lane alike, the
//               three values by lanes 0 .. 2, a field each.
//
// Duplicates.  The LAST line that gives a (file, day) its values wins (a stated deviation: the reference fails).  Pass 0
// takes an integer atomicMax of "line position + 1" per (file, day); pass 1 parses again and only the winner writes its
// three values.  A position is unique, so no result depends on which wave got there first; there are no floating-point
// atomics.  A line with a field only Python can decide takes no part: pass 1 lists the field with the winning position,
// and the caller settles such lines in position order.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "twx_ghcn_index.h"
#include "twx_raws.h"
#include "twx_qa_common.h"
#include "twx_raws_field.h"

#define RW_WAVES_PER_WG 4
#define RW_LINES_PER_WAVE 8
#define RW_WINDOW 1024                       // 64 lanes x 16 bytes
#define RW_NONE 0xffffffffu
#define RW_SKIP_LINES 7

// device counters
#define RW_D_LINES 0
#define RW_D_BODY 1
#define RW_D_SKIPPED 2
#define RW_D_VALUES 3
#define RW_D_DUPLICATES 4
#define RW_D_UNCERTAIN 5
#define RW_D_RAISE 6
#define RW_D_DATE_UNCERTAIN 7
#define RW_D_N 8

__global__ __launch_bounds__(256) void k_rw_fill(float *__restrict__ a, int64_t n, float v)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

__global__ __launch_bounds__(256) void k_rw_body(int nfiles, const int64_t *__restrict__ file_off, const uint32_t *__restrict__ cand,
                                                 uint32_t ncand, uint32_t *__restrict__ body_start)
{
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    if (f >= nfiles) return;
    const int64_t a = file_off[f], b = file_off[f + 1];
    uint32_t lo = 0, hi = ncand;                                  // the first candidate above the file's start
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)cand[mid] > a) hi = mid; else lo = mid + 1;
    }
    const uint64_t j = (uint64_t)lo + (RW_SKIP_LINES - 1);
    body_start[f] = (j < ncand && (int64_t)cand[j] < b) ? cand[j] : RW_NONE;
}

__global__ __launch_bounds__(256) void k_rw_stop(const uint8_t *__restrict__ buf, int64_t nbytes, int nfiles,
                                                 const int64_t *__restrict__ file_off, const uint32_t *__restrict__ body_start,
                                                 uint32_t *__restrict__ stop)
{
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= nbytes) return;                                     // both loads lie inside the zero-padded allocation
    const uint4 a = *reinterpret_cast<const uint4 *>(buf + p0);
    const uint4 b = *reinterpret_cast<const uint4 *>(buf + p0 + 16);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint8_t word[9] = {'C', 'o', 'p', 'y', 'r', 'i', 'g', 'h', 't'};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        bool hit = true;
#pragma unroll
        for (int c = 0; c < 9; ++c) hit = hit && (uint8_t)(w[(k + c) >> 2] >> (8 * ((k + c) & 3))) == word[c];
        if (hit) {                                                // (the padding is zero: a hit lies below nbytes)
            const int64_t q = p0 + k;
            const int f = gh_file_of(file_off, nfiles, q);
            if (q + 9 <= file_off[f + 1] && (uint32_t)q >= body_start[f]) atomicMin(&stop[f], (uint32_t)q);
        }
    }
}

namespace {

__device__ __forceinline__ void rw_list(uint32_t *__restrict__ list, uint32_t cap, unsigned long long *__restrict__ count,
                                        uint32_t f, uint32_t pos, uint32_t field, uint32_t off, uint32_t len, uint32_t win,
                                        uint32_t day, uint32_t start)
{
    const unsigned long long k = atomicAdd(count, 1ull);
    if (k < cap) {
        uint32_t *e = list + (size_t)k * TWXRW_ENTRY_WORDS;
        e[0] = f; e[1] = pos; e[2] = field; e[3] = off; e[4] = len; e[5] = win; e[6] = day; e[7] = start;
    }
}

}  // namespace

// PASS 0 claims the (file, day) slots and counts; PASS 1 writes what won and fills the two lists.
template <int PASS>
__global__ __launch_bounds__(256) void k_rw_line(const uint8_t *__restrict__ buf, int nfiles, const int64_t *__restrict__ file_off,
                                                 const uint32_t *__restrict__ cand, int64_t ncand, int64_t nlines,
                                                 const uint32_t *__restrict__ body_start, const uint32_t *__restrict__ stop,
                                                 int64_t ndays, int64_t min_ymd, int64_t max_ymd, int64_t day0,
                                                 uint32_t *__restrict__ win, float *__restrict__ val,
                                                 uint32_t *__restrict__ unc, uint32_t unc_cap, uint32_t *__restrict__ rse,
                                                 uint32_t rse_cap, unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * RW_WAVES_PER_WG + (threadIdx.x >> 6);
    const size_t plane = (size_t)nfiles * (size_t)ndays;
    unsigned long long c_lines = 0, c_body = 0, c_skipped = 0, c_values = 0, c_dup = 0;
    for (int r = 0; r < RW_LINES_PER_WAVE; ++r) {                 // everything but the window loads is the same in every lane
        const int64_t i = wave * RW_LINES_PER_WAVE + r;
        int f = 0;
        int64_t start = 0, fend = 0;
        if (!gh_line(i, nlines, nfiles, file_off, cand, &f, &start, &fend)) continue;
        ++c_lines;
        if (i < nfiles || (uint32_t)start < body_start[f]) continue;
        const int64_t j = i - nfiles;
        const uint32_t nx = j + 1 < ncand ? cand[j + 1] : RW_NONE;
        const int64_t lineend = (int64_t)nx <= fend ? (int64_t)nx - 1 : fend;     // start < lineend <= fend <= nbytes
        if ((int64_t)stop[f] < lineend) continue;                 // the line with the first "Copyright", or one after it
        ++c_body;

        // ---- tokens 0, 9, 10 and 14 ----
        uint32_t tpos[RW_NFIELDS] = {0u, 0u, 0u, 0u};
        int ntok = 0;
        uint32_t carry = 0;                                       // the previous window ended inside a token
        for (int64_t base = start & ~(int64_t)15; base < lineend && ntok < RW_NTOKENS; base += RW_WINDOW) {
            const int64_t p = base + 16 * lane;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (p < lineend) w = *reinterpret_cast<const uint4 *>(buf + p);       // aligned, starts below nbytes
            const int lo = (int)std::min<int64_t>(16, std::max<int64_t>(0, start - p));
            const int hi = (int)std::min<int64_t>(16, std::max<int64_t>(0, lineend - p));
            const uint32_t m = rw_nonspace16(w.x, w.y, w.z, w.w, lo, hi);
            uint32_t before = __shfl_up(m >> 15, 1);
            if (lane == 0) before = carry;
            const uint32_t s = m & ~((m << 1) | before) & 0xffffu;               // the bytes that start a token
            const int c = __popc(s);
            int incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            const int excl = ntok + incl - c;
#pragma unroll
            for (int q = 0; q < RW_NFIELDS; ++q) {
                const int T = rw_field_token(q);
                const bool mine = excl <= T && T < excl + c;
                const unsigned long long who = __ballot(mine);
                if (who) {
                    const uint32_t at = mine ? (uint32_t)(p + rw_nth_bit(s, T - excl)) : 0u;
                    tpos[q] = __shfl(at, __ffsll((long long)who) - 1);
                }
            }
            ntok += __shfl(incl, 63);
            carry = __shfl(m >> 15, 63);
        }

        // ---- the line's decision ----
        const uint32_t pos = (uint32_t)(start - file_off[f]);
        if (ntok == 0) {                                          // vals[0]: IndexError
            if (PASS == 1 && lane == 0)
                rw_list(rse, rse_cap, &cnt[RW_D_RAISE], (uint32_t)f, pos, TWXRW_RAISE_EMPTY, 0u, 0u, 0u, RW_NONE, (uint32_t)start);
            continue;
        }
        const int n0 = rw_token_len(buf + tpos[0], lineend - (int64_t)tpos[0]);
        int64_t didx = 0;
        const int ds = rw_date(buf + tpos[0], n0, min_ymd, max_ymd, day0, &didx);
        if (ds == RW_DATE_UNCERTAIN) {
            if (PASS == 1 && lane == 0) {
                rw_list(unc, unc_cap, &cnt[RW_D_UNCERTAIN], (uint32_t)f, pos, RW_FIELD_DATE, tpos[0] - (uint32_t)start, (uint32_t)n0,
                        0u, RW_NONE, (uint32_t)start);
                atomicAdd(&cnt[RW_D_DATE_UNCERTAIN], 1ull);
            }
            continue;
        }
        if (ds == RW_DATE_SKIP) { ++c_skipped; continue; }
        if (ds == RW_DATE_OUTSIDE) continue;
        if (ntok < RW_NTOKENS) {                                  // vals[9], vals[10] or vals[14]: the caller finds which raises
            if (PASS == 1 && lane == 0)
                rw_list(rse, rse_cap, &cnt[RW_D_RAISE], (uint32_t)f, pos, TWXRW_RAISE_FEW, 0u, (uint32_t)ntok, 0u, (uint32_t)didx,
                        (uint32_t)start);
            continue;
        }
        float v = 0.0f;
        int st = RW_OK, n = 0;
        if (lane < 3) {                                           // lane k: field k + 1
            const uint32_t tp = lane == 0 ? tpos[1] : (lane == 1 ? tpos[2] : tpos[3]);
            n = rw_token_len(buf + tp, lineend - (int64_t)tp);
            st = rw_value(buf + tp, n, lane + 1, &v);
        }
        const int st0 = __shfl(st, 0), st1 = __shfl(st, 1), st2 = __shfl(st, 2);
        const int n1 = __shfl(n, 0), n2 = __shfl(n, 1), n3 = __shfl(n, 2);
        const float v1 = __shfl(v, 0), v2 = __shfl(v, 1), v3 = __shfl(v, 2);
        const size_t slot = (size_t)f * (size_t)ndays + (size_t)didx;
        const uint32_t me = (uint32_t)start + 1u;
        if (st0 != RW_OK || st1 != RW_OK || st2 != RW_OK) {
            if (PASS == 1 && lane == 0) {
                const uint32_t w = win[slot];
                if (st0 != RW_OK)
                    rw_list(unc, unc_cap, &cnt[RW_D_UNCERTAIN], (uint32_t)f, pos, RW_FIELD_TMAX, tpos[1] - (uint32_t)start,
                            (uint32_t)n1, w, (uint32_t)didx, (uint32_t)start);
                if (st1 != RW_OK)
                    rw_list(unc, unc_cap, &cnt[RW_D_UNCERTAIN], (uint32_t)f, pos, RW_FIELD_TMIN, tpos[2] - (uint32_t)start,
                            (uint32_t)n2, w, (uint32_t)didx, (uint32_t)start);
                if (st2 != RW_OK)
                    rw_list(unc, unc_cap, &cnt[RW_D_UNCERTAIN], (uint32_t)f, pos, RW_FIELD_PRCP, tpos[3] - (uint32_t)start,
                            (uint32_t)n3, w, (uint32_t)didx, (uint32_t)start);
            }
            continue;
        }
        if (PASS == 0) {
            if (lane == 0) atomicMax(&win[slot], me);
            ++c_values;
        } else if (win[slot] == me) {
            if (lane == 0) {
                val[(size_t)GH_ELEM_TMAX * plane + slot] = v1;
                val[(size_t)GH_ELEM_TMIN * plane + slot] = v2;
                val[(size_t)GH_ELEM_PRCP * plane + slot] = v3;
            }
        } else {
            ++c_dup;
        }
    }
    if (lane == 0) {
        if (PASS == 0) {
            if (c_lines) atomicAdd(&cnt[RW_D_LINES], c_lines);
            if (c_body) atomicAdd(&cnt[RW_D_BODY], c_body);
            if (c_skipped) atomicAdd(&cnt[RW_D_SKIPPED], c_skipped);
            if (c_values) atomicAdd(&cnt[RW_D_VALUES], c_values);
        } else if (c_dup) {
            atomicAdd(&cnt[RW_D_DUPLICATES], c_dup);
        }
    }
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
namespace {

void rw_sort(uint32_t *list, size_t n)
{
    struct Row { uint32_t w[TWXRW_ENTRY_WORDS]; };
    Row *r = reinterpret_cast<Row *>(list);                        // buffer order, then field: the slots the atomics gave are gone
    std::sort(r, r + n, [](const Row &x, const Row &y) { return x.w[7] != y.w[7] ? x.w[7] < y.w[7] : x.w[2] < y.w[2]; });
}

}  // namespace

extern "C" int twxrw_parse(int device, const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off,
                           int32_t min_ymd, int32_t max_ymd, int64_t ndays, float *val, uint32_t *win, uint32_t *uncertain,
                           int64_t uncertain_cap, uint32_t *raise, int64_t raise_cap, int64_t *counts, float *kernel_ms,
                           char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nfiles < 1 || nfiles > INT32_MAX / 2 || nbytes < 0 || nbytes > TWXRW_MAX_BYTES)
        return qa_fail(errbuf, errlen, "twxrw_parse: need nfiles >= 1 and 0 <= nbytes <= TWXRW_MAX_BYTES");
    if (!file_off || file_off[0] != 0 || file_off[nfiles] != nbytes)
        return qa_fail(errbuf, errlen, "twxrw_parse: file_off must run from 0 to nbytes");
    for (int64_t f = 0; f < nfiles; ++f)
        if (file_off[f + 1] < file_off[f]) return qa_fail(errbuf, errlen, "twxrw_parse: file_off decreases");
    const int64_t y0 = min_ymd / 10000, m0 = (min_ymd / 100) % 100, d0 = min_ymd % 100;
    const int64_t y1 = max_ymd / 10000, m1 = (max_ymd / 100) % 100, d1 = max_ymd % 100;
    if (min_ymd < 0 || max_ymd < min_ymd || !gh_valid_date(y0, m0, d0) || !gh_valid_date(y1, m1, d1))
        return qa_fail(errbuf, errlen, "twxrw_parse: min_ymd .. max_ymd is not a period of calendar days");
    const int64_t day0 = gh_days_from_civil(y0, m0, d0);
    if (gh_days_from_civil(y1, m1, d1) - day0 + 1 != ndays)
        return qa_fail(errbuf, errlen, "twxrw_parse: ndays is not the number of days from min_ymd to max_ymd");
    if ((nbytes > 0 && !buf) || !val || !win || !counts || (uncertain_cap > 0 && !uncertain) || (raise_cap > 0 && !raise))
        return qa_fail(errbuf, errlen, "twxrw_parse: null buffer");
    if (uncertain_cap < 0 || uncertain_cap > INT32_MAX || raise_cap < 0 || raise_cap > INT32_MAX ||
        (double)nfiles * (double)ndays * 3.0 > (double)TWXRW_MAX_CELLS)
        return qa_fail(errbuf, errlen, "twxrw_parse: need 3 nfiles ndays <= TWXRW_MAX_CELLS and list capacities >= 0");
    const size_t plane = (size_t)nfiles * (size_t)ndays, cells = 3 * plane;
    float ms[TWXRW_NKERNELS];
    for (int i = 0; i < TWXRW_NKERNELS; ++i) ms[i] = 0.0f;
    unsigned long long cnt[RW_D_N];
    memset(cnt, 0, sizeof cnt);

    QACHK(hipSetDevice(device));
    QaBuf b_buf, b_off, b_cand, b_blk, b_val, b_win, b_body, b_stop, b_unc, b_rse, b_cnt;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_val.p, cells * 4));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_rw_fill, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, nullptr, static_cast<float *>(b_val.p),
                       (int64_t)cells, (float)RW_MISSING);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[0]));
    if (nbytes > 0) {
        void *dev[4] = {nullptr, nullptr, nullptr, nullptr};
        uint32_t ncand = 0;
        const int rc = gh_index_build(buf, nbytes, nfiles, file_off, dev, &ncand, &ms[1], errbuf, errlen);
        b_buf.p = dev[0], b_off.p = dev[1], b_cand.p = dev[2], b_blk.p = dev[3];
        if (rc != 0) return -1;
        const int64_t nlines = nfiles + (int64_t)ncand;
        QACHK(hipMalloc(&b_win.p, plane * 4));
        QACHK(hipMemset(b_win.p, 0, plane * 4));
        QACHK(hipMalloc(&b_body.p, (size_t)nfiles * 4));
        QACHK(hipMalloc(&b_stop.p, (size_t)nfiles * 4));
        QACHK(hipMemset(b_stop.p, 0xff, (size_t)nfiles * 4));
        QACHK(hipMalloc(&b_unc.p, std::max<size_t>(16, (size_t)uncertain_cap * TWXRW_ENTRY_WORDS * 4)));
        QACHK(hipMalloc(&b_rse.p, std::max<size_t>(16, (size_t)raise_cap * TWXRW_ENTRY_WORDS * 4)));
        QACHK(hipMalloc(&b_cnt.p, sizeof cnt));
        QACHK(hipMemset(b_cnt.p, 0, sizeof cnt));
        const uint8_t *d_buf = static_cast<const uint8_t *>(b_buf.p);
        const int64_t *d_off = static_cast<const int64_t *>(b_off.p);
        const uint32_t *d_cand = static_cast<const uint32_t *>(b_cand.p);
        QACHK(tm.start());
        hipLaunchKernelGGL(k_rw_body, dim3((unsigned)((nfiles + 255) / 256)), dim3(256), 0, nullptr, (int)nfiles, d_off, d_cand, ncand,
                           static_cast<uint32_t *>(b_body.p));
        QACHK(hipGetLastError());
        hipLaunchKernelGGL(k_rw_stop, dim3((unsigned)((nbytes + 4095) / 4096)), dim3(256), 0, nullptr, d_buf, nbytes, (int)nfiles, d_off,
                           static_cast<const uint32_t *>(b_body.p), static_cast<uint32_t *>(b_stop.p));
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[2]));
        const int64_t per_wg = RW_WAVES_PER_WG * RW_LINES_PER_WAVE;
        const unsigned grid = (unsigned)((nlines + per_wg - 1) / per_wg);
#define RW_LINE_ARGS                                                                                                         \
    d_buf, (int)nfiles, d_off, d_cand, (int64_t)ncand, nlines, static_cast<const uint32_t *>(b_body.p),                    \
        static_cast<const uint32_t *>(b_stop.p), ndays, (int64_t)min_ymd, (int64_t)max_ymd, day0,                          \
        static_cast<uint32_t *>(b_win.p), static_cast<float *>(b_val.p), static_cast<uint32_t *>(b_unc.p),                 \
        (uint32_t)uncertain_cap, static_cast<uint32_t *>(b_rse.p), (uint32_t)raise_cap,                                    \
        static_cast<unsigned long long *>(b_cnt.p)
        QACHK(tm.start());
        hipLaunchKernelGGL(k_rw_line<0>, dim3(grid), dim3(256), 0, nullptr, RW_LINE_ARGS);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[3]));
        QACHK(tm.start());
        hipLaunchKernelGGL(k_rw_line<1>, dim3(grid), dim3(256), 0, nullptr, RW_LINE_ARGS);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[4]));
#undef RW_LINE_ARGS
        QACHK(hipMemcpy(cnt, b_cnt.p, sizeof cnt, hipMemcpyDeviceToHost));
        const size_t nu = (size_t)std::min<int64_t>((int64_t)cnt[RW_D_UNCERTAIN], uncertain_cap);
        const size_t nr = (size_t)std::min<int64_t>((int64_t)cnt[RW_D_RAISE], raise_cap);
        if (nu > 0) {
            QACHK(hipMemcpy(uncertain, b_unc.p, nu * TWXRW_ENTRY_WORDS * 4, hipMemcpyDeviceToHost));
            rw_sort(uncertain, nu);
        }
        if (nr > 0) {
            QACHK(hipMemcpy(raise, b_rse.p, nr * TWXRW_ENTRY_WORDS * 4, hipMemcpyDeviceToHost));
            rw_sort(raise, nr);
        }
        if (cnt[RW_D_DATE_UNCERTAIN] > 0) QACHK(hipMemcpy(win, b_win.p, plane * 4, hipMemcpyDeviceToHost));
    }
    QACHK(hipMemcpy(val, b_val.p, cells * 4, hipMemcpyDeviceToHost));
    counts[TWXRW_C_LINES] = (int64_t)cnt[RW_D_LINES];
    counts[TWXRW_C_BODY] = (int64_t)cnt[RW_D_BODY];
    counts[TWXRW_C_SKIPPED] = (int64_t)cnt[RW_D_SKIPPED];
    counts[TWXRW_C_VALUES] = (int64_t)cnt[RW_D_VALUES];
    counts[TWXRW_C_DUPLICATES] = (int64_t)cnt[RW_D_DUPLICATES];
    counts[TWXRW_C_UNCERTAIN] = (int64_t)cnt[RW_D_UNCERTAIN];
    counts[TWXRW_C_RAISE] = (int64_t)cnt[RW_D_RAISE];
    counts[TWXRW_C_DATE_UNCERTAIN] = (int64_t)cnt[RW_D_DATE_UNCERTAIN];
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
