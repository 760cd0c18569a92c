// twx_prcpqa.hip -- libtwxqa.so: the non-spatial chain of the precipitation QA, run_qa_non_spatial (twx/qa/qa_prcp.py:135-176),
// and the two checks the reference defines but leaves out of its chain (_qa_streak :379-407, _qa_frequent :409-445), for many
// stations in one call.  The fourteenth translation unit of the library (include/twx_qa.h, twxpq_*).
//
// State.  As in twx_nonspatial.hip the flag array IS the working copy: an observation is in the series ("live") exactly
// while its flag is 1 (_update_obs_flags, :860-865, sets a flagged value to NaN and writes the number where the flag was 1),
// a check reads "flag == 1 ? value : NaN" and a removal is one byte store.  Every check decides on one snapshot: a kernel
// either owns the series it reads (one workgroup or wavefront per series, barriers between deciding and removing), writes
// its decisions into a mark array that a second kernel applies (the frequent-value check), or reads only its own day.
//
// k_pq_init      thread = (station, day): missing (2).
// k_pq_dups      one 256-thread workgroup per station: duplicate years (4), duplicate months of a year (6), the same
//                calendar month of two years (5), each side with >= 3 live values > 0, compared by position over the
//                shorter with early exit; then the impossible values (8).  LDS: 26 bytes per year, 3.6 KiB at the cap.
// k_pq_streak    one wavefront per station walks the live values > 0 in blocks of 64 days (k_ns_streak's ballots): a run
//                of >= 20 equal values is flagged when a different value ends it (9).
// k_pq_compact   one 256-thread workgroup per station: the day indices of the live values > 0, in order (a block scan).
// k_pq_frequent  thread = (station, start x of the compacted sequence): the window x .. x + 9, every value of it against
//                the four tiers; decisions go to a mark array.   k_pq_apply: the marks become 19.
// k_pq_gap       one 256-thread workgroup per (station, calendar month): the live values > 0 of the month over all years,
//                sorted in LDS (bitonic, float32); the first float32 step >= 30.0 gives the bound (10).  LDS 16 KiB.
// k_pq_pctiles   THE TABLE: one 256-thread workgroup per (station, row of the 366): the live values > 0 on the 29 month-days
//                around the row's date (of 2004) over all years are compacted into LDS (<= 29 per year,
//                TWXPQ_MAX_WINDOW_VALUES = 4096 floats = 16 KiB: 8 workgroups of 4 waves fill the 32 wave slots of a compute
//                unit with 128 KiB of its 160 KiB), sorted there (bitonic over the next power of two), and five threads
//                read the two order statistics of a percentile each and interpolate in fp64 (numpy's two-sided lerp).
//                The slot a value lands in depends on the order of an integer atomic; the sort erases it, so two calls give
//                the same bytes.
// k_pq_clim      thread = (station, day): a live value > 0 that is >= m x p95 of the row of the day's own year (15).
// fp64 on float32 values widened exactly for the percentiles and the comparisons against them; float32 where the
// reference's result is one float32 operation (the impossible bound, the gap step).  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_series.h"

#define PQ_OK 1                              // qa_prcp.py:37-57
#define PQ_MISSING 2
#define PQ_DUP_YEAR 4
#define PQ_DUP_MONTH 5
#define PQ_DUP_YEAR_MONTH 6
#define PQ_IMPOSS_VALUE 8
#define PQ_STREAK 9
#define PQ_GAP 10
#define PQ_CLIM_OUTLIER 15
#define PQ_FREQUENT 19
#define PQ_MAX_VALUE 182.88f                 // qa_prcp.py:61, rounded to float32 as the comparison does
#define PQ_STREAK_LEN 20                     // qa_prcp.py:72
#define PQ_GAP_THRES 30.0f                   // qa_prcp.py:73
#define PQ_MIN_DUP_VALUES 3                  // qa_prcp.py:266, 299, 362
#define PQ_FREQ_WINDOW 10                    // qa_prcp.py:427
#define PQ_MAX_YEARS (TWXPQ_MAX_WINDOW_VALUES / 29)
#define PQ_ROWS TWXPQ_PCTILE_ROWS
#define PQ_COLS TWXPQ_PCTILE_COLS

namespace {

// a value the percentile table, the streak, frequent-value, gap and outlier checks look at
__device__ __forceinline__ bool pq_wet(float v) { return v > 0.0f && qa_finitef(v); }

}  // namespace

__global__ __launch_bounds__(256) void k_pq_init(int64_t total, const float *__restrict__ prcp, uint8_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float v = prcp[i];
    flag[i] = v != v ? PQ_MISSING : PQ_OK;
}

__global__ __launch_bounds__(256) void k_pq_dups(int64_t ndays, QaCal cal, const float *__restrict__ prcp, uint8_t *flag)
{
    __shared__ int cnt_y[PQ_MAX_YEARS];
    __shared__ uint8_t dup_y[PQ_MAX_YEARS];
    __shared__ uint8_t cnt_m[PQ_MAX_YEARS * 12], dup_m[PQ_MAX_YEARS * 12];
    const int tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * (size_t)ndays;
    const int nd = (int)ndays, ny = cal.nyears, nm = ny * 12;
    const float *x = prcp + o;
    uint8_t *f = flag + o;
    // ---- check 4: duplicate years ----------------------------------------------------------------------------------
    for (int i = tid; i < ny; i += 256) { cnt_y[i] = 0; dup_y[i] = 0; }
    __syncthreads();
    for (int d = tid; d < nd; d += 256)
        if (f[d] == PQ_OK && pq_wet(x[d])) atomicAdd(&cnt_y[cal.yidx[d]], 1);            // (an integer count)
    __syncthreads();
    for (int p = tid; p < ny * ny; p += 256) {
        const int a = p / ny, b = p % ny;
        if (b <= a || cnt_y[a] < PQ_MIN_DUP_VALUES || cnt_y[b] < PQ_MIN_DUP_VALUES) continue;
        if (qa_same(x, f, cal.ystart[a], cal.ylen[a], cal.ystart[b], cal.ylen[b])) { dup_y[a] = 1; dup_y[b] = 1; }
    }
    __syncthreads();
    for (int d = tid; d < nd; d += 256)
        if (dup_y[cal.yidx[d]] && f[d] == PQ_OK) f[d] = PQ_DUP_YEAR;
    // ---- check 6: duplicate months within a year, then check 5: the same calendar month of two years ---------------
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        for (int i = tid; i < nm; i += 256) { cnt_m[i] = 0; dup_m[i] = 0; }
        __syncthreads();
        // a month has at most 31 days: the count fits a byte; one thread per (year, month) counts in day order
        for (int i = tid; i < nm; i += 256) {
            int c = 0;
            const int s0 = cal.mstart[i], len = cal.mlen[i];
            for (int j = 0; j < len; ++j) c += (f[s0 + j] == PQ_OK && pq_wet(x[s0 + j])) ? 1 : 0;
            cnt_m[i] = (uint8_t)c;
        }
        __syncthreads();
        if (pass == 0) {
            for (int p = tid; p < ny * 144; p += 256) {
                const int k = p / 144, m1 = (p % 144) / 12, m2 = p % 12;
                const int a = k * 12 + m1, b = k * 12 + m2;
                if (m2 <= m1 || m1 + 1 == cal.skip_month || cnt_m[a] < PQ_MIN_DUP_VALUES || cnt_m[b] < PQ_MIN_DUP_VALUES) continue;
                if (qa_same(x, f, cal.mstart[a], cal.mlen[a], cal.mstart[b], cal.mlen[b])) { dup_m[a] = 1; dup_m[b] = 1; }
            }
        } else {
            for (int p = tid; p < ny * ny * 12; p += 256) {
                const int m = p % 12, q = p / 12;
                const int ka = q / ny, kb = q % ny;
                const int a = ka * 12 + m, b = kb * 12 + m;
                if (kb <= ka || cnt_m[a] < PQ_MIN_DUP_VALUES || cnt_m[b] < PQ_MIN_DUP_VALUES) continue;
                if (qa_same(x, f, cal.mstart[a], cal.mlen[a], cal.mstart[b], cal.mlen[b])) { dup_m[a] = 1; dup_m[b] = 1; }
            }
        }
        __syncthreads();
        const uint8_t num = pass == 0 ? PQ_DUP_YEAR_MONTH : PQ_DUP_MONTH;
        for (int d = tid; d < nd; d += 256)
            if (dup_m[(int)cal.yidx[d] * 12 + cal.month[d] - 1] && f[d] == PQ_OK) f[d] = num;
    }
    __syncthreads();
    // ---- check 8: impossible values (float32 against float32(182.88), as numpy compares a float32 series) -----------
    for (int d = tid; d < nd; d += 256) {
        if (f[d] != PQ_OK) continue;
        const float v = x[d];
        if (v < 0.0f || v > PQ_MAX_VALUE) f[d] = PQ_IMPOSS_VALUE;
    }
}

__global__ __launch_bounds__(64) void k_pq_streak(int64_t ndays, const float *__restrict__ prcp, uint8_t *flag)
{
    const size_t o = (size_t)blockIdx.x * (size_t)ndays;
    // zeros and NaN are skipped and break no run (:392)
    qa_streak_walk<PQ_OK, PQ_STREAK, PQ_STREAK_LEN>(ndays, prcp + o, flag + o, [](float v) { return pq_wet(v); });
}

// the day indices of the live values > 0 of a station, in day order: cidx [nstn][ndays], ccnt [nstn]
__global__ __launch_bounds__(256) void k_pq_compact(int64_t ndays, const float *__restrict__ prcp,
                                                    const uint8_t *__restrict__ flag, int32_t *__restrict__ cidx,
                                                    int32_t *__restrict__ ccnt)
{
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t o = (size_t)blockIdx.x * (size_t)ndays;
    int base = 0;
    for (int64_t b0 = 0; b0 < ndays; b0 += 256) {                        // uniform
        const int64_t d = b0 + tid;
        const bool live = d < ndays && flag[o + d] == PQ_OK && pq_wet(prcp[o + d]);
        const uint64_t lm = __ballot(live);
        if (lane == 0) wsum[w] = __popcll(lm);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < 4; ++k) { const int c = wsum[k]; if (k < w) before += c; all += c; }
        if (live) cidx[o + (size_t)(base + before + __popcll(lm & (((uint64_t)1 << lane) - 1)))] = (int32_t)d;
        base += all;
        __syncthreads();
    }
    if (tid == 0) ccnt[blockIdx.x] = base;
}

__global__ __launch_bounds__(256) void k_pq_frequent(int64_t ndays, int64_t nstn, const int32_t *__restrict__ rowtab,
                                                     const float *__restrict__ prcp, const int32_t *__restrict__ cidx,
                                                     const int32_t *__restrict__ ccnt, const double *__restrict__ pct,
                                                     uint8_t *mark)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nstn * ndays) return;
    const int64_t s = i / ndays;
    const int xs = (int)(i % ndays), n = ccnt[s];
    if (xs >= n) return;
    const size_t o = (size_t)s * (size_t)ndays;
    const double *tab = pct + (size_t)s * PQ_ROWS * PQ_COLS;
    const int nwin = n - xs < PQ_FREQ_WINDOW ? n - xs : PQ_FREQ_WINDOW;  // shorter at the end of the sequence (:427)
    float w[PQ_FREQ_WINDOW];
    int dd[PQ_FREQ_WINDOW];
#pragma unroll
    for (int j = 0; j < PQ_FREQ_WINDOW; ++j) {
        dd[j] = j < nwin ? cidx[o + (size_t)(xs + j)] : -1;
        w[j] = j < nwin ? prcp[o + (size_t)dd[j]] : 0.0f;               // (0 equals no value of the sequence)
    }
#pragma unroll
    for (int a = 0; a < PQ_FREQ_WINDOW; ++a) {
        if (a >= nwin) continue;
        const float val = w[a];
        const double dv = (double)val;
        int cnt = 0;
        bool ok0 = true, ok1 = true, ok2 = true, ok3 = true;             // every percentile finite and val >= it
#pragma unroll
        for (int j = 0; j < PQ_FREQ_WINDOW; ++j) {
            if (j >= nwin || !(w[j] == val)) continue;
            ++cnt;
            const double *p = tab + (size_t)rowtab[dd[j]] * PQ_COLS;
            ok0 = ok0 && dv >= p[0];                                     // (a NaN percentile compares false)
            ok1 = ok1 && dv >= p[1];
            ok2 = ok2 && dv >= p[2];
            ok3 = ok3 && dv >= p[3];
        }
        // the elif chain of :436-443: a tier that fails in any clause falls through to the next
        if (!((cnt >= 9 && ok0) || (cnt >= 8 && ok1) || (cnt >= 7 && ok2) || (cnt >= 5 && ok3))) continue;
#pragma unroll
        for (int j = 0; j < PQ_FREQ_WINDOW; ++j)
            if (j < nwin && w[j] == val) mark[o + (size_t)dd[j]] = 1;    // (every writer stores 1)
    }
}

__global__ __launch_bounds__(256) void k_pq_apply(int64_t total, const uint8_t *__restrict__ mark, uint8_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (mark[i] && flag[i] == PQ_OK) flag[i] = PQ_FREQUENT;
}

__global__ __launch_bounds__(256) void k_pq_gap(int64_t ndays, QaCal cal, const float *__restrict__ prcp, uint8_t *flag)
{
    __shared__ float xs[TWXQA_MAX_GAP_VALUES];
    __shared__ int cnt, itop;
    const int tid = threadIdx.x;
    const int m = (int)(blockIdx.x % 12);
    const size_t o = (size_t)(blockIdx.x / 12) * (size_t)ndays;
    const float *x = prcp + o;
    uint8_t *f = flag + o;
    const int nslots = cal.nyears * 31;                                  // <= TWXQA_MAX_GAP_VALUES (host check)
    int np2 = 1;
    while (np2 < nslots) np2 <<= 1;
    if (tid == 0) { cnt = 0; itop = np2; }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < np2; i += 256) {
        float val = __builtin_inff();                                    // (no live value is infinite after check 8)
        if (i < nslots) {
            const int k = i / 31, j = i % 31, seg = k * 12 + m;
            if (j < cal.mlen[seg]) {
                const int d = cal.mstart[seg] + j;
                if (f[d] == PQ_OK && pq_wet(x[d])) { val = x[d]; ++mine; }
            }
        }
        xs[i] = val;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    const int n = cnt;
    if (n < 2) return;                                                   // uniform
    qa_lds_sort(xs, np2, tid);
    for (int i = 1 + tid; i < n; i += 256)
        if (xs[i] - xs[i - 1] >= PQ_GAP_THRES) atomicMin(&itop, i);      // the first step (:467-470); float32 difference
    __syncthreads();
    if (itop >= np2) return;
    const float bound = xs[itop];
    for (int i = tid; i < nslots; i += 256) {
        const int k = i / 31, j = i % 31, seg = k * 12 + m;
        if (j >= cal.mlen[seg]) continue;
        const int d = cal.mstart[seg] + j;
        if (f[d] != PQ_OK) continue;
        const float v = x[d];
        if (pq_wet(v) && v >= bound) f[d] = PQ_GAP;
    }
}

__global__ __launch_bounds__(256) void k_pq_pctiles(int64_t ndays, int nyears, const int2 *__restrict__ yr,
                                                    const float *__restrict__ prcp, const uint8_t *__restrict__ flag,
                                                    double *__restrict__ out)
{
    __shared__ float xs[TWXPQ_MAX_WINDOW_VALUES];
    __shared__ int cnt;
    const int tid = threadIdx.x;
    const int row = (int)(blockIdx.x % PQ_ROWS);                         // the date of 2004 with yday - 1 == row
    const size_t s = blockIdx.x / PQ_ROWS;
    const size_t so = s * (size_t)ndays;
    if (tid == 0) cnt = 0;
    __syncthreads();
    // ---- gather: thread = (year k, date j of the window); q is the date's index in a leap year's calendar.  The window
    // is row - 14 .. row + 14 of 2004's dates and wraps over the year end; Feb 29 (q == 59) is in it exactly for the rows
    // 45 .. 73, and a common year has no such day.  Every day of the axis has one (k, q): it is taken at most once.
    for (int i = tid; i < nyears * 32; i += 256) {
        const int k = i >> 5, j = i & 31;
        if (j >= 29) continue;
        int q = row - 14 + j;
        q = q < 0 ? q + PQ_ROWS : (q >= PQ_ROWS ? q - PQ_ROWS : q);
        const int64_t d = qa_date_day(q, yr[k], ndays);
        if (d < 0) continue;
        if (flag[so + d] != PQ_OK) continue;
        const float v = prcp[so + d];
        if (!pq_wet(v)) continue;
        xs[atomicAdd(&cnt, 1)] = v;                                      // <= 29 * nyears <= TWXPQ_MAX_WINDOW_VALUES (host check)
    }
    __syncthreads();
    const int n = cnt;
    double *o = out + (s * PQ_ROWS + (size_t)row) * PQ_COLS;
    if (n < TWXPQ_MIN_PERCENTILE_VALUES) {                               // uniform
        if (tid < PQ_COLS) o[tid] = __builtin_nan("");
        return;
    }
    int np2 = 32;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += 256) xs[i] = __builtin_inff();
    __syncthreads();
    qa_lds_sort(xs, np2, tid);
    if (tid < PQ_COLS) {
        // numpy's 'linear': virtual index (n - 1) q, gamma its fraction, a + (b - a) gamma below 0.5, b - (b - a)(1 - gamma)
        // from 0.5 on; q = 30 / 100 ... as np.true_divide forms them
        const double qs = tid == 0 ? 30.0 / 100.0 : tid == 1 ? 50.0 / 100.0 : tid == 2 ? 70.0 / 100.0
                        : tid == 3 ? 90.0 / 100.0 : 95.0 / 100.0;
        const double vi = (double)(n - 1) * qs;
        const int lo = (int)floor(vi);
        const int hi = lo + 1 < n ? lo + 1 : n - 1;
        const double g = vi - (double)lo;
        const double a = (double)xs[lo], b = (double)xs[hi], diff = b - a;
        o[tid] = g >= 0.5 ? b - diff * (1.0 - g) : a + diff * g;
    }
}

__global__ __launch_bounds__(256) void k_pq_clim(int64_t ndays, int64_t nstn, const int32_t *__restrict__ rowtab,
                                                 const float *__restrict__ prcp, const float *__restrict__ tavg,
                                                 const double *__restrict__ pct, uint8_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nstn * ndays) return;
    if (flag[i] != PQ_OK) return;
    const float v = prcp[i];
    if (!pq_wet(v)) return;
    const int64_t s = i / ndays, d = i % ndays;
    const double p95 = pct[((size_t)s * PQ_ROWS + (size_t)rowtab[d]) * PQ_COLS + 4];
    const float t = tavg[i];
    const double m = t < 0.0f ? 5.0 : 9.0;                               // (a NaN Tavg compares false: 9, :605-608)
    if ((double)v >= m * p95) flag[i] = PQ_CLIM_OUTLIER;                 // (a NaN row compares false)
}

// ---------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------
namespace {

// The calendar of a day axis, the years capped for the percentile table and, with gap_cap, for the chain's gap check.
int pq_cal(const char *who, int64_t ndays, const int32_t *ymd, bool gap_cap, QaCalendar &c, char *errbuf, int errlen)
{
    if (qa_cal_years(who, ndays, ymd, c, errbuf, errlen) != 0 ||
        qa_year_cap(who, c, 29, TWXPQ_MAX_WINDOW_VALUES, "a row of the percentile table holds at most TWXPQ_MAX_WINDOW_VALUES", "",
                    errbuf, errlen) != 0 ||
        (gap_cap && qa_year_cap(who, c, 31, TWXQA_MAX_GAP_VALUES, "the gap check sorts at most TWXQA_MAX_GAP_VALUES",
                                " of a calendar month", errbuf, errlen) != 0))
        return -1;
    return qa_cal_walk(who, ndays, ymd, c, errbuf, errlen);
}

bool pq_sizes_ok(int64_t nstn, int64_t ndays)
{
    return nstn >= 1 && ndays >= 1 && ndays <= INT32_MAX - 256 && nstn <= INT32_MAX / PQ_ROWS &&
           (nstn * ndays + 255) / 256 <= INT32_MAX;
}

}  // namespace

extern "C" int twxpq_non_spatial(int device, int64_t nstn, int64_t ndays, const float *prcp, const float *tavg,
                                 const int32_t *ymd, int32_t streak, int32_t frequent, uint8_t *flag, double *pctiles,
                                 float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (!pq_sizes_ok(nstn, ndays))
        return qa_fail(errbuf, errlen, "twxpq_non_spatial: need nstn >= 1, ndays >= 1 and fewer than 2^31 work items in one call");
    if (!prcp || !tavg || !ymd || !flag) return qa_fail(errbuf, errlen, "twxpq_non_spatial: null buffer");
    QaCalendar cal;
    if (pq_cal("twxpq_non_spatial", ndays, ymd, true, cal, errbuf, errlen) != 0) return -1;
    const size_t ns = (size_t)nstn, nd = (size_t)ndays;
    QACHK(hipSetDevice(device));
    QaBuf b_obs, b_flag, b_cal, b_pct, b_idx, b_cnt, b_mark;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_obs.p, 2 * ns * nd * 4));                  // prcp, then tavg: [2][nstn][ndays]
    float *d_prcp = static_cast<float *>(b_obs.p), *d_tavg = d_prcp + ns * nd;
    QACHK(hipMemcpy(d_prcp, prcp, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_tavg, tavg, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_flag.p, ns * nd));
    uint8_t *d_f = static_cast<uint8_t *>(b_flag.p);
    QaCal k;
    if (qa_upload_calendar(cal, cal.row, b_cal, k, errbuf, errlen) != 0) return -1;
    const size_t pct_bytes = ns * PQ_ROWS * PQ_COLS * 8;
    QACHK(hipMalloc(&b_pct.p, pct_bytes));                        // [nstn][366][5]
    double *d_pct = static_cast<double *>(b_pct.p);

    float ms[TWXPQ_NKERNELS];
    for (int i = 0; i < TWXPQ_NKERNELS; ++i) ms[i] = 0.0f;
    const unsigned g_day = (unsigned)((ns * nd + 255) / 256);
    // ---- missing (2) ---------------------------------------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pq_init, dim3(g_day), dim3(256), 0, nullptr, (int64_t)(ns * nd), (const float *)d_prcp, d_f);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[0]));
    // ---- the duplicates (4, 6, 5), impossible values (8) -----------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pq_dups, dim3((unsigned)ns), dim3(256), 0, nullptr, ndays, k, (const float *)d_prcp, d_f);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[1]));
    // ---- optional: streaks (9) ---------------------------------------------------------------------------------------------
    if (streak) {
        QACHK(tm.start());
        hipLaunchKernelGGL(k_pq_streak, dim3((unsigned)ns), dim3(64), 0, nullptr, ndays, (const float *)d_prcp, d_f);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[2]));
    }
    // ---- optional: frequent values (19), against the table of the series as it stands here ---------------------------------
    if (frequent) {
        QACHK(hipMalloc(&b_idx.p, ns * nd * 4));
        QACHK(hipMalloc(&b_cnt.p, ns * 4));
        QACHK(hipMalloc(&b_mark.p, ns * nd));
        QACHK(hipMemset(b_mark.p, 0, ns * nd));
        QACHK(tm.start());
        hipLaunchKernelGGL(k_pq_pctiles, dim3((unsigned)(ns * PQ_ROWS)), dim3(256), 0, nullptr, ndays, cal.nyears, k.yr,
                           (const float *)d_prcp, (const uint8_t *)d_f, d_pct);
        QACHK(hipGetLastError());
        hipLaunchKernelGGL(k_pq_compact, dim3((unsigned)ns), dim3(256), 0, nullptr, ndays, (const float *)d_prcp,
                           (const uint8_t *)d_f, static_cast<int32_t *>(b_idx.p), static_cast<int32_t *>(b_cnt.p));
        QACHK(hipGetLastError());
        hipLaunchKernelGGL(k_pq_frequent, dim3(g_day), dim3(256), 0, nullptr, ndays, nstn, k.row, (const float *)d_prcp,
                           (const int32_t *)b_idx.p, (const int32_t *)b_cnt.p, (const double *)d_pct,
                           static_cast<uint8_t *>(b_mark.p));
        QACHK(hipGetLastError());
        hipLaunchKernelGGL(k_pq_apply, dim3(g_day), dim3(256), 0, nullptr, (int64_t)(ns * nd),
                           (const uint8_t *)b_mark.p, d_f);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms[3]));
    }
    // ---- gaps (10) ---------------------------------------------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pq_gap, dim3((unsigned)(ns * 12)), dim3(256), 0, nullptr, ndays, k, (const float *)d_prcp, d_f);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[4]));
    // ---- the percentile table of what is left, then the outliers (15) ----------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pq_pctiles, dim3((unsigned)(ns * PQ_ROWS)), dim3(256), 0, nullptr, ndays, cal.nyears, k.yr,
                       (const float *)d_prcp, (const uint8_t *)d_f, d_pct);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[5]));
    if (pctiles) QACHK(hipMemcpy(pctiles, d_pct, pct_bytes, hipMemcpyDeviceToHost));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pq_clim, dim3(g_day), dim3(256), 0, nullptr, ndays, nstn, k.row, (const float *)d_prcp,
                       (const float *)d_tavg, (const double *)d_pct, d_f);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[6]));
    QACHK(hipMemcpy(flag, d_f, ns * nd, hipMemcpyDeviceToHost));
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxpq_percentiles(int device, int64_t nstn, int64_t ndays, const float *vals, const int32_t *ymd,
                                 double *pctiles, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (!pq_sizes_ok(nstn, ndays))
        return qa_fail(errbuf, errlen, "twxpq_percentiles: need nstn >= 1, ndays >= 1 and fewer than 2^31 work items in one call");
    if (!vals || !ymd || !pctiles) return qa_fail(errbuf, errlen, "twxpq_percentiles: null buffer");
    QaCalendar cal;
    if (pq_cal("twxpq_percentiles", ndays, ymd, false, cal, errbuf, errlen) != 0) return -1;
    const size_t ns = (size_t)nstn, nd = (size_t)ndays;
    QACHK(hipSetDevice(device));
    QaBuf b_obs, b_flag, b_cal, b_pct;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_obs.p, ns * nd * 4));
    QACHK(hipMemcpy(b_obs.p, vals, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_flag.p, ns * nd));
    QaCal k;
    if (qa_upload_calendar(cal, cal.row, b_cal, k, errbuf, errlen) != 0) return -1;
    const size_t pct_bytes = ns * PQ_ROWS * PQ_COLS * 8;
    QACHK(hipMalloc(&b_pct.p, pct_bytes));
    float ms = 0.0f;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pq_init, dim3((unsigned)((ns * nd + 255) / 256)), dim3(256), 0, nullptr, (int64_t)(ns * nd),
                       (const float *)b_obs.p, static_cast<uint8_t *>(b_flag.p));
    QACHK(hipGetLastError());
    hipLaunchKernelGGL(k_pq_pctiles, dim3((unsigned)(ns * PQ_ROWS)), dim3(256), 0, nullptr, ndays, cal.nyears, k.yr,
                       (const float *)b_obs.p, (const uint8_t *)b_flag.p, static_cast<double *>(b_pct.p));
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms));
    QACHK(hipMemcpy(pctiles, b_pct.p, pct_bytes, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}
