// twx_nonspatial.hip -- libtwxqa.so: step08's first run, run_qa_non_spatial (twx/qa/qa_temp.py:172-216), for many
// stations in one call.  The fourth translation unit of the library (include/twx_qa.h, twxqa_non_spatial).
//
// State.  The device holds the two input series and one flag byte per observation.  An observation is still in the
// series ("live") exactly while its flag is 1: every removal of the reference (_update_obs_flags, :1230-1237) sets a
// value to NaN and writes the check's number where the flag was 1, and a value whose flag is not 1 is NaN already.  So
// the flag array IS the working copy, a check reads "flag == 1 ? value : NaN", and a removal is one byte store.  Within a
// check every decision is taken on one snapshot: a kernel either owns what it reads (one workgroup or wavefront per
// series, barriers between deciding and removing) or reads neighbours through a liveness test that counts its own
// number as live (the two stencil checks: no earlier check can have written that number).
//
// k_ns_init      thread = (station, day): missing (2), naught (3).
// k_ns_dups      one 256-thread workgroup per station: duplicate years (4), duplicate months within a year (6),
//                duplicate calendar months across years (5) per variable, then duplicates within a month (7) and the
//                impossible values (8).  The pairs of a check are spread over the threads, each compares by position
//                with early exit (almost all pairs end at their first day); the per-year / per-month "has a value" and
//                "is a duplicate" bytes and the Tmin == Tmax counters are in LDS: 74 bytes per year, 9.6 KiB at the cap.
// k_ns_streak    one wavefront per (station, variable) walks the series in blocks of 64 days; runs of equal live values
//                come from ballots, a run's length from the ranks of its start and of the next start, carried across
//                blocks; a run of >= 20 is flagged when a different value ends it (9).
// k_ns_gap       one 256-thread workgroup per (station, variable, calendar month): the live values of the month over all
//                years (31 slots per year, +inf where there is none) are sorted in LDS (bitonic, float32), the median
//                and the steps are float32 as numpy's, the first step >= 10 on either side of the median gives the bounds
//                (10).  LDS: 4 bytes per slot: TWXQA_MAX_GAP_VALUES = 4096 costs 16 KiB per workgroup, and the 8
//                workgroups that fill a compute unit's 32 wave slots take 128 KiB of its 160 KiB.
// k_ns_norms     k_doy_norms of twx_corrob.hip (same gather, same 380 jobs, same exact medians) reading live values, with
//                the biweight standard deviation next to the mean (_biweight_mean_std, :1187-1212).  LDS 10 KiB.
// k_ns_clim      thread = (station, day): |z| >= 6 against the row of the day's own year (15), then Tmin > Tmax (11).
// k_ns_spike     thread = (station, day): spike / dip (13).
// k_ns_lagrange  thread = (station, day), a gather: the conditions of days x - 1, x, x + 1 from the values of
//                x - 2 .. x + 2 (12).
// k_ns_mega      one workgroup per station: k_mega_final's month extremes over the live values (18).
// Every reduction runs in a fixed order; integer atomics only count.  fp64 on float32 values widened exactly for the
// day-of-year rows, the z-score and the lagged range; float32 where the reference's result is one float32 operation.
// The library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_series.h"

#define NS_NJOBS 380                         // 365 rows + the 15 leap rows whose window holds Feb 29
#define NS_LEAP_FIRST 52                     // Feb 22 of the 366-row table
#define NS_MAX_YEARS (TWXQA_MAX_GAP_VALUES / 31)
#define NS_OK 1                              // qa_temp.py:41-59
#define NS_MISSING 2
#define NS_NAUGHT 3
#define NS_DUP_YEAR 4
#define NS_DUP_MONTH 5
#define NS_DUP_YEAR_MONTH 6
#define NS_DUP_WITHIN_MONTH 7
#define NS_IMPOSS_VALUE 8
#define NS_STREAK 9
#define NS_GAP 10
#define NS_INTERNAL_INCONSIST 11
#define NS_LAGRANGE_INCONSIST 12
#define NS_SPIKE_DIP 13
#define NS_CLIM_OUTLIER 15
#define NS_MEGA_INCONSIST 18
#define NS_TMAX_RECORD 57.7f                 // qa_temp.py:62-63, rounded to float32 as the comparison does
#define NS_TMIN_RECORD -89.4f
#define NS_STREAK_LEN 20                     // qa_temp.py:1241
#define NS_GAP_THRES 10.0f                   // qa_temp.py:1269
#define NS_SPIKE_THRES 25.0f                 // qa_temp.py:1298
#define NS_LAG_THRES 40.0                    // qa_temp.py:600
#define NS_CLIM_Z 6.0                        // qa_temp.py:1160
#define NS_DUP_DAYS 10                       // qa_temp.py:323

__global__ __launch_bounds__(256) void k_ns_init(int64_t total, const float *__restrict__ tmin,
                                                 const float *__restrict__ tmax, uint8_t *__restrict__ f_tmin,
                                                 uint8_t *__restrict__ f_tmax)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float a = tmin[i], b = tmax[i];
    uint8_t fa = a != a ? NS_MISSING : NS_OK, fb = b != b ? NS_MISSING : NS_OK;
    // np.round(v, 1) of a float32 is rint(v * 10) / 10 in float32 (:277); a NaN compares false
    const bool us = rintf(a * 10.0f) / 10.0f == -17.8f && rintf(b * 10.0f) / 10.0f == -17.8f;
    const bool nonus = a == 0.0f && b == 0.0f;
    if (us || nonus) { fa = NS_NAUGHT; fb = NS_NAUGHT; }
    f_tmin[i] = fa;
    f_tmax[i] = fb;
}

__global__ __launch_bounds__(256) void k_ns_dups(int64_t ndays, QaCal cal, const float *__restrict__ tmin,
                                                 const float *__restrict__ tmax, uint8_t *f_tmin, uint8_t *f_tmax)
{
    __shared__ uint8_t has_y[NS_MAX_YEARS], dup_y[NS_MAX_YEARS];
    __shared__ uint8_t has_m[NS_MAX_YEARS * 12], dup_m[NS_MAX_YEARS * 12];
    __shared__ int eq_m[NS_MAX_YEARS * 12];
    const int tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * (size_t)ndays;
    const int nd = (int)ndays, ny = cal.nyears, nm = ny * 12;
    for (int v = 0; v < 2; ++v) {
        const float *x = (v ? tmax : tmin) + o;
        uint8_t *f = (v ? f_tmax : f_tmin) + o;
        // ---- check 4: duplicate years ------------------------------------------------------------------------------
        for (int i = tid; i < ny; i += 256) { has_y[i] = 0; dup_y[i] = 0; }
        __syncthreads();
        for (int d = tid; d < nd; d += 256)
            if (f[d] == NS_OK) has_y[cal.yidx[d]] = 1;                   // (every writer stores 1)
        __syncthreads();
        for (int p = tid; p < ny * ny; p += 256) {
            const int a = p / ny, b = p % ny;
            if (b <= a || !has_y[a] || !has_y[b]) continue;
            if (qa_same(x, f, cal.ystart[a], cal.ylen[a], cal.ystart[b], cal.ylen[b])) { dup_y[a] = 1; dup_y[b] = 1; }
        }
        __syncthreads();
        for (int d = tid; d < nd; d += 256)
            if (dup_y[cal.yidx[d]] && f[d] == NS_OK) f[d] = NS_DUP_YEAR;
        // ---- check 6: duplicate months within a year, then check 5: the same calendar month of two years -----------
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();
            for (int i = tid; i < nm; i += 256) { has_m[i] = 0; dup_m[i] = 0; }
            __syncthreads();
            for (int d = tid; d < nd; d += 256)
                if (f[d] == NS_OK) has_m[(int)cal.yidx[d] * 12 + cal.month[d] - 1] = 1;
            __syncthreads();
            if (pass == 0) {
                for (int p = tid; p < ny * 144; p += 256) {
                    const int k = p / 144, m1 = (p % 144) / 12, m2 = p % 12;
                    const int a = k * 12 + m1, b = k * 12 + m2;
                    if (m2 <= m1 || m1 + 1 == cal.skip_month || !has_m[a] || !has_m[b]) continue;
                    if (qa_same(x, f, cal.mstart[a], cal.mlen[a], cal.mstart[b], cal.mlen[b])) { dup_m[a] = 1; dup_m[b] = 1; }
                }
            } else {
                for (int p = tid; p < ny * ny * 12; p += 256) {
                    const int m = p % 12, q = p / 12;
                    const int ka = q / ny, kb = q % ny;
                    const int a = ka * 12 + m, b = kb * 12 + m;
                    if (kb <= ka || !has_m[a] || !has_m[b]) continue;
                    if (qa_same(x, f, cal.mstart[a], cal.mlen[a], cal.mstart[b], cal.mlen[b])) { dup_m[a] = 1; dup_m[b] = 1; }
                }
            }
            __syncthreads();
            const uint8_t num = pass == 0 ? NS_DUP_YEAR_MONTH : NS_DUP_MONTH;
            for (int d = tid; d < nd; d += 256)
                if (dup_m[(int)cal.yidx[d] * 12 + cal.month[d] - 1] && f[d] == NS_OK) f[d] = num;
        }
        __syncthreads();
    }
    // ---- check 7: a (year, month) with >= 10 days of Tmin == Tmax, then check 8 on what is left ---------------------
    for (int i = tid; i < nm; i += 256) eq_m[i] = 0;
    __syncthreads();
    for (int d = tid; d < nd; d += 256)
        if (f_tmin[o + d] == NS_OK && f_tmax[o + d] == NS_OK && tmin[o + d] == tmax[o + d])
            atomicAdd(&eq_m[(int)cal.yidx[d] * 12 + cal.month[d] - 1], 1);
    __syncthreads();
    for (int d = tid; d < nd; d += 256) {
        const bool dup = eq_m[(int)cal.yidx[d] * 12 + cal.month[d] - 1] >= NS_DUP_DAYS;
        for (int v = 0; v < 2; ++v) {
            uint8_t *f = (v ? f_tmax : f_tmin) + o;
            if (f[d] != NS_OK) continue;
            const float val = (v ? tmax : tmin)[o + d];
            if (dup) f[d] = NS_DUP_WITHIN_MONTH;
            else if (val < NS_TMIN_RECORD || val > NS_TMAX_RECORD) f[d] = NS_IMPOSS_VALUE;
        }
    }
}

__global__ __launch_bounds__(64) void k_ns_streak(int64_t ndays, const float *__restrict__ obs, uint8_t *flag)
{
    const size_t o = (size_t)blockIdx.x * (size_t)ndays;                 // series (variable, station) of [2][nstn][ndays]
    qa_streak_walk<NS_OK, NS_STREAK, NS_STREAK_LEN>(ndays, obs + o, flag + o, [](float) { return true; });
}

__global__ __launch_bounds__(256) void k_ns_gap(int64_t ndays, QaCal cal, const float *__restrict__ obs, uint8_t *flag)
{
    __shared__ float xs[TWXQA_MAX_GAP_VALUES];
    __shared__ int cnt, itop, ibot;
    const int tid = threadIdx.x;
    const int m = (int)(blockIdx.x % 12);
    const size_t o = (size_t)(blockIdx.x / 12) * (size_t)ndays;          // series (variable, station)
    const float *x = obs + o;
    uint8_t *f = flag + o;
    const int nslots = cal.nyears * 31;                                  // <= TWXQA_MAX_GAP_VALUES (host check)
    int np2 = 1;
    while (np2 < nslots) np2 <<= 1;
    if (tid == 0) { cnt = 0; itop = np2; ibot = 0; }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < np2; i += 256) {
        float val = __builtin_inff();                                    // (no live value is infinite after check 8)
        if (i < nslots) {
            const int k = i / 31, j = i % 31, seg = k * 12 + m;
            if (j < cal.mlen[seg]) {
                const int d = cal.mstart[seg] + j;
                if (f[d] == NS_OK) { val = x[d]; ++mine; }
            }
        }
        xs[i] = val;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    const int n = cnt;
    if (n == 0) return;                                                  // uniform
    qa_lds_sort(xs, np2, tid);
    const int p = n >> 1;
    const float med = (n & 1) ? xs[p] : (xs[p - 1] + xs[p]) / 2.0f;      // numpy's float32 mean of the two
    for (int i = 1 + tid; i < n; i += 256) {
        const float lo = xs[i - 1], hi = xs[i];
        if (hi - lo >= NS_GAP_THRES) {
            if (lo >= med) atomicMin(&itop, i);                          // both values in the part >= median
            if (hi <= med) atomicMax(&ibot, i);                          // both values in the part <= median
        }
    }
    __syncthreads();
    const bool top = itop < np2, bot = ibot > 0;
    if (!top && !bot) return;
    const float btop = top ? xs[itop] : 0.0f, bbot = bot ? xs[ibot - 1] : 0.0f;
    for (int i = tid; i < nslots; i += 256) {
        const int k = i / 31, j = i % 31, seg = k * 12 + m;
        if (j >= cal.mlen[seg]) continue;
        const int d = cal.mstart[seg] + j;
        if (f[d] != NS_OK) continue;
        const float v = x[d];
        if ((top && v >= btop) || (bot && v <= bbot)) f[d] = NS_GAP;
    }
}

__global__ __launch_bounds__(256) void k_ns_norms(int64_t ndays, int64_t nstn, int nyears, const int2 *__restrict__ yr,
                                                  const float *__restrict__ obs, const uint8_t *__restrict__ flag,
                                                  double *__restrict__ out)
{
    __shared__ float xs[TWXQA_MAX_NORM_VALUES];
    __shared__ double red[256];
    __shared__ double mad_k[2];
    __shared__ int cnt;
    const int tid = threadIdx.x;
    const int job = (int)(blockIdx.x % NS_NJOBS);
    const int64_t s = blockIdx.x / NS_NJOBS;                             // series of [2][nstn][ndays]
    const bool leap_job = job >= 365;
    const int centre = leap_job ? NS_LEAP_FIRST + (job - 365) : job;     // row of the job's own table
    const int period = leap_job ? 366 : 365;
    if (tid == 0) cnt = 0;
    __syncthreads();
    // ---- gather: thread = (year k, date j of the window); q is the date's index in a leap year's calendar ----------
    const size_t so = (size_t)s * (size_t)ndays;
    for (int i = tid; i < nyears * 16; i += 256) {
        const int k = i >> 4, j = i & 15;
        if (j == 15) continue;
        int t = centre - 7 + j;
        t = t < 0 ? t + period : (t >= period ? t - period : t);
        const int q = (leap_job || t < 59) ? t : t + 1;
        const int64_t d = qa_date_day(q, yr[k], ndays);          // (a 365-row window never holds Feb 29: q != 59 there)
        if (d < 0) continue;
        if (flag[so + d] != NS_OK) continue;
        const float v = obs[so + d];
        if (!qa_finitef(v)) continue;
        xs[atomicAdd(&cnt, 1)] = v;                              // <= 15 * nyears <= TWXQA_MAX_NORM_VALUES (host check)
    }
    __syncthreads();
    const int n = cnt;
    double mean = __builtin_nan(""), sd = __builtin_nan("");
    if (n >= TWXQA_MIN_NORM_VALUES) {                            // uniform
        int np2 = 1;
        while (np2 < n) np2 <<= 1;
        for (int i = n + tid; i < np2; i += 256) xs[i] = __builtin_inff();
        __syncthreads();
        qa_lds_sort(xs, np2, tid);
        mean = qa_biweight<true>(xs, n, red, mad_k, tid, &sd);
    }
    if (tid == 0) {
        double *o = out + (size_t)((s % nstn) * 2 + s / nstn) * TWXQA_NORM_ROWS * 2;   // [nstn][2][731][mean, std]
        int r0, r1 = -1;
        if (leap_job) {
            r0 = 365 + centre;
        } else {
            r0 = job;
            if (job < NS_LEAP_FIRST) r1 = 365 + job;                       // Jan 1 .. Feb 21
            else if (job >= NS_LEAP_FIRST + 14) r1 = 365 + job + 1;        // Mar 8 .. Dec 31
        }
        o[2 * r0] = mean;
        o[2 * r0 + 1] = sd;
        if (r1 >= 0) { o[2 * r1] = mean; o[2 * r1 + 1] = sd; }
    }
}

__global__ __launch_bounds__(256) void k_ns_clim(int64_t ndays, int64_t nstn, const int32_t *__restrict__ normrow,
                                                 const float *__restrict__ tmin, const float *__restrict__ tmax,
                                                 const double *__restrict__ norms, uint8_t *__restrict__ f_tmin,
                                                 uint8_t *__restrict__ f_tmax)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nstn * ndays) return;
    const int64_t s = i / ndays, d = i % ndays;
    const int row = normrow[d];
    const float a = tmin[i], b = tmax[i];
    uint8_t fa = f_tmin[i], fb = f_tmax[i];
    const double *na = norms + ((size_t)(s * 2) * TWXQA_NORM_ROWS + row) * 2, *nb = na + TWXQA_NORM_ROWS * 2;
    // a row without a normal is NaN, and so is 0 / 0 of a row whose values are all the same: neither flags
    if (fa == NS_OK && fabs(((double)a - na[0]) / na[1]) >= NS_CLIM_Z) fa = NS_CLIM_OUTLIER;
    if (fb == NS_OK && fabs(((double)b - nb[0]) / nb[1]) >= NS_CLIM_Z) fb = NS_CLIM_OUTLIER;
    if (fa == NS_OK && fb == NS_OK && a > b) { fa = NS_INTERNAL_INCONSIST; fb = NS_INTERNAL_INCONSIST; }
    f_tmin[i] = fa;
    f_tmax[i] = fb;
}

// thread = (series, day) over both variables at once: [2][nstn][ndays] is one array of 2 * nstn series
__global__ __launch_bounds__(256) void k_ns_spike(int64_t ndays, int64_t nseries, const float *__restrict__ obs,
                                                  uint8_t *flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nseries * ndays) return;
    const int64_t d = i % ndays;
    if (d == 0 || d == ndays - 1 || flag[i] != NS_OK) return;            // the ends of the series have a NaN neighbour
    const uint8_t fp = flag[i - 1], fn = flag[i + 1];                    // a neighbour this check has just flagged was live
    if ((fp != NS_OK && fp != NS_SPIKE_DIP) || (fn != NS_OK && fn != NS_SPIKE_DIP)) return;
    const float cur = obs[i];
    if (fabsf(cur - obs[i - 1]) >= NS_SPIKE_THRES && fabsf(cur - obs[i + 1]) >= NS_SPIKE_THRES) flag[i] = NS_SPIKE_DIP;
}

__global__ __launch_bounds__(256) void k_ns_lagrange(int64_t ndays, int64_t nstn, const float *__restrict__ tmin,
                                                     const float *__restrict__ tmax, uint8_t *f_tmin, uint8_t *f_tmax)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nstn * ndays) return;
    const int64_t d = i % ndays;
    const double nan = __builtin_nan("");
    double lo[5], hi[5];                                                 // days d - 2 .. d + 2, NaN: not live / off the axis
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const int64_t e = d + c - 2;
        lo[c] = nan;
        hi[c] = nan;
        if (e >= 0 && e < ndays) {
            const uint8_t fa = f_tmin[i + c - 2], fb = f_tmax[i + c - 2];
            if (fa == NS_OK || fa == NS_LAGRANGE_INCONSIST) lo[c] = (double)tmin[i + c - 2];
            if (fb == NS_OK || fb == NS_LAGRANGE_INCONSIST) hi[c] = (double)tmax[i + c - 2];
        }
    }
    bool flag_lo = false, flag_hi = false;
#pragma unroll
    for (int c = 1; c <= 3; ++c) {                                       // the day x = d + c - 2 and its window
        double mx = nan, mn = nan;                                       // warmest Tmin, coldest Tmax of the window
#pragma unroll
        for (int w = c - 1; w <= c + 1; ++w) {
            if (lo[w] == lo[w] && !(mx >= lo[w])) mx = lo[w];
            if (hi[w] == hi[w] && !(mn <= hi[w])) mn = hi[w];
        }
        if (!(mx == mx) || !(mn == mn)) continue;                        // either variable has no value in the window
        const bool c_hi = hi[c] >= mx + NS_LAG_THRES;                    // Tmax[x] flags itself and the window of Tmin
        const bool c_lo = lo[c] <= mn - NS_LAG_THRES;                    // Tmin[x] flags itself and the window of Tmax
        if (c_hi) { flag_lo = true; if (c == 2) flag_hi = true; }
        if (c_lo) { flag_hi = true; if (c == 2) flag_lo = true; }
    }
    if (flag_lo && f_tmin[i] == NS_OK) f_tmin[i] = NS_LAGRANGE_INCONSIST;
    if (flag_hi && f_tmax[i] == NS_OK) f_tmax[i] = NS_LAGRANGE_INCONSIST;
}

__global__ __launch_bounds__(256) void k_ns_mega(int64_t ndays, const uint8_t *__restrict__ month,
                                                 const float *__restrict__ tmin, const float *__restrict__ tmax,
                                                 uint8_t *f_tmin, uint8_t *f_tmax)
{
    __shared__ float red[2][12][256];                            // 0: lowest Tmin, 1: highest Tmax of a calendar month
    const int tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * (size_t)ndays;
    const float inf = __builtin_inff();
    for (int m = 0; m < 12; ++m) { red[0][m][tid] = inf; red[1][m][tid] = -inf; }
    for (int64_t d = tid; d < ndays; d += 256) {                 // (a thread touches its own column of red only)
        const int m = month[d] - 1;
        const float a = tmin[o + d], b = tmax[o + d];
        if (f_tmin[o + d] == NS_OK && qa_finitef(a)) red[0][m][tid] = fminf(red[0][m][tid], a);
        if (f_tmax[o + d] == NS_OK && qa_finitef(b)) red[1][m][tid] = fmaxf(red[1][m][tid], b);
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            for (int m = 0; m < 12; ++m) {
                red[0][m][tid] = fminf(red[0][m][tid], red[0][m][tid + s]);
                red[1][m][tid] = fmaxf(red[1][m][tid], red[1][m][tid + s]);
            }
        }
        __syncthreads();
    }
    for (int64_t d = tid; d < ndays; d += 256) {
        const int m = month[d] - 1;
        const float lo = red[0][m][0], hi = red[1][m][0];
        if (lo == inf || hi == -inf) continue;                   // a month with no finite value on either side is skipped
        const float a = tmin[o + d], b = tmax[o + d];
        if (f_tmin[o + d] == NS_OK && qa_finitef(a) && a > hi) f_tmin[o + d] = NS_MEGA_INCONSIST;
        if (f_tmax[o + d] == NS_OK && qa_finitef(b) && b < lo) f_tmax[o + d] = NS_MEGA_INCONSIST;
    }
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
extern "C" int twxqa_non_spatial(int device, int64_t nstn, int64_t ndays, const float *tmin, const float *tmax,
                                 const int32_t *ymd, uint8_t *flag_tmin, uint8_t *flag_tmax, double *norms,
                                 float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || ndays > INT32_MAX - 64 || nstn > INT32_MAX / (2 * NS_NJOBS) ||
        (nstn * ndays + 255) / 256 * 2 > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxqa_non_spatial: need nstn >= 1, ndays >= 1 and fewer than 2^31 work items in one call");
    if (!tmin || !tmax || !ymd || !flag_tmin || !flag_tmax) return qa_fail(errbuf, errlen, "twxqa_non_spatial: null buffer");
    const char *who = "twxqa_non_spatial";
    QaCalendar cal;
    if (qa_cal_years(who, ndays, ymd, cal, errbuf, errlen) != 0 ||
        qa_year_cap(who, cal, 31, TWXQA_MAX_GAP_VALUES, "the gap check sorts at most TWXQA_MAX_GAP_VALUES", " of a calendar month",
                    errbuf, errlen) != 0 ||
        qa_year_cap(who, cal, 15, TWXQA_MAX_NORM_VALUES, "a row of the day-of-year normals holds at most TWXQA_MAX_NORM_VALUES",
                    "", errbuf, errlen) != 0 ||
        qa_cal_walk(who, ndays, ymd, cal, errbuf, errlen) != 0)
        return -1;
    const size_t ns = (size_t)nstn, nd = (size_t)ndays;
    QACHK(hipSetDevice(device));
    QaBuf b_obs, b_flag, b_cal, b_norm;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_obs.p, 2 * ns * nd * 4));                  // [2][nstn][ndays]
    float *d_tmin = static_cast<float *>(b_obs.p), *d_tmax = d_tmin + ns * nd;
    QACHK(hipMemcpy(d_tmin, tmin, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_tmax, tmax, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_flag.p, 2 * ns * nd));
    uint8_t *d_f0 = static_cast<uint8_t *>(b_flag.p), *d_f1 = d_f0 + ns * nd;
    QaCal k;
    if (qa_upload_calendar(cal, cal.normrow, b_cal, k, errbuf, errlen) != 0) return -1;
    QACHK(hipMalloc(&b_norm.p, ns * 2 * TWXQA_NORM_ROWS * 2 * 8)); // [nstn][2][731][2]
    double *d_norm = static_cast<double *>(b_norm.p);

    float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned g_day = (unsigned)((ns * nd + 255) / 256), g_day2 = (unsigned)((2 * ns * nd + 255) / 256);
    // ---- missing (2), naught (3) ---------------------------------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_init, dim3(g_day), dim3(256), 0, nullptr, (int64_t)(ns * nd), (const float *)d_tmin,
                       (const float *)d_tmax, d_f0, d_f1);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[0]));
    // ---- the duplicates (4, 6, 5, 7), impossible values (8) ----------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_dups, dim3((unsigned)ns), dim3(256), 0, nullptr, ndays, k, (const float *)d_tmin,
                       (const float *)d_tmax, d_f0, d_f1);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[1]));
    // ---- streaks (9) -------------------------------------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_streak, dim3((unsigned)(2 * ns)), dim3(64), 0, nullptr, ndays, (const float *)d_tmin, d_f0);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[2]));
    // ---- gaps (10) ---------------------------------------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_gap, dim3((unsigned)(2 * ns * 12)), dim3(256), 0, nullptr, ndays, k, (const float *)d_tmin, d_f0);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[3]));
    // ---- the day-of-year rows of what is left, then the outliers (15) and Tmin > Tmax (11) ---------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_norms, dim3((unsigned)(2 * ns * NS_NJOBS)), dim3(256), 0, nullptr, ndays, nstn, cal.nyears,
                       k.yr, (const float *)d_tmin, (const uint8_t *)d_f0, d_norm);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[4]));
    if (norms) QACHK(hipMemcpy(norms, d_norm, ns * 2 * TWXQA_NORM_ROWS * 2 * 8, hipMemcpyDeviceToHost));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_clim, dim3(g_day), dim3(256), 0, nullptr, ndays, nstn, k.row, (const float *)d_tmin,
                       (const float *)d_tmax, (const double *)d_norm, d_f0, d_f1);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[5]));
    // ---- spike / dip (13), then the lagged range (12) on what it left ------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_spike, dim3(g_day2), dim3(256), 0, nullptr, ndays, (int64_t)(2 * ns), (const float *)d_tmin, d_f0);
    QACHK(hipGetLastError());
    hipLaunchKernelGGL(k_ns_lagrange, dim3(g_day), dim3(256), 0, nullptr, ndays, nstn, (const float *)d_tmin,
                       (const float *)d_tmax, d_f0, d_f1);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[6]));
    // ---- mega-inconsistency (18) ---------------------------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_ns_mega, dim3((unsigned)ns), dim3(256), 0, nullptr, ndays, k.month, (const float *)d_tmin,
                       (const float *)d_tmax, d_f0, d_f1);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[7]));
    QACHK(hipMemcpy(flag_tmin, d_f0, ns * nd, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(flag_tmax, d_f1, ns * nd, hipMemcpyDeviceToHost));
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
