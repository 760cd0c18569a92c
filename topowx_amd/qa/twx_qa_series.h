// The calendar of a day axis and the series helpers that the step08 temperature QA and the precipitation QA share
// (twx_nonspatial.hip, twx_corrob.hip, twx_prcpqa.hip, twx_prcpcorrob.hip; qa_finitef also twx_infillmat.hip).  Internal, as
// twx_qa_common.h: everything has internal linkage.  The reference's calendar quirks live here once: the row of the day's
// own year, the Feb-29 windows, the count of distinct months behind the skipped month of check 6.
#ifndef TWX_QA_SERIES_H
#define TWX_QA_SERIES_H

#include "twx_qa_common.h"

#define QA_LIVE 1                            // an observation is in its series exactly while its flag is 1 (QA_OK of both chains)
#define QA_BIWEIGHT_C 7.5                    // qa_temp.py:1173, 1194

namespace {

// The tables of a day axis of consecutive calendar days.  qa_cal_years sets nyears, qa_cal_walk everything else.
struct QaCalendar {
    int y0 = 0, m0 = 0, d0 = 0;     // ymd[0]
    int nyears = 0;                 // the years the axis touches
    int ndistinct = 0;              // the distinct month numbers on the axis
    std::vector<int32_t> yr;        // [nyears][2]: Jan 1's series index (may lie before the axis), leap
    std::vector<int32_t> row;       // [ndays] yday - 1 of the day's own year: 0 .. 365
    std::vector<int32_t> normrow;   // [ndays] row of the 731-row normals: the 365-row table first, a leap year's day in the second
    std::vector<uint16_t> mday;     // [ndays] the month-day's index in a leap year's calendar (the date of 2004): 0 .. 365
    std::vector<uint8_t> month;     // [ndays] 1 .. 12
    std::vector<uint8_t> yidx;      // [ndays] index of the day's year among the years the axis touches
    std::vector<int32_t> ystart, ylen;      // [nyears] first day of the year that is on the axis, days of it on the axis
    std::vector<int32_t> mstart, mlen;      // [nyears][12] the same per month (length 0: none)
};

// ymd[0] is a date, and the years the axis touches: known before the walk, so that a caller can cap them first.
inline int qa_cal_years(const char *who, int64_t ndays, const int32_t *ymd, QaCalendar &c, char *errbuf, int errlen)
{
    const int32_t a = ymd[0];
    c.y0 = a / 10000, c.m0 = (a / 100) % 100, c.d0 = a % 100;
    if (a < 10101 || c.m0 < 1 || c.m0 > 12 || c.d0 < 1 || c.d0 > 31) {
        char msg[96];
        snprintf(msg, sizeof msg, "%s: ymd[0] is not a date", who);
        return qa_fail(errbuf, errlen, msg);
    }
    const int64_t zlast = qa_days_from_civil(c.y0, c.m0, c.d0) + ndays - 1;
    int64_t ylast = c.y0 + (ndays - 1) / 366;
    while (qa_days_from_civil(ylast + 1, 1, 1) <= zlast) ++ylast;
    c.nyears = (int)(ylast - c.y0 + 1);                              // ndays < 2^31: fits
    return 0;
}

// A kernel holds per_year values of every year in `cap` slots: "<what> = <cap> values<of> (<per_year> per year, <n> years)".
inline int qa_year_cap(const char *who, const QaCalendar &c, int per_year, int cap, const char *what, const char *of,
                       char *errbuf, int errlen)
{
    if ((int64_t)c.nyears * per_year <= cap) return 0;
    char msg[320];
    snprintf(msg, sizeof msg, "%s: the series touches %d years; %s = %d values%s (%d per year, %d years)", who, c.nyears, what,
             cap, of, per_year, cap / per_year);
    return qa_fail(errbuf, errlen, msg);
}

// The walk (after qa_cal_years): every day is the day after the one before it, and every table.  The tables are sized by
// c.nyears whatever it is, so the walk may run before a caller's cap (the count is never below the years walked: a ymd[0]
// like Feb 30 only moves the computed end later); yidx is a byte, and an entry whose kernels read it caps the years below 256.
inline int qa_cal_walk(const char *who, int64_t ndays, const int32_t *ymd, QaCalendar &c, char *errbuf, int errlen)
{
    char msg[160];
    const size_t nd = (size_t)ndays, ny = (size_t)c.nyears;
    c.row.resize(nd);
    c.normrow.resize(nd);
    c.mday.resize(nd);
    c.month.resize(nd);
    c.yidx.resize(nd);
    c.ystart.assign(ny, 0);
    c.ylen.assign(ny, 0);
    c.mstart.assign(ny * 12, 0);
    c.mlen.assign(ny * 12, 0);
    static const int mlen[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    static const int cum[12] = {0, 31, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335};    // a leap year's
    int y = c.y0, mth = c.m0, day = c.d0;
    size_t k = 0;
    bool seen[12] = {false, false, false, false, false, false, false, false, false, false, false, false};
    int64_t jan1 = qa_days_from_civil(y, 1, 1) - qa_days_from_civil(y, mth, day);
    c.yr.assign({(int32_t)jan1, qa_leap(y) ? 1 : 0});
    for (int64_t i = 0; i < ndays; ++i) {
        if (ymd[i] != y * 10000 + mth * 100 + day) {
            snprintf(msg, sizeof msg, "%s: ymd[%lld] = %d: the days are not consecutive calendar days", who, (long long)i,
                     (int)ymd[i]);
            return qa_fail(errbuf, errlen, msg);
        }
        c.row[(size_t)i] = (int32_t)(i - jan1);
        c.normrow[(size_t)i] = (int32_t)(i - jan1) + (qa_leap(y) ? 365 : 0);
        c.mday[(size_t)i] = (uint16_t)(cum[mth - 1] + day - 1);
        c.month[(size_t)i] = (uint8_t)mth;
        c.yidx[(size_t)i] = (uint8_t)k;
        seen[mth - 1] = true;
        if (c.ylen[k]++ == 0) c.ystart[k] = (int32_t)i;
        const size_t seg = k * 12 + (size_t)(mth - 1);
        if (c.mlen[seg]++ == 0) c.mstart[seg] = (int32_t)i;
        if (++day > mlen[mth - 1] + ((mth == 2 && qa_leap(y)) ? 1 : 0)) {
            day = 1;
            if (++mth > 12) {
                mth = 1;
                ++y;
                jan1 = i + 1;
                if (i + 1 < ndays) { ++k; c.yr.push_back((int32_t)jan1); c.yr.push_back(qa_leap(y) ? 1 : 0); }
            }
        }
    }
    for (int m = 0; m < 12; ++m) c.ndistinct += seen[m] ? 1 : 0;
    if (c.yr.size() != 2 * ny) {
        snprintf(msg, sizeof msg, "%s: calendar count mismatch", who);
        return qa_fail(errbuf, errlen, msg);
    }
    return 0;
}

// the calendar of a day axis on the device
struct QaCal {
    const uint8_t *month;      // [ndays] 1..12
    const uint8_t *yidx;       // [ndays] index of the day's year among the years the axis touches
    const int32_t *row;        // [ndays] the caller's row table: QaCalendar::normrow or QaCalendar::row
    const int32_t *ystart;     // [nyears] first day of the year that is on the axis
    const int32_t *ylen;       // [nyears] days of the year on the axis
    const int32_t *mstart;     // [nyears][12] first day of the month on the axis
    const int32_t *mlen;       // [nyears][12] days of the month on the axis (0: none)
    const int2 *yr;            // [nyears] (series index of Jan 1 -- may lie before the axis --, leap)
    int nyears;
    int skip_month;            // the month NUMBER never taken as the first of a pair by check 6 (qa_temp.py:360, qa_prcp.py:266)
};

// the device copy of the calendar with `row` as its row table; k's pointers point into b.p
inline int qa_upload_calendar(const QaCalendar &cal, const std::vector<int32_t> &row, QaBuf &b, QaCal &k, char *errbuf,
                              int errlen)
{
    const size_t nd = row.size(), ny = (size_t)cal.nyears;
    // int32 tables first (yr, row, ystart, ylen, mstart, mlen), then the bytes (month, yidx)
    const size_t o_yr = 0, o_row = o_yr + ny * 8, o_ys = o_row + nd * 4, o_yl = o_ys + ny * 4, o_ms = o_yl + ny * 4,
                 o_ml = o_ms + ny * 48, o_mth = o_ml + ny * 48, o_yi = o_mth + nd;
    QACHK(hipMalloc(&b.p, o_yi + nd));
    char *dc = static_cast<char *>(b.p);
    QAUP(dc + o_yr, cal.yr.data(), int32_t, ny * 2);
    QAUP(dc + o_row, row.data(), int32_t, nd);
    QAUP(dc + o_ys, cal.ystart.data(), int32_t, ny);
    QAUP(dc + o_yl, cal.ylen.data(), int32_t, ny);
    QAUP(dc + o_ms, cal.mstart.data(), int32_t, ny * 12);
    QAUP(dc + o_ml, cal.mlen.data(), int32_t, ny * 12);
    QAUP(dc + o_mth, cal.month.data(), uint8_t, nd);
    QAUP(dc + o_yi, cal.yidx.data(), uint8_t, nd);
    k.month = (const uint8_t *)(dc + o_mth);
    k.yidx = (const uint8_t *)(dc + o_yi);
    k.row = (const int32_t *)(dc + o_row);
    k.ystart = (const int32_t *)(dc + o_ys);
    k.ylen = (const int32_t *)(dc + o_yl);
    k.mstart = (const int32_t *)(dc + o_ms);
    k.mlen = (const int32_t *)(dc + o_ml);
    k.yr = (const int2 *)(dc + o_yr);
    k.nyears = cal.nyears;
    k.skip_month = cal.ndistinct - 1;
    return 0;
}

#ifdef __HIPCC__

__device__ __forceinline__ bool qa_finitef(float v) { return fabsf(v) <= 3.40282346638528859812e38f; }

// sum over the 256 threads of a workgroup, in a fixed tree order; every thread returns the same value
__device__ __forceinline__ double qa_block_sum(double v, double *red, int tid)
{
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// two stretches of one series compared by position over the shorter one: all == (a NaN or a removed value: no)
__device__ __forceinline__ bool qa_same(const float *__restrict__ x, const uint8_t *f, int a, int la, int b, int lb)
{
    const int n = la < lb ? la : lb;
    for (int j = 0; j < n; ++j) {
        if (f[a + j] != QA_LIVE || f[b + j] != QA_LIVE) return false;
        if (!(x[a + j] == x[b + j])) return false;
    }
    return true;
}

// The series index of the date q (its index in a leap year's calendar, 59: Feb 29) in the year y (x: series index of
// Jan 1, y: leap year); -1: a common year has no Feb 29, or the day is off the axis.
__device__ __forceinline__ int64_t qa_date_day(int q, int2 y, int64_t ndays)
{
    if (q == 59 && !y.y) return -1;
    const int64_t d = (int64_t)y.x + ((q < 59 || y.y) ? q : q - 1);
    return d < ndays ? d : -1;                                       // (d < 0: before the axis)
}

// Bitonic sort of xs[0, np2) in LDS, float32, ascending, by the 256 threads of a workgroup.  np2 is a power of two, the
// slots beyond the n values already hold +inf (they stay behind the values), every thread of the workgroup calls it
// (np2 uniform) after a barrier that follows the last store into xs, and it ends on a barrier.
__device__ __forceinline__ void qa_lds_sort(float *xs, int np2, int tid)
{
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const float a = xs[i], b = xs[ixj];
                    if ((a > b) == ((i & k) == 0)) { xs[i] = b; xs[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// The streak check of one series by one wavefront (lane = threadIdx.x of 64): the series is walked in blocks of 64 days;
// the values walked are those with flag OK for which wet(value) holds, the others are skipped and break no run.  Runs of
// equal values come from ballots, a run's length from the ranks (among the values walked) of its start and of the next
// start, carried across blocks; a run of >= LEN gets STREAK once a different value ends it -- in this block by the lane's
// own store, in the blocks before by the loop from carry_day.  A run that reaches the end of the series is never ended.
template <int OK, int STREAK, int LEN, class Wet>
__device__ __forceinline__ void qa_streak_walk(int64_t ndays, const float *x, uint8_t *f, Wet wet)
{
    const int lane = threadIdx.x;
    const uint64_t lt = ((uint64_t)1 << lane) - 1;                       // lanes below
    const uint64_t le = ((uint64_t)2 << lane) - 1;                       // lanes below and this one (lane 63: all)
    bool carry_has = false;                                              // a run is open from the blocks before
    float carry_val = 0.0f;
    int carry_rank = 0, rank_base = 0;                                   // rank and day of the open run's first value;
    int64_t carry_day = 0;                                               // ndays < 2^31
    for (int64_t b0 = 0; b0 < ndays; b0 += 64) {                         // uniform
        const int64_t d = b0 + lane;
        float v = 0.0f;
        bool live = d < ndays && f[d] == OK;
        if (live) { v = x[d]; live = wet(v); }
        const uint64_t lm = __ballot(live);
        if (lm == 0) continue;
        const uint64_t below = lm & lt;
        const float pv = __shfl(v, below ? 63 - __clzll(below) : lane);
        const bool start = live && (below ? !(v == pv) : (!carry_has || !(v == carry_val)));
        const uint64_t sm = __ballot(start);
        const int rank = rank_base + __popcll(below);
        const uint64_t s_le = sm & le, s_gt = sm & ~le;
        const int g = s_le ? 63 - __clzll(s_le) : -1;                    // the start of this lane's run, -1: the open run
        const int nx = s_gt ? __ffsll((unsigned long long)s_gt) - 1 : -1;  // the next start, -1: none in this block
        const int rank_g = __shfl(rank, g >= 0 ? g : lane), rank_nx = __shfl(rank, nx >= 0 ? nx : lane);
        if (live && nx >= 0 && rank_nx - (g >= 0 ? rank_g : carry_rank) >= LEN) f[d] = STREAK;
        if (sm != 0) {
            const int first = __ffsll((unsigned long long)sm) - 1, last = 63 - __clzll(sm);
            const int rank_first = rank_base + __popcll(lm & (((uint64_t)1 << first) - 1));
            if (carry_has && rank_first - carry_rank >= LEN)             // the open run ended here: its earlier blocks
                for (int64_t e = carry_day + lane; e < b0; e += 64)
                    if (f[e] == OK && wet(x[e])) f[e] = STREAK;
            carry_rank = rank_base + __popcll(lm & (((uint64_t)1 << last) - 1));
            carry_day = b0 + last;
        }
        carry_has = true;
        carry_val = __shfl(v, 63 - __clzll(lm));
        rank_base += __popcll(lm);
    }
}

// The statistics of a day-of-year row from its n >= 1 values sorted in xs (LDS), by the 256 threads of a workgroup after a
// barrier: numpy's median M, the median of |X - M| by counting -- left of the middle the deviations do not rise, right of it
// they do not fall, so the number of deviations below / not above a candidate is two binary searches, and the order
// statistics wanted are the candidates whose counts bracket them -- and the biweight mean (_biweight_mean), with SD the
// biweight standard deviation next to it (_biweight_mean_std); the plain mean and std(ddof = 1) where MAD == 0, an exact
// test.  The sums run in a fixed tree order.  red [256], mad_k [2]: LDS scratch.  Every thread returns the same values.
template <bool SD>
__device__ __forceinline__ double qa_biweight(const float *xs, int n, double *red, double *mad_k, int tid, double *sd)
{
    const int p = n >> 1;
    const double M = (n & 1) ? (double)xs[p] : ((double)xs[p - 1] + (double)xs[p]) / 2.0;
    const int k1 = (n - 1) >> 1, k2 = n >> 1;
    for (int i = tid; i < n; i += 256) {
        const double v = i < p ? M - (double)xs[i] : (double)xs[i] - M;
        int lo = 0, hi = p;                                      // first a with M - xs[a] <= v
        while (lo < hi) { const int m = (lo + hi) >> 1; if (M - (double)xs[m] <= v) hi = m; else lo = m + 1; }
        int c_le = p - lo;
        lo = 0; hi = p;                                          // first a with M - xs[a] < v
        while (lo < hi) { const int m = (lo + hi) >> 1; if (M - (double)xs[m] < v) hi = m; else lo = m + 1; }
        int c_lt = p - lo;
        lo = p; hi = n;                                          // first b with xs[b] - M > v
        while (lo < hi) { const int m = (lo + hi) >> 1; if ((double)xs[m] - M > v) hi = m; else lo = m + 1; }
        c_le += lo - p;
        lo = p; hi = n;                                          // first b with xs[b] - M >= v
        while (lo < hi) { const int m = (lo + hi) >> 1; if ((double)xs[m] - M >= v) hi = m; else lo = m + 1; }
        c_lt += lo - p;
        if (c_lt <= k1 && k1 < c_le) mad_k[0] = v;               // (equal values may all write: the same bits)
        if (c_lt <= k2 && k2 < c_le) mad_k[1] = v;
    }
    __syncthreads();
    const double MAD = (n & 1) ? mad_k[0] : (mad_k[0] + mad_k[1]) / 2.0;
    if (MAD == 0.0) {
        double sum = 0.0;
        for (int i = tid; i < n; i += 256) sum = sum + (double)xs[i];
        const double mean = qa_block_sum(sum, red, tid) / (double)n;
        if (SD) {
            double ss = 0.0;
            for (int i = tid; i < n; i += 256) { const double dx = (double)xs[i] - mean; ss = ss + dx * dx; }
            *sd = sqrt(qa_block_sum(ss, red, tid) / (double)(n - 1));
        }
        return mean;
    }
    const double scale = QA_BIWEIGHT_C * MAD;
    double num = 0.0, den = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double dx = (double)xs[i] - M;
        double u = dx / scale;
        if (fabs(u) >= 1.0) u = 1.0;
        const double u2 = u * u, h = 1.0 - u2, w = h * h;
        num = num + dx * w;
        den = den + w;
        if (SD) {
            s1 = s1 + (dx * dx) * (w * w);
            s2 = s2 + h * (1.0 - 5.0 * u2);
        }
    }
    num = qa_block_sum(num, red, tid);
    den = qa_block_sum(den, red, tid);
    if (SD) {
        s1 = qa_block_sum(s1, red, tid);
        s2 = qa_block_sum(s2, red, tid);
        *sd = sqrt((double)n * s1) / fabs(s2);
    }
    return M + num / den;
}

#endif  // __HIPCC__

}  // namespace

#endif  // TWX_QA_SERIES_H
