// twx_corrob.hip -- libtwxqa.so: the rest of step08's spatial QA stage (run_qa_spatial_only, twx/qa/qa_temp.py:218-258):
// the day-of-year normals (_get_norms_md_masks / _build_mean_norms / _biweight_mean, :1111-1130, 1171-1184, 1215-1228),
// the corroboration check (_qa_spatial_corrob / _get_spatial_corrob_flag, :740-813, 1017-1082) and _qa_mega_inconsist
// (:815-840).  The third translation unit of the library (include/twx_qa.h); the regression check that runs first is
// twxqa_spatial_regress of twx_spatial.hip, called as it is.
//
// k_doy_norms: one 256-thread workgroup per (series, table row job).  A series has two tables, 365 rows from the dates
// of 2003 and 366 rows from those of 2004; a row takes the finite days whose (month, day) is one of the 15 dates
// around the row's date.  Wherever no window holds Feb 29 the two tables have the same row, so there are 380 jobs, not
// 731: the 365 rows of the first table (351 of them also stored into the second) and the 15 rows Feb 22 .. Mar 7 of
// the second.  A job gathers its values year by year (thread = (year, date of the window)) into LDS, sorts them
// (bitonic, float32: exact, the observations are float32), takes numpy's median M, then the median of |X - M| by
// counting: left of the middle the deviations fall, right of it they rise, so the number of deviations below / not
// above a candidate is two binary searches, and the order statistics wanted are the candidates whose counts bracket
// them.  Both medians are exact (no histogram), so MAD == 0 is an exact test.  The sums run over the sorted values in
// a fixed tree order: the result does not depend on the order of the gather.
// LDS: 4 bytes per value + 2 KiB of reduction scratch: TWXQA_MAX_NORM_VALUES = 2048 costs 10 KiB per workgroup, and the
// 8 workgroups that fill a compute unit's 32 wave slots take 80 KiB of its 160 KiB.
//
// k_radius_dist: one wavefront per target; pass 0 counts the stations within 75 km (as k_qa_radius, same arithmetic),
// pass 1 collects (distance, row) in LDS and writes them rank-sorted by distance, equal distances in table order.
//
// k_corrob: one wavefront per (target, variable, block of 64 days); a lane owns a day x and reads days x - 1, x, x + 1
// of each neighbour in distance order, counting finite observations and taking, per day, the first 7 finite anomalies
// |obs - own normal|.  The neighbour walk ends once every lane has its counts and either its 3 x 7 or a corroborating
// anomaly.  A day with the three counts >= 3 and NO anomaly within ANOMALY_CUTOFF is flagged -- also when the list of
// anomalies is empty (the reference's difs.size == 0 case, kept for parity).
//
// k_mega_final: one workgroup per target: the month-of-year extremes of the series after both removals, the
// mega-inconsistency flags, and the final flag numbers 1 / 2 / 16 / 17 / 18.
// fp64 throughout; the observations are float32 widened exactly.  The library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_series.h"

#define CB_NJOBS 380                         // 365 rows + the 15 leap rows whose window holds Feb 29
#define CB_LEAP_FIRST 52                     // Feb 22 of the 366-row table
#define CB_QA_OK 1                           // qa_temp.py:41-59
#define CB_QA_MISSING 2
#define CB_QA_SPATIAL_REGRESS 16
#define CB_QA_SPATIAL_CORROB 17
#define CB_QA_MEGA_INCONSIST 18

namespace {

__device__ __forceinline__ bool cb_finite(double v) { return fabs(v) <= 1.79769313486231570e308; }

}  // namespace

__global__ __launch_bounds__(256) void k_doy_norms(int64_t ndays, int nyears, const int2 *__restrict__ yr,
                                                   const float *__restrict__ obs, const int32_t *__restrict__ rows,
                                                   const uint8_t *__restrict__ mask, double *__restrict__ out,
                                                   int ostride, int ooff)
{
    __shared__ float xs[TWXQA_MAX_NORM_VALUES];
    __shared__ double red[256];
    __shared__ double mad_k[2];
    __shared__ int cnt;
    const int tid = threadIdx.x;
    const int job = (int)(blockIdx.x % CB_NJOBS);
    const int64_t s = blockIdx.x / CB_NJOBS;
    const bool leap_job = job >= 365;
    const int centre = leap_job ? CB_LEAP_FIRST + (job - 365) : job;     // row of the job's own table
    const int period = leap_job ? 366 : 365;
    if (tid == 0) cnt = 0;
    __syncthreads();

    // ---- gather: thread = (year k, date j of the window); q is the date's index in a leap year's calendar ----------
    const float *src = obs + (size_t)rows[s] * (size_t)ndays;
    const uint8_t *msk = mask ? mask + (size_t)s * (size_t)ndays : nullptr;
    for (int i = tid; i < nyears * 16; i += 256) {
        const int k = i >> 4, j = i & 15;
        if (j == 15) continue;
        int t = centre - 7 + j;
        t = t < 0 ? t + period : (t >= period ? t - period : t);
        const int q = (leap_job || t < 59) ? t : t + 1;
        const int64_t d = qa_date_day(q, yr[k], ndays);          // (a 365-row window never holds Feb 29: q != 59 there)
        if (d < 0) continue;
        if (msk && msk[d]) continue;
        const float v = src[d];
        if (!qa_finitef(v)) continue;
        xs[atomicAdd(&cnt, 1)] = v;                              // <= 15 * nyears <= TWXQA_MAX_NORM_VALUES (host check)
    }
    __syncthreads();
    const int n = cnt;
    double result = __builtin_nan("");
    if (n >= TWXQA_MIN_NORM_VALUES) {                            // uniform
        // ---- bitonic sort, ascending, padded with +inf to a power of two ----------------------------------------
        int np2 = 1;
        while (np2 < n) np2 <<= 1;
        for (int i = n + tid; i < np2; i += 256) xs[i] = __builtin_inff();
        __syncthreads();
        qa_lds_sort(xs, np2, tid);
        result = qa_biweight<false>(xs, n, red, mad_k, tid, nullptr);
    }
    if (tid == 0) {
        double *o = out + ((size_t)s * ostride + ooff) * TWXQA_NORM_ROWS;   // table (s, ooff) of [nseries][ostride][731]
        if (leap_job) {
            o[365 + centre] = result;
        } else {
            o[job] = result;
            if (job < CB_LEAP_FIRST) o[365 + job] = result;                      // Jan 1 .. Feb 21
            else if (job >= CB_LEAP_FIRST + 14) o[365 + job + 1] = result;       // Mar 8 .. Dec 31
        }
    }
}

__global__ __launch_bounds__(64) void k_radius_dist(int64_t nstn, const double *__restrict__ lon,
                                                    const double *__restrict__ lat, const int32_t *__restrict__ target_idx,
                                                    int fill, int32_t *__restrict__ count,
                                                    const int64_t *__restrict__ csr_off, int32_t *__restrict__ csr_ngh,
                                                    double *__restrict__ csr_dist)
{
    __shared__ double ld[TWXQA_MAX_RADIUS_NGH];
    __shared__ int32_t lj[TWXQA_MAX_RADIUS_NGH];
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int32_t self = target_idx[t];
    const double lat1rad = lat[self] * QA_RADIAN, lon1rad = lon[self] * QA_RADIAN;
    const double cos1 = cos(lat1rad);
    int64_t pos = 0;
    int room = 0;
    if (fill) {                                                  // a target over the cap has an empty list
        pos = csr_off[t];
        room = (int)(csr_off[t + 1] - pos);                      // <= TWXQA_MAX_RADIUS_NGH
        if (room == 0) return;
    }
    int32_t n = 0;
    for (int64_t j0 = 0; j0 < nstn; j0 += 64) {                  // uniform
        const int64_t j = j0 + lane;
        bool in = false;
        double dist = 0.0;
        if (j < nstn && j != self) {
            dist = qa_dist_km(lat1rad, lon1rad, cos1, lat[j], lon[j]);
            in = dist <= TWXQA_NGH_RADIUS_KM;
        }
        const uint64_t b = __ballot(in);
        if (fill && in) {
            const int k = n + __popcll(b & (((uint64_t)1 << lane) - 1));
            if (k < room) { ld[k] = dist; lj[k] = (int32_t)j; }
        }
        n += __popcll(b);
    }
    if (!fill) {
        if (lane == 0) count[t] = n;
        return;
    }
    __syncthreads();
    const int m = n < room ? n : room;
    for (int i = lane; i < m; i += 64) {                         // rank sort: ascending distance, then table order
        const double di = ld[i];
        int rank = 0;
        for (int k = 0; k < m; ++k) {
            const double dk = ld[k];
            rank += (dk < di || (dk == di && k < i)) ? 1 : 0;
        }
        csr_ngh[pos + rank] = lj[i];
        csr_dist[pos + rank] = di;
    }
}

__global__ __launch_bounds__(64) void k_corrob(int64_t ndays, int nblk, const float *__restrict__ tmin,
                                               const float *__restrict__ tmax, const int32_t *__restrict__ normrow,
                                               const int32_t *__restrict__ target_idx, const int64_t *__restrict__ csr_off,
                                               const int32_t *__restrict__ csr_ngh, const int32_t *__restrict__ slot,
                                               int64_t nslot, const double *__restrict__ nnorm,
                                               const double *__restrict__ tnorm, const uint8_t *__restrict__ r_tmin,
                                               const uint8_t *__restrict__ r_tmax, uint8_t *__restrict__ c_tmin,
                                               uint8_t *__restrict__ c_tmax)
{
    const int lane = threadIdx.x;
    const int64_t item = blockIdx.x;                             // (t * 2 + v) * nblk + blk
    const int blk = (int)(item % nblk);
    const int64_t tv = item / nblk;
    const int v = (int)(tv & 1);
    const int64_t t = tv >> 1;
    const int64_t n0 = csr_off[t];
    const int nngh = (int)(csr_off[t + 1] - n0);
    if (nngh < TWXQA_MIN_NGHS) return;                           // uniform (qa_temp.py:763)
    const float *obs = v ? tmax : tmin;
    const int64_t x = (int64_t)blk * 64 + lane;
    const bool active = x >= 1 && x <= ndays - 2;                // not the first / last day of the series (:805)
    const double nan = __builtin_nan("");
    double anom = nan;
    int row[3] = {0, 0, 0};
    if (active) {
        const uint8_t removed = (v ? r_tmax : r_tmin)[(size_t)t * ndays + x];
        const double val = removed ? nan : (double)obs[(size_t)target_idx[t] * ndays + x];
        row[0] = normrow[x - 1];
        row[1] = normrow[x];
        row[2] = normrow[x + 1];
        anom = fabs(val - tnorm[((size_t)t * 2 + v) * TWXQA_NORM_ROWS + row[1]]);
    }
    const bool test = active && cb_finite(anom);
    int nfin[3] = {0, 0, 0}, ntake[3] = {0, 0, 0};
    bool corrob = false;
    for (int q = 0; q < nngh; ++q) {                             // uniform
        const bool counted = nfin[0] >= TWXQA_MIN_NGHS && nfin[1] >= TWXQA_MIN_NGHS && nfin[2] >= TWXQA_MIN_NGHS;
        const bool full = ntake[0] >= TWXQA_MAX_NGHS && ntake[1] >= TWXQA_MAX_NGHS && ntake[2] >= TWXQA_MAX_NGHS;
        const bool want = test && !(counted && (full || corrob));
        if (__ballot(want) == 0) break;
        const int32_t j = csr_ngh[n0 + q];
        if (want) {
            const float *col = obs + (size_t)j * ndays + (x - 1);
            const double *nn = nnorm + ((size_t)v * nslot + slot[j]) * TWXQA_NORM_ROWS;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double o = (double)col[c];
                if (cb_finite(o)) {
                    ++nfin[c];
                    if (ntake[c] < TWXQA_MAX_NGHS) {
                        const double a = fabs(o - nn[row[c]]);
                        if (cb_finite(a)) {
                            ++ntake[c];
                            if (!(fabs(a - anom) >= TWXQA_ANOMALY_CUTOFF)) corrob = true;
                        }
                    }
                }
            }
        }
    }
    if (test && nfin[0] >= TWXQA_MIN_NGHS && nfin[1] >= TWXQA_MIN_NGHS && nfin[2] >= TWXQA_MIN_NGHS && !corrob)
        (v ? c_tmax : c_tmin)[(size_t)t * ndays + x] = 1;
}

__global__ __launch_bounds__(256) void k_mega_final(int64_t ndays, const float *__restrict__ tmin,
                                                    const float *__restrict__ tmax, const uint8_t *__restrict__ month,
                                                    const int32_t *__restrict__ target_idx, const uint8_t *__restrict__ r_tmin,
                                                    const uint8_t *__restrict__ r_tmax, const uint8_t *__restrict__ c_tmin,
                                                    const uint8_t *__restrict__ c_tmax, uint8_t *__restrict__ f_tmin,
                                                    uint8_t *__restrict__ f_tmax)
{
    __shared__ float red[2][12][256];                            // 0: lowest Tmin, 1: highest Tmax of a calendar month
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const size_t o0 = (size_t)target_idx[t] * ndays, f0 = (size_t)t * ndays;
    const float inf = __builtin_inff();
    for (int m = 0; m < 12; ++m) { red[0][m][tid] = inf; red[1][m][tid] = -inf; }
    for (int64_t d = tid; d < ndays; d += 256) {                 // (a thread touches its own column of red only)
        const int m = month[d] - 1;
        const float a = tmin[o0 + d], b = tmax[o0 + d];
        if (qa_finitef(a) && !r_tmin[f0 + d] && !c_tmin[f0 + d]) red[0][m][tid] = fminf(red[0][m][tid], a);
        if (qa_finitef(b) && !r_tmax[f0 + d] && !c_tmax[f0 + d]) red[1][m][tid] = fmaxf(red[1][m][tid], b);
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
        const bool both = lo != inf && hi != -inf;               // a month with no finite value on either side is skipped
        const float a = tmin[o0 + d], b = tmax[o0 + d];
        uint8_t fa = CB_QA_OK, fb = CB_QA_OK;
        if (a != a) fa = CB_QA_MISSING;
        else if (r_tmin[f0 + d]) fa = CB_QA_SPATIAL_REGRESS;
        else if (c_tmin[f0 + d]) fa = CB_QA_SPATIAL_CORROB;
        else if (both && qa_finitef(a) && a > hi) fa = CB_QA_MEGA_INCONSIST;
        if (b != b) fb = CB_QA_MISSING;
        else if (r_tmax[f0 + d]) fb = CB_QA_SPATIAL_REGRESS;
        else if (c_tmax[f0 + d]) fb = CB_QA_SPATIAL_CORROB;
        else if (both && qa_finitef(b) && b < lo) fb = CB_QA_MEGA_INCONSIST;
        f_tmin[f0 + d] = fa;
        f_tmax[f0 + d] = fb;
    }
}

// ---------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------
namespace {

// The calendar of a day axis; these entries report a day out of sequence before the cap on the years.
int cb_cal(const char *who, int64_t ndays, const int32_t *ymd, QaCalendar &c, char *errbuf, int errlen)
{
    if (qa_cal_years(who, ndays, ymd, c, errbuf, errlen) != 0 || qa_cal_walk(who, ndays, ymd, c, errbuf, errlen) != 0) return -1;
    return qa_year_cap(who, c, 15, TWXQA_MAX_NORM_VALUES, "a row of the day-of-year normals holds at most TWXQA_MAX_NORM_VALUES",
                       "", errbuf, errlen);
}

}  // namespace

extern "C" int twxqa_doy_norms(int device, int64_t nseries, int64_t ndays, const float *series, const int32_t *ymd,
                               double *norms, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nseries < 1 || ndays < 1 || ndays > INT32_MAX - 64 || nseries * CB_NJOBS > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxqa_doy_norms: need nseries >= 1, ndays >= 1 and nseries * 380 < 2^31");
    if (!series || !ymd || !norms) return qa_fail(errbuf, errlen, "twxqa_doy_norms: null buffer");
    QaCalendar cal;
    if (cb_cal("twxqa_doy_norms", ndays, ymd, cal, errbuf, errlen) != 0) return -1;
    const size_t ns = (size_t)nseries, nd = (size_t)ndays;
    QACHK(hipSetDevice(device));
    QaBuf b_obs, b_yr, b_rows, b_out;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_obs.p, ns * nd * 4));
    QACHK(hipMemcpy(b_obs.p, series, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_yr.p, cal.yr.size() * 4));
    QACHK(hipMemcpy(b_yr.p, cal.yr.data(), cal.yr.size() * 4, hipMemcpyHostToDevice));
    std::vector<int32_t> rows(ns);
    for (size_t i = 0; i < ns; ++i) rows[i] = (int32_t)i;
    QACHK(hipMalloc(&b_rows.p, ns * 4));
    QACHK(hipMemcpy(b_rows.p, rows.data(), ns * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_out.p, ns * TWXQA_NORM_ROWS * 8));
    float ms = 0.0f;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_doy_norms, dim3((unsigned)(ns * CB_NJOBS)), dim3(256), 0, nullptr, ndays, cal.nyears,
                       (const int2 *)b_yr.p, (const float *)b_obs.p, (const int32_t *)b_rows.p, (const uint8_t *)nullptr,
                       (double *)b_out.p, 1, 0);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms));
    if (kernel_ms) kernel_ms[0] = ms;
    QACHK(hipMemcpy(norms, b_out.p, ns * TWXQA_NORM_ROWS * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int twxqa_spatial_only(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                                  const float *tmin, const float *tmax, const int32_t *ymd, int64_t ntarget,
                                  const int32_t *target_idx, uint8_t *flag_tmin, uint8_t *flag_tmax, double *norms,
                                  int32_t *status, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || ntarget < 1 || nstn > INT32_MAX || ndays > INT32_MAX - 64 || ntarget > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxqa_spatial_only: need nstn >= 1, ndays >= 1 and ntarget >= 1");
    if (!lon || !lat || !tmin || !tmax || !ymd || !target_idx || !flag_tmin || !flag_tmax)
        return qa_fail(errbuf, errlen, "twxqa_spatial_only: null buffer");
    QaCalendar cal;
    if (cb_cal("twxqa_spatial_only", ndays, ymd, cal, errbuf, errlen) != 0) return -1;
    const size_t nt = (size_t)ntarget, ns = (size_t)nstn, nd = (size_t)ndays;
    const int nblk = (int)((ndays + 63) / 64);
    if ((int64_t)nblk * 2 * ntarget > INT32_MAX || (2 * nstn + 2 * ntarget) * CB_NJOBS > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxqa_spatial_only: more than 2^31 - 1 work items in one call");

    // ---- 1. the regression check, as it stands (it validates the coordinates and the target list) -----------------
    float ms[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> reg(2 * nt * nd);
    if (twxqa_spatial_regress(device, nstn, ndays, lon, lat, tmin, tmax, ymd, ntarget, target_idx, reg.data(),
                              reg.data() + nt * nd, nullptr, nullptr, nullptr, nullptr, ms, errbuf, errlen) != 0)
        return -1;

    QACHK(hipSetDevice(device));
    QaBuf b_geo, b_obs, b_tgt, b_csr, b_cal, b_slot, b_rows, b_nnorm, b_tnorm, b_flag;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_geo.p, ns * 16));
    double *d_lon = static_cast<double *>(b_geo.p), *d_lat = d_lon + ns;
    QACHK(hipMemcpy(d_lon, lon, ns * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_lat, lat, ns * 8, hipMemcpyHostToDevice));
    // per target: csr offsets (int64, nt + 1), index, count
    QACHK(hipMalloc(&b_tgt.p, (nt + 1) * 8 + nt * 8));
    int64_t *d_off = static_cast<int64_t *>(b_tgt.p);
    int32_t *d_idx = (int32_t *)(d_off + nt + 1), *d_cnt = d_idx + nt;
    QACHK(hipMemcpy(d_idx, target_idx, nt * 4, hipMemcpyHostToDevice));

    // ---- 2. the radius lists in distance order: count, scan on the host, fill + sort ------------------------------
    float ms_a = 0.0f, ms_b = 0.0f;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_radius_dist, dim3((unsigned)nt), dim3(64), 0, nullptr, nstn, (const double *)d_lon,
                       (const double *)d_lat, (const int32_t *)d_idx, 0, d_cnt, (const int64_t *)nullptr, (int32_t *)nullptr,
                       (double *)nullptr);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms_a));
    std::vector<int32_t> cnt(nt), tst(nt);
    std::vector<int64_t> off(nt + 1);
    QACHK(hipMemcpy(cnt.data(), d_cnt, nt * 4, hipMemcpyDeviceToHost));
    off[0] = 0;
    for (size_t i = 0; i < nt; ++i) {                            // a list above the cap is not built: the target says so
        tst[i] = cnt[i] > TWXQA_MAX_RADIUS_NGH ? TWXQA_SP_NGH_CAP : (cnt[i] < TWXQA_MIN_NGHS ? TWXQA_SP_FEW_NGHS : TWXQA_SP_OK);
        off[i + 1] = off[i] + (tst[i] == TWXQA_SP_NGH_CAP ? 0 : cnt[i]);
    }
    QACHK(hipMemcpy(d_off, off.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
    const size_t ncsr = (size_t)off[nt];
    QACHK(hipMalloc(&b_csr.p, std::max<size_t>(16, ncsr * 12)));
    double *d_dist = static_cast<double *>(b_csr.p);
    int32_t *d_csr = (int32_t *)(d_dist + ncsr);
    if (ncsr > 0) {
        QACHK(tm.start());
        hipLaunchKernelGGL(k_radius_dist, dim3((unsigned)nt), dim3(64), 0, nullptr, nstn, (const double *)d_lon,
                           (const double *)d_lat, (const int32_t *)d_idx, 1, d_cnt, (const int64_t *)d_off, d_csr, d_dist);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms_b));
    }
    ms[2] = ms_a + ms_b;
    // the stations that are somebody's neighbour get normals: their slot in the table, -1 for the rest
    std::vector<int32_t> csr(ncsr), slot(ns, -1), rows;
    if (ncsr > 0) QACHK(hipMemcpy(csr.data(), d_csr, ncsr * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nt; ++i) {
        if (tst[i] != TWXQA_SP_OK) continue;                     // (a list shorter than 3 is never walked)
        for (int64_t k = off[i]; k < off[i + 1]; ++k) slot[(size_t)csr[(size_t)k]] = 0;
    }
    for (size_t j = 0; j < ns; ++j)
        if (slot[j] == 0) { slot[j] = (int32_t)rows.size(); rows.push_back((int32_t)j); }
    const size_t nslot = rows.size();

    // ---- 3. the normals: neighbours from the pool as it is, targets without the days the regression check removed --
    QACHK(hipMalloc(&b_obs.p, 2 * ns * nd * 4));
    float *d_tmin = static_cast<float *>(b_obs.p), *d_tmax = d_tmin + ns * nd;
    QACHK(hipMemcpy(d_tmin, tmin, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_tmax, tmax, ns * nd * 4, hipMemcpyHostToDevice));
    // calendar: years (int2), normrow (int32), month (uint8)
    const size_t cal_yr = 0, cal_row = cal_yr + cal.yr.size() * 4, cal_mth = cal_row + nd * 4;
    QACHK(hipMalloc(&b_cal.p, cal_mth + nd));
    char *dc = static_cast<char *>(b_cal.p);
    QACHK(hipMemcpy(dc + cal_yr, cal.yr.data(), cal.yr.size() * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(dc + cal_row, cal.normrow.data(), nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(dc + cal_mth, cal.month.data(), nd, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_slot.p, ns * 4));
    QACHK(hipMemcpy(b_slot.p, slot.data(), ns * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_rows.p, std::max<size_t>(4, nslot * 4)));
    if (nslot > 0) QACHK(hipMemcpy(b_rows.p, rows.data(), nslot * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_nnorm.p, std::max<size_t>(8, 2 * nslot * TWXQA_NORM_ROWS * 8)));
    double *d_nnorm = static_cast<double *>(b_nnorm.p);
    QACHK(hipMalloc(&b_tnorm.p, 2 * nt * TWXQA_NORM_ROWS * 8));   // [nt][2][731]
    double *d_tnorm = static_cast<double *>(b_tnorm.p);
    // flags: regress (2), corrob (2), final (2), each [nt][nd]
    QACHK(hipMalloc(&b_flag.p, 6 * nt * nd));
    uint8_t *d_reg = static_cast<uint8_t *>(b_flag.p), *d_cor = d_reg + 2 * nt * nd, *d_fin = d_cor + 2 * nt * nd;
    QACHK(hipMemcpy(d_reg, reg.data(), 2 * nt * nd, hipMemcpyHostToDevice));
    QACHK(hipMemset(d_cor, 0, 2 * nt * nd));
    QACHK(tm.start());
    for (int v = 0; v < 2; ++v) {
        const float *d_obs = v ? d_tmax : d_tmin;
        if (nslot > 0) {
            hipLaunchKernelGGL(k_doy_norms, dim3((unsigned)(nslot * CB_NJOBS)), dim3(256), 0, nullptr, ndays, cal.nyears,
                               (const int2 *)(dc + cal_yr), d_obs, (const int32_t *)b_rows.p, (const uint8_t *)nullptr,
                               d_nnorm + (size_t)v * nslot * TWXQA_NORM_ROWS, 1, 0);
            QACHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_doy_norms, dim3((unsigned)(nt * CB_NJOBS)), dim3(256), 0, nullptr, ndays, cal.nyears,
                           (const int2 *)(dc + cal_yr), d_obs, (const int32_t *)d_idx, (const uint8_t *)(d_reg + (size_t)v * nt * nd),
                           d_tnorm, 2, v);
        QACHK(hipGetLastError());
    }
    QACHK(tm.stop_set(&ms[3]));

    // ---- 4. the corroboration check -----------------------------------------------------------------------------
    if (norms) QACHK(hipMemcpy(norms, d_tnorm, 2 * nt * TWXQA_NORM_ROWS * 8, hipMemcpyDeviceToHost));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_corrob, dim3((unsigned)(nt * 2 * (size_t)nblk)), dim3(64), 0, nullptr, ndays, nblk,
                       (const float *)d_tmin, (const float *)d_tmax, (const int32_t *)(dc + cal_row), (const int32_t *)d_idx,
                       (const int64_t *)d_off, (const int32_t *)d_csr, (const int32_t *)b_slot.p, (int64_t)nslot,
                       (const double *)d_nnorm, (const double *)d_tnorm, (const uint8_t *)d_reg,
                       (const uint8_t *)(d_reg + nt * nd), d_cor, d_cor + nt * nd);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[4]));

    // ---- 5. mega-inconsistency and the final flag numbers --------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_mega_final, dim3((unsigned)nt), dim3(256), 0, nullptr, ndays, (const float *)d_tmin,
                       (const float *)d_tmax, (const uint8_t *)(dc + cal_mth), (const int32_t *)d_idx, (const uint8_t *)d_reg,
                       (const uint8_t *)(d_reg + nt * nd), (const uint8_t *)d_cor, (const uint8_t *)(d_cor + nt * nd), d_fin,
                       d_fin + nt * nd);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[5]));
    QACHK(hipMemcpy(flag_tmin, d_fin, nt * nd, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(flag_tmax, d_fin + nt * nd, nt * nd, hipMemcpyDeviceToHost));
    if (status) memcpy(status, tst.data(), nt * 4);
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
