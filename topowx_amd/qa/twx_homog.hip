// twx_homog.hip -- libtwxqa.so: the array work on either side of the external PHA program, as include/twx_qa.h states it:
// twxhm_obs_cnt (add_obs_cnt), twxhm_monthly_means (add_monthly_means / TairAggregate.daily_to_mthly), twxhm_tobs_shift
// (_tobs_shift_tmax) and twxhm_homog_daily (HomogDaily.homog_stn).  Its own translation unit; the buffer list and the event
// timer it shares with the other units are twx_qa_common.h's.
//
// A record is station-major, [nstn][ndays] float32 with NaN for "no value"; an entry walks it in batches of whole stations
// that fit workspace_bytes.
// k_hm_cnt, k_hm_tobs, k_hm_delta: one workgroup of 256 per station; integer counts meet in a shuffle tree and through LDS
// (integers: any tree gives the same answer).
// k_hm_means: a workgroup of 128 stages the days of 128 consecutive months of one station in LDS with 16-byte loads, then
// lane g adds month g's days from LDS in day order (fp64).
// k_hm_apply: the batch as one flat array, four days a thread, 16-byte loads and stores.
// Every loop is bounded by ndays / 256, by the 31 days of a month, by the adjustments of one station, by 64 or by 4; nothing
// waits on another workgroup; no float atomics: two calls give the same bytes whatever workspace_bytes.  The library is
// built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define HM_THREADS 256
#define HM_NW (HM_THREADS / 64)
#define HM_MM TWXHM_MTHS_PER_GROUP           // months and threads of a workgroup of k_hm_means
#define HM_STAGE (HM_MM * 31 + 8)            // floats of its LDS
#define HM_FLT_MAX 3.402823466e+38f
#define HM_NAN_BITS 0x7fc00000u
#define HM_NMONTHS 12
#define HM_NO_ADJ_BIT 1
#define HM_OVERLAP_BIT 2

namespace {

__device__ __forceinline__ bool hm_finite(float v) { return fabsf(v) <= HM_FLT_MAX; }

// the sums of v[0 .. M - 1] over the workgroup of HM_THREADS, in every thread (integers)
template <int M>
__device__ __forceinline__ void hm_block_sum(int (&v)[M], int *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < M; ++m) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[m] += __shfl_xor(v[m], s, 64);
    }
    __syncthreads();                                             // the scratch of a previous reduction has been read
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) lds[w * M + m] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
        int s = lds[m];
#pragma unroll
        for (int x = 1; x < HM_NW; ++x) s += lds[x * M + m];
        v[m] = s;
    }
}

__device__ __forceinline__ double hm_round2(double x) { return rint(x * 100.0) / 100.0; }

}  // namespace

// obs: the batch's rows; cnt is indexed by first + blockIdx.x
__global__ __launch_bounds__(HM_THREADS) void k_hm_cnt(const float *__restrict__ obs, const int8_t *__restrict__ day_month,
                                                       int ndays, int first_day, int last_day, int64_t first,
                                                       int32_t *__restrict__ cnt)
{
    __shared__ int lds[HM_NW * HM_NMONTHS];
    const int b = blockIdx.x, k = threadIdx.x;
    const float *__restrict__ row = obs + (int64_t)b * ndays;
    int c[HM_NMONTHS];
#pragma unroll
    for (int m = 0; m < HM_NMONTHS; ++m) c[m] = 0;
    for (int d = first_day + k; d <= last_day; d += HM_THREADS) {        // first_day >= 0, last_day < ndays
        const int mon = day_month[d];
        const int one = hm_finite(row[d]) ? 1 : 0;
#pragma unroll
        for (int m = 0; m < HM_NMONTHS; ++m) c[m] += (mon == m + 1) ? one : 0;
    }
    hm_block_sum(c, lds);
    if (k == 0) {
#pragma unroll
        for (int m = 0; m < HM_NMONTHS; ++m) cnt[(first + b) * HM_NMONTHS + m] = c[m];
    }
}

// obs: the batch's rows, total = its number of floats; mth_mean / mth_miss are indexed by first + blockIdx.y
__global__ __launch_bounds__(HM_MM) void k_hm_means(const float *__restrict__ obs, int64_t total, int ndays, int nmth,
                                                    const int32_t *__restrict__ mth_first,
                                                    const int32_t *__restrict__ mth_ndays, int max_miss, int64_t first,
                                                    float *__restrict__ mth_mean, int16_t *__restrict__ mth_miss)
{
    __shared__ float stage[HM_STAGE];
    const int b = blockIdx.y, k = threadIdx.x;
    const int g0 = blockIdx.x * HM_MM;                           // < nmth by the grid
    const int g1 = g0 + HM_MM < nmth ? g0 + HM_MM : nmth;
    const int d0 = mth_first[g0], d1 = mth_first[g1 - 1] + mth_ndays[g1 - 1];   // consecutive months: d1 - d0 <= 31 HM_MM
    const int64_t e0 = (int64_t)b * ndays + d0, e1 = (int64_t)b * ndays + d1;   // e1 <= total
    const int64_t es = e0 & ~(int64_t)3;                         // the 16-byte boundary at or below (the buffer is aligned)
    const int nvec = (int)((e1 - es + 3) >> 2);                  // 4 nvec <= 31 HM_MM + 3 + 3 < HM_STAGE
    for (int v = k; v < nvec; v += HM_MM) {
        const int64_t q = es + 4 * (int64_t)v;
        float4 x;
        if (q + 4 <= total) {
            x = *(const float4 *)(obs + q);
        } else {                                                 // the last, partial vector of the batch
            x.x = q < total ? obs[q] : 0.0f;
            x.y = q + 1 < total ? obs[q + 1] : 0.0f;
            x.z = q + 2 < total ? obs[q + 2] : 0.0f;
            x.w = 0.0f;
        }
        *(float4 *)(stage + 4 * v) = x;
    }
    __syncthreads();
    const int g = g0 + k;
    if (g < g1) {
        const int nd = mth_ndays[g];                             // 1 .. 31
        const float *__restrict__ p = stage + (mth_first[g] - d0) + (int)(e0 - es);
        const float v0 = p[0];
        int n = hm_finite(v0) ? 1 : 0;
        double sum = n ? (double)v0 : 0.0;
        for (int j = 1; j < nd; ++j) {                           // day order; a masked day adds +0.0 as numpy's filled(0)
            const float v = p[j];
            const bool f = hm_finite(v);
            sum = sum + (f ? (double)v : 0.0);
            n += f ? 1 : 0;
        }
        const int miss = nd - n;
        const bool masked = n == 0 || (max_miss >= 0 && miss > max_miss);
        const int64_t o = (first + b) * nmth + g;
        mth_mean[o] = masked ? __uint_as_float(HM_NAN_BITS) : (float)(sum / (double)n);
        mth_miss[o] = (int16_t)miss;
    }
}

// tmax, tobs, out: the batch's rows; nshift is indexed by first + blockIdx.x
__global__ __launch_bounds__(HM_THREADS) void k_hm_tobs(const float *__restrict__ tmax, const float *__restrict__ tobs,
                                                        int ndays, int64_t first, float *__restrict__ out,
                                                        int32_t *__restrict__ nshift)
{
    __shared__ int lds[HM_NW];
    const int b = blockIdx.x, k = threadIdx.x;
    const int64_t row = (int64_t)b * ndays;
    const float *__restrict__ tx = tmax + row;
    const float *__restrict__ to = tobs + row;
    int c[1] = {0};
    for (int d = 1 + k; d < ndays; d += HM_THREADS) {
        const float t = to[d], tp = to[d - 1];
        const bool am = t > 0.0f && t < 1100.0f;
        const bool okp = !(tp > 0.0f && tp < 1100.0f) && hm_finite(tx[d - 1]);
        c[0] += (am && !okp) ? 1 : 0;
    }
    hm_block_sum(c, lds);
    const bool shift = c[0] > 1;                                 // uniform
    for (int d = k; d < ndays; d += HM_THREADS) {
        const uint32_t bits = ((const uint32_t *)tx)[d];
        uint32_t o = bits;
        if (shift) {
            const float t = to[d];
            const bool ok = !(t > 0.0f && t < 1100.0f) && hm_finite(__uint_as_float(bits));
            o = ok ? bits : HM_NAN_BITS;
            if (!ok && d + 1 < ndays) {
                const float tn = to[d + 1];
                if (tn > 0.0f && tn < 1100.0f) o = ((const uint32_t *)tx)[d + 1];
            }
        }
        ((uint32_t *)out)[row + d] = o;
    }
    if (k == 0) nshift[first + b] = c[0];
}

// every array is the whole call's; one workgroup per station
__global__ __launch_bounds__(HM_THREADS) void k_hm_delta(int nmth, const float *__restrict__ mth_mean,
                                                         const int16_t *__restrict__ mth_miss,
                                                         const int32_t *__restrict__ pha, const int32_t *__restrict__ mth_ymd,
                                                         const int32_t *__restrict__ mth_ndays,
                                                         const int64_t *__restrict__ adj_off,
                                                         const int32_t *__restrict__ adj_start,
                                                         const int32_t *__restrict__ adj_end, const double *__restrict__ adj,
                                                         double *__restrict__ delta, int32_t *__restrict__ status,
                                                         int32_t *__restrict__ nchanged)
{
    __shared__ int lds[HM_NW * 2];
    const int64_t s = blockIdx.x;
    const int k = threadIdx.x;
    const int64_t a0 = adj_off[s], a1 = adj_off[s + 1];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int c[2] = {0, 0};                                           // the error bits, the changed months
    for (int g = k; g < nmth; g += HM_THREADS) {
        const int64_t o = s * nmth + g;
        const float mm = mth_mean[o];
        const int32_t v = pha[o];
        const bool has_m = mm == mm, has_h = v != TWXHM_PHA_MISSING;
        double dl = nan;
        if (has_m && has_h) {
            const double m = hm_round2((double)mm), h = hm_round2((double)v / 100.0);
            if (m != h) { dl = h - m; c[1] += 1; }
        } else if (has_h && (int)mth_miss[o] < mth_ndays[g]) {
            const int ymd = mth_ymd[g];
            if (a1 <= a0) {
                c[0] |= HM_NO_ADJ_BIT;
            } else if (ymd < adj_start[a0]) {
                dl = hm_round2(-adj[a0]);
            } else {
                int n = 0;
                double d = 0.0;
                for (int64_t a = a0; a < a1; ++a) {
                    if (adj_start[a] <= ymd && adj_end[a] >= ymd) { ++n; d = -adj[a]; }
                }
                if (n > 1) c[0] |= HM_OVERLAP_BIT;
                else dl = hm_round2(n == 1 ? d : 0.0);
            }
        }
        delta[o] = dl;
    }
    {                                                            // the bits: an OR in the wavefront, then across them
        const int lane = k & 63, w = k >> 6;
        int bits = c[0], cnt = c[1];
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) { bits |= __shfl_xor(bits, x, 64); cnt += __shfl_xor(cnt, x, 64); }
        if (lane == 0) { lds[w * 2] = bits; lds[w * 2 + 1] = cnt; }
        __syncthreads();                                         // also: every delta of the row has been written
        bits = 0; cnt = 0;
#pragma unroll
        for (int x = 0; x < HM_NW; ++x) { bits |= lds[x * 2]; cnt += lds[x * 2 + 1]; }
        c[0] = bits; c[1] = cnt;
    }
    if (c[0] != 0) {                                             // uniform: the row is NaN
        for (int g = k; g < nmth; g += HM_THREADS) delta[s * nmth + g] = nan;
    }
    if (k == 0) {
        status[s] = (c[0] & HM_OVERLAP_BIT) ? TWXHM_OVERLAP : (c[0] & HM_NO_ADJ_BIT) ? TWXHM_NO_ADJ : TWXHM_OK;
        nchanged[s] = c[0] != 0 ? 0 : c[1];
    }
}

namespace {

// one day of k_hm_apply: the flat index e < total of the batch, its station and day
__device__ __forceinline__ uint32_t hm_apply_one(uint32_t bits, int st, int d, int64_t first, int nmth,
                                                 const int32_t *__restrict__ day_mth, const double *__restrict__ delta,
                                                 const int32_t *__restrict__ status)
{
    if (status[first + st] != TWXHM_OK) return HM_NAN_BITS;
    const int g = day_mth[d];
    if (g < 0) return bits;
    const double dl = delta[(first + st) * nmth + g];
    if (!(dl == dl)) return bits;                                // untouched
    return __float_as_uint((float)((double)__uint_as_float(bits) + dl));
}

}  // namespace

// obs, out: the batch's rows as one flat array of total < 2^31 floats; delta and status are the whole call's
__global__ __launch_bounds__(HM_THREADS) void k_hm_apply(const float *__restrict__ obs, int total, int ndays, int nmth,
                                                         const int32_t *__restrict__ day_mth,
                                                         const double *__restrict__ delta,
                                                         const int32_t *__restrict__ status, int64_t first,
                                                         float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    const int64_t e64 = 4 * t;
    if (e64 >= total) return;
    const int e = (int)e64;
    int st = e / ndays, d = e - st * ndays;
    if (e + 4 <= total) {
        const uint4 x = *(const uint4 *)(obs + e);
        uint4 y;
        y.x = hm_apply_one(x.x, st, d, first, nmth, day_mth, delta, status);
        if (++d == ndays) { d = 0; ++st; }
        y.y = hm_apply_one(x.y, st, d, first, nmth, day_mth, delta, status);
        if (++d == ndays) { d = 0; ++st; }
        y.z = hm_apply_one(x.z, st, d, first, nmth, day_mth, delta, status);
        if (++d == ndays) { d = 0; ++st; }
        y.w = hm_apply_one(x.w, st, d, first, nmth, day_mth, delta, status);
        *(uint4 *)(out + e) = y;
    } else {                                                     // the scalar tail of the batch: at most 3 days
        for (int i = e; i < total; ++i) {
            ((uint32_t *)out)[i] = hm_apply_one(((const uint32_t *)obs)[i], st, d, first, nmth, day_mth, delta, status);
            if (++d == ndays) { d = 0; ++st; }
        }
    }
}

namespace {

// the stations of one batch: as many as fit the budget, at least one, fewer than 2^31 floats
int64_t hm_batch(int64_t workspace_bytes, int64_t ndays, int64_t bytes_a_day)
{
    if (workspace_bytes <= 0) workspace_bytes = TWXSC_WORKSPACE_BYTES;
    int64_t n = workspace_bytes / (ndays * bytes_a_day);
    const int64_t cap = (int64_t)(INT32_MAX - 4) / ndays;
    if (n > cap) n = cap;
    return n < 1 ? 1 : n;
}

// the shape checks every entry shares; 0 if fine
int hm_shape(const char *fn, int64_t nstn, int64_t ndays, char *errbuf, int errlen)
{
    char msg[256];
    if (nstn < 1 || nstn > INT32_MAX / 2 || ndays < 1 || ndays > TWXSC_MAX_DAYS) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nstn <= %d and 1 <= ndays <= %d", fn, INT32_MAX / 2, TWXSC_MAX_DAYS);
        return qa_fail(errbuf, errlen, msg);
    }
    return 0;
}

// the month list: consecutive runs of 1 .. 31 days inside the axis; 0 if fine
int hm_months(const char *fn, int64_t ndays, int32_t nmth, const int32_t *mth_first, const int32_t *mth_ndays, char *errbuf,
              int errlen)
{
    char msg[256];
    if (nmth < 1 || nmth > TWXHM_MAX_MONTHS) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nmth <= %d", fn, TWXHM_MAX_MONTHS);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int32_t g = 0; g < nmth; ++g) {
        const int64_t d0 = mth_first[g], nd = mth_ndays[g];
        if (nd < 1 || nd > 31 || d0 < 0 || d0 + nd > ndays) {
            snprintf(msg, sizeof msg, "%s: month %d lies outside the day axis or has not 1 .. 31 days", fn, (int)g);
            return qa_fail(errbuf, errlen, msg);
        }
        if (g > 0 && d0 != (int64_t)mth_first[g - 1] + mth_ndays[g - 1]) {
            snprintf(msg, sizeof msg, "%s: month %d does not start where month %d ends", fn, (int)g, (int)g - 1);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    return 0;
}

}  // namespace

extern "C" int twxhm_obs_cnt(int device, int64_t nstn, int64_t ndays, const float *obs, const int8_t *day_month,
                             int64_t first_day, int64_t last_day, int64_t workspace_bytes, int32_t *cnt, int32_t *counts,
                             float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxhm_obs_cnt";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (hm_shape(fn, nstn, ndays, errbuf, errlen)) return -1;
    if (!obs || !day_month || !cnt) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (first_day < 0 || last_day >= ndays || first_day > last_day) {
        snprintf(msg, sizeof msg, "%s: need 0 <= first_day <= last_day < ndays", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t d = 0; d < ndays; ++d) {
        if (day_month[d] < 1 || day_month[d] > HM_NMONTHS) {
            snprintf(msg, sizeof msg, "%s: day_month[%lld] is outside 1 .. 12", fn, (long long)d);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const size_t NS = (size_t)nstn, ND = (size_t)ndays;
    const int64_t per = hm_batch(workspace_bytes, ndays, 4);
    const size_t NBMAX = (size_t)(per < nstn ? per : nstn);

    QACHK(hipSetDevice(device));
    QaPool bufs;
    float *w_obs;
    int8_t *d_mon;
    int32_t *d_cnt;
    const auto t_alloc = std::chrono::steady_clock::now();
    QAALLOC(bufs, w_obs, float, NBMAX * ND); QAALLOC(bufs, d_mon, int8_t, ND); QAALLOC(bufs, d_cnt, int32_t, NS * HM_NMONTHS);
    QAUP(d_mon, day_month, int8_t, ND);
    QaTimer tm;
    float ms[TWXHM_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) { QACHK(tm.init()); ms[2] = qa_since(t_alloc); }
    int nbatches = 0;
    for (int64_t first = 0; first < nstn; first += per) {
        const size_t NB = (size_t)(nstn - first < per ? nstn - first : per);
        const auto t_up = std::chrono::steady_clock::now();
        QAUP(w_obs, obs + (size_t)first * ND, float, NB * ND);
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[2] += qa_since(t_up); QACHK(tm.start()); }
        hipLaunchKernelGGL(k_hm_cnt, dim3((unsigned)NB), dim3(HM_THREADS), 0, nullptr, (const float *)w_obs,
                           (const int8_t *)d_mon, (int)ndays, (int)first_day, (int)last_day, first, d_cnt);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        else QACHK(hipDeviceSynchronize());                      // the next batch overwrites the rows
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(cnt, d_cnt, int32_t, NS * HM_NMONTHS);
    ms[3] = qa_since(t_down);
    if (counts) { counts[0] = nbatches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxhm_monthly_means(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t nmth,
                                   const int32_t *mth_first, const int32_t *mth_ndays, int32_t max_miss,
                                   int64_t workspace_bytes, float *mth_mean, int16_t *mth_miss, int32_t *counts,
                                   float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxhm_monthly_means";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (hm_shape(fn, nstn, ndays, errbuf, errlen)) return -1;
    if (!obs || !mth_first || !mth_ndays || !mth_mean || !mth_miss) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (hm_months(fn, ndays, nmth, mth_first, mth_ndays, errbuf, errlen)) return -1;
    const size_t NS = (size_t)nstn, ND = (size_t)ndays, NM = (size_t)nmth;
    int64_t per = hm_batch(workspace_bytes, ndays, 4);
    if (per > 65535) per = 65535;                                // the grid's y extent
    const size_t NBMAX = (size_t)(per < nstn ? per : nstn);
    const unsigned ngrp = (unsigned)((nmth + HM_MM - 1) / HM_MM);

    QACHK(hipSetDevice(device));
    QaPool bufs;
    float *w_obs, *d_mean;
    int16_t *d_miss;
    int32_t *d_mf, *d_mn;
    const auto t_alloc = std::chrono::steady_clock::now();
    QAALLOC(bufs, w_obs, float, NBMAX * ND); QAALLOC(bufs, d_mean, float, NS * NM); QAALLOC(bufs, d_miss, int16_t, NS * NM);
    QAALLOC(bufs, d_mf, int32_t, NM); QAALLOC(bufs, d_mn, int32_t, NM);
    QAUP(d_mf, mth_first, int32_t, NM);
    QAUP(d_mn, mth_ndays, int32_t, NM);
    QaTimer tm;
    float ms[TWXHM_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) { QACHK(tm.init()); ms[2] = qa_since(t_alloc); }
    int nbatches = 0;
    for (int64_t first = 0; first < nstn; first += per) {
        const size_t NB = (size_t)(nstn - first < per ? nstn - first : per);
        const auto t_up = std::chrono::steady_clock::now();
        QAUP(w_obs, obs + (size_t)first * ND, float, NB * ND);
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[2] += qa_since(t_up); QACHK(tm.start()); }
        hipLaunchKernelGGL(k_hm_means, dim3(ngrp, (unsigned)NB), dim3(HM_MM), 0, nullptr, (const float *)w_obs,
                           (int64_t)(NB * ND), (int)ndays, (int)nmth, (const int32_t *)d_mf, (const int32_t *)d_mn,
                           (int)max_miss, first, d_mean, d_miss);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        else QACHK(hipDeviceSynchronize());                      // the next batch overwrites the rows
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(mth_mean, d_mean, float, NS * NM);
    QADOWN(mth_miss, d_miss, int16_t, NS * NM);
    ms[3] = qa_since(t_down);
    if (counts) { counts[0] = nbatches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxhm_tobs_shift(int device, int64_t nstn, int64_t ndays, const float *tmax, const float *tobs,
                                int64_t workspace_bytes, float *out, int32_t *nshift, int32_t *counts, float *kernel_ms,
                                char *errbuf, int errlen)
{
    const char *fn = "twxhm_tobs_shift";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (hm_shape(fn, nstn, ndays, errbuf, errlen)) return -1;
    if (!tmax || !tobs || !out || !nshift) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    const size_t NS = (size_t)nstn, ND = (size_t)ndays;
    const int64_t per = hm_batch(workspace_bytes, ndays, 12);
    const size_t NBMAX = (size_t)(per < nstn ? per : nstn);

    QACHK(hipSetDevice(device));
    QaPool bufs;
    float *w_tmax, *w_tobs, *w_out;
    int32_t *d_ns;
    const auto t_alloc = std::chrono::steady_clock::now();
    QAALLOC(bufs, w_tmax, float, NBMAX * ND); QAALLOC(bufs, w_tobs, float, NBMAX * ND); QAALLOC(bufs, w_out, float, NBMAX * ND);
    QAALLOC(bufs, d_ns, int32_t, NS);
    QaTimer tm;
    float ms[TWXHM_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) { QACHK(tm.init()); ms[2] = qa_since(t_alloc); }
    int nbatches = 0;
    for (int64_t first = 0; first < nstn; first += per) {
        const size_t NB = (size_t)(nstn - first < per ? nstn - first : per);
        const size_t at = (size_t)first * ND;
        const auto t_up = std::chrono::steady_clock::now();
        QAUP(w_tmax, tmax + at, float, NB * ND);
        QAUP(w_tobs, tobs + at, float, NB * ND);
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[2] += qa_since(t_up); QACHK(tm.start()); }
        hipLaunchKernelGGL(k_hm_tobs, dim3((unsigned)NB), dim3(HM_THREADS), 0, nullptr, (const float *)w_tmax,
                           (const float *)w_tobs, (int)ndays, first, w_out, d_ns);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        const auto t_down = std::chrono::steady_clock::now();    // the copy waits for the launch (null stream)
        QADOWN(out + at, w_out, float, NB * ND);
        ms[3] += qa_since(t_down);
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(nshift, d_ns, int32_t, NS);
    ms[3] += qa_since(t_down);
    if (counts) { counts[0] = nbatches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxhm_homog_daily(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t nmth,
                                 const float *mth_mean, const int16_t *mth_miss, const int32_t *pha, const int32_t *mth_ymd,
                                 const int32_t *mth_first, const int32_t *mth_ndays, const int64_t *adj_off,
                                 const int32_t *adj_ymd_start, const int32_t *adj_ymd_end, const double *adj,
                                 int64_t workspace_bytes, double *delta, float *out, int32_t *status, int32_t *nchanged,
                                 int32_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxhm_homog_daily";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (hm_shape(fn, nstn, ndays, errbuf, errlen)) return -1;
    if (!obs || !mth_mean || !mth_miss || !pha || !mth_ymd || !mth_first || !mth_ndays || !adj_off || !delta || !out ||
        !status || !nchanged) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (hm_months(fn, ndays, nmth, mth_first, mth_ndays, errbuf, errlen)) return -1;
    if (adj_off[0] != 0) {
        snprintf(msg, sizeof msg, "%s: adj_off must start at 0", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t s = 0; s < nstn; ++s) {
        if (adj_off[s + 1] < adj_off[s]) {
            snprintf(msg, sizeof msg, "%s: adj_off must ascend (station %lld)", fn, (long long)s);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const int64_t nadj = adj_off[nstn];
    if (nadj > 0 && (!adj_ymd_start || !adj_ymd_end || !adj)) {
        snprintf(msg, sizeof msg, "%s: null adjustment list", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t s = 0; s < nstn; ++s) {
        for (int64_t a = adj_off[s] + 1; a < adj_off[s + 1]; ++a) {
            if (adj_ymd_start[a] < adj_ymd_start[a - 1]) {
                snprintf(msg, sizeof msg, "%s: the adjustments of station %lld are not sorted by ymd_start", fn, (long long)s);
                return qa_fail(errbuf, errlen, msg);
            }
        }
    }
    const size_t NS = (size_t)nstn, ND = (size_t)ndays, NM = (size_t)nmth, NA = (size_t)nadj;
    const int64_t per = hm_batch(workspace_bytes, ndays, 8);
    const size_t NBMAX = (size_t)(per < nstn ? per : nstn);
    std::vector<int32_t> day_mth(ND, -1);                        // a day's month, -1: none
    for (int32_t g = 0; g < nmth; ++g)
        for (int32_t j = 0; j < mth_ndays[g]; ++j) day_mth[(size_t)mth_first[g] + j] = g;

    QACHK(hipSetDevice(device));
    QaPool bufs;
    float *w_obs, *w_out, *d_mean;
    int16_t *d_miss;
    int32_t *d_pha, *d_ymd, *d_mn, *d_dm, *d_as, *d_ae, *d_status, *d_nch;
    int64_t *d_off;
    double *d_adj, *d_delta;
    const auto t_alloc = std::chrono::steady_clock::now();
    QAALLOC(bufs, w_obs, float, NBMAX * ND); QAALLOC(bufs, w_out, float, NBMAX * ND);
    QAALLOC(bufs, d_mean, float, NS * NM); QAALLOC(bufs, d_miss, int16_t, NS * NM); QAALLOC(bufs, d_pha, int32_t, NS * NM);
    QAALLOC(bufs, d_ymd, int32_t, NM); QAALLOC(bufs, d_mn, int32_t, NM); QAALLOC(bufs, d_dm, int32_t, ND);
    QAALLOC(bufs, d_off, int64_t, NS + 1); QAALLOC(bufs, d_as, int32_t, NA); QAALLOC(bufs, d_ae, int32_t, NA);
    QAALLOC(bufs, d_adj, double, NA); QAALLOC(bufs, d_delta, double, NS * NM);
    QAALLOC(bufs, d_status, int32_t, NS); QAALLOC(bufs, d_nch, int32_t, NS);
    QAUP(d_mean, mth_mean, float, NS * NM); QAUP(d_miss, mth_miss, int16_t, NS * NM); QAUP(d_pha, pha, int32_t, NS * NM);
    QAUP(d_ymd, mth_ymd, int32_t, NM); QAUP(d_mn, mth_ndays, int32_t, NM); QAUP(d_dm, day_mth.data(), int32_t, ND);
    QAUP(d_off, adj_off, int64_t, NS + 1);
    if (NA) { QAUP(d_as, adj_ymd_start, int32_t, NA); QAUP(d_ae, adj_ymd_end, int32_t, NA); QAUP(d_adj, adj, double, NA); }
    QaTimer tm;
    float ms[TWXHM_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) { QACHK(tm.init()); QACHK(hipDeviceSynchronize()); ms[2] = qa_since(t_alloc); QACHK(tm.start()); }
    hipLaunchKernelGGL(k_hm_delta, dim3((unsigned)NS), dim3(HM_THREADS), 0, nullptr, (int)nmth, (const float *)d_mean,
                       (const int16_t *)d_miss, (const int32_t *)d_pha, (const int32_t *)d_ymd, (const int32_t *)d_mn,
                       (const int64_t *)d_off, (const int32_t *)d_as, (const int32_t *)d_ae, (const double *)d_adj, d_delta,
                       d_status, d_nch);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
    int nbatches = 0;
    for (int64_t first = 0; first < nstn; first += per) {
        const size_t NB = (size_t)(nstn - first < per ? nstn - first : per);
        const size_t at = (size_t)first * ND;
        const int total = (int)(NB * ND);                        // < 2^31 by hm_batch
        const auto t_up = std::chrono::steady_clock::now();
        QAUP(w_obs, obs + at, float, NB * ND);
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[2] += qa_since(t_up); QACHK(tm.start()); }
        const unsigned nblk = (unsigned)(((int64_t)total + 4 * HM_THREADS - 1) / (4 * HM_THREADS));
        hipLaunchKernelGGL(k_hm_apply, dim3(nblk), dim3(HM_THREADS), 0, nullptr, (const float *)w_obs, total, (int)ndays,
                           (int)nmth, (const int32_t *)d_dm, (const double *)d_delta, (const int32_t *)d_status, first, w_out);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[1]));
        const auto t_down = std::chrono::steady_clock::now();    // the copy waits for the launch (null stream)
        QADOWN(out + at, w_out, float, NB * ND);
        ms[3] += qa_since(t_down);
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(delta, d_delta, double, NS * NM);
    QADOWN(status, d_status, int32_t, NS);
    QADOWN(nchanged, d_nch, int32_t, NS);
    ms[3] += qa_since(t_down);
    if (counts) { counts[0] = nbatches + 1; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
