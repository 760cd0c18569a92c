// twx_serial.hip -- libtwxqa.so: the serially-complete station database of step18 (create_serially_complete_db,
// twx/infill/post_infill.py:106-149, with add_monthly_normals / TairAggregate.daily_to_mthly_norms) and step17's check of a
// whole series (has_bad_infill, scripts/step17_find_bad_infill_stns.py:40-68), as include/twx_qa.h states them
// (twxsc_serial_complete, twxsc_series_check).  Its own translation unit: the block sum it shares with twx_infillchk.hip
// is restated, nothing there is edited; the buffer list and the event timer are twx_qa_common.h's.
//
// A series is one station's ndays <= TWXSC_MAX_DAYS days, station-major.  One workgroup of 256 (4 wavefronts) per series.
//
// k_sc_select: thread k owns the contiguous flags k c .. k c + c - 1, c = ceil(ndays / 256), and reduces them to the run
// monoid (length, longest prefix run, longest suffix run, longest run); the 64 lanes meet in a shuffle-down tree that keeps
// the order, the four wavefronts in order through LDS.  Integer arithmetic: any tree gives the same answer.  The
// select-and-write pass follows with thread k on the days k, k + 256, ...: coalesced, 4 + 1 bytes in and out a day.
// k_sc_norms: the monthly normals of the device-resident batch; one thread per (year, month) group adds its days in day
// order, one thread per month adds its years in year order.  LDS: one double per group.
// k_sc_series: k_ck_check's "impossible" and "change point" paragraphs on a float32 series widened exactly, with the same
// order of every sum (a thread's rows in row order, the 64 lanes in a butterfly, the wavefronts in order; the prefix sums
// an exclusive scan of the 256 chunk sums plus a walk of the thread's own chunk) and no cap of 8192 rows: the chunk is
// read again from global memory (4 B a row, L2 resident), nothing of length ndays is kept in LDS or in registers.
// Every loop is bounded by c, by the days of a group, by 64 or by 4; nothing waits on another workgroup; no float atomics,
// so two calls give the same bytes whatever workspace_bytes.  fp64 throughout; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define SC_NW 4                              // wavefronts of a workgroup
#define SC_THREADS (64 * SC_NW)
#define SC_NRED 4                            // values of one workgroup reduction at most
#define SC_DBL_MAX 1.7976931348623157e308
#define SC_FLT_MAX 3.402823466e+38f
#define SC_NO_TAU 0x7fffffff
#define SC_NMONTHS 12

namespace {

// a value is missing if it is non-finite or compares equal to fill
__device__ __forceinline__ bool sc_missing(float v, float fill) { return !(fabsf(v) <= SC_FLT_MAX) || v == fill; }

struct ScRun {                                                   // the runs of ones of a stretch of bits
    int len, pre, suf, best;                                     // all ones iff pre == len
};

__device__ __forceinline__ ScRun sc_join(const ScRun &l, const ScRun &r)   // l then r
{
    ScRun o;
    o.len = l.len + r.len;
    o.pre = l.pre == l.len ? l.len + r.pre : l.pre;
    o.suf = r.suf == r.len ? r.len + l.suf : r.suf;
    const int mid = l.suf + r.pre;
    o.best = l.best > r.best ? l.best : r.best;
    if (mid > o.best) o.best = mid;
    return o;
}

// the sums of v[0 .. M - 1] over the workgroup, in every thread: butterfly in the wavefront, the wavefronts in order
template <int M>
__device__ __forceinline__ void sc_block_sum(double (&v)[M], double *lds)
{
    static_assert(M <= SC_NRED, "the reduction scratch holds SC_NRED values per wavefront");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < M; ++m) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[m] = v[m] + __shfl_xor(v[m], s, 64);
    }
    __syncthreads();                                             // the scratch of the previous reduction has been read
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) lds[w * SC_NRED + m] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double s = lds[m];
#pragma unroll
        for (int x = 1; x < SC_NW; ++x) s = s + lds[x * SC_NRED + m];
        v[m] = s;
    }
}

__device__ __forceinline__ bool sc_less(double v, int t, double bv, int bt) { return v < bv || (v == bv && t < bt); }

}  // namespace

// tair, tinf, flag, serial, flag_out: the batch's rows (tinf and flag null together: the row is tair; serial / flag_out
// null: not written); max_run, nmissing, all_infill are indexed by first + blockIdx.x
__global__ __launch_bounds__(SC_THREADS) void k_sc_select(const float *__restrict__ tair, const float *__restrict__ tinf,
                                                          const int8_t *__restrict__ flag, int ndays, int run_threshold,
                                                          float fill, float *__restrict__ serial,
                                                          int8_t *__restrict__ flag_out, int64_t first,
                                                          int32_t *__restrict__ max_run, int32_t *__restrict__ nmissing,
                                                          uint8_t *__restrict__ all_infill)
{
    __shared__ int lds[SC_NW * 4];
    const int b = blockIdx.x, k = threadIdx.x, lane = k & 63, w = k >> 6;
    const int64_t row = (int64_t)b * ndays;
    int best = 0;
    if (flag) {                                                  // uniform
        const int8_t *__restrict__ f = flag + row;
        const int c = (ndays + SC_THREADS - 1) / SC_THREADS;     // <= TWXSC_MAX_DAYS / 256
        const int r0 = k * c;                                    // < TWXSC_MAX_DAYS + 256
        ScRun a = {0, 0, 0, 0};
        int cur = 0;
        bool ones = true;
        for (int j = 0; j < c; ++j) {
            const int r = r0 + j;
            if (r < ndays) {
                const bool one = f[r] != 0;
                ++a.len;
                cur = one ? cur + 1 : 0;
                if (cur > a.best) a.best = cur;
                if (one && ones) a.pre = a.len;
                if (!one) ones = false;
            }
        }
        a.suf = cur;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {                       // lane 0 ends with lanes 0 .. 63 joined in order
            ScRun o;
            o.len = __shfl_down(a.len, s, 64); o.pre = __shfl_down(a.pre, s, 64);
            o.suf = __shfl_down(a.suf, s, 64); o.best = __shfl_down(a.best, s, 64);
            if (lane + s < 64) a = sc_join(a, o);
        }
        if (lane == 0) { lds[w * 4] = a.len; lds[w * 4 + 1] = a.pre; lds[w * 4 + 2] = a.suf; lds[w * 4 + 3] = a.best; }
        __syncthreads();
        ScRun t = {lds[0], lds[1], lds[2], lds[3]};
#pragma unroll
        for (int x = 1; x < SC_NW; ++x) {
            const ScRun o = {lds[x * 4], lds[x * 4 + 1], lds[x * 4 + 2], lds[x * 4 + 3]};
            t = sc_join(t, o);
        }
        best = t.best;
        __syncthreads();                                         // lds is used again below
    }
    const bool all = flag && best >= run_threshold;              // uniform
    const uint32_t *__restrict__ src = (const uint32_t *)((all ? tinf : tair) + row);
    const uint32_t fill_bits = __float_as_uint(fill);
    int nmiss = 0;
    for (int d = k; d < ndays; d += SC_THREADS) {
        const uint32_t bits = src[d];
        const bool miss = sc_missing(__uint_as_float(bits), fill);
        if (miss) ++nmiss;
        if (serial) ((uint32_t *)serial)[row + d] = miss ? fill_bits : bits;
        if (flag_out) flag_out[row + d] = (int8_t)((all || (flag && flag[row + d] != 0)) ? 1 : 0);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) nmiss += __shfl_xor(nmiss, s, 64);
    if (lane == 0) lds[w] = nmiss;
    __syncthreads();
    if (k == 0) {
        max_run[first + b] = best;
        nmissing[first + b] = lds[0] + lds[1] + lds[2] + lds[3];
        all_infill[first + b] = all ? 1 : 0;
    }
}

// the normals of the batch's rows: the row of series first + blockIdx.x is tinf's if all_infill says so, else tair's
__global__ __launch_bounds__(SC_THREADS) void k_sc_norms(const float *__restrict__ tair, const float *__restrict__ tinf,
                                                         const uint8_t *__restrict__ all_infill, int ndays, float fill,
                                                         int ngroups, const int32_t *__restrict__ group_first,
                                                         const int32_t *__restrict__ group_ndays, int max_miss,
                                                         int64_t first, double *__restrict__ norm,
                                                         int32_t *__restrict__ norm_nmths)
{
    __shared__ double mean[TWXSC_MAX_GROUPS];                    // NaN: the group is masked
    const int b = blockIdx.x, k = threadIdx.x;
    const int64_t s = first + b;
    const float *__restrict__ src = ((tinf && all_infill[s]) ? tinf : tair) + (int64_t)b * ndays;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int g = k; g < ngroups; g += SC_THREADS) {
        const int nd = group_ndays[g];
        double m = nan;
        if (nd > 0) {
            const int d0 = group_first[g];
            double sum = 0.0;
            int n = 0;
            for (int j = 0; j < nd; ++j) {                       // day order
                const float v = src[d0 + j];
                if (!sc_missing(v, fill)) { sum = sum + (double)v; ++n; }
            }
            if (n > 0 && !(max_miss >= 0 && nd - n > max_miss)) m = sum / (double)n;
        }
        mean[g] = m;
    }
    __syncthreads();
    if (k < SC_NMONTHS) {
        double sum = 0.0;
        int n = 0;
        for (int g = k; g < ngroups; g += SC_NMONTHS) {          // year order
            const double m = mean[g];
            if (m == m) { sum = sum + m; ++n; }
        }
        norm[s * SC_NMONTHS + k] = n > 0 ? sum / (double)n : nan;
        norm_nmths[s * SC_NMONTHS + k] = n;
    }
}

namespace {

struct ScChk {
    int32_t *nimpossible, *nmissing, *cpt_tau, *reasons, *status;
    double *cpt_stat;
};

}  // namespace

// series: the batch's rows; the outputs are indexed by first + blockIdx.x
__global__ __launch_bounds__(SC_THREADS) void k_sc_series(const float *__restrict__ series, int N, float fill, double pen,
                                                          double imp_high, double imp_low, int64_t first, ScChk out)
{
    __shared__ double lds[SC_NW * SC_NRED];
    const int b = blockIdx.x, k = threadIdx.x, lane = k & 63, w = k >> 6;
    const int64_t item = first + b;
    const float *__restrict__ fit = series + (int64_t)b * N;
    const int c = (N + SC_THREADS - 1) / SC_THREADS;             // <= TWXSC_MAX_DAYS / 256
    const int r0 = k * c;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // pass 1: the sum of the mean and the counts (exact in fp64)
    double a[3] = {0.0, 0.0, 0.0};                               // sum fit, nimpossible, nmissing
    for (int j = 0; j < c; ++j) {
        const int r = r0 + j;
        if (r < N) {
            const float v = fit[r];
            const double f = (double)v;
            a[0] = a[0] + f;
            if (f > imp_high) a[1] = a[1] + 1.0;
            if (f < imp_low) a[1] = a[1] + 1.0;
            if (sc_missing(v, fill)) a[2] = a[2] + 1.0;
        }
    }
    sc_block_sum(a, lds);
    if (a[2] > 0.0) {                                            // uniform: every thread holds the same sums
        if (k == 0) {
            out.nimpossible[item] = 0; out.nmissing[item] = (int32_t)a[2]; out.cpt_tau[item] = 0;
            out.cpt_stat[item] = nan; out.reasons[item] = TWXCK_UNFITTED; out.status[item] = TWXCK_NOT_FITTED;
        }
        return;
    }
    const double mu = a[0] / (double)N;
    int32_t reasons = 0;
    if (a[1] > 0.0) reasons |= TWXCK_IMPOSSIBLE;

    double stat = nan;
    int tau_best = 0;
    if (N >= 4) {                                                // uniform
        // pass 2: the thread's chunk sum of (fit - mu)^2, then the exclusive scan of the 256 chunk sums
        double q = 0.0;
        for (int j = 0; j < c; ++j) {
            const int r = r0 + j;
            if (r < N) {
                const double d = (double)fit[r] - mu;
                q = q + d * d;
            }
        }
        double incl = q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double t = __shfl_up(incl, d, 64);
            if (lane >= d) incl = incl + t;
        }
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.0;
        __syncthreads();                                         // the scratch of pass 1's reduction has been read
        if (lane == 63) lds[w] = incl;
        __syncthreads();
        double base = 0.0, total = lds[0];
#pragma unroll
        for (int x = 1; x < SC_NW; ++x) {
            if (x == w) base = total;                            // ((t0 + t1) + ..) of the wavefronts before this one
            total = total + lds[x];
        }
        const double y_off = (w == 0) ? excl : base + excl;

        // pass 3: tmp(tau) over the thread's chunk
        double best = __longlong_as_double(0x7ff0000000000000ll), part = 0.0;
        int bt = SC_NO_TAU;
        for (int j = 0; j < c; ++j) {
            const int r = r0 + j;
            if (r < N) {
                const double d = (double)fit[r] - mu;
                part = part + d * d;
                const int tau = r + 1;
                if (tau >= 2 && tau <= N - 2) {
                    const double y = y_off + part;
                    double s1 = y / (double)tau, sn = (total - y) / (double)(N - tau);
                    if (s1 <= 0.0) s1 = TWXCK_VAR_FLOOR;
                    if (sn <= 0.0) sn = TWXCK_VAR_FLOOR;
                    const double tmp = (double)tau * log(s1) + (double)(N - tau) * log(sn);
                    if (sc_less(tmp, tau, best, bt)) { best = tmp; bt = tau; }
                }
            }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const double ov = __shfl_xor(best, m, 64);
            const int ot = __shfl_xor(bt, m, 64);
            if (sc_less(ov, ot, best, bt)) { best = ov; bt = ot; }
        }
        __syncthreads();                                         // the wavefront totals have been read
        if (lane == 0) { lds[w * 2] = best; lds[w * 2 + 1] = (double)bt; }       // a tau is exact in fp64
        __syncthreads();
        best = lds[0]; bt = (int)lds[1];
#pragma unroll
        for (int x = 1; x < SC_NW; ++x) {
            const double ov = lds[x * 2];
            const int ot = (int)lds[x * 2 + 1];
            if (sc_less(ov, ot, best, bt)) { best = ov; bt = ot; }
        }
        if (bt != SC_NO_TAU) {
            const double null = (double)N * log(total / (double)N);
            stat = null - best;
            tau_best = bt;
            if (pen == pen && stat >= pen) reasons |= TWXCK_VAR_CHGPT;
        }
    }
    if (k == 0) {
        out.nimpossible[item] = (int32_t)a[1];
        out.nmissing[item] = 0;
        out.cpt_stat[item] = stat;
        out.cpt_tau[item] = tau_best;
        out.reasons[item] = reasons;
        out.status[item] = N >= 4 ? TWXCK_OK : TWXCK_FEW_ROWS;
    }
}

namespace {

// the series of one batch: as many as fit the budget, at least one
int64_t sc_batch(int64_t workspace_bytes, int64_t ndays, int64_t bytes_a_day)
{
    const int64_t n = workspace_bytes / (ndays * bytes_a_day);
    return n < 1 ? 1 : n;
}

}  // namespace

extern "C" int twxsc_serial_complete(int device, int64_t nseries, int64_t ndays, const float *tair,
                                     const float *tair_infilled, const int8_t *flag, int32_t run_threshold, float fill,
                                     int32_t ngroups, const int32_t *group_first, const int32_t *group_ndays,
                                     int32_t max_miss, int64_t workspace_bytes, float *serial, int8_t *flag_out,
                                     int32_t *max_run, int32_t *nmissing, uint8_t *all_infill, double *norm,
                                     int32_t *norm_nmths, int32_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxsc_serial_complete";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nseries < 1 || nseries > INT32_MAX / 2 || ndays < 1 || ndays > TWXSC_MAX_DAYS) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nseries <= %d and 1 <= ndays <= %d", fn, INT32_MAX / 2, TWXSC_MAX_DAYS);
        return qa_fail(errbuf, errlen, msg);
    }
    if ((tair_infilled == nullptr) != (flag == nullptr)) {
        snprintf(msg, sizeof msg, "%s: tair_infilled and flag must be given together or both be null", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    const bool norms = group_first != nullptr;
    if (!tair || !max_run || !nmissing || !all_infill || (flag && (!serial || !flag_out)) ||
        (norms && (!group_ndays || !norm || !norm_nmths))) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!std::isfinite(fill)) {
        snprintf(msg, sizeof msg, "%s: fill must be finite", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (norms) {
        if (ngroups < SC_NMONTHS || ngroups > TWXSC_MAX_GROUPS || ngroups % SC_NMONTHS != 0) {
            snprintf(msg, sizeof msg, "%s: ngroups must be a multiple of 12 in 12 .. %d", fn, TWXSC_MAX_GROUPS);
            return qa_fail(errbuf, errlen, msg);
        }
        int64_t end = 0;                                         // the first day after the groups so far
        for (int32_t g = 0; g < ngroups; ++g) {
            const int64_t nd = group_ndays[g], d0 = group_first[g];
            if (nd == 0) continue;
            if (nd < 0 || d0 < 0 || d0 + nd > ndays) {
                snprintf(msg, sizeof msg, "%s: group %d lies outside the day axis", fn, (int)g);
                return qa_fail(errbuf, errlen, msg);
            }
            if (d0 < end) {
                snprintf(msg, sizeof msg, "%s: group %d is not after the groups before it (ascending, disjoint)", fn, (int)g);
                return qa_fail(errbuf, errlen, msg);
            }
            end = d0 + nd;
        }
    }
    if (workspace_bytes <= 0) workspace_bytes = TWXSC_WORKSPACE_BYTES;
    const size_t NS = (size_t)nseries, ND = (size_t)ndays;
    const int64_t bytes_a_day = 4 + (flag ? 5 : 0) + (serial ? 4 : 0) + (flag_out ? 1 : 0);
    const int64_t per = sc_batch(workspace_bytes, ndays, bytes_a_day);
    const size_t NBMAX = (size_t)(per < nseries ? per : nseries);

    QACHK(hipSetDevice(device));
    QaPool bufs;
    int32_t *d_run, *d_miss, *d_nm = nullptr, *d_gf = nullptr, *d_gn = nullptr;
    uint8_t *d_all;
    double *d_norm = nullptr;
    float *w_tair, *w_tinf = nullptr, *w_serial = nullptr;
    int8_t *w_flag = nullptr, *w_fout = nullptr;
    const auto t_alloc = std::chrono::steady_clock::now();
    QAALLOC(bufs, d_run, int32_t, NS); QAALLOC(bufs, d_miss, int32_t, NS); QAALLOC(bufs, d_all, uint8_t, NS);
    if (norms) {
        QAALLOC(bufs, d_norm, double, NS * SC_NMONTHS); QAALLOC(bufs, d_nm, int32_t, NS * SC_NMONTHS);
        QAALLOC(bufs, d_gf, int32_t, ngroups); QAALLOC(bufs, d_gn, int32_t, ngroups);
        QAUP(d_gf, group_first, int32_t, ngroups);
        QAUP(d_gn, group_ndays, int32_t, ngroups);
    }
    QAALLOC(bufs, w_tair, float, NBMAX * ND);
    if (flag) { QAALLOC(bufs, w_tinf, float, NBMAX * ND); QAALLOC(bufs, w_flag, int8_t, NBMAX * ND); }
    if (serial) QAALLOC(bufs, w_serial, float, NBMAX * ND);
    if (flag_out) QAALLOC(bufs, w_fout, int8_t, NBMAX * ND);
    QaTimer tm;
    float ms[TWXSC_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) { QACHK(tm.init()); ms[2] = qa_since(t_alloc); }
    int nbatches = 0, nlaunches = 0;
    for (int64_t first = 0; first < nseries; first += per) {     // runs of series that fit the budget
        const size_t NB = (size_t)(nseries - first < per ? nseries - first : per);
        const size_t at = (size_t)first * ND;
        const auto t_up = std::chrono::steady_clock::now();
        QAUP(w_tair, tair + at, float, NB * ND);
        if (flag) { QAUP(w_tinf, tair_infilled + at, float, NB * ND); QAUP(w_flag, flag + at, int8_t, NB * ND); }
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[2] += qa_since(t_up); QACHK(tm.start()); }
        hipLaunchKernelGGL(k_sc_select, dim3((unsigned)NB), dim3(SC_THREADS), 0, nullptr, (const float *)w_tair,
                           (const float *)w_tinf, (const int8_t *)w_flag, (int)ndays, (int)run_threshold, fill, w_serial,
                           w_fout, first, d_run, d_miss, d_all);
        QACHK(hipGetLastError());
        ++nlaunches;
        if (kernel_ms) { QACHK(tm.stop_add(&ms[0])); }
        if (norms) {
            if (kernel_ms) QACHK(tm.start());
            hipLaunchKernelGGL(k_sc_norms, dim3((unsigned)NB), dim3(SC_THREADS), 0, nullptr, (const float *)w_tair,
                               (const float *)w_tinf, (const uint8_t *)d_all, (int)ndays, fill, (int)ngroups,
                               (const int32_t *)d_gf, (const int32_t *)d_gn, (int)max_miss, first, d_norm, d_nm);
            QACHK(hipGetLastError());
            ++nlaunches;
            if (kernel_ms) { QACHK(tm.stop_add(&ms[1])); }
        }
        const auto t_down = std::chrono::steady_clock::now();    // the copies wait for the launches (null stream)
        if (serial) QADOWN(serial + at, w_serial, float, NB * ND);
        if (flag_out) QADOWN(flag_out + at, w_fout, int8_t, NB * ND);
        if (!serial && !flag_out) QACHK(hipDeviceSynchronize()); // the next batch overwrites the inputs
        ms[3] += qa_since(t_down);
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(max_run, d_run, int32_t, NS);
    QADOWN(nmissing, d_miss, int32_t, NS);
    QADOWN(all_infill, d_all, uint8_t, NS);
    if (norms) { QADOWN(norm, d_norm, double, NS * SC_NMONTHS); QADOWN(norm_nmths, d_nm, int32_t, NS * SC_NMONTHS); }
    ms[3] += qa_since(t_down);
    if (counts) { counts[0] = nlaunches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxsc_series_check(int device, int64_t nseries, int64_t ndays, const float *series, float fill, double pen,
                                  double impossible_high, double impossible_low, int64_t workspace_bytes,
                                  int32_t *nimpossible, int32_t *nmissing, double *cpt_stat, int32_t *cpt_tau,
                                  int32_t *reasons, int32_t *status, int32_t *counts, float *kernel_ms, char *errbuf,
                                  int errlen)
{
    const char *fn = "twxsc_series_check";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nseries < 1 || nseries > INT32_MAX / 2 || ndays < 1 || ndays > TWXSC_MAX_DAYS) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nseries <= %d and 1 <= ndays <= %d", fn, INT32_MAX / 2, TWXSC_MAX_DAYS);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!series || !nimpossible || !nmissing || !cpt_stat || !cpt_tau || !reasons || !status) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!std::isfinite(fill) || !std::isfinite(impossible_high) || !std::isfinite(impossible_low)) {
        snprintf(msg, sizeof msg, "%s: fill, impossible_high and impossible_low must be finite", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (workspace_bytes <= 0) workspace_bytes = TWXSC_WORKSPACE_BYTES;
    const size_t NS = (size_t)nseries, ND = (size_t)ndays;
    const int64_t per = sc_batch(workspace_bytes, ndays, 4);
    const size_t NBMAX = (size_t)(per < nseries ? per : nseries);

    QACHK(hipSetDevice(device));
    QaPool bufs;
    ScChk d_out;
    float *w_series;
    const auto t_alloc = std::chrono::steady_clock::now();
    QAALLOC(bufs, d_out.nimpossible, int32_t, NS); QAALLOC(bufs, d_out.nmissing, int32_t, NS);
    QAALLOC(bufs, d_out.cpt_tau, int32_t, NS); QAALLOC(bufs, d_out.reasons, int32_t, NS);
    QAALLOC(bufs, d_out.status, int32_t, NS); QAALLOC(bufs, d_out.cpt_stat, double, NS);
    QAALLOC(bufs, w_series, float, NBMAX * ND);
    QaTimer tm;
    float ms[TWXSC_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) { QACHK(tm.init()); ms[2] = qa_since(t_alloc); }
    int nbatches = 0;
    for (int64_t first = 0; first < nseries; first += per) {
        const size_t NB = (size_t)(nseries - first < per ? nseries - first : per);
        const auto t_up = std::chrono::steady_clock::now();
        QAUP(w_series, series + (size_t)first * ND, float, NB * ND);
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[2] += qa_since(t_up); QACHK(tm.start()); }
        hipLaunchKernelGGL(k_sc_series, dim3((unsigned)NB), dim3(SC_THREADS), 0, nullptr, (const float *)w_series, (int)ndays,
                           fill, pen, impossible_high, impossible_low, first, d_out);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        else QACHK(hipDeviceSynchronize());                      // the next batch overwrites the rows
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(nimpossible, d_out.nimpossible, int32_t, NS);
    QADOWN(nmissing, d_out.nmissing, int32_t, NS);
    QADOWN(cpt_tau, d_out.cpt_tau, int32_t, NS);
    QADOWN(reasons, d_out.reasons, int32_t, NS);
    QADOWN(status, d_out.status, int32_t, NS);
    QADOWN(cpt_stat, d_out.cpt_stat, double, NS);
    ms[3] = qa_since(t_down);
    if (counts) { counts[0] = nbatches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
