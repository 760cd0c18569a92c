// twx_infillchk.hip -- libtwxqa.so: the check of step16's fits (_is_nonoptimal_infill, twx/infill/infill_daily.py:563-595,
// with hasVarChgPt of twx/infill/rpy/pca_infill.R:306-310) restated as include/twx_qa.h states it, for every item of one
// call (twxck_infill_check).  Its own translation unit; the buffer list and the event timer it shares with the other
// units are twx_qa_common.h's.
//
// An item is a fitted series and the target's observations on the same N <= TWXCK_MAX_ROWS days.  One workgroup of 256 (4
// wavefronts) per item; thread k owns the contiguous rows k c .. k c + c - 1, c = ceil(N / 256), so a prefix sum over the
// rows is an exclusive scan of 256 chunk sums plus a walk of the thread's own chunk, and nothing of length N is kept in
// LDS (the chunks are read again from global memory: 16 B a row, 128 KiB at the cap, L2 resident).
//
// Pass 1: the counts and the sums of the three means and of |fit - obs|.  Pass 2: the centred sums of r and every
// thread's chunk sum of (fit - mu)^2.  Scan: shuffle-up inside a wavefront, the four wavefront totals added in order.
// Pass 3: every thread walks its chunk in row order, forms y2[tau] from its scan offset and keeps its smallest tmp(tau)
// with the lowest tau; the workgroup arg-min compares (tmp, tau) lexicographically, so the first tau wins whatever the
// shape of the reduction.  A sum is a thread's rows in row order, the 64 lanes in a butterfly, the wavefronts in order
// through LDS; there are no float atomics, so two calls give the same bytes whatever workspace_bytes.  Every loop is
// bounded by c, by 64 or by 4; nothing waits on another workgroup.  LDS: 4 x 8 doubles.  fp64 throughout; the library is
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

#define CK_NW 4                              // wavefronts of a workgroup
#define CK_THREADS (64 * CK_NW)
#define CK_NRED 8                            // values of one workgroup reduction at most
#define CK_DBL_MAX 1.7976931348623157e308
#define CK_NO_TAU 0x7fffffff

namespace {

__device__ __forceinline__ bool ck_finite(double v) { return fabs(v) <= CK_DBL_MAX; }

// the sums of v[0 .. M - 1] over the workgroup, in every thread: butterfly in the wavefront, the wavefronts in order
template <int M>
__device__ __forceinline__ void ck_block_sum(double (&v)[M], double *lds)
{
    static_assert(M <= CK_NRED, "the reduction scratch holds CK_NRED values per wavefront");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < M; ++m) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[m] = v[m] + __shfl_xor(v[m], s, 64);
    }
    __syncthreads();                                             // the scratch of the previous reduction has been read
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) lds[w * CK_NRED + m] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double s = lds[m];
#pragma unroll
        for (int x = 1; x < CK_NW; ++x) s = s + lds[x * CK_NRED + m];
        v[m] = s;
    }
}

__device__ __forceinline__ bool ck_less(double v, int t, double bv, int bt) { return v < bv || (v == bv && t < bt); }

struct CkOut {
    int32_t *nobs, *nimpossible, *cpt_tau, *reasons, *status;
    double *mae, *r2, *cpt_stat;
};

__device__ __forceinline__ void ck_write_unfitted(const CkOut &o, int64_t i, int32_t status)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    o.nobs[i] = 0; o.nimpossible[i] = 0; o.cpt_tau[i] = 0;
    o.mae[i] = nan; o.r2[i] = nan; o.cpt_stat[i] = nan;
    o.reasons[i] = TWXCK_UNFITTED;
    o.status[i] = status;
}

}  // namespace

// b_off [nb + 1]: the rows of batch item b in fit / obs (an item above the cap has none); b_n [nb]: its N, or
// TWXCK_MAX_ROWS + 1 for an item above the cap; pen and the outputs are indexed by first_item + b
__global__ __launch_bounds__(CK_THREADS) void k_ck_check(const int64_t *__restrict__ b_off, const int32_t *__restrict__ b_n,
                                                         const double *__restrict__ fit_all,
                                                         const double *__restrict__ obs_all, const double *__restrict__ pen,
                                                         int64_t first_item, double mae_max, double r2_min, double imp_high,
                                                         double imp_low, CkOut out)
{
    __shared__ double lds[CK_NW * CK_NRED];
    const int b = blockIdx.x, k = threadIdx.x, lane = k & 63, w = k >> 6;
    const int64_t item = first_item + b;
    const int N = b_n[b];
    if (N > TWXCK_MAX_ROWS) {                                    // uniform over the workgroup
        if (k == 0) ck_write_unfitted(out, item, TWXCK_ROW_CAP);
        return;
    }
    const double *__restrict__ fit = fit_all + b_off[b];
    const double *__restrict__ obs = obs_all + b_off[b];
    const int c = (N + CK_THREADS - 1) / CK_THREADS;             // <= 32
    const int r0 = k * c;                                        // <= 255 * 32

    // pass 1: counts, the sums of the means, sum |fit - obs|
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};           // sum fit; over V: sum obs, sum fit, sum |fit - obs|, nobs;
                                                                 // nimpossible; non-finite fits (counts are exact in fp64)
    for (int j = 0; j < c; ++j) {
        const int r = r0 + j;
        if (r < N) {
            const double f = fit[r], o = obs[r];
            a[0] = a[0] + f;
            if (f > imp_high) a[5] = a[5] + 1.0;
            if (f < imp_low) a[5] = a[5] + 1.0;
            if (!ck_finite(f)) a[6] = a[6] + 1.0;
            if (ck_finite(o)) {
                a[1] = a[1] + o;
                a[2] = a[2] + f;
                a[3] = a[3] + fabs(f - o);
                a[4] = a[4] + 1.0;
            }
        }
    }
    ck_block_sum(a, lds);
    if (a[6] > 0.0) {                                            // uniform: every thread holds the same sums
        if (k == 0) ck_write_unfitted(out, item, TWXCK_NOT_FITTED);
        return;
    }
    const double nobs = a[4];
    const double mu = a[0] / (double)N, xbar = a[1] / nobs, ybar = a[2] / nobs, mae = a[3] / nobs;      // 0 / 0: NaN

    // pass 2: the centred sums over V and the thread's chunk sum of (fit - mu)^2
    double s[3] = {0.0, 0.0, 0.0};                               // ssxm, ssym, ssxym
    double q = 0.0;
    for (int j = 0; j < c; ++j) {
        const int r = r0 + j;
        if (r < N) {
            const double f = fit[r], o = obs[r];
            const double d = f - mu;
            q = q + d * d;
            if (ck_finite(o)) {
                const double dx = o - xbar, dy = f - ybar;
                s[0] = s[0] + dx * dx;
                s[1] = s[1] + dy * dy;
                s[2] = s[2] + dx * dy;
            }
        }
    }
    ck_block_sum(s, lds);
    double r2;
    if (nobs == 0.0) {
        r2 = __longlong_as_double(0x7ff8000000000000ll);
    } else if (s[0] == 0.0 || s[1] == 0.0) {
        r2 = 0.0;
    } else {
        double r = s[2] / sqrt(s[0] * s[1]);
        if (r > 1.0) r = 1.0;
        if (r < -1.0) r = -1.0;
        r2 = r * r;
    }
    int32_t reasons = 0;
    if (mae > mae_max || r2 < r2_min) reasons |= TWXCK_LOW_PERF;
    if (a[5] > 0.0) reasons |= TWXCK_IMPOSSIBLE;

    double stat = __longlong_as_double(0x7ff8000000000000ll);
    int tau_best = 0;
    if (N >= 4) {                                                // uniform
        // the exclusive scan of the 256 chunk sums
        double incl = q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double t = __shfl_up(incl, d, 64);
            if (lane >= d) incl = incl + t;
        }
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.0;
        __syncthreads();                                         // the scratch of pass 2's reduction has been read
        if (lane == 63) lds[w] = incl;
        __syncthreads();
        double base = 0.0, total = lds[0];
#pragma unroll
        for (int x = 1; x < CK_NW; ++x) {
            if (x == w) base = total;                            // ((t0 + t1) + ..) of the wavefronts before this one
            total = total + lds[x];
        }
        const double y_off = (w == 0) ? excl : base + excl;

        // pass 3: tmp(tau) over the thread's chunk
        double best = __longlong_as_double(0x7ff0000000000000ll), part = 0.0;
        int bt = CK_NO_TAU;
        for (int j = 0; j < c; ++j) {
            const int r = r0 + j;
            if (r < N) {
                const double d = fit[r] - mu;
                part = part + d * d;
                const int tau = r + 1;
                if (tau >= 2 && tau <= N - 2) {
                    const double y = y_off + part;
                    double s1 = y / (double)tau, sn = (total - y) / (double)(N - tau);
                    if (s1 <= 0.0) s1 = TWXCK_VAR_FLOOR;
                    if (sn <= 0.0) sn = TWXCK_VAR_FLOOR;
                    const double tmp = (double)tau * log(s1) + (double)(N - tau) * log(sn);
                    if (ck_less(tmp, tau, best, bt)) { best = tmp; bt = tau; }
                }
            }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const double ov = __shfl_xor(best, m, 64);
            const int ot = __shfl_xor(bt, m, 64);
            if (ck_less(ov, ot, best, bt)) { best = ov; bt = ot; }
        }
        __syncthreads();                                         // the wavefront totals have been read
        if (lane == 0) { lds[w * 2] = best; lds[w * 2 + 1] = (double)bt; }       // a tau is exact in fp64
        __syncthreads();
        best = lds[0]; bt = (int)lds[1];
#pragma unroll
        for (int x = 1; x < CK_NW; ++x) {
            const double ov = lds[x * 2];
            const int ot = (int)lds[x * 2 + 1];
            if (ck_less(ov, ot, best, bt)) { best = ov; bt = ot; }
        }
        if (bt != CK_NO_TAU) {
            const double null = (double)N * log(total / (double)N);
            stat = null - best;
            tau_best = bt;
            const double p = pen[item];
            if (p == p && stat >= p) reasons |= TWXCK_VAR_CHGPT;
        }
    }
    if (k == 0) {
        out.nobs[item] = (int32_t)nobs;
        out.nimpossible[item] = (int32_t)a[5];
        out.mae[item] = mae;
        out.r2[item] = r2;
        out.cpt_stat[item] = stat;
        out.cpt_tau[item] = tau_best;
        out.reasons[item] = reasons;
        out.status[item] = N >= 4 ? TWXCK_OK : TWXCK_FEW_ROWS;
    }
}

extern "C" int twxck_infill_check(int device, int64_t nitem, const int64_t *off, const double *fit, const double *obs,
                                  const double *pen, double mae_max, double r2_min, double impossible_high,
                                  double impossible_low, int64_t workspace_bytes, int32_t *nobs, double *mae, double *r2,
                                  int32_t *nimpossible, double *cpt_stat, int32_t *cpt_tau, int32_t *reasons,
                                  int32_t *status, int32_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxck_infill_check";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nitem < 1 || nitem > INT32_MAX / 2) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nitem <= %d", fn, INT32_MAX / 2);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!off || !pen || !nobs || !mae || !r2 || !nimpossible || !cpt_stat || !cpt_tau || !reasons || !status) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!std::isfinite(mae_max) || !std::isfinite(r2_min) || !std::isfinite(impossible_high) || !std::isfinite(impossible_low)) {
        snprintf(msg, sizeof msg, "%s: mae_max, r2_min, impossible_high and impossible_low must be finite (defaults: "
                 "TWXCK_DEFAULT_*)", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (off[0] != 0) {
        snprintf(msg, sizeof msg, "%s: off[0] = %lld, not 0", fn, (long long)off[0]);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t i = 0; i < nitem; ++i)
        if (off[i + 1] < off[i]) {
            snprintf(msg, sizeof msg, "%s: off decreases at item %lld", fn, (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
    if (off[nitem] > 0 && (!fit || !obs)) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (workspace_bytes <= 0) workspace_bytes = TWXCK_WORKSPACE_BYTES;
    const size_t NI = (size_t)nitem;

    QACHK(hipSetDevice(device));
    QaPool bufs;
    CkOut d_out;
    double *d_pen;
    QAALLOC(bufs, d_pen, double, NI);
    QAALLOC(bufs, d_out.nobs, int32_t, NI); QAALLOC(bufs, d_out.nimpossible, int32_t, NI);
    QAALLOC(bufs, d_out.cpt_tau, int32_t, NI); QAALLOC(bufs, d_out.reasons, int32_t, NI);
    QAALLOC(bufs, d_out.status, int32_t, NI);
    QAALLOC(bufs, d_out.mae, double, NI); QAALLOC(bufs, d_out.r2, double, NI); QAALLOC(bufs, d_out.cpt_stat, double, NI);
    QAUP_NZ(d_pen, pen, double, NI);
    QaTimer tm;
    float ms[TWXCK_NTIMES] = {0.0f, 0.0f, 0.0f};
    if (kernel_ms) QACHK(tm.init());
    // batches of consecutive items whose rows fit the budget (at least one item each); an item above the cap has no rows
    int nbatches = 0;
    std::vector<int64_t> boff;
    std::vector<int32_t> bn;
    std::vector<double> hfit, hobs;
    for (int64_t first = 0; first < nitem;) {
        const auto t_up = std::chrono::steady_clock::now();
        boff.assign(1, 0);
        bn.clear();
        int64_t last = first;
        for (; last < nitem; ++last) {
            const int64_t n = off[last + 1] - off[last];
            const int64_t rows = n > TWXCK_MAX_ROWS ? 0 : n;
            if (last > first && (boff.back() + rows) * 16 > workspace_bytes) break;
            boff.push_back(boff.back() + rows);
            bn.push_back(n > TWXCK_MAX_ROWS ? TWXCK_MAX_ROWS + 1 : (int32_t)n);
        }
        const size_t NB = (size_t)(last - first), NR = (size_t)boff.back();
        hfit.resize(NR);
        hobs.resize(NR);
        for (size_t b = 0; b < NB; ++b) {
            const size_t rows = (size_t)(boff[b + 1] - boff[b]);
            if (rows) {
                memcpy(hfit.data() + boff[b], fit + off[first + (int64_t)b], rows * 8);
                memcpy(hobs.data() + boff[b], obs + off[first + (int64_t)b], rows * 8);
            }
        }
        ++nbatches;
        QaPool ws;                                               // freed at the end of the batch
        int64_t *w_off;
        int32_t *w_n;
        double *w_fit, *w_obs;
        QAALLOC(ws, w_off, int64_t, NB + 1); QAALLOC(ws, w_n, int32_t, NB);
        QAALLOC(ws, w_fit, double, NR); QAALLOC(ws, w_obs, double, NR);
        QAUP_NZ(w_off, boff.data(), int64_t, NB + 1);
        QAUP_NZ(w_n, bn.data(), int32_t, NB);
        QAUP_NZ(w_fit, hfit.data(), double, NR);
        QAUP_NZ(w_obs, hobs.data(), double, NR);
        if (kernel_ms) {
            QACHK(hipDeviceSynchronize());
            ms[1] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
            QACHK(tm.start());
        }
        hipLaunchKernelGGL(k_ck_check, dim3((unsigned)NB), dim3(CK_THREADS), 0, nullptr, (const int64_t *)w_off,
                           (const int32_t *)w_n, (const double *)w_fit, (const double *)w_obs, (const double *)d_pen, first,
                           mae_max, r2_min, impossible_high, impossible_low, d_out);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        else QACHK(hipDeviceSynchronize());                      // the batch's buffers are freed next
        first = last;
    }
    const auto t_down = std::chrono::steady_clock::now();
    QACHK(hipMemcpy(nobs, d_out.nobs, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(nimpossible, d_out.nimpossible, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(cpt_tau, d_out.cpt_tau, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(reasons, d_out.reasons, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(status, d_out.status, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(mae, d_out.mae, NI * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(r2, d_out.r2, NI * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(cpt_stat, d_out.cpt_stat, NI * 8, hipMemcpyDeviceToHost));
    ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    if (counts) { counts[0] = nbatches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
