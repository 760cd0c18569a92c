// twx_outlier.hip -- libtwxqa.so: step20's leave-one-out outlier screen (XvalOutlier, twx/interp/optimize.py:84-207;
// include/twx_qa.h).  Its own translation unit and library: the kriging / daily kernels of libtwxhip are not rebuilt
// or touched, and none of their headers is included (the few device helpers needed are restated below; the host scaffold
// is twx_qa_common.h's).
//
// k_outlier_wls: one wavefront per left-out station, one 16-lane DPP row per (station, target) item, four targets at a
// time (13 targets = 4 rounds; the fourth round holds one).  The design of k_gwr_z (csrc/twx_daily.h): a lane walks
// the neighbours r = tr, tr + 16, ... and keeps the 15 sums of the lower triangle of M = X'WX and the 5 sums of
// b = X'W(y - y0) in registers; they are reduced once over the row (row_shr steps, the total of lane 15 broadcast back
// with row_newbcast: every lane of a row holds the same bits) and the 5x5 system is Cholesky-solved redundantly by every
// lane.  The neighbour list and weights of the station are loaded once per wave, into registers, for all 13 targets.
//
// Columns are shifted to the left-out station: x = [1, lst - lst0, elev - elev0, lon - lon0, lat - lat0] and
// y = norm - norm0, so the prediction at the station minus its own normal is the intercept beta_0 itself (no separate
// prediction step; the cancellation of a large intercept against large slopes does not arise).
// fp64 throughout, fused multiply-adds written out (the library is built with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define QA_SLOTS ((TWXQA_MAX_K + 15) / 16)   // neighbours per lane
// a pivot below this fraction of its column's diagonal is a column (numerically) inside the span of the previous ones:
// 1 - R^2 of that column's weighted regression on the others.  Exact rank loss rounds to ~1e-16 here (a constant
// predictor, fewer than 5 usable rows); real station predictors stay many orders above it.
#define QA_PIVOT_REL 1e-13

namespace {

// (as csrc/twx_device.h) one DPP step of a sum: lanes without a source add +0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_step(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
    return v + __hiloint2double(hi, lo);
}

// (as csrc/twx_daily.h) sum over the 16 lanes of a DPP row, returned in all of them
__device__ __forceinline__ double row16_sum(double v)
{
    v = dpp_add_step<0x111, 0xf>(v);           // row_shr:1
    v = dpp_add_step<0x112, 0xf>(v);           // row_shr:2
    v = dpp_add_step<0x114, 0xf>(v);           // row_shr:4
    v = dpp_add_step<0x118, 0xf>(v);           // row_shr:8 -> lane 15 of the row holds the row's sum
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x15f, 0xf, 0xf, false);   // row_newbcast:15
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x15f, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570e308; }

}  // namespace

__global__ __launch_bounds__(256) void k_outlier_wls(int64_t nstn, const double *__restrict__ lon,
                                                     const double *__restrict__ lat, const double *__restrict__ elev,
                                                     const double *__restrict__ lst13, const double *__restrict__ norm13,
                                                     int64_t npts, const double *__restrict__ pt, int k,
                                                     const int32_t *__restrict__ idx, const double *__restrict__ wgt,
                                                     const int32_t *__restrict__ knn_status, double *__restrict__ err,
                                                     int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63, tr = lane & 15, row = lane >> 4;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npts) return;                                   // wave-uniform: one station per wave
    double *e_out = err + p * TWXQA_NTARGET;
    int32_t *s_out = status + p * TWXQA_NTARGET;
    const int kst = knn_status[p];
    if (kst != 0) {                                          // wave-uniform
        if (lane < TWXQA_NTARGET) { e_out[lane] = __builtin_nan(""); s_out[lane] = kst; }
        return;
    }
    const double *pp = pt + p * TWXQA_PT_STRIDE;
    const double lon0 = pp[0], lat0 = pp[1], elev0 = pp[2];
    const int nslot = (k + 15) >> 4;                         // uniform

    // ---- the station's neighbours: loaded once, kept for the 13 targets ----------------------------------------
    // (the station columns themselves are gathered again per round: they come back from the caches, and holding them
    // for the four rounds would cost 60 more registers and half the resident waves)
    int32_t nj[QA_SLOTS];
    double nw[QA_SLOTS];
#pragma unroll
    for (int s = 0; s < QA_SLOTS; ++s) {
        nj[s] = -1; nw[s] = 0.0;
        const int r = tr + 16 * s;
        if (s < nslot && r < k) {
            const int32_t j = idx[p * k + r];
            if (j >= 0 && j < nstn) { nj[s] = j; nw[s] = wgt[p * k + r]; }   // (the host checked every index)
        }
    }
    const bool geo0_ok = finite_d(lon0) && finite_d(lat0) && finite_d(elev0);

    for (int t0 = 0; t0 < TWXQA_NTARGET; t0 += 4) {        // uniform
        const int t = t0 + row;
        const bool act = t < TWXQA_NTARGET;
        const double lst0 = act ? pp[3 + t] : 0.0, y0 = act ? pp[3 + TWXQA_NTARGET + t] : 0.0;
        // the station's own predictor or normal missing: patsy's predict gives NaN (err = NaN, status ok)
        const bool pt_ok = act && geo0_ok && finite_d(lst0) && finite_d(y0);
        const double *lst_t = lst13 + (size_t)(act ? t : 0) * nstn;
        const double *norm_t = norm13 + (size_t)(act ? t : 0) * nstn;

        // ---- pass over this lane's neighbours: M (lower triangle) and b ---------------------------------------
        double M[5][5], b[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            b[a] = 0.0;
#pragma unroll
            for (int c = 0; c <= a; ++c) M[a][c] = 0.0;
        }
#pragma unroll
        for (int s = 0; s < QA_SLOTS; ++s) {
            if (s < nslot && pt_ok && nj[s] >= 0) {
                const int32_t j = nj[s];
                const double xl = lst_t[j], yn = norm_t[j];
                const double x[5] = {1.0, xl - lst0, elev[j] - elev0, lon[j] - lon0, lat[j] - lat0};
                // patsy drops a row with a missing predictor or response from that fit
                if (finite_d(x[1]) && finite_d(x[2]) && finite_d(x[3]) && finite_d(x[4]) && finite_d(yn)) {
                    const double y = yn - y0;
#pragma unroll
                    for (int a = 0; a < 5; ++a) {
                        const double wx = nw[s] * x[a];
                        b[a] = fma(wx, y, b[a]);
#pragma unroll
                        for (int c = 0; c <= a; ++c) M[a][c] = fma(wx, x[c], M[a][c]);
                    }
                }
            }
        }
        // ---- one reduction per sum over the row (all 64 lanes active) --------------------------------------------
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            b[a] = row16_sum(b[a]);
#pragma unroll
            for (int c = 0; c <= a; ++c) M[a][c] = row16_sum(M[a][c]);
        }
        // ---- Cholesky M = L L' in place, then L L' beta = b; err = beta_0 -----------------------------------------
        bool singular = false;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double diag = M[i][i];
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double s = M[i][j];
#pragma unroll
                for (int q = 0; q < j; ++q) s = fma(-M[i][q], M[j][q], s);
                if (i == j) {
                    if (!(s > QA_PIVOT_REL * diag) || !finite_d(s)) { singular = true; s = 1.0; }
                    M[i][i] = sqrt(s);
                } else {
                    M[i][j] = s / M[j][j];
                }
            }
        }
        double z[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            double s = b[i];
#pragma unroll
            for (int q = 0; q < i; ++q) s = fma(-M[i][q], z[q], s);
            z[i] = s / M[i][i];
        }
#pragma unroll
        for (int i = 4; i >= 0; --i) {
            double s = z[i];
#pragma unroll
            for (int q = i + 1; q < 5; ++q) s = fma(-M[q][i], z[q], s);
            z[i] = s / M[i][i];
        }
        if (act && tr == 0) {
            if (!pt_ok) { e_out[t] = __builtin_nan(""); s_out[t] = TWXQA_OK; }
            else if (singular || !finite_d(z[0])) { e_out[t] = __builtin_nan(""); s_out[t] = TWXQA_SINGULAR; }
            else { e_out[t] = z[0]; s_out[t] = TWXQA_OK; }
        }
    }
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
extern "C" int twxqa_outlier_wls(int device, int64_t nstn, const double *lon, const double *lat, const double *elev,
                                 const double *lst13, const double *norm13, int64_t npts, const double *pt, int32_t k,
                                 const int32_t *idx, const double *wgt, const int32_t *knn_status, double *err,
                                 int32_t *status, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || npts < 1 || k < 1 || k > TWXQA_MAX_K || nstn > INT32_MAX || npts > ((int64_t)1 << 33))
        return qa_fail(errbuf, errlen, "twxqa_outlier_wls: need nstn >= 1, npts >= 1 and 1 <= k <= TWXQA_MAX_K");
    if (!lon || !lat || !elev || !lst13 || !norm13 || !pt || !idx || !wgt || !knn_status || !err || !status)
        return qa_fail(errbuf, errlen, "twxqa_outlier_wls: null buffer");
    // every neighbour index the kernel will read must lie in the pool
    for (int64_t p = 0; p < npts; ++p) {
        if (knn_status[p] != 0) continue;
        for (int32_t r = 0; r < k; ++r) {
            const int32_t j = idx[p * k + r];
            if (j < 0 || j >= nstn) {
                char msg[160];
                snprintf(msg, sizeof msg, "twxqa_outlier_wls: neighbour index %d of point %lld outside [0, %lld)", (int)j,
                         (long long)p, (long long)nstn);
                return qa_fail(errbuf, errlen, msg);
            }
        }
    }
    QACHK(hipSetDevice(device));
    const size_t n = (size_t)nstn, np = (size_t)npts, nk = np * (size_t)k;
    const size_t off_lon = 0, off_lat = off_lon + n * 8, off_elev = off_lat + n * 8, off_lst = off_elev + n * 8,
                 off_norm = off_lst + 13 * n * 8, off_pt = off_norm + 13 * n * 8, off_wgt = off_pt + np * TWXQA_PT_STRIDE * 8,
                 off_err = off_wgt + nk * 8, off_idx = off_err + np * TWXQA_NTARGET * 8, off_kst = off_idx + nk * 4,
                 off_st = off_kst + np * 4, total = off_st + np * TWXQA_NTARGET * 4;
    QaBuf buf;
    QACHK(hipMalloc(&buf.p, total));
    char *d = static_cast<char *>(buf.p);
    QACHK(hipMemcpy(d + off_lon, lon, n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_lat, lat, n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_elev, elev, n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_lst, lst13, 13 * n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_norm, norm13, 13 * n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_pt, pt, np * TWXQA_PT_STRIDE * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_wgt, wgt, nk * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_idx, idx, nk * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d + off_kst, knn_status, np * 4, hipMemcpyHostToDevice));
    QaTimer tm;
    if (kernel_ms) {
        QACHK(tm.init());
        QACHK(tm.start());
    }
    hipLaunchKernelGGL(k_outlier_wls, dim3((unsigned)((npts + 3) / 4)), dim3(256), 0, nullptr, (int64_t)nstn,
                       (const double *)(d + off_lon), (const double *)(d + off_lat), (const double *)(d + off_elev),
                       (const double *)(d + off_lst), (const double *)(d + off_norm), (int64_t)npts,
                       (const double *)(d + off_pt), (int)k, (const int32_t *)(d + off_idx),
                       (const double *)(d + off_wgt), (const int32_t *)(d + off_kst), (double *)(d + off_err),
                       (int32_t *)(d + off_st));
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_set(kernel_ms));
    QACHK(hipMemcpy(err, d + off_err, np * TWXQA_NTARGET * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(status, d + off_st, np * TWXQA_NTARGET * 4, hipMemcpyDeviceToHost));
    return 0;
}
