// twx_ppca.hip -- libtwxqa.so: the estimator of step16 (twx/infill/rpy/pca_infill.R: pcaMethods' pca(method = 'ppca'), EM
// for probabilistic PCA with missing values) restated as include/twx_qa.h states it, for every item of one call
// (twxpp_ppca_fit).  Its own translation unit: the column gather it shares with twx_emnorm.hip is restated, nothing
// there is edited; the wave sum, the buffer list and the event timer are twx_qa_common.h's.
//
// An item is a matrix of N <= TWXPP_MAX_ROWS days by D <= TWXPP_MAX_COLS columns (the target, its station columns as
// float32 rows of the station-major observations, the float64 columns of one optional extra set), standardised with the
// item's norms / stds, and a number of components d <= TWXPP_MAX_PCS.  One workgroup of 256 (4 wavefronts) per item.
//
// Layout.  Lane j of a wavefront owns column j of the row the wavefront works on; rows are dealt to the wavefronts
// (row r to wavefront r % 4).  A row is gathered, standardised, centred with M; a hidden entry is refilled as the dot
// product of the row's previous X (global workspace, two buffers of N x d) and the previous C (LDS).  No filled copy of Y
// is stored.  Ye C is formed by lane (k, h): h sums the columns 32 h .. 32 h + 31 in ascending order and the two halves are
// added; lane j keeps row j of the partial Ye'X in 32 registers, lane (k, h) the entries (h + 2 t, k) of the partial X'X in
// 16.  The partial sums go to LDS in wavefront order ((w0 + w1) + w2) + w3; there are no float atomics, so two calls give
// the same bytes whatever iters_per_launch and workspace_bytes.  The d x d inverses (Gauss-Jordan without pivoting), the
// orthonormalisation (modified Gram-Schmidt, twice) and the eigen-problem (cyclic Jacobi, fixed sweep order, at most
// PP_SWEEPS sweeps) are done by wavefront 0 in LDS.  sum (C X' - Ye')^2 takes a second pass over the rows with the new C:
// the expanded form would cancel.  Every loop is bounded by a row, column, component, sweep or iteration count; nothing
// waits on another workgroup.
//
// k_pp_prep: M, the count of missing values, the set-up X and ss.  k_pp_iter: up to iters_per_launch iterations of the
// unfinished items, and for an item that stops the whole post-processing (basis, eigen-problem, scores, R2cum, fit).
//
// LDS of k_pp_iter: C and Ye'X / the new C 2 x 16.5 KiB, S, Sx, CtC and the inverse scratch 4 x 8 KiB, per wavefront one
// row (512 B) and three d-vectors (768 B) 5 KiB, reduction scratch 1.1 KiB: 71.3 KiB, two workgroups fit a compute unit's
// 160 KiB.  fp64 throughout; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define PP_D TWXPP_MAX_COLS                  // 64: one lane per column
#define PP_K TWXPP_MAX_PCS                   // 32: the stride of every d-indexed array
#define PP_NW 4                              // wavefronts of a workgroup
#define PP_THREADS (64 * PP_NW)
#define PP_SWEEPS 30                         // Jacobi sweeps at most
#define PP_DBL_MAX 1.7976931348623157e308
#define PP_CS (PP_K + 1)                     // the row stride of C in LDS and in the workspace: lane j walks row j, and a
                                             // stride of 32 doubles would put every lane on one bank
#define PP_WS_C (PP_D * PP_CS)               // doubles of C in the per-item workspace
#define PP_WS_FIXED (PP_WS_C + PP_D + 4)     // C, M, then ss / old / missing

static_assert(PP_D == 64 && PP_K == 32, "the lane layout assumes 64 columns and 32 components");

namespace {

__device__ __forceinline__ bool pp_finite(double v) { return fabs(v) <= PP_DBL_MAX; }

// orders the LDS traffic of the lanes of one wavefront
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct PpIn {
    const float *obs;            // [nstn][ndays]
    int64_t ndays;
    const int32_t *gdays;        // the used days sorted by group
    const int32_t *goff;         // [ngroups + 1]
    const int32_t *item_target, *item_group, *item_set, *item_npcs;
    const int64_t *col_off;
    const int32_t *col_idx;
    const int32_t *set_ncol;
    const int64_t *set_off;
    const double *set_vals;
    const int64_t *par_off;      // [nitem + 1]: the item's columns in norms / stds
    const double *norms, *stds;
    const int64_t *c0_off;       // [nitem + 1]
    const double *c0;            // per item [d][D]: column-major [D, d]
};

struct PpCol {                   // column c (0 = target) of an item, as lane c sees it
    const float *pf;             // station row, or nullptr
    const double *pd;            // extra column, or nullptr
    double norm, sd;
};

__device__ __forceinline__ int pp_ncols(const PpIn &in, int item, int *nst)
{
    *nst = (int)(in.col_off[item + 1] - in.col_off[item]);
    const int s = in.item_set[item];
    return 1 + *nst + (s >= 0 ? in.set_ncol[s] : 0);
}

__device__ __forceinline__ PpCol pp_column(const PpIn &in, int item, int c, int nst, int D)
{
    PpCol col = {nullptr, nullptr, 0.0, 1.0};
    if (c >= D) return col;
    if (c == 0) col.pf = in.obs + (int64_t)in.item_target[item] * in.ndays;
    else if (c <= nst) col.pf = in.obs + (int64_t)in.col_idx[in.col_off[item] + c - 1] * in.ndays;
    else {
        const int s = in.item_set[item], g = in.item_group[item];
        const int64_t nrows = in.goff[g + 1] - in.goff[g];
        col.pd = in.set_vals + in.set_off[s] + (int64_t)(c - 1 - nst) * nrows;
    }
    col.norm = in.norms[in.par_off[item] + c];
    col.sd = in.stds[in.par_off[item] + c];
    return col;
}

// the standardised value of the column on row r of the item (NaN: not a column)
__device__ __forceinline__ double pp_value(const PpCol &col, const int32_t *days, int r)
{
    const double v = col.pf ? (double)col.pf[days[r]] : (col.pd ? col.pd[r] : NAN);
    return (v - col.norm) / col.sd;
}

// Ye of row r for lane j: y - M where observed, else the refill from the row's previous X (xo, in LDS) and the previous C,
// or 0 when xo is null (the set-up).  *o: observed.
__device__ __forceinline__ double pp_row(const PpCol &col, double M, const int32_t *days, int r, int j, int D, int d,
                                         const double *C, const double *xo, bool *o)
{
    const double y = pp_value(col, days, r);
    *o = j < D && pp_finite(y);
    if (*o) return y - M;
    double acc = 0.0;
    if (j < D && xo)
        for (int k = 0; k < d; ++k) acc = acc + xo[k] * C[j * PP_CS + k];
    return acc;
}

// (ye C)_k for lane (k = lane & 31, h = lane >> 5), both halves return the sum; ye [64] in LDS
__device__ __forceinline__ double pp_project(const double *C, const double *ye, int D, int lane)
{
    const int k = lane & 31, h = lane >> 5;
    const int j1 = min(D, 32 * h + 32);
    double part = 0.0;
    for (int j = 32 * h; j < j1; ++j) part = part + ye[j] * C[j * PP_CS + k];
    const double other = __shfl_xor(part, 32, 64);
    return h == 0 ? part + other : other + part;
}

// W [d][d] (stride 32) <- its inverse, in place, by one wavefront: Gauss-Jordan without pivoting, the pivot row divided by
// the pivot.  *logpiv: the sum of the logs of the pivots.  Returns true if a pivot is <= 0 or not finite.
__device__ __forceinline__ bool pp_invert(double *W, int d, int lane, double *logpiv)
{
    const int c = lane & 31, h = lane >> 5;
    double lp = 0.0;
    bool bad = false;
    for (int p = 0; p < d; ++p) {
        const double piv = W[p * PP_K + p];
        if (!(piv > 0.0) || !pp_finite(piv)) { bad = true; break; }
        lp = lp + log(piv);
        const double prow = c < d ? W[p * PP_K + c] : 0.0;
        double f[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) f[t] = h + 2 * t < d ? W[(h + 2 * t) * PP_K + p] : 0.0;
        wave_sync();
        const double rowc = c == p ? 1.0 / piv : prow / piv;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int i = h + 2 * t;
            if (i < d && c < d) {
                double v;
                if (i == p) v = rowc;
                else if (c == p) v = -f[t] / piv;
                else v = W[i * PP_K + c] - f[t] * rowc;
                W[i * PP_K + c] = v;
            }
        }
        wave_sync();
    }
    *logpiv = lp;
    return bad;
}

// sum over the d x d entries of A o B (B may be null: the sum of A's diagonal), every wavefront for itself
__device__ __forceinline__ double pp_dot_dd(const double *A, const double *B, int d, int lane)
{
    double acc = 0.0;
    for (int e = lane; e < PP_K * PP_K; e += 64) {
        const int i = e >> 5, c = e & 31;
        if (i < d && c < d) {
            if (B) acc = acc + A[e] * B[e];
            else if (i == c) acc = acc + A[e];
        }
    }
    return qa_wave_sum(acc);
}

// CtC = C'C over the rows j < D, by the workgroup
__device__ __forceinline__ void pp_ctc(const double *C, double *CtC, int D, int d, int tid)
{
    for (int e = tid; e < PP_K * PP_K; e += PP_THREADS) {
        const int k = e >> 5, l = e & 31;
        double acc = 0.0;
        if (k < d && l < d)
            for (int j = 0; j < D; ++j) acc = acc + C[j * PP_CS + k] * C[j * PP_CS + l];
        CtC[e] = acc;
    }
}

// the partial sums of the wavefronts into dst, in wavefront order; acc[t] belongs to entry idx(t) (or -1)
#define PP_COMBINE(dst, count, idx_expr, acc)                                   \
    for (int w_ = 0; w_ < PP_NW; ++w_) {                                        \
        if (wave == w_) {                                                       \
            _Pragma("unroll") for (int t = 0; t < (count); ++t) {               \
                const int ix_ = (idx_expr);                                     \
                if (ix_ >= 0) (dst)[ix_] = w_ == 0 ? (acc)[t] : (dst)[ix_] + (acc)[t]; \
            }                                                                   \
        }                                                                       \
        __syncthreads();                                                        \
    }

}  // namespace

__global__ __launch_bounds__(PP_THREADS) void k_pp_prep(PpIn in, int first_item, const int64_t *__restrict__ ws_xoff,
                                                        double *__restrict__ ws_fixed, double *__restrict__ ws_x,
                                                        uint8_t *__restrict__ done, int32_t *__restrict__ status)
{
    __shared__ double sC[PP_WS_C];
    __shared__ double sW[PP_K * PP_K];
    __shared__ double wYe[PP_NW][PP_D], wT[PP_NW][PP_K], wX[PP_NW][PP_K];
    __shared__ double sM[PP_D], sCnt[PP_D], sRed[PP_NW];
    __shared__ int s_bad;
    const int slot = blockIdx.x, item = first_item + slot;
    if (done[item]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = in.item_group[item];
    const int32_t *days = in.gdays + in.goff[g];
    const int N = in.goff[g + 1] - in.goff[g];
    int nst;
    const int D = pp_ncols(in, item, &nst);
    const int d = in.item_npcs[item];
    if (tid == 0) s_bad = 0;
    // column means over the observed values
    for (int c = wave; c < D; c += PP_NW) {
        const PpCol col = pp_column(in, item, c, nst, D);
        double cnt = 0.0, s1 = 0.0;
        for (int r = lane; r < N; r += 64) {
            const double y = pp_value(col, days, r);
            if (pp_finite(y)) { cnt = cnt + 1.0; s1 = s1 + y; }
        }
        cnt = qa_wave_sum(cnt); s1 = qa_wave_sum(s1);
        if (lane == 0) { sCnt[c] = cnt; sM[c] = s1 / cnt; }
    }
    __syncthreads();
    double nobs = 0.0;
    bool empty = false;
    for (int c = 0; c < D; ++c) { empty = empty || sCnt[c] == 0.0; nobs = nobs + sCnt[c]; }
    if (empty) {
        if (tid == 0) { status[item] = TWXPP_EMPTY_COLUMN; done[item] = 1; }
        return;
    }
    const double missing = (double)N * (double)D - nobs;
    // C = C0 (column-major in the input)
    const double *c0 = in.c0 + in.c0_off[item];
    for (int e = tid; e < PP_WS_C; e += PP_THREADS) {
        const int j = e / PP_CS, k = e % PP_CS;
        sC[e] = j < D && k < d ? c0[(int64_t)k * D + j] : 0.0;
    }
    __syncthreads();
    pp_ctc(sC, sW, D, d, tid);
    __syncthreads();
    if (wave == 0) {
        double lp;
        if (pp_invert(sW, d, lane, &lp) && lane == 0) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) { status[item] = TWXPP_NUMERIC; done[item] = 1; }
        return;
    }
    // X = (Ye C) CtC^-1 with the hidden entries of Ye 0, and the residual over the observed positions
    const PpCol col = pp_column(in, item, lane, nst, D);
    const double M = lane < D ? sM[lane] : 0.0;
    double *X0 = ws_x + ws_xoff[slot];
    double racc = 0.0;
    const int k = lane & 31;
    for (int r = wave; r < N; r += PP_NW) {
        bool o;
        const double ye = pp_row(col, M, days, r, lane, D, d, sC, nullptr, &o);
        wYe[wave][lane] = ye;
        wave_sync();
        const double t = pp_project(sC, wYe[wave], D, lane);
        if (lane < 32) wT[wave][lane] = lane < d ? t : 0.0;
        wave_sync();
        double x = 0.0;
        for (int m = 0; m < d; ++m) x = x + wT[wave][m] * sW[m * PP_K + k];
        if (lane < d) { wX[wave][lane] = x; X0[(int64_t)r * d + lane] = x; }
        wave_sync();
        if (o) {
            double rec = 0.0;
            for (int m = 0; m < d; ++m) rec = rec + wX[wave][m] * sC[lane * PP_CS + m];
            const double e = rec - ye;
            racc = racc + e * e;
        }
        wave_sync();
    }
    racc = qa_wave_sum(racc);
    if (lane == 0) sRed[wave] = racc;
    __syncthreads();
    const double ss = (((sRed[0] + sRed[1]) + sRed[2]) + sRed[3]) / ((double)N * (double)D - missing);
    double *fx = ws_fixed + (int64_t)slot * PP_WS_FIXED;
    for (int e = tid; e < PP_WS_C; e += PP_THREADS) fx[e] = sC[e];
    if (tid < PP_D) fx[PP_WS_C + tid] = tid < D ? sM[tid] : 0.0;
    if (tid == 0) {
        fx[PP_WS_C + PP_D] = ss;
        fx[PP_WS_C + PP_D + 1] = INFINITY;                         // old
        fx[PP_WS_C + PP_D + 2] = missing;
    }
}

__global__ __launch_bounds__(PP_THREADS) void k_pp_iter(PpIn in, int first_item, const int32_t *__restrict__ act,
                                                        const int64_t *__restrict__ ws_xoff, double *__restrict__ ws_fixed,
                                                        double *__restrict__ ws_x, const int64_t *__restrict__ fit_off,
                                                        double threshold, int maxits, int iters_per_launch,
                                                        uint8_t *__restrict__ done, int32_t *__restrict__ status,
                                                        int32_t *__restrict__ iters, double *__restrict__ rel_out,
                                                        double *__restrict__ fit, double *__restrict__ r2cum,
                                                        double *__restrict__ c_out, double *__restrict__ m_out)
{
    __shared__ double sC[PP_WS_C];                             // the previous C
    __shared__ double sB[PP_WS_C];                             // Ye'X, then the new C, the basis, the rotated C
    __shared__ double sS[PP_K * PP_K], sSx[PP_K * PP_K], sCtC[PP_K * PP_K], sW[PP_K * PP_K];
    __shared__ double wYe[PP_NW][PP_D], wXo[PP_NW][PP_K], wT[PP_NW][PP_K], wX[PP_NW][PP_K];
    __shared__ double sRed[PP_NW][PP_K + 1];
    __shared__ double s_lp;
    __shared__ int s_bad, s_order[PP_K];
    const int slot = act[blockIdx.x], item = first_item + slot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = lane & 31, h = lane >> 5;
    const int g = in.item_group[item];
    const int32_t *days = in.gdays + in.goff[g];
    const int N = in.goff[g + 1] - in.goff[g];
    int nst;
    const int D = pp_ncols(in, item, &nst);
    const int d = in.item_npcs[item];
    double *fx = ws_fixed + (int64_t)slot * PP_WS_FIXED;
    double *Xb = ws_x + ws_xoff[slot];
    const int64_t xsz = (int64_t)N * d;
    for (int e = tid; e < PP_WS_C; e += PP_THREADS) sC[e] = fx[e];
    if (tid < PP_D) sB[tid * PP_CS + PP_K] = 0.0;                  // the padding column: copied with the rest, never data
    if (tid == 0) s_bad = 0;
    __syncthreads();
    pp_ctc(sC, sCtC, D, d, tid);
    const PpCol col = pp_column(in, item, lane, nst, D);
    const double M = lane < D ? fx[PP_WS_C + lane] : 0.0;
    double ss = fx[PP_WS_C + PP_D], old = fx[PP_WS_C + PP_D + 1];
    const double missing = fx[PP_WS_C + PP_D + 2];
    const double dn = (double)N, dd = (double)D;
    int it = iters[item];                                          // completed iterations: count - 1
    int state = -1;                                                // -1: running; else the final status
    double rel = 0.0;
    __syncthreads();

    for (int step = 0; step < iters_per_launch && state < 0; ++step) {
        const double *Xo = Xb + (it & 1) * xsz;
        double *Xn = Xb + ((it + 1) & 1) * xsz;
        if (!(ss > 0.0) || !pp_finite(ss)) { state = TWXPP_NUMERIC; break; }
        // Sx = (I + CtC / ss)^-1
        for (int e = tid; e < PP_K * PP_K; e += PP_THREADS) {
            const int i = e >> 5, c = e & 31;
            sSx[e] = i < d && c < d ? (i == c ? 1.0 : 0.0) + sCtC[e] / ss : 0.0;
        }
        __syncthreads();
        if (wave == 0) {
            double lp;
            const bool bad = pp_invert(sSx, d, lane, &lp);
            if (lane == 0) { s_lp = lp; if (bad) s_bad = 1; }
        }
        __syncthreads();
        if (s_bad) { state = TWXPP_NUMERIC; break; }
        const double ss_old = ss;
        // pass 1: refill, X = ((Ye C) Sx) / ss, the partial Ye'X and X'X
        double yacc[PP_K], sacc[16];
#pragma unroll
        for (int t = 0; t < PP_K; ++t) yacc[t] = 0.0;
#pragma unroll
        for (int t = 0; t < 16; ++t) sacc[t] = 0.0;
        for (int r = wave; r < N; r += PP_NW) {
            if (lane < d) wXo[wave][lane] = Xo[(int64_t)r * d + lane];
            wave_sync();
            bool o;
            const double ye = pp_row(col, M, days, r, lane, D, d, sC, wXo[wave], &o);
            wYe[wave][lane] = ye;
            wave_sync();
            const double t = pp_project(sC, wYe[wave], D, lane);
            if (lane < 32) wT[wave][lane] = lane < d ? t : 0.0;
            wave_sync();
            double x = 0.0;
            for (int m = 0; m < d; ++m) x = x + wT[wave][m] * sSx[m * PP_K + k];
            x = x / ss;
            if (lane < 32) wX[wave][lane] = lane < d ? x : 0.0;
            if (lane < d) Xn[(int64_t)r * d + lane] = x;
            wave_sync();
#pragma unroll
            for (int t2 = 0; t2 < PP_K; ++t2)
                if (t2 < d) yacc[t2] = yacc[t2] + ye * wX[wave][t2];
#pragma unroll
            for (int t2 = 0; t2 < 16; ++t2)
                if (h + 2 * t2 < d) sacc[t2] = sacc[t2] + wX[wave][h + 2 * t2] * x;
            wave_sync();
        }
        PP_COMBINE(sB, PP_K, lane * PP_CS + t, yacc)
        PP_COMBINE(sS, 16, ((h + 2 * t < d && k < d) ? (h + 2 * t) * PP_K + k : -1), sacc)
        // C = (Ye'X) (S + N Sx)^-1
        for (int e = tid; e < PP_K * PP_K; e += PP_THREADS) {
            const int i = e >> 5, c = e & 31;
            sW[e] = i < d && c < d ? sS[e] + dn * sSx[e] : 0.0;
        }
        __syncthreads();
        if (wave == 0) {
            double lp;
            if (pp_invert(sW, d, lane, &lp) && lane == 0) s_bad = 1;
        }
        {
            double rowv[PP_K];
#pragma unroll
            for (int m = 0; m < PP_K; ++m) rowv[m] = sB[lane * PP_CS + m];
            __syncthreads();
            if (s_bad) { state = TWXPP_NUMERIC; break; }
            for (int c = wave; c < d; c += PP_NW) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < PP_K; ++m)
                    if (m < d) acc = acc + rowv[m] * sW[m * PP_K + c];
                sB[lane * PP_CS + c] = acc;
            }
        }
        __syncthreads();
        pp_ctc(sB, sCtC, D, d, tid);
        // pass 2: sum (C X' - Ye')^2 with the new C and the new X, Ye as pass 1 filled it
        double racc = 0.0;
        for (int r = wave; r < N; r += PP_NW) {
            if (lane < d) { wXo[wave][lane] = Xo[(int64_t)r * d + lane]; wX[wave][lane] = Xn[(int64_t)r * d + lane]; }
            wave_sync();
            bool o;
            const double ye = pp_row(col, M, days, r, lane, D, d, sC, wXo[wave], &o);
            if (lane < D) {
                double rec = 0.0;
                for (int m = 0; m < d; ++m) rec = rec + wX[wave][m] * sB[lane * PP_CS + m];
                const double e = rec - ye;
                racc = racc + e * e;
            }
            wave_sync();
        }
        racc = qa_wave_sum(racc);
        if (lane == 0) sRed[wave][0] = racc;
        __syncthreads();
        const double res = ((sRed[0][0] + sRed[1][0]) + sRed[2][0]) + sRed[3][0];
        const double cs = pp_dot_dd(sCtC, sSx, d, lane);
        const double trsx = pp_dot_dd(sSx, nullptr, d, lane), trs = pp_dot_dd(sS, nullptr, d, lane);
        ss = (res + dn * cs + missing * ss_old) / (dn * dd);
        if (!(ss > 0.0) || !pp_finite(ss)) { state = TWXPP_NUMERIC; break; }
        const double objective = dn * (dd * log(ss) + trsx + s_lp) + trs - missing * log(ss_old);
        rel = fabs(1.0 - objective / old);
        old = objective;
        ++it;
        if (rel < threshold && it + 1 > 5) state = TWXPP_OK;
        else if (it + 1 > maxits) state = TWXPP_MAXITS;
        __syncthreads();                                         // sRed, s_lp and the matrices are written again
        if (state < 0) {
            for (int e = tid; e < PP_WS_C; e += PP_THREADS) sC[e] = sB[e];
            __syncthreads();
        }
    }

    if (state == TWXPP_NUMERIC) {
        if (tid == 0) { done[item] = 1; status[item] = TWXPP_NUMERIC; iters[item] = it; rel_out[item] = NAN; }
        return;                                                  // fit / r2cum keep the NaN the host filled them with
    }
    if (state < 0) {                                             // sC holds the current C
        for (int e = tid; e < PP_WS_C; e += PP_THREADS) fx[e] = sC[e];
        if (tid == 0) { fx[PP_WS_C + PP_D] = ss; fx[PP_WS_C + PP_D + 1] = old; iters[item] = it; rel_out[item] = rel; }
        return;
    }

    // the item stops: sC / Xo are what the last iteration filled Ye from, sB is the last C
    const double *Xo = Xb + ((it - 1) & 1) * xsz;
    if (wave == 0) {                                             // the basis: lane j owns row j, nothing is shared
        bool bad = false;
        for (int c = 0; c < d && !bad; ++c) {
            double ck = sB[lane * PP_CS + c];
            for (int pass = 0; pass < 2; ++pass)
                for (int m = 0; m < c; ++m) {
                    const double qm = sB[lane * PP_CS + m];
                    const double dot = qa_wave_sum(qm * ck);
                    ck = ck - dot * qm;
                }
            const double nrm = sqrt(qa_wave_sum(ck * ck));
            if (!(nrm > 0.0) || !pp_finite(nrm)) bad = true;
            else sB[lane * PP_CS + c] = ck / nrm;
        }
        if (bad && lane == 0) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) { done[item] = 1; status[item] = TWXPP_NUMERIC; iters[item] = it; rel_out[item] = NAN; }
        return;
    }
    {   // T = Ye Q: its column sums and T'T
        double sacc[16], tsum = 0.0;
#pragma unroll
        for (int t = 0; t < 16; ++t) sacc[t] = 0.0;
        for (int r = wave; r < N; r += PP_NW) {
            if (lane < d) wXo[wave][lane] = Xo[(int64_t)r * d + lane];
            wave_sync();
            bool o;
            const double ye = pp_row(col, M, days, r, lane, D, d, sC, wXo[wave], &o);
            wYe[wave][lane] = ye;
            wave_sync();
            const double t = pp_project(sB, wYe[wave], D, lane);
            if (lane < 32) wT[wave][lane] = lane < d ? t : 0.0;
            wave_sync();
            if (k < d) tsum = tsum + t;
#pragma unroll
            for (int t2 = 0; t2 < 16; ++t2)
                if (h + 2 * t2 < d) sacc[t2] = sacc[t2] + wT[wave][h + 2 * t2] * t;
            wave_sync();
        }
        PP_COMBINE(sS, 16, ((h + 2 * t < d && k < d) ? (h + 2 * t) * PP_K + k : -1), sacc)
        if (lane < 32) sRed[wave][lane] = tsum;
        __syncthreads();
        if (tid < 32) wT[0][tid] = ((sRed[0][tid] + sRed[1][tid]) + sRed[2][tid]) + sRed[3][tid];
        __syncthreads();
        for (int e = tid; e < PP_K * PP_K; e += PP_THREADS) {
            const int i = e >> 5, c = e & 31;
            sW[e] = i < d && c < d ? (sS[e] - wT[0][i] * wT[0][c] / dn) / (dn - 1.0) : 0.0;
            sSx[e] = i == c ? 1.0 : 0.0;                         // the eigenvectors start as I
        }
        __syncthreads();
    }
    if (wave == 0) {                                             // cyclic Jacobi on sW, eigenvectors in the columns of sSx
        for (int sweep = 0; sweep < PP_SWEEPS; ++sweep) {
            double off = 0.0, dia = 0.0;
            for (int e = lane; e < PP_K * PP_K; e += 64) {
                const int i = e >> 5, c = e & 31;
                if (i < d && c < d) {
                    if (i == c) dia = dia + sW[e] * sW[e];
                    else off = off + sW[e] * sW[e];
                }
            }
            off = qa_wave_sum(off); dia = qa_wave_sum(dia);
            if (!(off > 1e-40 * dia)) break;
            for (int p = 0; p < d - 1; ++p)
                for (int q = p + 1; q < d; ++q) {
                    const double apq = sW[p * PP_K + q];
                    if (apq == 0.0) continue;
                    const double theta = (sW[q * PP_K + q] - sW[p * PP_K + p]) / (2.0 * apq);
                    const double t = theta == 0.0 ? 1.0 : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    double *A = h == 0 ? sW : sSx;               // lanes 0..31 the matrix, 32..63 the eigenvectors
                    wave_sync();
                    if (k < d) {
                        const double ap = A[k * PP_K + p], aq = A[k * PP_K + q];
                        A[k * PP_K + p] = c * ap - s * aq;
                        A[k * PP_K + q] = s * ap + c * aq;
                    }
                    wave_sync();
                    if (h == 0 && k < d) {
                        const double ap = sW[p * PP_K + k], aq = sW[q * PP_K + k];
                        sW[p * PP_K + k] = c * ap - s * aq;
                        sW[q * PP_K + k] = s * ap + c * aq;
                    }
                    wave_sync();
                }
        }
        wave_sync();
        if (lane == 0) {                                         // eigenvalues descending, equal ones in index order
            unsigned used = 0u;
            for (int c = 0; c < d; ++c) {
                int best = -1;
                for (int m = 0; m < d; ++m)
                    if (!((used >> m) & 1u) && (best < 0 || sW[m * PP_K + m] > sW[best * PP_K + best])) best = m;
                used |= 1u << best;
                s_order[c] = best;
            }
        }
        wave_sync();
        double rowv[PP_K];                                       // C = Q V, row j by lane j
#pragma unroll
        for (int m = 0; m < PP_K; ++m) rowv[m] = sB[lane * PP_CS + m];
        for (int c = 0; c < d; ++c) {
            const int oc = s_order[c];
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < PP_K; ++m)
                if (m < d) acc = acc + rowv[m] * sSx[m * PP_K + oc];
            sB[lane * PP_CS + c] = acc;
        }
    }
    __syncthreads();
    {   // the scores X = Ye C, the fit of column 0 and R2cum
        double err[PP_K], den = 0.0;
#pragma unroll
        for (int t = 0; t < PP_K; ++t) err[t] = 0.0;
        const double norm0 = in.norms[in.par_off[item]], sd0 = in.stds[in.par_off[item]];
        const double M0 = fx[PP_WS_C];
        double *fo = fit + fit_off[item];
        for (int r = wave; r < N; r += PP_NW) {
            if (lane < d) wXo[wave][lane] = Xo[(int64_t)r * d + lane];
            wave_sync();
            bool o;
            const double ye = pp_row(col, M, days, r, lane, D, d, sC, wXo[wave], &o);
            wYe[wave][lane] = ye;
            wave_sync();
            const double x = pp_project(sB, wYe[wave], D, lane);
            if (lane < 32) wX[wave][lane] = lane < d ? x : 0.0;
            wave_sync();
            if (lane == 0) {
                double f = 0.0;
                for (int m = 0; m < d; ++m) f = f + wX[wave][m] * sB[m];
                fo[r] = (f + M0) * sd0 + norm0;
            }
            if (o) {
                double rec = 0.0;
#pragma unroll
                for (int t = 0; t < PP_K; ++t)
                    if (t < d) {
                        rec = rec + wX[wave][t] * sB[lane * PP_CS + t];
                        const double e = ye - rec;
                        err[t] = err[t] + e * e;
                    }
                den = den + ye * ye;
            }
            wave_sync();
        }
#pragma unroll
        for (int t = 0; t < PP_K; ++t)
            if (t < d) {
                const double v = qa_wave_sum(err[t]);
                if (lane == 0) sRed[wave][t] = v;
            }
        den = qa_wave_sum(den);
        if (lane == 0) sRed[wave][PP_K] = den;
        __syncthreads();
        if (tid < d) {
            const double e = ((sRed[0][tid] + sRed[1][tid]) + sRed[2][tid]) + sRed[3][tid];
            const double dt = ((sRed[0][PP_K] + sRed[1][PP_K]) + sRed[2][PP_K]) + sRed[3][PP_K];
            r2cum[(int64_t)item * PP_K + tid] = 1.0 - e / dt;
        }
    }
    if (c_out)
        for (int e = tid; e < PP_D * PP_K; e += PP_THREADS)
            if ((e >> 5) < D && (e & 31) < d) c_out[(int64_t)item * PP_D * PP_K + e] = sB[(e >> 5) * PP_CS + (e & 31)];
    if (m_out && tid < D) m_out[(int64_t)item * PP_D + tid] = fx[PP_WS_C + tid];
    if (tid == 0) { done[item] = 1; status[item] = state; iters[item] = it; rel_out[item] = rel; }
}

extern "C" int twxpp_ppca_fit(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t ngroups,
                              const int8_t *group, int64_t nitem, const int32_t *item_target, const int32_t *item_group,
                              const int32_t *item_matrix_status, const int32_t *item_npcs, const int64_t *col_off,
                              const int32_t *col_idx, int64_t nset, const int32_t *set_group, const int32_t *set_ncol,
                              const double *set_vals, const int32_t *item_set, const double *norms, const double *stds,
                              const double *c0, double threshold, int32_t maxits, int32_t iters_per_launch,
                              int64_t workspace_bytes, double *fit, double *r2cum, int32_t *iters, double *rel,
                              int32_t *status, double *c_out, double *m_out, int32_t *counts, float *kernel_ms,
                              char *errbuf, int errlen)
{
    const char *fn = "twxpp_ppca_fit";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || nitem < 1 || nstn > INT32_MAX || ndays > INT32_MAX || nitem > INT32_MAX / 2 ||
        ngroups < 1 || ngroups > 127 || nset < 0 || nset > INT32_MAX) {
        snprintf(msg, sizeof msg, "%s: need nstn, ndays, nitem >= 1, 1 <= ngroups <= 127 and nset >= 0", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!obs || !group || !item_target || !item_group || !item_npcs || !col_off || !norms || !stds || !c0 || !fit ||
        !r2cum || !iters || !rel || !status || (nset > 0 && (!set_group || !set_ncol || !set_vals || !item_set))) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!(threshold > 0.0) || !std::isfinite(threshold) || maxits < 1) {
        snprintf(msg, sizeof msg, "%s: threshold and maxits must be positive (defaults: TWXPP_DEFAULT_THRESHOLD, TWXPP_DEFAULT_MAXITS)", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (iters_per_launch <= 0) iters_per_launch = TWXPP_ITERS_PER_LAUNCH;
    if (workspace_bytes <= 0) workspace_bytes = TWXPP_WORKSPACE_BYTES;
    // the used days sorted by group, in day order within a group
    std::vector<int32_t> goff((size_t)ngroups + 1, 0);
    for (int64_t d = 0; d < ndays; ++d) {
        if (group[d] < -1 || group[d] >= ngroups) {
            snprintf(msg, sizeof msg, "%s: group[%lld] = %d outside -1 .. %d", fn, (long long)d, (int)group[d], ngroups - 1);
            return qa_fail(errbuf, errlen, msg);
        }
        if (group[d] >= 0) ++goff[(size_t)group[d] + 1];
    }
    for (int g = 0; g < ngroups; ++g) goff[(size_t)g + 1] += goff[(size_t)g];
    std::vector<int32_t> gdays((size_t)goff[(size_t)ngroups]), fillpos(goff.begin(), goff.end() - 1);
    for (int64_t d = 0; d < ndays; ++d)
        if (group[d] >= 0) gdays[(size_t)fillpos[(size_t)group[d]]++] = (int32_t)d;
    std::vector<int64_t> set_off((size_t)nset + 1, 0);
    for (int64_t s = 0; s < nset; ++s) {
        if (set_group[s] < 0 || set_group[s] >= ngroups || set_ncol[s] < 0) {
            snprintf(msg, sizeof msg, "%s: extra-column set %lld: group %d, %d columns", fn, (long long)s, (int)set_group[s],
                     (int)set_ncol[s]);
            return qa_fail(errbuf, errlen, msg);
        }
        const int64_t rows = goff[(size_t)set_group[s] + 1] - goff[(size_t)set_group[s]];
        set_off[(size_t)s + 1] = set_off[(size_t)s] + rows * set_ncol[s];
    }
    const size_t NI = (size_t)nitem;
    std::vector<int32_t> h_status(NI, TWXPP_OK), h_iset(NI, -1);
    std::vector<uint8_t> h_done(NI, 0);
    std::vector<int64_t> par_off(NI + 1, 0), c0_off(NI + 1, 0), fit_off(NI + 1, 0);
    for (int64_t i = 0; i < nitem; ++i) {
        if (item_target[i] < 0 || item_target[i] >= nstn || item_group[i] < 0 || item_group[i] >= ngroups) {
            snprintf(msg, sizeof msg, "%s: item %lld: target %d outside [0, %lld) or group %d outside [0, %d)", fn,
                     (long long)i, (int)item_target[i], (long long)nstn, (int)item_group[i], ngroups);
            return qa_fail(errbuf, errlen, msg);
        }
        if (col_off[i + 1] < col_off[i] || (i == 0 && col_off[0] != 0) || (col_off[i + 1] > col_off[i] && !col_idx)) {
            snprintf(msg, sizeof msg, "%s: col_off is not a CSR offset array at item %lld", fn, (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
        const int64_t s = item_set ? item_set[i] : -1;
        if (s < -1 || s >= nset || (s >= 0 && set_group[s] != item_group[i])) {
            snprintf(msg, sizeof msg, "%s: item %lld names extra-column set %lld (of %lld; it must be of the item's group)", fn,
                     (long long)i, (long long)s, (long long)nset);
            return qa_fail(errbuf, errlen, msg);
        }
        h_iset[(size_t)i] = (int32_t)s;
        for (int64_t c = col_off[i]; c < col_off[i + 1]; ++c)
            if (col_idx[c] < 0 || col_idx[c] >= nstn) {
                snprintf(msg, sizeof msg, "%s: item %lld: column index %d outside [0, %lld)", fn, (long long)i,
                         (int)col_idx[c], (long long)nstn);
                return qa_fail(errbuf, errlen, msg);
            }
        const int64_t D = 1 + (col_off[i + 1] - col_off[i]) + (s >= 0 ? set_ncol[s] : 0);
        const int64_t d = item_npcs[i];
        const int64_t rows = goff[(size_t)item_group[i] + 1] - goff[(size_t)item_group[i]];
        const bool nomat = item_matrix_status && item_matrix_status[i] != TWXIF_OK;
        if (!nomat && (d < 1 || d > D || rows <= d)) {
            snprintf(msg, sizeof msg, "%s: item %lld: %lld components for %lld rows by %lld columns (need 1 <= d <= D and N > d)",
                     fn, (long long)i, (long long)d, (long long)rows, (long long)D);
            return qa_fail(errbuf, errlen, msg);
        }
        par_off[(size_t)i + 1] = par_off[(size_t)i] + D;
        c0_off[(size_t)i + 1] = c0_off[(size_t)i] + (nomat ? 0 : D * d);
        fit_off[(size_t)i + 1] = fit_off[(size_t)i] + rows;
        int32_t st = TWXPP_OK;
        if (nomat) st = TWXPP_NO_MATRIX;
        else if (rows > TWXPP_MAX_ROWS) st = TWXPP_ROW_CAP;
        else if (D > TWXPP_MAX_COLS) st = TWXPP_COL_CAP;
        else if (d > TWXPP_MAX_PCS) st = TWXPP_PCS_CAP;
        if (st != TWXPP_OK) { h_status[(size_t)i] = st; h_done[(size_t)i] = 1; }
    }
    const int64_t ncolidx = col_off[nitem], npar = par_off[NI], nc0 = c0_off[NI], nfit = fit_off[NI];

    QACHK(hipSetDevice(device));
    const auto t_up = std::chrono::steady_clock::now();
    QaPool bufs;
    float *d_obs;
    int32_t *d_gdays, *d_goff, *d_itarget, *d_igroup, *d_iset, *d_inpcs, *d_colidx, *d_setncol, *d_iters, *d_status;
    int64_t *d_coloff, *d_setoff, *d_paroff, *d_c0off, *d_fitoff;
    double *d_setvals, *d_norms, *d_stds, *d_c0, *d_fit, *d_r2, *d_rel, *d_cout = nullptr, *d_mout = nullptr;
    uint8_t *d_done;
    const size_t NS = (size_t)nstn, ND = (size_t)ndays, G = (size_t)ngroups, NSET = (size_t)nset;
    QAALLOC(bufs, d_obs, float, NS * ND);
    QAALLOC(bufs, d_gdays, int32_t, gdays.size()); QAALLOC(bufs, d_goff, int32_t, G + 1);
    QAALLOC(bufs, d_itarget, int32_t, NI); QAALLOC(bufs, d_igroup, int32_t, NI); QAALLOC(bufs, d_iset, int32_t, NI);
    QAALLOC(bufs, d_inpcs, int32_t, NI);
    QAALLOC(bufs, d_coloff, int64_t, NI + 1); QAALLOC(bufs, d_colidx, int32_t, ncolidx);
    QAALLOC(bufs, d_setncol, int32_t, NSET); QAALLOC(bufs, d_setoff, int64_t, NSET + 1);
    QAALLOC(bufs, d_setvals, double, set_off[NSET]);
    QAALLOC(bufs, d_paroff, int64_t, NI + 1); QAALLOC(bufs, d_c0off, int64_t, NI + 1); QAALLOC(bufs, d_fitoff, int64_t, NI + 1);
    QAALLOC(bufs, d_norms, double, npar); QAALLOC(bufs, d_stds, double, npar); QAALLOC(bufs, d_c0, double, nc0);
    QAALLOC(bufs, d_iters, int32_t, NI); QAALLOC(bufs, d_status, int32_t, NI); QAALLOC(bufs, d_done, uint8_t, NI);
    QAALLOC(bufs, d_fit, double, nfit); QAALLOC(bufs, d_r2, double, NI * PP_K); QAALLOC(bufs, d_rel, double, NI);
    QAUP_NZ(d_obs, obs, float, NS * ND);
    QAUP_NZ(d_gdays, gdays.data(), int32_t, gdays.size());
    QAUP_NZ(d_goff, goff.data(), int32_t, G + 1);
    QAUP_NZ(d_itarget, item_target, int32_t, NI);
    QAUP_NZ(d_igroup, item_group, int32_t, NI);
    QAUP_NZ(d_iset, h_iset.data(), int32_t, NI);
    QAUP_NZ(d_inpcs, item_npcs, int32_t, NI);
    QAUP_NZ(d_coloff, col_off, int64_t, NI + 1);
    QAUP_NZ(d_colidx, col_idx, int32_t, ncolidx);
    QAUP_NZ(d_setncol, set_ncol, int32_t, NSET);
    QAUP_NZ(d_setoff, set_off.data(), int64_t, NSET + 1);
    QAUP_NZ(d_setvals, set_vals, double, set_off[NSET]);
    QAUP_NZ(d_paroff, par_off.data(), int64_t, NI + 1);
    QAUP_NZ(d_c0off, c0_off.data(), int64_t, NI + 1);
    QAUP_NZ(d_fitoff, fit_off.data(), int64_t, NI + 1);
    QAUP_NZ(d_norms, norms, double, npar);
    QAUP_NZ(d_stds, stds, double, npar);
    QAUP_NZ(d_c0, c0, double, nc0);
    QAUP_NZ(d_status, h_status.data(), int32_t, NI);
    QAUP_NZ(d_done, h_done.data(), uint8_t, NI);
    QACHK(hipMemset(d_iters, 0, NI * 4));
    QACHK(hipMemset(d_fit, 0xff, (size_t)nfit * 8));             // all bits set: a NaN
    QACHK(hipMemset(d_r2, 0xff, NI * PP_K * 8));
    QACHK(hipMemset(d_rel, 0xff, NI * 8));
    if (c_out) { QAALLOC(bufs, d_cout, double, NI * PP_D * PP_K); QACHK(hipMemset(d_cout, 0xff, NI * PP_D * PP_K * 8)); }
    if (m_out) { QAALLOC(bufs, d_mout, double, NI * PP_D); QACHK(hipMemset(d_mout, 0xff, NI * PP_D * 8)); }
    PpIn in = {d_obs, ndays, d_gdays, d_goff, d_itarget, d_igroup, d_iset, d_inpcs, d_coloff, d_colidx, d_setncol, d_setoff,
               d_setvals, d_paroff, d_norms, d_stds, d_c0off, d_c0};

    QaTimer tm;
    float ms[TWXPP_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) {
        QACHK(tm.init());
        QACHK(hipDeviceSynchronize());
        ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    }
    // batches of consecutive items under the workspace budget (at least one item each)
    int rounds = 0, nbatches = 0;
    std::vector<int64_t> xoff;
    std::vector<int32_t> act;
    std::vector<uint8_t> bdone;
    for (int64_t first = 0; first < nitem;) {
        xoff.clear();
        int64_t x_total = 0, bytes = 0, last = first;
        for (; last < nitem; ++last) {
            const int64_t rows = goff[(size_t)item_group[last] + 1] - goff[(size_t)item_group[last]];
            const int64_t xd = h_done[(size_t)last] ? 0 : 2 * rows * item_npcs[last];
            const int64_t need = (int64_t)PP_WS_FIXED * 8 + 8 + 4 + xd * 8;
            if (last > first && bytes + need > workspace_bytes) break;
            xoff.push_back(x_total);
            x_total += xd;
            bytes += need;
        }
        const size_t NB = (size_t)(last - first);
        ++nbatches;
        QaPool ws;                                               // freed at the end of the batch
        int64_t *w_xoff;
        int32_t *w_act;
        double *w_fixed, *w_x;
        QAALLOC(ws, w_xoff, int64_t, NB); QAALLOC(ws, w_act, int32_t, NB);
        QAALLOC(ws, w_fixed, double, NB * PP_WS_FIXED); QAALLOC(ws, w_x, double, x_total);
        QAUP_NZ(w_xoff, xoff.data(), int64_t, NB);
        if (kernel_ms) QACHK(tm.start());
        hipLaunchKernelGGL(k_pp_prep, dim3((unsigned)NB), dim3(PP_THREADS), 0, nullptr, in, (int)first,
                           (const int64_t *)w_xoff, w_fixed, w_x, d_done, d_status);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        bdone.resize(NB);
        const int64_t max_rounds = ((int64_t)maxits + iters_per_launch - 1) / iters_per_launch;
        for (int64_t round = 0;; ++round) {
            QACHK(hipMemcpy(bdone.data(), d_done + first, NB, hipMemcpyDeviceToHost));
            act.clear();
            for (size_t b = 0; b < NB; ++b)
                if (!bdone[b]) act.push_back((int32_t)b);
            if (act.empty()) break;
            if (round >= max_rounds) {                           // every launch advances each of its items or ends it
                snprintf(msg, sizeof msg, "%s: internal error: %lld launches for maxits %d", fn, (long long)round, (int)maxits);
                return qa_fail(errbuf, errlen, msg);
            }
            QAUP_NZ(w_act, act.data(), int32_t, act.size());
            if (kernel_ms) QACHK(tm.start());
            hipLaunchKernelGGL(k_pp_iter, dim3((unsigned)act.size()), dim3(PP_THREADS), 0, nullptr, in, (int)first,
                               (const int32_t *)w_act, (const int64_t *)w_xoff, w_fixed, w_x, (const int64_t *)d_fitoff,
                               threshold, (int)maxits, (int)iters_per_launch, d_done, d_status, d_iters, d_rel, d_fit, d_r2,
                               d_cout, d_mout);
            QACHK(hipGetLastError());
            if (kernel_ms) QACHK(tm.stop_add(&ms[1]));
            ++rounds;
        }
        first = last;
    }
    const auto t_down = std::chrono::steady_clock::now();
    QACHK(hipMemcpy(fit, d_fit, (size_t)nfit * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(r2cum, d_r2, NI * PP_K * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(rel, d_rel, NI * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(iters, d_iters, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(status, d_status, NI * 4, hipMemcpyDeviceToHost));
    if (c_out) QACHK(hipMemcpy(c_out, d_cout, NI * PP_D * PP_K * 8, hipMemcpyDeviceToHost));
    if (m_out) QACHK(hipMemcpy(m_out, d_mout, NI * PP_D * 8, hipMemcpyDeviceToHost));
    ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    if (counts) { counts[0] = rounds; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
