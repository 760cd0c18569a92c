// twx_emnorm.hip -- libtwxqa.so: the mean / variance estimator of step14 (twx/infill/rpy/norm_infill.R: prelim.norm,
// em.norm, getparam.norm, of which the reference keeps mu[1] and sigma[1, 1]) restated from Schafer (1997, section 5.3)
// for every (target, day group) item of one call (include/twx_qa.h, twxem_mean_variance).  Its own translation unit;
// the helpers it shares with the other units (the wave sums, the buffer list, the event timer) are twx_qa_common.h's.
//
// An item is a matrix of up to TWXEM_MAX_ROWS days by P <= 31 columns: the target, its station columns (float32 rows of
// the station-major observations) and the columns of one optional extra set (float64).  theta is the symmetric
// 32 x 32 array of the header, index 0 the constant, index j = column j - 1; entries above P stay 0.
//
// k_em_prep: one workgroup of 256 per item.  A wavefront takes the columns w, w + 4, ...: a lane sums the rows lane,
// lane + 64, ... in order and an xor butterfly combines the 64 partial sums (cnt, sum, sum of squares), and ORs the
// column's bit into the row's mask (an integer LDS atomic; the result does not depend on the order).  The rows are then
// sorted by the 64-bit key (mask << 32 | row) with a bitonic network in LDS -- the keys are distinct, so equal masks
// keep day order -- and thread 0 walks the sorted keys once and writes the table of runs: a run is a stretch of equal
// masks of at most TWXEM_RUN_ROWS rows (a longer stretch is cut, so that no single wavefront is left with the one large
// pattern of an item).  Written per item: the row permutation, the run starts, cnt / xbar / sdv and the start theta.
//
// k_em_iter: one workgroup of 256 (4 wavefronts) per unfinished item, up to iters_per_launch iterations.  theta lives in
// LDS.  Wavefront w takes the runs w, w + 4, ...: it copies theta into its own W (lane l owns W[i][j], j = l % 32,
// i = l / 32 + 2 t, t = 0 .. 15, in registers and in LDS), sweeps it on the observed indices in ascending order, then
// walks the run's rows: the standardised row goes to 32 doubles of LDS, the lanes of missing columns replace theirs by
// the regression prediction, and every lane adds y_i y_j to its 16 registers of the partial T.  Only wavefront-level
// synchronisation is used inside a run.  The partial Ts go to LDS (into the W buffers) and are added in wavefront
// order; no float atomics anywhere, so every sum has a fixed order and two calls give the same bytes.  The mask of a run
// is the ballot of its first row's finite columns, so no mask table is stored; the matrix itself is re-gathered from
// the observations in every iteration, so the workspace holds 8 bytes per row and theta, not a standardised copy.
//
// LDS: k_em_prep 64 KiB of keys (8 B x TWXEM_MAX_ROWS) + 0.8 KiB of column statistics = 64.8 KiB; k_em_iter 8 KiB theta
// + 4 x 8 KiB W + 4 x 256 B rows + 0.6 KiB = 41.6 KiB: three workgroups of it fit a compute unit's 160 KiB.
// fp64 throughout; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define EM_D 32                              // theta is EM_D x EM_D: the constant and up to 31 columns
#define EM_NW 4                              // wavefronts of a k_em_iter workgroup
#define EM_THREADS (64 * EM_NW)
#define EM_DBL_MAX 1.7976931348623157e308

namespace {

__device__ __forceinline__ bool em_finite(double v) { return fabs(v) <= EM_DBL_MAX; }

// orders the LDS traffic of the lanes of one wavefront (its instructions issue in order; this keeps the compiler from
// moving a lane's read above another lane's write)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what a kernel needs to find the columns of an item
struct EmIn {
    const float *obs;            // [nstn][ndays]
    int64_t ndays;
    const int32_t *gdays;        // the used days sorted by group
    const int32_t *goff;         // [ngroups + 1]
    const int32_t *item_target, *item_group, *item_set;
    const int64_t *col_off;
    const int32_t *col_idx;
    const int32_t *set_ncol;
    const int64_t *set_off;
    const double *set_vals;
};

// the value of column c (0 = target) of the item on row r of its group; lane-invariant parts are resolved by em_column
struct EmCol {
    const float *pf;             // station row, or nullptr
    const double *pd;            // extra column, or nullptr
};

__device__ __forceinline__ EmCol em_column(const EmIn &in, int item, int c, int nst)
{
    EmCol col = {nullptr, nullptr};
    if (c == 0) col.pf = in.obs + (int64_t)in.item_target[item] * in.ndays;
    else if (c <= nst) col.pf = in.obs + (int64_t)in.col_idx[in.col_off[item] + c - 1] * in.ndays;
    else {
        const int s = in.item_set[item], g = in.item_group[item];
        const int64_t nrows = in.goff[g + 1] - in.goff[g];
        col.pd = in.set_vals + in.set_off[s] + (int64_t)(c - 1 - nst) * nrows;
    }
    return col;
}

__device__ __forceinline__ int em_ncols(const EmIn &in, int item, int *nst)
{
    *nst = (int)(in.col_off[item + 1] - in.col_off[item]);
    const int s = in.item_set[item];
    return 1 + *nst + (s >= 0 ? in.set_ncol[s] : 0);
}

}  // namespace

__global__ __launch_bounds__(256) void k_em_prep(EmIn in, int first_item, const int64_t *__restrict__ ws_row_off,
                                                 int32_t *__restrict__ ws_perm, int32_t *__restrict__ ws_runs,
                                                 int32_t *__restrict__ ws_nruns, double *__restrict__ ws_stat,
                                                 double *__restrict__ ws_theta, uint8_t *__restrict__ done,
                                                 int32_t *__restrict__ status)
{
    __shared__ unsigned long long keys[TWXEM_MAX_ROWS];
    __shared__ double s_cnt[EM_D], s_xbar[EM_D], s_sdv[EM_D];
    const int slot = blockIdx.x, item = first_item + slot;
    if (done[item]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = in.item_group[item];
    const int32_t *days = in.gdays + in.goff[g];
    const int nrows = in.goff[g + 1] - in.goff[g];
    if (nrows > TWXEM_MAX_ROWS) return;                          // the host has marked it TWXEM_ROW_CAP
    int nst;
    const int P = em_ncols(in, item, &nst);
    int npad = 1;
    while (npad < nrows) npad <<= 1;
    for (int r = tid; r < npad; r += 256) keys[r] = r < nrows ? (unsigned long long)r : ~0ull;
    __syncthreads();
    for (int c = wave; c < P; c += 4) {
        const EmCol col = em_column(in, item, c, nst);
        double cnt = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = lane; r < nrows; r += 64) {
            const double x = col.pf ? (double)col.pf[days[r]] : col.pd[r];
            if (em_finite(x)) {
                cnt = cnt + 1.0;
                s1 = s1 + x;
                s2 = s2 + x * x;
                atomicOr((unsigned *)&keys[r] + 1, 1u << (c + 1));
            }
        }
        cnt = qa_wave_sum(cnt); s1 = qa_wave_sum(s1); s2 = qa_wave_sum(s2);
        if (lane == 0) {
            const double xbar = s1 / cnt;
            double sdv = sqrt((s2 - s1 * s1 / cnt) / cnt);
            if (sdv == 0.0) sdv = 1.0;
            s_cnt[c + 1] = cnt; s_xbar[c + 1] = xbar; s_sdv[c + 1] = sdv;
        }
    }
    __syncthreads();
    bool empty = false;
    for (int c = 0; c < P; ++c) empty = empty || s_cnt[c + 1] == 0.0;
    if (empty) {
        if (tid == 0) { status[item] = TWXEM_EMPTY_COLUMN; done[item] = 1; }
        return;
    }
    if (tid < EM_D) {
        const bool used = tid >= 1 && tid <= P;
        ws_stat[(int64_t)slot * 2 * EM_D + tid] = used ? s_xbar[tid] : 0.0;
        ws_stat[(int64_t)slot * 2 * EM_D + EM_D + tid] = used ? s_sdv[tid] : 1.0;
    }
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long a = keys[i], b = keys[p];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[p] = a; }
                }
            }
            __syncthreads();
        }
    const int64_t ro = ws_row_off[slot];
    int32_t *perm = ws_perm + ro, *runs = ws_runs + ro + slot;     // rows + 1 entries of runs per item
    for (int r = tid; r < nrows; r += 256) perm[r] = (int32_t)(keys[r] & 0xffffffffull);
    if (tid == 0) {
        int nr = 0, start = 0;
        for (int i = 1; i <= nrows; ++i)
            if (i == nrows || (keys[i] >> 32) != (keys[start] >> 32) || i - start == TWXEM_RUN_ROWS) {
                runs[nr++] = start;
                start = i;
            }
        runs[nr] = nrows;
        ws_nruns[slot] = nr;
    }
    double *theta = ws_theta + (int64_t)slot * EM_D * EM_D;
    for (int e = tid; e < EM_D * EM_D; e += 256) {
        const int i = e >> 5, j = e & 31;
        theta[e] = e == 0 ? -1.0 : (i == j && i <= P ? 1.0 : 0.0);
    }
}

__global__ __launch_bounds__(EM_THREADS) void k_em_iter(EmIn in, int first_item, const int32_t *__restrict__ act,
                                                        const int64_t *__restrict__ ws_row_off,
                                                        const int32_t *__restrict__ ws_perm,
                                                        const int32_t *__restrict__ ws_runs,
                                                        const int32_t *__restrict__ ws_nruns,
                                                        const double *__restrict__ ws_stat, double *__restrict__ ws_theta,
                                                        double criterion, int maxits, int iters_per_launch,
                                                        uint8_t *__restrict__ done, int32_t *__restrict__ status,
                                                        int32_t *__restrict__ iters, double *__restrict__ delta,
                                                        double *__restrict__ mean, double *__restrict__ variance,
                                                        double *__restrict__ mu_out, double *__restrict__ sigma_out)
{
    __shared__ double s_theta[EM_D * EM_D];
    __shared__ double s_w[EM_NW][EM_D * EM_D];
    __shared__ double s_y[EM_NW][EM_D];
    __shared__ double s_xbar[EM_D], s_sdv[EM_D], s_red[EM_NW];
    __shared__ int s_bad;
    const int slot = act[blockIdx.x], item = first_item + slot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int g = in.item_group[item];
    const int32_t *days = in.gdays + in.goff[g];
    const int nrows = in.goff[g + 1] - in.goff[g];
    int nst;
    const int P = em_ncols(in, item, &nst);
    const int64_t ro = ws_row_off[slot];
    const int32_t *perm = ws_perm + ro, *runs = ws_runs + ro + slot;
    const int nruns = ws_nruns[slot];
    double *theta_g = ws_theta + (int64_t)slot * EM_D * EM_D;
    for (int e = tid; e < EM_D * EM_D; e += EM_THREADS) s_theta[e] = theta_g[e];
    if (tid < EM_D) {
        s_xbar[tid] = ws_stat[(int64_t)slot * 2 * EM_D + tid];
        s_sdv[tid] = ws_stat[(int64_t)slot * 2 * EM_D + EM_D + tid];
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const bool isvar = j >= 1 && j <= P;
    EmCol col = {nullptr, nullptr};
    if (isvar) col = em_column(in, item, j - 1, nst);
    const double xbar = s_xbar[j], sdv = s_sdv[j];
    const unsigned colmask = (unsigned)((1ull << (P + 1)) - 2ull);   // bits 1 .. P
    const double dn = (double)nrows;
    double *W = s_w[wave], *Y = s_y[wave];
    int it = iters[item];
    int state = -1;                                              // -1: running; else the final status
    double dl = 0.0;

    for (int step = 0; step < iters_per_launch && state < 0; ++step) {
        double T[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) T[t] = 0.0;
        bool bad = false;
        for (int run = wave; run < nruns && !bad; run += EM_NW) {
            const int r0 = runs[run], r1 = runs[run + 1];
            // the run's mask: the finite columns of its first row
            double x;
            {
                const int r = perm[r0];
                x = col.pf ? (double)col.pf[days[r]] : (col.pd ? col.pd[r] : NAN);
            }
            const unsigned mask = (unsigned)(__ballot(lane < 32 && isvar && em_finite(x)) & 0xffffffffull);
            const unsigned miss = ~mask & colmask;
            double Wr[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                Wr[t] = s_theta[(h + 2 * t) * EM_D + j];
                W[(h + 2 * t) * EM_D + j] = Wr[t];
            }
            wave_sync();
            for (unsigned m = mask; m != 0u; m &= m - 1u) {
                const int k = __ffs(m) - 1;
                const double d = W[k * EM_D + k];
                if (!(d > 0.0) || !em_finite(d)) { bad = true; break; }
                const double rinv = 1.0 / d;
                const double cj = W[k * EM_D + j];
                double ci[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) ci[t] = W[(h + 2 * t) * EM_D + k];
                wave_sync();
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int i = h + 2 * t;
                    double v = Wr[t] - (ci[t] * cj) * rinv;
                    if (i == k) v = cj * rinv;
                    if (j == k) v = ci[t] * rinv;
                    if (i == k && j == k) v = -rinv;
                    Wr[t] = v;
                    W[i * EM_D + j] = v;
                }
                wave_sync();
            }
            if (bad) break;
            for (int q = r0; q < r1; ++q) {
                if (q > r0) {
                    const int r = perm[q];
                    x = col.pf ? (double)col.pf[days[r]] : (col.pd ? col.pd[r] : NAN);
                }
                double y = 0.0;
                if (j == 0) y = 1.0;
                else if ((mask >> j) & 1u) y = (x - xbar) / sdv;
                if (lane < 32) Y[j] = y;
                wave_sync();
                if (miss != 0u) {
                    double acc = W[j];
                    for (unsigned m = mask; m != 0u; m &= m - 1u) {
                        const int o = __ffs(m) - 1;
                        acc = acc + W[o * EM_D + j] * Y[o];
                    }
                    if ((miss >> j) & 1u) {
                        y = acc;
                        if (lane < 32) Y[j] = y;
                    }
                    wave_sync();
                }
#pragma unroll
                for (int t = 0; t < 16; ++t) T[t] = T[t] + Y[h + 2 * t] * y;
                wave_sync();
            }
            if (miss != 0u) {
                const double cntr = (double)(r1 - r0);
#pragma unroll
                for (int t = 0; t < 16; ++t)
                    if (((miss >> j) & 1u) && ((miss >> (h + 2 * t)) & 1u)) T[t] = T[t] + cntr * Wr[t];
            }
        }
        if (bad) s_bad = 1;
#pragma unroll
        for (int t = 0; t < 16; ++t) W[(h + 2 * t) * EM_D + j] = T[t];
        __syncthreads();
        if (s_bad) { state = TWXEM_NUMERIC; break; }
        // the partial Ts in wavefront order
        for (int e = tid; e < EM_D * EM_D; e += EM_THREADS) {
            double s = s_w[0][e];
#pragma unroll
            for (int w = 1; w < EM_NW; ++w) s = s + s_w[w][e];
            s_w[0][e] = s;
        }
        __syncthreads();
        double dmax = 0.0;
        for (int e = tid; e < EM_D * EM_D; e += EM_THREADS) {
            const int i = e >> 5, jj = e & 31;
            double v;
            if (e == 0) v = -1.0;
            else if (i == 0) v = s_w[0][jj] / dn;
            else if (jj == 0) v = s_w[0][i] / dn;
            else v = s_w[0][e] / dn - (s_w[0][i] / dn) * (s_w[0][jj] / dn);
            double ch = fabs(v - s_theta[e]);
            if (ch != ch) ch = INFINITY;
            dmax = fmax(dmax, ch);
            s_theta[e] = v;
        }
        dmax = qa_wave_max(dmax);
        if (lane == 0) s_red[wave] = dmax;
        __syncthreads();
        dl = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
        ++it;
        if (dl <= criterion) state = TWXEM_OK;
        else if (it >= maxits) state = TWXEM_MAXITS;
        __syncthreads();                                         // s_red and s_w are written again in the next iteration
    }

    if (state == TWXEM_NUMERIC) {
        if (tid == 0) {
            done[item] = 1; status[item] = TWXEM_NUMERIC; iters[item] = it;
            delta[item] = NAN; mean[item] = NAN; variance[item] = NAN;
        }
        return;                                                  // mu_out / sigma_out keep the NaN the host filled them with
    }
    for (int e = tid; e < EM_D * EM_D; e += EM_THREADS) theta_g[e] = s_theta[e];
    if (tid == 0) { iters[item] = it; delta[item] = dl; }
    if (state < 0) return;
    if (tid == 0) {
        done[item] = 1; status[item] = state;
        mean[item] = s_theta[1] * s_sdv[1] + s_xbar[1];
        variance[item] = s_theta[EM_D + 1] * s_sdv[1] * s_sdv[1];
    }
    if (mu_out) {
        const int C = TWXEM_MAX_COLS;
        for (int e = tid; e < EM_D * EM_D; e += EM_THREADS) {
            const int i = e >> 5, jj = e & 31;
            if (jj < 1 || jj > P || i > P) continue;
            if (i == 0) mu_out[(int64_t)item * C + jj - 1] = s_theta[jj] * s_sdv[jj] + s_xbar[jj];
            else sigma_out[((int64_t)item * C + i - 1) * C + jj - 1] = s_theta[e] * s_sdv[i] * s_sdv[jj];
        }
    }
}

extern "C" int twxem_mean_variance(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t ngroups,
                                   const int8_t *group, int64_t nitem, const int32_t *item_target,
                                   const int32_t *item_group, const int32_t *item_matrix_status, const int64_t *col_off,
                                   const int32_t *col_idx, int64_t nset, const int32_t *set_group, const int32_t *set_ncol,
                                   const double *set_vals, const int32_t *item_set, double criterion, int32_t maxits,
                                   int32_t iters_per_launch, int64_t workspace_bytes, double *mean, double *variance,
                                   int32_t *iters, double *delta, int32_t *status, double *mu, double *sigma,
                                   int32_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxem_mean_variance";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || nitem < 1 || nstn > INT32_MAX || ndays > INT32_MAX || nitem > INT32_MAX / 2 ||
        ngroups < 1 || ngroups > 127 || nset < 0 || nset > INT32_MAX) {
        snprintf(msg, sizeof msg, "%s: need nstn, ndays, nitem >= 1, 1 <= ngroups <= 127 and nset >= 0", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!obs || !group || !item_target || !item_group || !col_off || !mean || !variance || !iters || !delta || !status ||
        (nset > 0 && (!set_group || !set_ncol || !set_vals || !item_set)) || ((mu == nullptr) != (sigma == nullptr))) {
        snprintf(msg, sizeof msg, "%s: null buffer (mu and sigma go together)", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!(criterion > 0.0) || !std::isfinite(criterion) || maxits < 1) {
        snprintf(msg, sizeof msg, "%s: criterion and maxits must be positive (defaults: TWXEM_DEFAULT_CRITERION, TWXEM_DEFAULT_MAXITS)", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (iters_per_launch <= 0) iters_per_launch = TWXEM_ITERS_PER_LAUNCH;
    if (workspace_bytes <= 0) workspace_bytes = TWXEM_WORKSPACE_BYTES;
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
        if (set_group[s] < 0 || set_group[s] >= ngroups || set_ncol[s] < 0 || set_ncol[s] > TWXEM_MAX_COLS) {
            snprintf(msg, sizeof msg, "%s: extra-column set %lld: group %d, %d columns (at most TWXEM_MAX_COLS = %d in all)",
                     fn, (long long)s, (int)set_group[s], (int)set_ncol[s], TWXEM_MAX_COLS);
            return qa_fail(errbuf, errlen, msg);
        }
        const int64_t rows = goff[(size_t)set_group[s] + 1] - goff[(size_t)set_group[s]];
        set_off[(size_t)s + 1] = set_off[(size_t)s] + rows * set_ncol[s];
    }
    const size_t NI = (size_t)nitem;
    std::vector<int32_t> h_status(NI, TWXEM_OK), h_iset(NI, -1);
    std::vector<uint8_t> h_done(NI, 0);
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
        const int64_t ncol = 1 + (col_off[i + 1] - col_off[i]) + (s >= 0 ? set_ncol[s] : 0);
        if (ncol > TWXEM_MAX_COLS) {
            snprintf(msg, sizeof msg, "%s: item %lld has %lld columns, TWXEM_MAX_COLS is %d", fn, (long long)i,
                     (long long)ncol, TWXEM_MAX_COLS);
            return qa_fail(errbuf, errlen, msg);
        }
        for (int64_t c = col_off[i]; c < col_off[i + 1]; ++c)
            if (col_idx[c] < 0 || col_idx[c] >= nstn) {
                snprintf(msg, sizeof msg, "%s: item %lld: column index %d outside [0, %lld)", fn, (long long)i,
                         (int)col_idx[c], (long long)nstn);
                return qa_fail(errbuf, errlen, msg);
            }
        const int64_t rows = goff[(size_t)item_group[i] + 1] - goff[(size_t)item_group[i]];
        if (item_matrix_status && item_matrix_status[i] != TWXIF_OK) { h_status[(size_t)i] = TWXEM_NO_MATRIX; h_done[(size_t)i] = 1; }
        else if (rows > TWXEM_MAX_ROWS) { h_status[(size_t)i] = TWXEM_ROW_CAP; h_done[(size_t)i] = 1; }
    }
    const int64_t ncolidx = col_off[nitem];

    QACHK(hipSetDevice(device));
    const auto t_up = std::chrono::steady_clock::now();
    QaPool bufs;
    float *d_obs;
    int32_t *d_gdays, *d_goff, *d_itarget, *d_igroup, *d_iset, *d_colidx, *d_setncol, *d_iters, *d_status;
    int64_t *d_coloff, *d_setoff;
    double *d_setvals, *d_mean, *d_var, *d_delta, *d_mu = nullptr, *d_sigma = nullptr;
    uint8_t *d_done;
    const size_t NS = (size_t)nstn, ND = (size_t)ndays, G = (size_t)ngroups, NSET = (size_t)nset;
    const size_t C = TWXEM_MAX_COLS;
    QAALLOC(bufs, d_obs, float, NS * ND);
    QAALLOC(bufs, d_gdays, int32_t, gdays.size()); QAALLOC(bufs, d_goff, int32_t, G + 1);
    QAALLOC(bufs, d_itarget, int32_t, NI); QAALLOC(bufs, d_igroup, int32_t, NI); QAALLOC(bufs, d_iset, int32_t, NI);
    QAALLOC(bufs, d_coloff, int64_t, NI + 1); QAALLOC(bufs, d_colidx, int32_t, ncolidx);
    QAALLOC(bufs, d_setncol, int32_t, NSET); QAALLOC(bufs, d_setoff, int64_t, NSET + 1);
    QAALLOC(bufs, d_setvals, double, set_off[NSET]);
    QAALLOC(bufs, d_iters, int32_t, NI); QAALLOC(bufs, d_status, int32_t, NI); QAALLOC(bufs, d_done, uint8_t, NI);
    QAALLOC(bufs, d_mean, double, NI); QAALLOC(bufs, d_var, double, NI); QAALLOC(bufs, d_delta, double, NI);
    QAUP_NZ(d_obs, obs, float, NS * ND);
    QAUP_NZ(d_gdays, gdays.data(), int32_t, gdays.size());
    QAUP_NZ(d_goff, goff.data(), int32_t, G + 1);
    QAUP_NZ(d_itarget, item_target, int32_t, NI);
    QAUP_NZ(d_igroup, item_group, int32_t, NI);
    QAUP_NZ(d_iset, h_iset.data(), int32_t, NI);
    QAUP_NZ(d_coloff, col_off, int64_t, NI + 1);
    QAUP_NZ(d_colidx, col_idx, int32_t, ncolidx);
    QAUP_NZ(d_setncol, set_ncol, int32_t, NSET);
    QAUP_NZ(d_setoff, set_off.data(), int64_t, NSET + 1);
    QAUP_NZ(d_setvals, set_vals, double, set_off[NSET]);
    QAUP_NZ(d_status, h_status.data(), int32_t, NI);
    QAUP_NZ(d_done, h_done.data(), uint8_t, NI);
    QACHK(hipMemset(d_iters, 0, NI * 4));
    QACHK(hipMemset(d_mean, 0xff, NI * 8));                      // all bits set: a NaN
    QACHK(hipMemset(d_var, 0xff, NI * 8));
    QACHK(hipMemset(d_delta, 0xff, NI * 8));
    if (mu) {
        QAALLOC(bufs, d_mu, double, NI * C); QAALLOC(bufs, d_sigma, double, NI * C * C);
        QACHK(hipMemset(d_mu, 0xff, NI * C * 8));
        QACHK(hipMemset(d_sigma, 0xff, NI * C * C * 8));
    }
    EmIn in = {d_obs, ndays, d_gdays, d_goff, d_itarget, d_igroup, d_iset, d_coloff, d_colidx, d_setncol, d_setoff, d_setvals};

    QaTimer tm;
    float ms[TWXEM_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) {
        QACHK(tm.init());
        QACHK(hipDeviceSynchronize());
        ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    }
    // batches of consecutive items under the workspace budget (at least one item each)
    const int64_t fixed = (int64_t)(EM_D * EM_D + 2 * EM_D) * 8 + 8 + 4 + 4 + 4;
    int rounds = 0, nbatches = 0;
    std::vector<int64_t> row_off;
    std::vector<int32_t> act;
    std::vector<uint8_t> bdone;
    for (int64_t first = 0; first < nitem;) {
        row_off.clear();
        int64_t rows_total = 0, bytes = 0, last = first;
        for (; last < nitem; ++last) {
            const int64_t rows = h_done[(size_t)last] ? 0 : goff[(size_t)item_group[last] + 1] - goff[(size_t)item_group[last]];
            const int64_t need = fixed + rows * 8;
            if (last > first && bytes + need > workspace_bytes) break;
            row_off.push_back(rows_total);
            rows_total += rows;
            bytes += need;
        }
        const size_t NB = (size_t)(last - first);
        ++nbatches;
        QaPool ws;                                               // freed at the end of the batch
        int64_t *w_rowoff;
        int32_t *w_perm, *w_runs, *w_nruns, *w_act;
        double *w_stat, *w_theta;
        QAALLOC(ws, w_rowoff, int64_t, NB); QAALLOC(ws, w_perm, int32_t, rows_total);
        QAALLOC(ws, w_runs, int32_t, (size_t)rows_total + NB); QAALLOC(ws, w_nruns, int32_t, NB); QAALLOC(ws, w_act, int32_t, NB);
        QAALLOC(ws, w_stat, double, NB * 2 * EM_D); QAALLOC(ws, w_theta, double, NB * EM_D * EM_D);
        QAUP_NZ(w_rowoff, row_off.data(), int64_t, NB);
        QACHK(hipMemset(w_nruns, 0, NB * 4));
        if (kernel_ms) QACHK(tm.start());
        hipLaunchKernelGGL(k_em_prep, dim3((unsigned)NB), dim3(256), 0, nullptr, in, (int)first, (const int64_t *)w_rowoff,
                           w_perm, w_runs, w_nruns, w_stat, w_theta, d_done, d_status);
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
            hipLaunchKernelGGL(k_em_iter, dim3((unsigned)act.size()), dim3(EM_THREADS), 0, nullptr, in, (int)first,
                               (const int32_t *)w_act, (const int64_t *)w_rowoff, (const int32_t *)w_perm,
                               (const int32_t *)w_runs, (const int32_t *)w_nruns, (const double *)w_stat, w_theta, criterion,
                               (int)maxits, (int)iters_per_launch, d_done, d_status, d_iters, d_delta, d_mean, d_var, d_mu,
                               d_sigma);
            QACHK(hipGetLastError());
            if (kernel_ms) QACHK(tm.stop_add(&ms[1]));
            ++rounds;
        }
        first = last;
    }
    const auto t_down = std::chrono::steady_clock::now();
    QACHK(hipMemcpy(mean, d_mean, NI * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(variance, d_var, NI * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(delta, d_delta, NI * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(iters, d_iters, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(status, d_status, NI * 4, hipMemcpyDeviceToHost));
    if (mu) {
        QACHK(hipMemcpy(mu, d_mu, NI * C * 8, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(sigma, d_sigma, NI * C * C * 8, hipMemcpyDeviceToHost));
    }
    ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    if (counts) { counts[0] = rounds; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
