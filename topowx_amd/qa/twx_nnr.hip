// twx_nnr.hip -- libtwxqa.so: the principal components of the reanalysis columns of the infill family (pca_svd of
// twx/utils/pca.py:26-76 as _InfillMatrix.infill calls it, twx/infill/infill_normals.py:347-356, and its step16
// counterpart), as include/twx_qa.h states it, for every (column set, day group) item of one call (twxnr_components).
// Its own translation unit; the wave sum, the buffer list and the event timer it shares with the other units are
// twx_qa_common.h's.
//
// The route is the eigen-decomposition of the P x P Gram matrix of the standardised columns, not an SVD of the N x P
// matrix: N x P float64 (2200 x 32 in the reference's shape) does not fit in LDS, P x P does.  The price is accuracy in
// the components of small variance, which the cuts discard.
//
// k_nr_gram    one workgroup of 256 (4 wavefronts) per item.  Wavefront w owns the columns j = w, w + 4, ..: a lane adds
//              its days lane, lane + 64, .. in ascending order, the 64 lanes meet in a butterfly; the mean first, then the
//              centred sum of squares (two passes: hgt is ~5500 with a spread of ~100, raw moments would cancel).  Then the
//              Gram matrix over tiles of 64 days: the standardised tile goes to LDS (column-major, row stride 65 doubles),
//              thread (tj, tk) of a 16 x 16 grid owns the B x B block of entries at (tj B, tk B) (B = 2 for P <= 32, else
//              4) and adds the days of the tile in day order.  Every entry is ONE thread's sum over the days in ascending
//              order, so the matrix is symmetric to the bit and two calls give the same bytes.  Nothing row-sized lives
//              in LDS, so there is no row cap.
//              LDS: tile 64 x 65 x 8 B = 33 280 B + mean / sd 2 x 64 x 8 B + the column verdicts 64 x 4 B = 34 560 B.
// k_nr_eig     one wavefront per item.  Cyclic Jacobi on the Gram matrix A in LDS with the rotation accumulator V, round-
//              robin (circle method) pair order: step t of a sweep rotates the m / 2 disjoint pairs ((t + k) mod (m - 1),
//              (t - k) mod (m - 1)), k = 1 .., and (t, m - 1), m = P rounded up to even (a pair with the padding index is
//              skipped).  Lane k forms the rotation of pair k; the lanes share the columns of A and V, then the rows of
//              A; the rotated entry is set to 0.  The order is fixed.  A sweep starts only while the off-diagonal norm is
//              above eps x trace; after TWXNR_MAX_SWEEPS the item is TWXNR_NOCONV.
//              LDS: A and V, 2 x P x P x 8 B for the largest P of the call: 64 KiB at the cap, 16 KiB at P = 32; the
//              rotations, the order and the cuts travel in registers (shuffles), no other LDS.
// k_nr_scores  one workgroup of 256 per item that keeps a component, a lane per day; the leading loadings in LDS; eight
//              components at a time, each the sum over the columns in ascending order.
//              LDS: loadings 64 x 64 x 8 B = 32 KiB + mean / sd 1 KiB = 33 792 B.
// fp64 throughout on the float32 columns widened exactly; the library is built with -ffp-contract=off; no float atomics.
// Every loop is bounded by the rows of an item, by P or by TWXNR_MAX_SWEEPS; nothing waits on another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define NR_NW 4                              // wavefronts of a workgroup of k_nr_gram / k_nr_scores
#define NR_THREADS (64 * NR_NW)
#define NR_TILE 64                           // days of a Gram tile
#define NR_TS (NR_TILE + 1)                  // row stride of the tile in LDS
#define NR_KB 8                              // components of one pass of k_nr_scores
#define NR_DBL_MAX 1.7976931348623157e308
#define NR_EPS 2.220446049250313e-16

namespace {

__device__ __forceinline__ bool nr_finite(double v) { return fabs(v) <= NR_DBL_MAX; }

struct NrTab {                               // the items of a call: item = set * ngroups + group
    const float *cols;                       // [ncol][ndays]
    const int32_t *set_off, *set_col;        // [nset + 1], columns of the sets
    const int64_t *sq_off;                   // [nset + 1]: sum of P^2 over the sets before
    const int32_t *grp_off, *grp_day;        // [ngroups + 1], day indices of the groups in day order
    int64_t ndays;
    int32_t ngroups;
};

// the B x B blocks of the Gram matrix over the tiles of 64 days; tile, s_mean, s_sd in LDS
template <int B>
__device__ __forceinline__ void nr_gram_blocks(const NrTab &t, int c0, int P, int r0, int n, double *tile,
                                               const double *s_mean, const double *s_sd, double *gram)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = (tid >> 4) * B, k0 = (tid & 15) * B;
    const int PP = (P + B - 1) / B * B;                          // <= 16 B
    const bool active = j0 < P && k0 < P;
    double acc[B][B];
#pragma unroll
    for (int a = 0; a < B; ++a)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[a][b] = 0.0;
    for (int t0 = 0; t0 < n; t0 += NR_TILE) {
        __syncthreads();                                         // the previous tile has been read
        for (int j = w; j < PP; j += NR_NW) {
            const int r = t0 + lane;
            double z = 0.0;
            if (j < P && r < n) {
                const float *x = t.cols + (int64_t)t.set_col[c0 + j] * t.ndays;
                z = ((double)x[t.grp_day[r0 + r]] - s_mean[j]) / s_sd[j];
            }
            tile[j * NR_TS + lane] = z;
        }
        __syncthreads();
        const int rows = n - t0 < NR_TILE ? n - t0 : NR_TILE;
        if (active) {
            for (int r = 0; r < rows; ++r) {
                double za[B], zb[B];
#pragma unroll
                for (int a = 0; a < B; ++a) { za[a] = tile[(j0 + a) * NR_TS + r]; zb[a] = tile[(k0 + a) * NR_TS + r]; }
#pragma unroll
                for (int a = 0; a < B; ++a)
#pragma unroll
                    for (int b = 0; b < B; ++b) acc[a][b] = acc[a][b] + za[a] * zb[b];
            }
        }
    }
    if (active) {
        const double den = (double)(n - 1);
#pragma unroll
        for (int a = 0; a < B; ++a)
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (j0 + a < P && k0 + b < P) gram[(j0 + a) * P + (k0 + b)] = acc[a][b] / den;
    }
}

}  // namespace

// mean_sd [2][sum of P x ngroups]: the mean and the standard deviation (ddof = 1) of every column of every item;
// gram: the items' P x P matrices, item (s, g) at ngroups sq_off[s] + g P^2; status / bad_col [nitem]
__global__ __launch_bounds__(NR_THREADS) void k_nr_gram(NrTab t, int64_t ms_total, double *__restrict__ mean_sd,
                                                        double *__restrict__ gram_all, int32_t *__restrict__ status,
                                                        int32_t *__restrict__ bad_col)
{
    __shared__ double tile[NR_TILE * NR_TS];
    __shared__ double s_mean[TWXNR_MAX_COLS], s_sd[TWXNR_MAX_COLS];
    __shared__ int32_t s_bad[TWXNR_MAX_COLS];
    const int item = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = item / t.ngroups, g = item % t.ngroups;
    const int c0 = t.set_off[s], P = t.set_off[s + 1] - c0;      // 1 .. TWXNR_MAX_COLS (checked by the entry)
    const int r0 = t.grp_off[g], n = t.grp_off[g + 1] - r0;
    const int64_t po = (int64_t)t.ngroups * c0 + (int64_t)g * P;
    const int64_t qo = (int64_t)t.ngroups * t.sq_off[s] + (int64_t)g * P * P;
    if (n < 2) {                                                 // uniform over the workgroup
        if (tid == 0) { status[item] = TWXNR_FEW_ROWS; bad_col[item] = -1; }
        return;
    }
    for (int j = w; j < P; j += NR_NW) {
        const float *x = t.cols + (int64_t)t.set_col[c0 + j] * t.ndays;
        double sum = 0.0, nbad = 0.0;
        for (int r = lane; r < n; r += 64) {
            const double v = (double)x[t.grp_day[r0 + r]];
            if (!nr_finite(v)) nbad = nbad + 1.0;
            sum = sum + v;
        }
        sum = qa_wave_sum(sum);
        nbad = qa_wave_sum(nbad);
        const double mean = sum / (double)n;
        double ss = 0.0;
        for (int r = lane; r < n; r += 64) {
            const double d = (double)x[t.grp_day[r0 + r]] - mean;
            ss = ss + d * d;
        }
        ss = qa_wave_sum(ss);
        const double sd = sqrt(ss / (double)(n - 1));
        if (lane == 0) {
            s_mean[j] = mean;
            s_sd[j] = sd;
            s_bad[j] = nbad > 0.0 ? 1 : (sd > 0.0 ? 0 : 2);
            mean_sd[po + j] = mean;
            mean_sd[ms_total + po + j] = sd;
        }
    }
    __syncthreads();
    int bad = -1, kind = 0;                                      // the first non-finite column, else the first constant one
    for (int j = 0; j < P; ++j)
        if (s_bad[j] == 1) { bad = j; kind = 1; break; }
    if (bad < 0)
        for (int j = 0; j < P; ++j)
            if (s_bad[j] == 2) { bad = j; kind = 2; break; }
    if (bad >= 0) {                                              // uniform: every thread reads the same verdicts
        if (tid == 0) { status[item] = kind == 1 ? TWXNR_NONFINITE : TWXNR_CONSTANT; bad_col[item] = bad; }
        return;
    }
    if (P <= 32) nr_gram_blocks<2>(t, c0, P, r0, n, tile, s_mean, s_sd, gram_all + qo);
    else nr_gram_blocks<4>(t, c0, P, r0, n, tile, s_mean, s_sd, gram_all + qo);
    if (tid == 0) { status[item] = TWXNR_OK; bad_col[item] = -1; }
}

// var_explain / eigval at the offsets of mean_sd, loadings at those of gram: component k of an item is the row
// loadings[k P .. k P + P - 1]; ncomp [nitem][nthr]; sweeps [nitem]
__global__ __launch_bounds__(64) void k_nr_eig(NrTab t, int32_t pmax, const double *__restrict__ gram_all, int32_t nthr,
                                               const double *__restrict__ max_var, int32_t *__restrict__ status,
                                               int32_t *__restrict__ ncomp, int32_t *__restrict__ sweeps,
                                               double *__restrict__ var_explain, double *__restrict__ eigval,
                                               double *__restrict__ loadings)
{
    extern __shared__ double nr_lds[];
    double *A = nr_lds, *V = nr_lds + (size_t)pmax * pmax;       // stride P of the item, P <= pmax
    const int item = blockIdx.x, lane = threadIdx.x;
    const int s = item / t.ngroups, g = item % t.ngroups;
    const int c0 = t.set_off[s], P = t.set_off[s + 1] - c0;
    const int64_t po = (int64_t)t.ngroups * c0 + (int64_t)g * P;
    const int64_t qo = (int64_t)t.ngroups * t.sq_off[s] + (int64_t)g * P * P;
    if (status[item] != TWXNR_OK) {                              // uniform
        if (lane == 0) {
            sweeps[item] = 0;
            for (int v = 0; v < nthr; ++v) ncomp[item * nthr + v] = 0;
        }
        return;
    }
    const int PP2 = P * P;
    for (int x = lane; x < PP2; x += 64) {
        A[x] = gram_all[qo + x];
        V[x] = (x / P == x % P) ? 1.0 : 0.0;
    }
    __syncthreads();
    double trace = 0.0;
    for (int j = 0; j < P; ++j) trace = trace + A[j * P + j];
    const double tol2 = (NR_EPS * trace) * (NR_EPS * trace);
    const int m = P + (P & 1), npair = m >> 1;
    int nsweep = 0;
    bool conv = false;
    for (;;) {
        double off2 = 0.0;
        for (int x = lane; x < PP2; x += 64)
            if (x / P != x % P) off2 = off2 + A[x] * A[x];
        off2 = qa_wave_sum(off2);                                // the same in every lane
        if (off2 <= tol2) { conv = true; break; }
        if (nsweep == TWXNR_MAX_SWEEPS) break;
        ++nsweep;
        for (int step = 0; step < m - 1; ++step) {
            // lane k: the rotation of pair k (Rutishauser's formulas: the smaller root of t^2 + 2 theta t - 1 = 0)
            int p = 0, q = -1;
            double c = 1.0, sn = 0.0;
            if (lane < npair) {
                int a, b;
                if (lane == 0) { a = step % (m - 1); b = m - 1; }
                else { a = (step + lane) % (m - 1); b = (step - lane + (m - 1)) % (m - 1); }
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                if (hi < P) {
                    const double apq = A[lo * P + hi];
                    if (apq != 0.0) {
                        const double theta = (A[hi * P + hi] - A[lo * P + lo]) / (2.0 * apq);
                        const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        sn = tt * c;
                        p = lo; q = hi;
                    }
                }
            }
            __syncthreads();                                     // every rotation has been formed from the old A
            const int nwork = npair * P;
            for (int x0 = 0; x0 < nwork; x0 += 64) {             // columns p, q of A and V; every lane shuffles
                const int x = x0 + lane;
                const int k = x < nwork ? x / P : 0, i = x % P;
                const int kp = __shfl(p, k, 64), kq = __shfl(q, k, 64);
                const double kc = __shfl(c, k, 64), ks = __shfl(sn, k, 64);
                if (x < nwork && kq >= 0) {
                    double u = A[i * P + kp], v = A[i * P + kq];
                    A[i * P + kp] = kc * u - ks * v;
                    A[i * P + kq] = ks * u + kc * v;
                    u = V[i * P + kp]; v = V[i * P + kq];
                    V[i * P + kp] = kc * u - ks * v;
                    V[i * P + kq] = ks * u + kc * v;
                }
            }
            __syncthreads();
            for (int x0 = 0; x0 < nwork; x0 += 64) {             // rows p, q of A
                const int x = x0 + lane;
                const int k = x < nwork ? x / P : 0, i = x % P;
                const int kp = __shfl(p, k, 64), kq = __shfl(q, k, 64);
                const double kc = __shfl(c, k, 64), ks = __shfl(sn, k, 64);
                if (x < nwork && kq >= 0) {
                    const double u = A[kp * P + i], v = A[kq * P + i];
                    A[kp * P + i] = kc * u - ks * v;
                    A[kq * P + i] = ks * u + kc * v;
                }
            }
            __syncthreads();
            if (q >= 0) { A[p * P + q] = 0.0; A[q * P + p] = 0.0; }
            __syncthreads();
        }
    }
    // eigenvalues descending, ties by index; lane k ends with component k
    const double lam = lane < P ? A[lane * P + lane] : 0.0;
    int rank = 0;
    for (int i = 0; i < P; ++i) {
        const double li = __shfl(lam, i, 64);
        if (li > lam || (li == lam && i < lane)) ++rank;
    }
    int mine = 0;                                                // the column of V that is component `lane`
    for (int i = 0; i < P; ++i) {
        const int ri = __shfl(rank, i, 64);
        if (ri == lane) mine = i;
    }
    const double lamk = __shfl(lam, mine, 64);
    double total = 0.0;
    for (int k = 0; k < P; ++k) total = total + __shfl(lamk, k, 64);
    const double ve = lamk / total;
    if (lane < P) {
        var_explain[po + lane] = ve;
        eigval[po + lane] = lamk;
        double big = -1.0, sign = 1.0;                           // the largest-magnitude loading (the first on a tie) positive
        for (int j = 0; j < P; ++j) {
            const double v = V[j * P + mine];
            if (fabs(v) > big) { big = fabs(v); sign = v < 0.0 ? -1.0 : 1.0; }
        }
        for (int j = 0; j < P; ++j) loadings[qo + (int64_t)lane * P + j] = sign * V[j * P + mine];
    }
    for (int v = 0; v < nthr; ++v) {
        const double mv = max_var[v];
        double cum = 0.0;
        int nc = P;                                              // never reached (rounding at a cut near 1): every component
        for (int k = 0; k < P; ++k) {
            cum = cum + __shfl(ve, k, 64);
            if (cum >= mv) { nc = k + 1; break; }                // uniform: every lane adds the same values
        }
        if (lane == 0) ncomp[item * nthr + v] = nc;
    }
    if (lane == 0) {
        sweeps[item] = nsweep;
        status[item] = conv ? TWXNR_OK : TWXNR_NOCONV;
    }
}

// keep [nitem]: the leading components whose scores are formed; score_off [nitem + 1]; the scores of an item are
// keep[item] columns of n days each, column after column
__global__ __launch_bounds__(NR_THREADS) void k_nr_scores(NrTab t, int64_t ms_total, const double *__restrict__ mean_sd,
                                                          const double *__restrict__ loadings,
                                                          const int32_t *__restrict__ keep,
                                                          const int64_t *__restrict__ score_off, double *__restrict__ scores)
{
    __shared__ double s_load[TWXNR_MAX_COLS * TWXNR_MAX_COLS];
    __shared__ double s_mean[TWXNR_MAX_COLS], s_sd[TWXNR_MAX_COLS];
    const int item = blockIdx.x, tid = threadIdx.x;
    const int kk = keep[item];
    if (kk <= 0) return;                                         // uniform
    const int s = item / t.ngroups, g = item % t.ngroups;
    const int c0 = t.set_off[s], P = t.set_off[s + 1] - c0;
    const int r0 = t.grp_off[g], n = t.grp_off[g + 1] - r0;
    const int64_t po = (int64_t)t.ngroups * c0 + (int64_t)g * P;
    const int64_t qo = (int64_t)t.ngroups * t.sq_off[s] + (int64_t)g * P * P;
    for (int x = tid; x < kk * P; x += NR_THREADS) s_load[x] = loadings[qo + x];         // kk <= P <= 64
    if (tid < P) { s_mean[tid] = mean_sd[po + tid]; s_sd[tid] = mean_sd[ms_total + po + tid]; }
    __syncthreads();
    double *out = scores + score_off[item];
    for (int r = tid; r < n; r += NR_THREADS) {
        const int64_t day = t.grp_day[r0 + r];
        for (int kc = 0; kc < kk; kc += NR_KB) {
            double acc[NR_KB];
#pragma unroll
            for (int a = 0; a < NR_KB; ++a) acc[a] = 0.0;
            for (int j = 0; j < P; ++j) {
                const double z = ((double)t.cols[(int64_t)t.set_col[c0 + j] * t.ndays + day] - s_mean[j]) / s_sd[j];
#pragma unroll
                for (int a = 0; a < NR_KB; ++a)
                    if (kc + a < kk) acc[a] = acc[a] + z * s_load[(kc + a) * P + j];
            }
#pragma unroll
            for (int a = 0; a < NR_KB; ++a)
                if (kc + a < kk) out[(int64_t)(kc + a) * n + r] = acc[a];
        }
    }
}

#define NRBAD(...)                                                                      \
    do {                                                                                \
        snprintf(msg, sizeof msg, __VA_ARGS__);                                         \
        return qa_fail(errbuf, errlen, msg);                                            \
    } while (0)

extern "C" int twxnr_components(int device, int64_t ndays, int64_t ncol, const float *cols, int64_t nset,
                                const int64_t *set_off, const int32_t *set_col, int32_t ngroups, const int8_t *group,
                                int32_t nthr, const double *max_var, int32_t *status, int32_t *bad_col, int32_t *ncomp,
                                int32_t *sweeps, double *mean, double *sd, double *var_explain, double *eigval,
                                double *loadings, int64_t *score_off, int64_t score_cap, double *scores,
                                float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxnr_components";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (ndays < 1 || ndays > INT32_MAX || ncol < 1 || ncol > INT32_MAX || nset < 1 || nset > (1 << 20))
        NRBAD("%s: need 1 <= ndays, ncol <= %d and 1 <= nset <= %d", fn, INT32_MAX, 1 << 20);
    if (ngroups < 1 || ngroups > TWXIF_MAX_GROUPS) NRBAD("%s: need 1 <= ngroups <= TWXIF_MAX_GROUPS (%d)", fn, TWXIF_MAX_GROUPS);
    if (nthr < 1 || nthr > TWXNR_MAX_CUTS) NRBAD("%s: need 1 <= nthr <= TWXNR_MAX_CUTS (%d)", fn, TWXNR_MAX_CUTS);
    if (!cols || !set_off || !set_col || !group || !max_var || !status || !bad_col || !ncomp || !sweeps || !mean || !sd ||
        !var_explain || !eigval || !loadings || !score_off || score_cap < 0 || (score_cap > 0 && !scores))
        NRBAD("%s: null buffer", fn);
    for (int v = 0; v < nthr; ++v)
        if (!(max_var[v] > 0.0 && max_var[v] < 1.0)) NRBAD("%s: max_var[%d] must lie in (0, 1)", fn, v);
    if (set_off[0] != 0) NRBAD("%s: set_off[0] = %lld, not 0", fn, (long long)set_off[0]);
    int pmax = 0;
    for (int64_t s = 0; s < nset; ++s) {
        const int64_t p = set_off[s + 1] - set_off[s];
        if (p < 1 || p > TWXNR_MAX_COLS)
            NRBAD("%s: set %lld has %lld columns, need 1 .. TWXNR_MAX_COLS (%d)", fn, (long long)s, (long long)p, TWXNR_MAX_COLS);
        if (p > pmax) pmax = (int)p;
    }
    const int64_t ntot = set_off[nset];
    for (int64_t x = 0; x < ntot; ++x)
        if (set_col[x] < 0 || set_col[x] >= ncol)
            NRBAD("%s: set_col[%lld] = %d outside 0 .. ncol - 1", fn, (long long)x, set_col[x]);
    std::vector<int32_t> grp_off((size_t)ngroups + 1, 0), grp_day;
    for (int64_t d = 0; d < ndays; ++d) {
        if (group[d] < -1 || group[d] >= ngroups)
            NRBAD("%s: group[%lld] = %d outside -1 .. ngroups - 1", fn, (long long)d, (int)group[d]);
        if (group[d] >= 0) ++grp_off[(size_t)group[d] + 1];
    }
    for (int g = 0; g < ngroups; ++g) grp_off[(size_t)g + 1] += grp_off[(size_t)g];
    grp_day.resize((size_t)grp_off[(size_t)ngroups]);
    {
        std::vector<int32_t> at(grp_off.begin(), grp_off.end() - 1);
        for (int64_t d = 0; d < ndays; ++d)
            if (group[d] >= 0) grp_day[(size_t)at[(size_t)group[d]]++] = (int32_t)d;
    }
    const int64_t nitem = nset * ngroups;                        // <= 2^20 x 12
    std::vector<int32_t> h_set_off((size_t)nset + 1);
    std::vector<int64_t> h_sq_off((size_t)nset + 1, 0);
    for (int64_t s = 0; s <= nset; ++s) h_set_off[(size_t)s] = (int32_t)set_off[s];      // <= 2^20 x 64
    for (int64_t s = 0; s < nset; ++s) {
        const int64_t p = set_off[s + 1] - set_off[s];
        h_sq_off[(size_t)s + 1] = h_sq_off[(size_t)s] + p * p;
    }
    const size_t NI = (size_t)nitem, MS = (size_t)(ntot * ngroups), SQ = (size_t)(h_sq_off[(size_t)nset] * ngroups);

    QACHK(hipSetDevice(device));
    float ms[TWXNR_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const auto t_up = std::chrono::steady_clock::now();
    QaPool bufs;
    NrTab tab;
    float *d_cols;
    int32_t *d_set_off, *d_set_col, *d_grp_off, *d_grp_day, *d_status, *d_bad, *d_ncomp, *d_sweeps, *d_keep;
    int64_t *d_sq_off, *d_score_off;
    double *d_max_var, *d_ms, *d_gram, *d_ve, *d_ev, *d_load, *d_scores = nullptr;
    QAALLOC(bufs, d_cols, float, (size_t)ncol * (size_t)ndays);
    QAALLOC(bufs, d_set_off, int32_t, (size_t)nset + 1); QAALLOC(bufs, d_set_col, int32_t, (size_t)ntot);
    QAALLOC(bufs, d_sq_off, int64_t, (size_t)nset + 1);
    QAALLOC(bufs, d_grp_off, int32_t, (size_t)ngroups + 1); QAALLOC(bufs, d_grp_day, int32_t, grp_day.size());
    QAALLOC(bufs, d_max_var, double, (size_t)nthr);
    QAALLOC(bufs, d_status, int32_t, NI); QAALLOC(bufs, d_bad, int32_t, NI); QAALLOC(bufs, d_sweeps, int32_t, NI);
    QAALLOC(bufs, d_keep, int32_t, NI); QAALLOC(bufs, d_ncomp, int32_t, NI * (size_t)nthr);
    QAALLOC(bufs, d_score_off, int64_t, NI + 1);
    QAALLOC(bufs, d_ms, double, 2 * MS); QAALLOC(bufs, d_ve, double, MS); QAALLOC(bufs, d_ev, double, MS);
    QAALLOC(bufs, d_gram, double, SQ); QAALLOC(bufs, d_load, double, SQ);
    QAUP_NZ(d_cols, cols, float, (size_t)ncol * (size_t)ndays);
    QAUP_NZ(d_set_off, h_set_off.data(), int32_t, (size_t)nset + 1); QAUP_NZ(d_set_col, set_col, int32_t, (size_t)ntot);
    QAUP_NZ(d_sq_off, h_sq_off.data(), int64_t, (size_t)nset + 1);
    QAUP_NZ(d_grp_off, grp_off.data(), int32_t, (size_t)ngroups + 1); QAUP_NZ(d_grp_day, grp_day.data(), int32_t, grp_day.size());
    QAUP_NZ(d_max_var, max_var, double, (size_t)nthr);
    // an item that is not decomposed leaves its slots of the packed outputs NaN
    QACHK(hipMemset(d_ms, 0xff, 2 * MS * 8)); QACHK(hipMemset(d_ve, 0xff, MS * 8)); QACHK(hipMemset(d_ev, 0xff, MS * 8));
    QACHK(hipMemset(d_load, 0xff, SQ * 8));
    tab.cols = d_cols; tab.set_off = d_set_off; tab.set_col = d_set_col; tab.sq_off = d_sq_off; tab.grp_off = d_grp_off;
    tab.grp_day = d_grp_day; tab.ndays = ndays; tab.ngroups = ngroups;
    QaTimer tm;
    if (kernel_ms) {
        QACHK(tm.init());
        QACHK(hipDeviceSynchronize());
        ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
        QACHK(tm.start());
    }
    hipLaunchKernelGGL(k_nr_gram, dim3((unsigned)NI), dim3(NR_THREADS), 0, nullptr, tab, (int64_t)MS, d_ms, d_gram, d_status,
                       d_bad);
    QACHK(hipGetLastError());
    if (kernel_ms) { QACHK(tm.stop_add(&ms[0])); QACHK(tm.start()); }
    hipLaunchKernelGGL(k_nr_eig, dim3((unsigned)NI), dim3(64), (size_t)2 * pmax * pmax * sizeof(double), nullptr, tab,
                       (int32_t)pmax, (const double *)d_gram, nthr, (const double *)d_max_var, d_status, d_ncomp, d_sweeps,
                       d_ve, d_ev, d_load);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_add(&ms[1]));
    // the host lays the scores out: per item the components of its largest cut
    QADOWN_NZ(status, d_status, int32_t, NI);
    QADOWN_NZ(ncomp, d_ncomp, int32_t, NI * (size_t)nthr);
    std::vector<int32_t> keep(NI, 0);
    score_off[0] = 0;
    for (size_t i = 0; i < NI; ++i) {
        if (status[i] == TWXNR_OK)
            for (int v = 0; v < nthr; ++v) keep[i] = ncomp[i * (size_t)nthr + v] > keep[i] ? ncomp[i * (size_t)nthr + v] : keep[i];
        const int g = (int)(i % (size_t)ngroups);
        score_off[i + 1] = score_off[i] + (int64_t)keep[i] * (grp_off[(size_t)g + 1] - grp_off[(size_t)g]);
    }
    if (score_off[NI] > score_cap)
        NRBAD("%s: the scores need %lld entries, score_cap is %lld", fn, (long long)score_off[NI], (long long)score_cap);
    if (score_off[NI] > 0) {
        QAALLOC(bufs, d_scores, double, (size_t)score_off[NI]);
        QAUP_NZ(d_keep, keep.data(), int32_t, NI);
        QAUP_NZ(d_score_off, score_off, int64_t, NI + 1);
        if (kernel_ms) QACHK(tm.start());
        hipLaunchKernelGGL(k_nr_scores, dim3((unsigned)NI), dim3(NR_THREADS), 0, nullptr, tab, (int64_t)MS,
                           (const double *)d_ms, (const double *)d_load, (const int32_t *)d_keep,
                           (const int64_t *)d_score_off, d_scores);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[2]));
    }
    QACHK(hipDeviceSynchronize());
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN_NZ(status, d_status, int32_t, NI);
    QADOWN_NZ(bad_col, d_bad, int32_t, NI);
    QADOWN_NZ(sweeps, d_sweeps, int32_t, NI);
    QADOWN_NZ(mean, d_ms, double, MS);
    QADOWN_NZ(sd, d_ms + MS, double, MS);
    QADOWN_NZ(var_explain, d_ve, double, MS);
    QADOWN_NZ(eigval, d_ev, double, MS);
    QADOWN_NZ(loadings, d_load, double, SQ);
    QADOWN_NZ(scores, d_scores, double, (size_t)score_off[NI]);
    ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_down).count();
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
