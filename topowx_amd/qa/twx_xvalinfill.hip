// twx_xvalinfill.hip -- libtwxqa.so: the two ends of step15's cross-validation of the infill (twx/infill/xval_infill.py,
// scripts/step15_mpi_xval_infill.py): which observations of a station are hidden from its own infill (twxxv_holdout,
// XvalInfill.__init__:73-86 in closed form) and how the infilled series compares with them (twxxv_score, run_xval:153-154
// with the writer's np.ma arithmetic, step15:127-134).  The chain between them is the library's own: twxxv_infill_matrix
// (twx_infillmat.hip), twxem_mean_variance, twxpp_ppca_fit, twxck_infill_check.  Its own translation unit; the helpers it
// shares with the other units of the library (the buffer list, the event timer) are twx_qa_common.h's.
//
// k_xv_holdout: one wavefront per row, walked from the last day backwards in chunks of 64.  The reference keeps the last
// nkeep finite days (np.nonzero(fin)[0][-nkeep:]) and hides every other finite day: day d is held iff it is finite and at
// least nkeep finite days lie after it.  A ballot of "finite" and a popcount of the lanes above give the finite days after
// d within the chunk, the count of the later chunks is carried wave-uniform.  nkeep == 0 holds nothing: [-0:] is the whole
// list.  The row is moved as 32-bit words, so what is not held keeps its bits (NaN payloads and infinities included).
//
// k_xv_score: one workgroup of 256 per series, one pass over it.  Thread i keeps thirteen accumulators in registers (the
// twelve groups, then the whole series) and adds infill - obs and |infill - obs| of its scored days i, i + 256, ... to
// them in ascending order; for each of the thirteen the 256 partial sums meet in a halving tree in LDS.  A fixed order, no float atomics: the same bits in every call.  fp64 on the float32 observations
// widened exactly; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define XV_NAN_BITS 0x7fc00000u                                 // the float32 quiet NaN numpy writes for np.nan

namespace {

__device__ __forceinline__ bool xv_finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

}  // namespace

__global__ __launch_bounds__(64) void k_xv_holdout(int64_t ndays, int32_t nkeep, const uint32_t *__restrict__ rows,
                                                   uint8_t *__restrict__ held, uint32_t *__restrict__ train,
                                                   int32_t *__restrict__ nheld, int32_t *__restrict__ nfinite)
{
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * ndays;
    int32_t after = 0, nh = 0;                                   // wave-uniform: finite days of the later chunks, held days
    for (int64_t c0 = ((ndays - 1) / 64) * 64; c0 >= 0; c0 -= 64) {     // uniform
        const int64_t d = c0 + lane;
        const bool in = d < ndays;
        const uint32_t v = in ? rows[base + d] : XV_NAN_BITS;
        const bool fin = in && xv_finite_bits(v);
        const uint64_t b = __ballot(fin);
        const uint64_t above = lane == 63 ? (uint64_t)0 : b >> (lane + 1);
        const bool h = fin && nkeep > 0 && after + __popcll(above) >= nkeep;
        if (in) {
            held[base + d] = h ? 1 : 0;
            train[base + d] = h ? XV_NAN_BITS : v;
        }
        nh += __popcll(__ballot(h));
        after += __popcll(b);
    }
    if (lane == 0) { nheld[blockIdx.x] = nh; nfinite[blockIdx.x] = after; }
}

__global__ __launch_bounds__(256) void k_xv_score(int64_t ndays, const double *__restrict__ infill,
                                                  const float *__restrict__ obs, const uint8_t *__restrict__ held,
                                                  const int8_t *__restrict__ group, int32_t *__restrict__ o_n,
                                                  double *__restrict__ o_bias, double *__restrict__ o_mae,
                                                  float *__restrict__ obs_out, float *__restrict__ infill_out)
{
    __shared__ double r_dif[256], r_abs[256];
    __shared__ int32_t r_n[256];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, base = s * ndays;
    // one pass over the series: thirteen accumulators per thread (the groups, then the whole series), picked by a compare
    // in fully unrolled loops, so they stay in registers and nothing is indexed by a run-time group number
    double sd[TWXXV_NSCORES], sa[TWXXV_NSCORES];
    int32_t n[TWXXV_NSCORES];
#pragma unroll
    for (int p = 0; p < TWXXV_NSCORES; ++p) { sd[p] = 0.0; sa[p] = 0.0; n[p] = 0; }
    const float nanf32 = __uint_as_float(XV_NAN_BITS);
    for (int64_t d = tid; d < ndays; d += 256) {
        const double f = infill[base + d];
        const float o = obs[base + d];
        const bool scored = held[base + d] != 0 && fabs(f) <= 1.79769313486231570815e308;
        obs_out[base + d] = scored ? o : nanf32;
        infill_out[base + d] = scored ? (float)f : nanf32;
        const int g = group[d];
        const double dif = f - (double)o, adif = fabs(dif);
#pragma unroll
        for (int p = 0; p < TWXXV_NSCORES; ++p) {
            const bool in = scored && (p == TWXXV_NGROUPS || g == p);
            sd[p] = in ? sd[p] + dif : sd[p];
            sa[p] = in ? sa[p] + adif : sa[p];
            n[p] += in ? 1 : 0;
        }
    }
#pragma unroll
    for (int p = 0; p < TWXXV_NSCORES; ++p) {                    // the same halving tree for each of the thirteen
        r_dif[tid] = sd[p]; r_abs[tid] = sa[p]; r_n[tid] = n[p];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) {
                r_dif[tid] = r_dif[tid] + r_dif[tid + w];
                r_abs[tid] = r_abs[tid] + r_abs[tid + w];
                r_n[tid] = r_n[tid] + r_n[tid + w];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int32_t nn = r_n[0];
            const int64_t o = s * TWXXV_NSCORES + p;
            o_n[o] = nn;
            o_bias[o] = nn > 0 ? r_dif[0] / (double)nn : __builtin_nan("");
            o_mae[o] = nn > 0 ? r_abs[0] / (double)nn : __builtin_nan("");
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------

extern "C" int twxxv_holdout(int device, int64_t nstn, int64_t ndays, const float *obs, int64_t ntarget,
                             const int32_t *target_idx, int32_t nkeep, uint8_t *held, float *train_obs, int32_t *nheld,
                             int32_t *nfinite, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxxv_holdout";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || ntarget < 1 || nstn > INT32_MAX || ndays > INT32_MAX || ntarget > INT32_MAX || nkeep < 0) {
        snprintf(msg, sizeof msg, "%s: need nstn, ndays, ntarget >= 1 and nkeep >= 0", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!obs || !target_idx || !held || !train_obs || !nheld || !nfinite) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t t = 0; t < ntarget; ++t)
        if (target_idx[t] < 0 || target_idx[t] >= nstn) {
            snprintf(msg, sizeof msg, "%s: target index %d outside [0, %lld)", fn, (int)target_idx[t], (long long)nstn);
            return qa_fail(errbuf, errlen, msg);
        }
    QACHK(hipSetDevice(device));
    QaPool bufs;
    const size_t NT = (size_t)ntarget, ND = (size_t)ndays;
    uint32_t *d_rows, *d_train;
    uint8_t *d_held;
    int32_t *d_nheld, *d_nfin;
    QAALLOC(bufs, d_rows, uint32_t, NT * ND); QAALLOC(bufs, d_train, uint32_t, NT * ND); QAALLOC(bufs, d_held, uint8_t, NT * ND);
    QAALLOC(bufs, d_nheld, int32_t, NT); QAALLOC(bufs, d_nfin, int32_t, NT);
    for (size_t t = 0; t < NT; ++t)                               // only the targets' rows go up
        QACHK(hipMemcpy(d_rows + t * ND, obs + (size_t)target_idx[t] * ND, ND * 4, hipMemcpyHostToDevice));
    QaTimer tm;
    if (kernel_ms) { QACHK(tm.init()); QACHK(tm.start()); }
    hipLaunchKernelGGL(k_xv_holdout, dim3((unsigned)ntarget), dim3(64), 0, nullptr, ndays, nkeep,
                       (const uint32_t *)d_rows, d_held, d_train, d_nheld, d_nfin);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_set(kernel_ms));
    QACHK(hipMemcpy(held, d_held, NT * ND, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(train_obs, d_train, NT * ND * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(nheld, d_nheld, NT * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(nfinite, d_nfin, NT * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int twxxv_score(int device, int64_t nseries, int64_t ndays, const double *infill, const float *obs,
                           const uint8_t *held, const int8_t *group, int32_t *n, double *bias, double *mae,
                           float *obs_out, float *infill_out, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxxv_score";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nseries < 1 || ndays < 1 || nseries > INT32_MAX || ndays > INT32_MAX) {
        snprintf(msg, sizeof msg, "%s: need nseries, ndays >= 1", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!infill || !obs || !held || !group || !n || !bias || !mae || !obs_out || !infill_out) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t d = 0; d < ndays; ++d)
        if (group[d] < -1 || group[d] >= TWXXV_NGROUPS) {
            snprintf(msg, sizeof msg, "%s: group[%lld] = %d outside -1 .. %d", fn, (long long)d, (int)group[d],
                     TWXXV_NGROUPS - 1);
            return qa_fail(errbuf, errlen, msg);
        }
    QACHK(hipSetDevice(device));
    QaPool bufs;
    const size_t NS = (size_t)nseries, ND = (size_t)ndays, NO = NS * (TWXXV_NGROUPS + 1);
    double *d_infill, *d_bias, *d_mae;
    float *d_obs, *d_oo, *d_io;
    uint8_t *d_held;
    int8_t *d_group;
    int32_t *d_n;
    QAALLOC(bufs, d_infill, double, NS * ND); QAALLOC(bufs, d_obs, float, NS * ND); QAALLOC(bufs, d_held, uint8_t, NS * ND);
    QAALLOC(bufs, d_group, int8_t, ND); QAALLOC(bufs, d_n, int32_t, NO); QAALLOC(bufs, d_bias, double, NO); QAALLOC(bufs, d_mae, double, NO);
    QAALLOC(bufs, d_oo, float, NS * ND); QAALLOC(bufs, d_io, float, NS * ND);
    QACHK(hipMemcpy(d_infill, infill, NS * ND * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_obs, obs, NS * ND * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_held, held, NS * ND, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_group, group, ND, hipMemcpyHostToDevice));
    QaTimer tm;
    if (kernel_ms) { QACHK(tm.init()); QACHK(tm.start()); }
    hipLaunchKernelGGL(k_xv_score, dim3((unsigned)nseries), dim3(256), 0, nullptr, ndays, (const double *)d_infill,
                       (const float *)d_obs, (const uint8_t *)d_held, (const int8_t *)d_group, d_n, d_bias, d_mae, d_oo,
                       d_io);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_set(kernel_ms));
    QACHK(hipMemcpy(n, d_n, NO * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(bias, d_bias, NO * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(mae, d_mae, NO * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(obs_out, d_oo, NS * ND * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(infill_out, d_io, NS * ND * 4, hipMemcpyDeviceToHost));
    return 0;
}
