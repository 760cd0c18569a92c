// twx_prcpcorrob.hip -- libtwxqa.so: the spatial corroboration check of the precipitation QA, _qa_spatial_corrob /
// _get_spatial_corrob_flag (twx/qa/qa_prcp.py:614-664, 683-782; flag 17), for many targets in one call.  The fifteenth
// translation unit of the library (include/twx_qa.h, twxpc_*).  With it run_qa_spatial_only (:178-215) and run_qa_all
// (:87-133) are complete; _qa_yr_clim_outlier, which the reference never calls, stays out.
//
// State.  As in twx_prcpqa.hip the flag byte is the working copy: a target's series is "flag == 1 ? pool value : NaN", and
// 17 is written only where the flag is 1.  A NEIGHBOUR's observations are the pool's values as they are, no QA applied
// (load_all_stn_obs).  No kernel before the last writes a flag: every decision is taken on the series as it was given.
//
// THE QUIRK, kept: the array the target's percentile is compared with (:760) holds the OBSERVATIONS in cm of all finite
// neighbours on the three days, not capped at 7 and not percentiles.  So no neighbour percentile is ever ranked (only
// whether a neighbour's row holds more than 20 values matters), a day that reaches the threshold step needs the minimum and
// maximum over ALL finite neighbours next to those of the first 7, and a percentile less than 1 away from that range gives
// a threshold ABOVE 26.924.
//
// k_pc_radius    one wavefront per target; pass 0 counts the stations within 75 km (k_radius_dist's arithmetic), pass 1
//                collects (distance, row) in LDS and writes the rows rank-sorted by distance, equal distances in table
//                order.  LDS 3 KiB.
// k_pc_rowcounts one 256-thread workgroup per station that is some target's neighbour (the pool row) and per target (its
//                masked series): a 366-bin histogram of the finite values > 0 by month-day (a leap year's calendar) in LDS,
//                integer atomics; then the circular 29-bin sums: [366] uint16, the sizes of _build_pors' rows (the windows of
//                k_pq_pctiles).  LDS 1.4 KiB.
// k_pc_walk      one wavefront per (target, block of 64 days), a lane per day x.  It walks the neighbours in distance order
//                and reads days x - 1, x, x + 1 of each station-major row (adjacent lanes, adjacent addresses).  Per day of
//                the triple: the finite count (saturating at 7: it serves ">= 3" and "the first 7"), the basis count
//                (saturating at 3); over the triple: minimum / maximum of the first 7 and of all.  Integers and min / max
//                only: no order dependence.  A lane is done once its value lies inside the first-7 range (the range only
//                grows: it can no longer be flagged); the walk ends when every lane is.  Result per day: a state byte (0
//                nothing, 3 flag: decided against 26.924, 2 needs the percentile) and, for state 2, the first-7 extreme and
//                the all-neighbour range.  No LDS.
// k_pc_rank      one 256-thread workgroup per (target, row of the 366) that has a state-2 day (<= one per year): the window of
//                the masked series compacted into LDS as k_pq_pctiles does, then a wavefront per candidate day counts
//                left = #(a < v), right = #(a <= v) with ballots -- no sort: nyears candidates x 29 nyears values is less
//                than the compare-exchanges of a bitonic sort of the window -- and lane 0 forms scipy's percentileofscore
//                (kind "rank"), pctile_dif, the threshold and the decision in fp64.  LDS 16 KiB: 8 workgroups per compute
//                unit, as k_pq_pctiles.
// k_pc_apply     thread = (target, day): state 3 becomes 17 where the flag is 1.
// No floating-point atomics; the slot a window value lands in depends on an integer atomic, the counts do not: two calls
// give the same bytes.  fp64 on float32 values widened exactly.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_series.h"

#define PC_OK 1                              // qa_prcp.py:37-57
#define PC_SPATIAL_CORROB 17
#define PC_ROWS TWXPQ_PCTILE_ROWS
#define PC_MIN_NGHS 3                        // qa_prcp.py:70-71
#define PC_MAX_NGHS 7
#define PC_THRES 26.924                      // MAX_SPATIAL_COLLAB_THRES, cm (:64)
#define PC_THRES_MM (26.924 * 10.0)          // MAX_SPATIAL_COLLAB_THRES_MM (:65), the product as Python forms it
#define PC_ST_NONE 0
#define PC_ST_RANK 2
#define PC_ST_FLAG 3

namespace {

__device__ __forceinline__ bool pc_wet(float v) { return v > 0.0f && qa_finitef(v); }

}  // namespace

__global__ __launch_bounds__(64) void k_pc_radius(int64_t nstn, const double *__restrict__ lon,
                                                  const double *__restrict__ lat, const int32_t *__restrict__ target_idx,
                                                  int fill, int32_t *__restrict__ count,
                                                  const int64_t *__restrict__ csr_off, int32_t *__restrict__ csr_ngh)
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
    }
}

// block b < nslot: the pool row rows[b] as it is; block nslot + t: target t's series under its flags (flag may be null:
// every series as it is, rows == null: series b).  cnt [gridDim.x][366]
__global__ __launch_bounds__(256) void k_pc_rowcounts(int64_t ndays, int nslot, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ target_idx,
                                                      const uint16_t *__restrict__ mday, const float *__restrict__ prcp,
                                                      const uint8_t *__restrict__ flag, uint16_t *__restrict__ cnt)
{
    __shared__ int hist[PC_ROWS];
    const int tid = threadIdx.x;
    const int b = (int)blockIdx.x;
    const bool masked = b >= nslot;
    const size_t s = masked ? (size_t)target_idx[b - nslot] : (rows ? (size_t)rows[b] : (size_t)b);
    const float *x = prcp + s * (size_t)ndays;
    const uint8_t *f = masked ? flag + (size_t)(b - nslot) * (size_t)ndays : nullptr;
    for (int i = tid; i < PC_ROWS; i += 256) hist[i] = 0;
    __syncthreads();
    for (int64_t d = tid; d < ndays; d += 256) {
        if (f && f[d] != PC_OK) continue;
        if (pc_wet(x[d])) atomicAdd(&hist[mday[d]], 1);          // (an integer count)
    }
    __syncthreads();
    for (int r = tid; r < PC_ROWS; r += 256) {
        int sum = 0;
        for (int j = -14; j <= 14; ++j) {
            int q = r + j;
            q = q < 0 ? q + PC_ROWS : (q >= PC_ROWS ? q - PC_ROWS : q);
            sum += hist[q];
        }
        cnt[(size_t)b * PC_ROWS + (size_t)r] = (uint16_t)sum;    // <= 29 * nyears <= TWXPQ_MAX_WINDOW_VALUES (host check)
    }
}

__global__ __launch_bounds__(64) void k_pc_walk(int64_t ndays, int nblk, const float *__restrict__ prcp,
                                                const uint8_t *__restrict__ flag, const int32_t *__restrict__ target_idx,
                                                const int64_t *__restrict__ csr_off, const int32_t *__restrict__ csr_ngh,
                                                const int32_t *__restrict__ slot, const uint16_t *__restrict__ cnt_pool,
                                                const uint16_t *__restrict__ cnt_tgt, const uint16_t *__restrict__ rowtab,
                                                uint8_t *__restrict__ state, float *__restrict__ ext7,
                                                float *__restrict__ rng_lo, float *__restrict__ rng_hi,
                                                double *__restrict__ o_abs, double *__restrict__ o_thres)
{
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x / nblk;
    const int64_t x = (int64_t)(blockIdx.x % nblk) * 64 + lane;
    const int64_t k0 = csr_off[t], k1 = csr_off[t + 1];
    if (k1 - k0 < PC_MIN_NGHS) return;                           // uniform: fewer than 3 neighbours, or over the cap
    const size_t to = (size_t)t * (size_t)ndays;
    float v = 0.0f;
    bool act = x >= 1 && x < ndays - 1 && flag[to + x] == PC_OK;  // not the first or the last day (:654)
    if (act) { v = prcp[(size_t)target_idx[t] * (size_t)ndays + x]; act = !(v != v); }
    int r0 = 0, r1 = 0, r2 = 0;
    if (act) { r0 = rowtab[x - 1]; r1 = rowtab[x]; r2 = rowtab[x + 1]; }
    int nf0 = 0, nf1 = 0, nf2 = 0, nb0 = 0, nb1 = 0, nb2 = 0;
    float mn7 = __builtin_inff(), mx7 = -__builtin_inff(), mnA = __builtin_inff(), mxA = -__builtin_inff();
    bool done = !act;
    for (int64_t k = k0; k < k1; ++k) {                          // uniform
        if (__ballot(!done) == 0) break;
        const int32_t j = csr_ngh[k];
        if (done) continue;
        const float *o = prcp + (size_t)j * (size_t)ndays + x;
        const uint16_t *c = cnt_pool + (size_t)slot[j] * PC_ROWS;
        const float a0 = o[-1], a1 = o[0], a2 = o[1];
#define PC_DAY(a, nf, nb, r)                                                                   \
        if (qa_finitef(a)) {                                                                   \
            if (nf < PC_MAX_NGHS) { mn7 = fminf(mn7, a); mx7 = fmaxf(mx7, a); ++nf; }          \
            mnA = fminf(mnA, a); mxA = fmaxf(mxA, a);                                          \
            if (nb < PC_MIN_NGHS && c[r] > TWXPQ_MIN_PERCENTILE_VALUES) ++nb;                  \
        }
        PC_DAY(a0, nf0, nb0, r0)
        PC_DAY(a1, nf1, nb1, r1)
        PC_DAY(a2, nf2, nb2, r2)
#undef PC_DAY
        done = v >= mn7 && v <= mx7;                             // inside the range of the first 7: never flagged (:700-706)
    }
    if (done) return;
    if (nf0 < PC_MIN_NGHS || nf1 < PC_MIN_NGHS || nf2 < PC_MIN_NGHS) return;     // (:693)
    const float e = v > mx7 ? mx7 : mn7;
    const double ad = fabs((double)v - (double)e);
    if (o_abs) o_abs[to + x] = ad;
    const bool basis = cnt_tgt[(size_t)t * PC_ROWS + (size_t)r1] > TWXPQ_MIN_PERCENTILE_VALUES &&            // (:708, 758)
                       nb0 >= PC_MIN_NGHS && nb1 >= PC_MIN_NGHS && nb2 >= PC_MIN_NGHS;
    if (basis) {
        state[to + x] = PC_ST_RANK;
        ext7[to + x] = e;
        rng_lo[to + x] = mnA;
        rng_hi[to + x] = mxA;
    } else {
        if (o_thres) o_thres[to + x] = PC_THRES;
        if (ad > PC_THRES) state[to + x] = PC_ST_FLAG;
    }
}

__global__ __launch_bounds__(256) void k_pc_rank(int64_t ndays, int nyears, const int2 *__restrict__ yr,
                                                 const uint16_t *__restrict__ rowtab, const float *__restrict__ prcp,
                                                 const uint8_t *__restrict__ flag, const int32_t *__restrict__ target_idx,
                                                 uint8_t *__restrict__ state, const float *__restrict__ ext7,
                                                 const float *__restrict__ rng_lo, const float *__restrict__ rng_hi,
                                                 double *__restrict__ o_pct, double *__restrict__ o_thres)
{
    __shared__ float xs[TWXPQ_MAX_WINDOW_VALUES];
    __shared__ int cnt;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = (int)(blockIdx.x % PC_ROWS);
    const size_t t = blockIdx.x / PC_ROWS;
    const size_t to = t * (size_t)ndays;
    const float *x = prcp + (size_t)target_idx[t] * (size_t)ndays;
    // the days of this row: one per year, yday - 1 == row of the day's own year
    int any = 0;
    for (int k = tid; k < nyears; k += 256) {
        const int64_t d = (int64_t)yr[k].x + row;
        if (d >= 0 && d < ndays && rowtab[d] == row && state[to + d] == PC_ST_RANK) any = 1;
    }
    if (!__syncthreads_or(any)) return;                          // uniform
    if (tid == 0) cnt = 0;
    __syncthreads();
    // the window, gathered as k_pq_pctiles gathers it
    for (int i = tid; i < nyears * 32; i += 256) {
        const int k = i >> 5, j = i & 31;
        if (j >= 29) continue;
        int q = row - 14 + j;
        q = q < 0 ? q + PC_ROWS : (q >= PC_ROWS ? q - PC_ROWS : q);
        const int64_t d = qa_date_day(q, yr[k], ndays);
        if (d < 0) continue;
        if (flag[to + d] != PC_OK) continue;
        const float v = x[d];
        if (!pc_wet(v)) continue;
        xs[atomicAdd(&cnt, 1)] = v;                              // <= 29 * nyears <= TWXPQ_MAX_WINDOW_VALUES (host check)
    }
    __syncthreads();
    const int n = cnt;
    for (int k = w; k < nyears; k += 4) {                        // uniform in a wavefront
        const int64_t d = (int64_t)yr[k].x + row;
        if (d < 0 || d >= ndays || rowtab[d] != row || state[to + d] != PC_ST_RANK) continue;
        const float v = x[d];
        int left = 0, right = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const float a = i < n ? xs[i] : __builtin_inff();
            left += __popcll(__ballot(i < n && a < v));
            right += __popcll(__ballot(i < n && a <= v));
        }
        if (lane != 0) continue;
        // scipy's percentileofscore, kind "rank": (left + right + (left < right)) * (50.0 / n)
        const double pct = (double)(left + right + (left < right ? 1 : 0)) * (50.0 / (double)n);
        const double hi = (double)rng_hi[to + d], lo = (double)rng_lo[to + d];
        const double dif = pct > hi ? fabs(pct - hi) : (pct < lo ? fabs(pct - lo) : 0.0);         // (:762-767)
        const double thres = dif == 0.0 ? PC_THRES : ((-45.72 * log(dif)) + PC_THRES_MM) / 10.0;  // (:769-772)
        const double ad = fabs((double)v - (double)ext7[to + d]);
        if (o_pct) o_pct[to + d] = pct;
        if (o_thres) o_thres[to + d] = thres;
        state[to + d] = ad > thres ? PC_ST_FLAG : PC_ST_NONE;
    }
}

__global__ __launch_bounds__(256) void k_pc_apply(int64_t total, const uint8_t *__restrict__ state, uint8_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (state[i] == PC_ST_FLAG && flag[i] == PC_OK) flag[i] = PC_SPATIAL_CORROB;
}

// ---------------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------------
namespace {

// The calendar of a day axis, the years capped for the rows of the percentile basis.
int pc_cal(const char *who, int64_t ndays, const int32_t *ymd, QaCalendar &c, char *errbuf, int errlen)
{
    if (qa_cal_years(who, ndays, ymd, c, errbuf, errlen) != 0 ||
        qa_year_cap(who, c, 29, TWXPQ_MAX_WINDOW_VALUES, "a row of the percentile basis holds at most TWXPQ_MAX_WINDOW_VALUES", "",
                    errbuf, errlen) != 0)
        return -1;
    return qa_cal_walk(who, ndays, ymd, c, errbuf, errlen);
}

}  // namespace

extern "C" int twxpc_spatial_corrob(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                                    const float *prcp, const int32_t *ymd, int64_t ntarget, const int32_t *target_idx,
                                    uint8_t *flags, int32_t *status, double *abs_dif, double *pctile, double *thres,
                                    float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || ntarget < 1 || nstn > INT32_MAX || ndays > INT32_MAX - 256 || ntarget > INT32_MAX / PC_ROWS)
        return qa_fail(errbuf, errlen, "twxpc_spatial_corrob: need nstn >= 1, ndays >= 1 and ntarget >= 1");
    if (!lon || !lat || !prcp || !ymd || !target_idx || !flags) return qa_fail(errbuf, errlen, "twxpc_spatial_corrob: null buffer");
    const int64_t nblk64 = (ndays + 63) / 64;
    if (nblk64 * ntarget > INT32_MAX || (ntarget * ndays + 255) / 256 > INT32_MAX || (nstn + ntarget) > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxpc_spatial_corrob: more than 2^31 - 1 work items in one call");
    QaCalendar cal;
    if (pc_cal("twxpc_spatial_corrob", ndays, ymd, cal, errbuf, errlen) != 0) return -1;
    for (int64_t i = 0; i < ntarget; ++i) {
        if (target_idx[i] < 0 || target_idx[i] >= nstn) {
            char msg[160];
            snprintf(msg, sizeof msg, "twxpc_spatial_corrob: target_idx[%lld] = %d is not a row of the pool (nstn = %lld)",
                     (long long)i, (int)target_idx[i], (long long)nstn);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const size_t nt = (size_t)ntarget, ns = (size_t)nstn, nd = (size_t)ndays;
    const int nblk = (int)nblk64;
    float ms[TWXPC_NKERNELS];
    for (int i = 0; i < TWXPC_NKERNELS; ++i) ms[i] = 0.0f;

    QACHK(hipSetDevice(device));
    QaBuf b_geo, b_tgt, b_csr, b_obs, b_flag, b_cal, b_slot, b_rows, b_cnt, b_state, b_work, b_out;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_geo.p, ns * 16));
    double *d_lon = static_cast<double *>(b_geo.p), *d_lat = d_lon + ns;
    QACHK(hipMemcpy(d_lon, lon, ns * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_lat, lat, ns * 8, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_tgt.p, (nt + 1) * 8 + nt * 8));           // csr offsets (int64, nt + 1), index, count
    int64_t *d_off = static_cast<int64_t *>(b_tgt.p);
    int32_t *d_idx = (int32_t *)(d_off + nt + 1), *d_ncnt = d_idx + nt;
    QACHK(hipMemcpy(d_idx, target_idx, nt * 4, hipMemcpyHostToDevice));

    // ---- 1. the radius lists in distance order: count, scan on the host, fill + sort ----------------------------------
    float ms_a = 0.0f, ms_b = 0.0f;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pc_radius, dim3((unsigned)nt), dim3(64), 0, nullptr, nstn, (const double *)d_lon,
                       (const double *)d_lat, (const int32_t *)d_idx, 0, d_ncnt, (const int64_t *)nullptr, (int32_t *)nullptr);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms_a));
    std::vector<int32_t> ncnt(nt), tst(nt);
    std::vector<int64_t> off(nt + 1);
    QACHK(hipMemcpy(ncnt.data(), d_ncnt, nt * 4, hipMemcpyDeviceToHost));
    off[0] = 0;
    for (size_t i = 0; i < nt; ++i) {                            // a list above the cap is not built: the target says so
        tst[i] = ncnt[i] > TWXQA_MAX_RADIUS_NGH ? TWXQA_SP_NGH_CAP : (ncnt[i] < PC_MIN_NGHS ? TWXQA_SP_FEW_NGHS : TWXQA_SP_OK);
        off[i + 1] = off[i] + (tst[i] == TWXQA_SP_NGH_CAP ? 0 : ncnt[i]);
    }
    if (status) memcpy(status, tst.data(), nt * 4);
    QACHK(hipMemcpy(d_off, off.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
    const size_t ncsr = (size_t)off[nt];
    QACHK(hipMalloc(&b_csr.p, std::max<size_t>(16, ncsr * 4)));
    int32_t *d_csr = static_cast<int32_t *>(b_csr.p);
    if (ncsr > 0) {
        QACHK(tm.start());
        hipLaunchKernelGGL(k_pc_radius, dim3((unsigned)nt), dim3(64), 0, nullptr, nstn, (const double *)d_lon,
                           (const double *)d_lat, (const int32_t *)d_idx, 1, d_ncnt, (const int64_t *)d_off, d_csr);
        QACHK(hipGetLastError());
        QACHK(tm.stop_set(&ms_b));
    }
    ms[0] = ms_a + ms_b;
    // the stations that are a walked target's neighbour get row counts: their slot, -1 for the rest
    std::vector<int32_t> csr(ncsr), slot(ns, -1), rows;
    if (ncsr > 0) QACHK(hipMemcpy(csr.data(), d_csr, ncsr * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nt; ++i) {
        if (tst[i] != TWXQA_SP_OK) continue;                     // (a list shorter than 3 is never walked)
        for (int64_t k = off[i]; k < off[i + 1]; ++k) slot[(size_t)csr[(size_t)k]] = 0;
    }
    for (size_t j = 0; j < ns; ++j)
        if (slot[j] == 0) { slot[j] = (int32_t)rows.size(); rows.push_back((int32_t)j); }
    const size_t nslot = rows.size();

    // ---- 2. the row counts: neighbours from the pool as it is, targets under their flags -----------------------------
    QACHK(hipMalloc(&b_obs.p, ns * nd * 4));
    float *d_prcp = static_cast<float *>(b_obs.p);
    QACHK(hipMemcpy(d_prcp, prcp, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_flag.p, nt * nd));
    uint8_t *d_f = static_cast<uint8_t *>(b_flag.p);
    QACHK(hipMemcpy(d_f, flags, nt * nd, hipMemcpyHostToDevice));
    const size_t ny = (size_t)cal.nyears;
    QACHK(hipMalloc(&b_cal.p, ny * 8 + nd * 4));                  // years (int2), row, mday (uint16)
    int2 *d_yr = static_cast<int2 *>(b_cal.p);
    uint16_t *d_row = (uint16_t *)(d_yr + ny), *d_mday = d_row + nd;
    QACHK(hipMemcpy(d_yr, cal.yr.data(), ny * 8, hipMemcpyHostToDevice));
    const std::vector<uint16_t> row16(cal.row.begin(), cal.row.end());       // yday - 1: 0 .. 365 (k_pc_walk, k_pc_rank take 16 bits)
    QACHK(hipMemcpy(d_row, row16.data(), nd * 2, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_mday, cal.mday.data(), nd * 2, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_slot.p, ns * 4));
    QACHK(hipMemcpy(b_slot.p, slot.data(), ns * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_rows.p, std::max<size_t>(4, nslot * 4)));
    if (nslot > 0) QACHK(hipMemcpy(b_rows.p, rows.data(), nslot * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_cnt.p, (nslot + nt) * PC_ROWS * 2));       // [nslot + nt][366]
    uint16_t *d_cntp = static_cast<uint16_t *>(b_cnt.p), *d_cntt = d_cntp + nslot * PC_ROWS;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pc_rowcounts, dim3((unsigned)(nslot + nt)), dim3(256), 0, nullptr, ndays, (int)nslot,
                       (const int32_t *)b_rows.p, (const int32_t *)d_idx, (const uint16_t *)d_mday, (const float *)d_prcp,
                       (const uint8_t *)d_f, d_cntp);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[1]));

    // ---- 3. the walk ---------------------------------------------------------------------------------------------------
    QACHK(hipMalloc(&b_state.p, nt * nd));
    uint8_t *d_state = static_cast<uint8_t *>(b_state.p);
    QACHK(hipMemset(d_state, PC_ST_NONE, nt * nd));
    QACHK(hipMalloc(&b_work.p, 3 * nt * nd * 4));                 // first-7 extreme, all-neighbour minimum and maximum
    float *d_ext = static_cast<float *>(b_work.p), *d_lo = d_ext + nt * nd, *d_hi = d_lo + nt * nd;
    double *d_abs = nullptr, *d_pct = nullptr, *d_thr = nullptr;
    const int nout = (abs_dif ? 1 : 0) + (pctile ? 1 : 0) + (thres ? 1 : 0);
    if (nout) {
        QACHK(hipMalloc(&b_out.p, (size_t)nout * nt * nd * 8));
        QACHK(hipMemset(b_out.p, 0xff, (size_t)nout * nt * nd * 8));      // (all bits set: a NaN)
        double *p = static_cast<double *>(b_out.p);
        if (abs_dif) { d_abs = p; p += nt * nd; }
        if (pctile) { d_pct = p; p += nt * nd; }
        if (thres) d_thr = p;
    }
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pc_walk, dim3((unsigned)(nt * (size_t)nblk)), dim3(64), 0, nullptr, ndays, nblk,
                       (const float *)d_prcp, (const uint8_t *)d_f, (const int32_t *)d_idx, (const int64_t *)d_off,
                       (const int32_t *)d_csr, (const int32_t *)b_slot.p, (const uint16_t *)d_cntp, (const uint16_t *)d_cntt,
                       (const uint16_t *)d_row, d_state, d_ext, d_lo, d_hi, d_abs, d_thr);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[2]));

    // ---- 4. the rank, the threshold and the flag -----------------------------------------------------------------------
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pc_rank, dim3((unsigned)(nt * PC_ROWS)), dim3(256), 0, nullptr, ndays, cal.nyears,
                       (const int2 *)d_yr, (const uint16_t *)d_row, (const float *)d_prcp, (const uint8_t *)d_f,
                       (const int32_t *)d_idx, d_state, (const float *)d_ext, (const float *)d_lo, (const float *)d_hi,
                       d_pct, d_thr);
    QACHK(hipGetLastError());
    hipLaunchKernelGGL(k_pc_apply, dim3((unsigned)((nt * nd + 255) / 256)), dim3(256), 0, nullptr, (int64_t)(nt * nd),
                       (const uint8_t *)d_state, d_f);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[3]));
    QACHK(hipMemcpy(flags, d_f, nt * nd, hipMemcpyDeviceToHost));
    if (abs_dif) QACHK(hipMemcpy(abs_dif, d_abs, nt * nd * 8, hipMemcpyDeviceToHost));
    if (pctile) QACHK(hipMemcpy(pctile, d_pct, nt * nd * 8, hipMemcpyDeviceToHost));
    if (thres) QACHK(hipMemcpy(thres, d_thr, nt * nd * 8, hipMemcpyDeviceToHost));
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxpc_pors_counts(int device, int64_t nstn, int64_t ndays, const float *vals, const int32_t *ymd,
                                 uint16_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || nstn > INT32_MAX || ndays > INT32_MAX - 256)
        return qa_fail(errbuf, errlen, "twxpc_pors_counts: need nstn >= 1 and ndays >= 1");
    if (!vals || !ymd || !counts) return qa_fail(errbuf, errlen, "twxpc_pors_counts: null buffer");
    QaCalendar cal;
    if (pc_cal("twxpc_pors_counts", ndays, ymd, cal, errbuf, errlen) != 0) return -1;
    const size_t ns = (size_t)nstn, nd = (size_t)ndays;
    QACHK(hipSetDevice(device));
    QaBuf b_obs, b_cal, b_cnt;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_obs.p, ns * nd * 4));
    QACHK(hipMemcpy(b_obs.p, vals, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_cal.p, nd * 2));
    QACHK(hipMemcpy(b_cal.p, cal.mday.data(), nd * 2, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_cnt.p, ns * PC_ROWS * 2));
    float ms = 0.0f;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_pc_rowcounts, dim3((unsigned)ns), dim3(256), 0, nullptr, ndays, (int)ns, (const int32_t *)nullptr,
                       (const int32_t *)nullptr, (const uint16_t *)b_cal.p, (const float *)b_obs.p, (const uint8_t *)nullptr,
                       static_cast<uint16_t *>(b_cnt.p));
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms));
    QACHK(hipMemcpy(counts, b_cnt.p, ns * PC_ROWS * 2, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}
