// twx_spatial.hip -- libtwxqa.so: step08's spatial regression check of daily Tmin / Tmax (_qa_spatial_regress,
// twx/qa/qa_temp.py:688-738, 858-1015; include/twx_qa.h).  A translation unit of its own next to twx_outlier.hip; both
// are linked into libtwxqa.so by one hipcc command (build.sh).
//
// k_qa_radius: one wavefront per target station walks the station table 64 rows at a time and ballots the rows
// within TWXQA_NGH_RADIUS_KM (haversine, util_geo.py:24-40).  Pass 0 counts them, pass 1 writes them at the CSR offset
// the host scanned from the counts; a lane's position is the popcount of the ballot below it, so the list keeps the
// ascending table order of the reference's boolean-mask gather (qa_temp.py:699-701).  The target itself is left out
// by index.
//
// k_spatial_regress: one 64-lane workgroup (one wavefront) per (target, variable, year-month) item.  Lane l holds
// series day ws - 1 + l: the window [ws, we) of the month +- 15 days is lanes 1..nwin (nwin <= 61), lanes 0 and
// nwin + 1 are the day before and after it (a neighbour's previous / next day of the SERIES, qa_temp.py:895-897; a
// day outside the series reads as missing).  Stages, all wave-uniform in control flow:
//   1. neighbour models: per neighbour of the CSR list the overlap mask by ballot, then wave sums for the means and
//      the centred sums -> index-of-agreement weight (perf_metrics.py:59-62), slope and intercept of
//      linregress(ngh, stn).  Valid neighbours go to LDS as (weight, slope, intercept, column).
//   2. rank sort by weight, largest first (equal weights: the earlier table row first; the golden inputs have none).
//   3. estimate: walk the sorted list; a lane takes the finite value of (previous, own, next) nearest its observation
//      (strict <: the first wins a tie) and accumulates until it holds TWXQA_MAX_NGHS contributions.
//   4. Pearson's r over the estimated window days, residual statistics over the same days, flags on the month's days.
// A workgroup is one wave: the __syncthreads() between the stages only orders the wave's own LDS traffic.
//
// LDS: an entry is 32 bytes, the rank list 2 bytes: 34 * TWXQA_MAX_RADIUS_NGH = 8704 bytes per wave, so the 160 KiB of
// a CU hold 18 waves (4.5 per SIMD); a cap of 512 would leave 9 (2 per SIMD).  That arithmetic sized the cap at 256.
// The premise behind it -- that this kernel's time is the latency of its column loads and that it wants about 4 waves
// per SIMD to cover it -- is an assumption: no occupancy sweep and no counter run was made for it.  The station
// density of the reference's domain gives about 25 stations in a 75 km circle; 256 is ten times that.
// fp64 throughout; the observations are float32 widened exactly.  The library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define SP_NGH_CORR 0.8                      // qa_temp.py:67
#define SP_RESID_CUTOFF 8.0                  // qa_temp.py:68
#define SP_RESID_STD_CUTOFF 4.0              // qa_temp.py:69
#define SP_MTH_BUFFER 15                     // qa_temp.py:858

namespace {

// (as twx_outlier.hip) one DPP step of a sum: lanes without a source add +0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_step(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
    return v + __hiloint2double(hi, lo);
}

// sum over the 64 lanes, the same bits in all of them: the 16-lane DPP row sum of twx_outlier.hip, then the four row
// totals exchanged across rows (a + b and b + a round alike, so every lane ends with the same value)
__device__ __forceinline__ double wave_sum(double v)
{
    v = dpp_add_step<0x111, 0xf>(v);           // row_shr:1
    v = dpp_add_step<0x112, 0xf>(v);           // row_shr:2
    v = dpp_add_step<0x114, 0xf>(v);           // row_shr:4
    v = dpp_add_step<0x118, 0xf>(v);           // row_shr:8 -> lane 15 of the row holds the row's sum
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x15f, 0xf, 0xf, false);   // row_newbcast:15
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x15f, 0xf, 0xf, false);
    v = __hiloint2double(hi, lo);
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570e308; }

struct NghEnt {
    double w, slope, icpt;
    int32_t col, pad;
};

}  // namespace

__global__ __launch_bounds__(256) void k_qa_radius(int64_t nstn, const double *__restrict__ lon,
                                                   const double *__restrict__ lat, int64_t ntarget,
                                                   const int32_t *__restrict__ target_idx, int fill,
                                                   int32_t *__restrict__ count, const int64_t *__restrict__ csr_off,
                                                   int32_t *__restrict__ csr_ngh)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntarget) return;                                // wave-uniform: one target per wave
    const int32_t self = target_idx[t];
    const double lat1rad = lat[self] * QA_RADIAN, lon1rad = lon[self] * QA_RADIAN;
    const double cos1 = cos(lat1rad);
    int64_t pos = 0, room = 0;
    if (fill) {                                              // a target over the cap has an empty list (off[t+1] == off[t])
        pos = csr_off[t];
        room = csr_off[t + 1] - pos;
        if (room == 0) return;
    }
    int32_t n = 0;
    for (int64_t j0 = 0; j0 < nstn; j0 += 64) {              // uniform
        const int64_t j = j0 + lane;
        bool in = false;
        if (j < nstn && j != self) {
            in = qa_dist_km(lat1rad, lon1rad, cos1, lat[j], lon[j]) <= TWXQA_NGH_RADIUS_KM;
        }
        const uint64_t b = __ballot(in);
        if (fill && in) {
            const int64_t k = n + __popcll(b & (((uint64_t)1 << lane) - 1));
            if (k < room) csr_ngh[pos + k] = (int32_t)j;     // (room is this pass's own count of pass 0)
        }
        n += __popcll(b);
    }
    if (!fill && lane == 0) count[t] = n;
}

__global__ __launch_bounds__(64) void k_spatial_regress(int64_t ndays, int nmonths, const float *__restrict__ tmin,
                                                        const float *__restrict__ tmax, const int4 *__restrict__ mon,
                                                        const int32_t *__restrict__ target_idx,
                                                        const int32_t *__restrict__ tstatus,
                                                        const int64_t *__restrict__ csr_off,
                                                        const int32_t *__restrict__ csr_ngh, uint8_t *__restrict__ flag_tmin,
                                                        uint8_t *__restrict__ flag_tmax, double *__restrict__ est,
                                                        double *__restrict__ item_r, int32_t *__restrict__ item_nvalid,
                                                        int32_t *__restrict__ item_status)
{
    __shared__ NghEnt ent[TWXQA_MAX_RADIUS_NGH];
    __shared__ uint16_t order[TWXQA_MAX_RADIUS_NGH];
    const int lane = threadIdx.x;
    const int64_t item = blockIdx.x;                         // (t * 2 + v) * nmonths + m
    const int m = (int)(item % nmonths);
    const int64_t tv = item / nmonths;
    const int v = (int)(tv & 1);
    const int64_t t = tv >> 1;
    const double nan = __builtin_nan("");
    double r_out = nan;
    int nvalid = 0, st = TWXQA_SP_OK;

    const float *obs = v ? tmax : tmin;
    const int4 mw = mon[m];                                  // x, y: window [ws, we)   z, w: month [ms, me)
    const int nwin = mw.y - mw.x;                            // <= 61
    const int64_t d = (int64_t)mw.x - 1 + lane;
    const bool in_series = lane <= nwin + 1 && d >= 0 && d < ndays;
    const bool in_win = lane >= 1 && lane <= nwin;
    const bool in_mth = in_win && d >= mw.z && d < mw.w;
    const int32_t self = target_idx[t];
    const double tobs = in_win ? (double)obs[(size_t)self * ndays + d] : nan;
    const bool tfin = in_win && finite_d(tobs);
    const int ntw = __popcll(__ballot(tfin));
    const int64_t n0 = csr_off[t];
    const int nngh = (int)(csr_off[t + 1] - n0);

    // the reference tests the station's neighbour count first (qa_temp.py:711), then the window (:732)
    if (tstatus[t] != TWXQA_SP_OK) st = tstatus[t];
    else if (nngh < TWXQA_MIN_NGHS) st = TWXQA_SP_FEW_NGHS;
    else if (ntw < TWXQA_MIN_DAYS_MTH_WINDOW) st = TWXQA_SP_FEW_DAYS;

    if (st == TWXQA_SP_OK) {
        // ---- 1. neighbour models (qa_temp.py:942-979, 1000-1008) -------------------------------------------------
        for (int q = 0; q < nngh; ++q) {                     // uniform
            const int32_t j = csr_ngh[n0 + q];
            const double nv = in_series ? (double)obs[(size_t)j * ndays + d] : nan;
            const bool ov = tfin && finite_d(nv);
            const uint64_t ob = __ballot(ov);
            const int cnt = __popcll(ob);
            if (cnt < TWXQA_MIN_DAYS_MTH_WINDOW) continue;
            // more than one distinct value on either side (np.unique(...).size > 1, :960): any value unlike the first
            const int f = __ffsll((unsigned long long)ob) - 1;
            const double ft = __shfl(tobs, f), fn = __shfl(nv, f);
            if (__ballot(ov && tobs != ft) == 0 || __ballot(ov && nv != fn) == 0) continue;
            const double s_mean = wave_sum(ov ? tobs : 0.0) / cnt, n_mean = wave_sum(ov ? nv : 0.0) / cnt;
            const double ds = tobs - s_mean, dn = nv - n_mean;
            const double sxx = wave_sum(ov ? dn * dn : 0.0), sxy = wave_sum(ov ? dn * ds : 0.0);
            const double num = wave_sum(ov ? fabs(nv - tobs) : 0.0);
            const double den = wave_sum(ov ? fabs(nv - s_mean) + fabs(ds) : 0.0);
            const double slope = sxy / sxx;
            if (lane == 0) {
                NghEnt e;
                e.w = 1.0 - num / den;
                e.slope = slope;
                e.icpt = s_mean - slope * n_mean;
                e.col = j;
                e.pad = 0;
                ent[nvalid] = e;
            }
            ++nvalid;                                        // <= nngh <= TWXQA_MAX_RADIUS_NGH
        }
        if (nvalid < TWXQA_MIN_NGHS) st = TWXQA_SP_FEW_VALID;
    }

    if (st == TWXQA_SP_OK) {
        // ---- 2. sort by weight, largest first (qa_temp.py:982-992) -----------------------------------------------
        __syncthreads();
        for (int i = lane; i < nvalid; i += 64) {
            const double wi = ent[i].w;
            int rank = 0;
            for (int k = 0; k < nvalid; ++k) {
                const double wk = ent[k].w;
                rank += (wk > wi || (wk == wi && k < i)) ? 1 : 0;
            }
            order[rank] = (uint16_t)i;
        }
        __syncthreads();

        // ---- 3. the weighted estimate of every window day (qa_temp.py:886-924) -----------------------------------
        int n = 0;
        double swe = 0.0, sw = 0.0;
        for (int k = 0; k < nvalid; ++k) {                   // uniform
            const bool want = tfin && n < TWXQA_MAX_NGHS;
            if (__ballot(want) == 0) break;
            const NghEnt e = ent[order[k]];
            const double cv = in_series ? (double)obs[(size_t)e.col * ndays + d] : nan;
            const double pv = __shfl_up(cv, 1), xv = __shfl_down(cv, 1);
            if (want) {
                double best = nan, bd = 0.0;
                bool have = false;
                const double cand[3] = {pv, cv, xv};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double dif = fabs(cand[c] - tobs);
                    if (finite_d(cand[c]) && (!have || dif < bd)) { best = cand[c]; bd = dif; have = true; }
                }
                if (have) {
                    swe = swe + (e.icpt + e.slope * best) * e.w;
                    sw = sw + e.w;
                    ++n;
                }
            }
        }
        const bool has = tfin && n >= TWXQA_MIN_NGHS;
        const double ev = has ? swe / sw : nan;
        if (est && in_mth && has) est[((size_t)t * 2 + v) * ndays + d] = ev;

        // ---- 4. correlation, residuals, flags (qa_temp.py:927-937) -----------------------------------------------
        const int ne = __popcll(__ballot(has));
        if (ne < 2) {
            st = TWXQA_SP_DEGENERATE;
        } else {
            const double o_mean = wave_sum(has ? tobs : 0.0) / ne, e_mean = wave_sum(has ? ev : 0.0) / ne;
            const double xo = tobs - o_mean, xe = ev - e_mean;
            const double soo = wave_sum(has ? xo * xo : 0.0), see = wave_sum(has ? xe * xe : 0.0);
            const double soe = wave_sum(has ? xo * xe : 0.0);
            double r = soe / (sqrt(soo) * sqrt(see));
            if (r > 1.0) r = 1.0;
            if (r < -1.0) r = -1.0;
            r_out = r;
            if (!finite_d(r)) {
                st = TWXQA_SP_DEGENERATE;
            } else if (r >= SP_NGH_CORR) {
                const double resid = fabs(tobs - ev);
                const double r_mean = wave_sum(has ? resid : 0.0) / ne;
                const double rd = resid - r_mean;
                const double r_sd = sqrt(wave_sum(has ? rd * rd : 0.0) / ne);
                if (!(r_sd > 0.0) || !finite_d(r_sd)) {
                    st = TWXQA_SP_DEGENERATE;
                } else if (in_mth && has && resid >= SP_RESID_CUTOFF && fabs(rd / r_sd) >= SP_RESID_STD_CUTOFF) {
                    (v ? flag_tmax : flag_tmin)[(size_t)t * ndays + d] = 1;
                }
            }
        }
    }
    if (lane == 0) {
        item_r[item] = r_out;
        item_nvalid[item] = nvalid;
        item_status[item] = st;
    }
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
namespace {

int32_t ymd_from_days(int64_t z)                                 // the inverse of qa_days_from_civil, as yyyymmdd
{
    z += 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153;
    const int day = (int)(doy - (153 * mp + 2) / 5 + 1);
    const int mth = (int)(mp < 10 ? mp + 3 : mp - 9);
    const int64_t y = yoe + era * 400 + (mth <= 2);
    return (int32_t)(y * 10000 + mth * 100 + day);
}

}  // namespace

extern "C" int twxqa_spatial_nmonths(int64_t ndays, const int32_t *ymd)
{
    if (ndays < 1 || !ymd) return -1;
    const int32_t a = ymd[0], b = ymd[ndays - 1];
    const int64_t n = ((int64_t)(b / 10000) * 12 + (b / 100) % 100) - ((int64_t)(a / 10000) * 12 + (a / 100) % 100) + 1;
    return n >= 1 && n <= INT32_MAX ? (int)n : -1;
}

extern "C" int twxqa_spatial_regress(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                                     const float *tmin, const float *tmax, const int32_t *ymd, int64_t ntarget,
                                     const int32_t *target_idx, uint8_t *flag_tmin, uint8_t *flag_tmax, double *est,
                                     double *item_r, int32_t *item_nvalid, int32_t *item_status, float *kernel_ms,
                                     char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || ntarget < 1 || nstn > INT32_MAX || ndays > INT32_MAX - 64 || ntarget > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxqa_spatial_regress: need nstn >= 1, ndays >= 1 and ntarget >= 1");
    if (!lon || !lat || !tmin || !tmax || !ymd || !target_idx || !flag_tmin || !flag_tmax)
        return qa_fail(errbuf, errlen, "twxqa_spatial_regress: null buffer");
    char msg[192];
    for (int64_t i = 0; i < nstn; ++i) {
        if (!std::isfinite(lon[i]) || !std::isfinite(lat[i])) {
            snprintf(msg, sizeof msg, "twxqa_spatial_regress: non-finite longitude / latitude of station %lld", (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    for (int64_t i = 0; i < ntarget; ++i) {
        if (target_idx[i] < 0 || target_idx[i] >= nstn) {
            snprintf(msg, sizeof msg, "twxqa_spatial_regress: target index %d (entry %lld) outside [0, %lld)",
                     (int)target_idx[i], (long long)i, (long long)nstn);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    // the day axis: a valid first date, then consecutive calendar days
    const int32_t ymd0 = ymd[0];
    const int y0 = ymd0 / 10000, m0 = (ymd0 / 100) % 100, dd0 = ymd0 % 100;
    if (ymd0 < 10101 || m0 < 1 || m0 > 12 || dd0 < 1) return qa_fail(errbuf, errlen, "twxqa_spatial_regress: ymd[0] is not a date");
    const int64_t z0 = qa_days_from_civil(y0, m0, dd0);
    for (int64_t i = 0; i < ndays; ++i) {
        if (ymd_from_days(z0 + i) != ymd[i]) {
            snprintf(msg, sizeof msg, "twxqa_spatial_regress: ymd[%lld] = %d: the days are not consecutive calendar days",
                     (long long)i, (int)ymd[i]);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    // one item per calendar month the series touches: window [ws, we) = month -+ 15 days, month [ms, me), clipped
    const int nmonths = twxqa_spatial_nmonths(ndays, ymd);
    if (nmonths < 1 || (int64_t)nmonths * 2 * ntarget > INT32_MAX)
        return qa_fail(errbuf, errlen, "twxqa_spatial_regress: more than 2^31 - 1 items in one call");
    std::vector<int32_t> mon((size_t)nmonths * 4);
    for (int k = 0; k < nmonths; ++k) {
        const int mi = m0 - 1 + k, y = y0 + mi / 12, mth = mi % 12 + 1;
        const int64_t a = qa_days_from_civil(y, mth, 1) - z0;
        const int64_t b = qa_days_from_civil(mth == 12 ? y + 1 : y, mth == 12 ? 1 : mth + 1, 1) - z0;
        mon[4 * k + 0] = (int32_t)std::max<int64_t>(0, a - SP_MTH_BUFFER);
        mon[4 * k + 1] = (int32_t)std::min<int64_t>(ndays, b + SP_MTH_BUFFER);
        mon[4 * k + 2] = (int32_t)std::max<int64_t>(0, a);
        mon[4 * k + 3] = (int32_t)std::min<int64_t>(ndays, b);
    }
    const size_t nitems = (size_t)nmonths * 2 * (size_t)ntarget, nt = (size_t)ntarget, ns = (size_t)nstn, nd = (size_t)ndays;

    QACHK(hipSetDevice(device));
    QaBuf b_geo, b_obs, b_tgt, b_csr, b_flag, b_est, b_item;
    QACHK(hipMalloc(&b_geo.p, ns * 16));
    double *d_lon = static_cast<double *>(b_geo.p), *d_lat = d_lon + ns;
    QACHK(hipMemcpy(d_lon, lon, ns * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_lat, lat, ns * 8, hipMemcpyHostToDevice));
    // per target: csr offsets (int64, nt + 1), index, count, status; then the month table
    const size_t off_off = 0, off_idx = off_off + (nt + 1) * 8, off_cnt = off_idx + nt * 4, off_st = off_cnt + nt * 4,
                 off_mon = (off_st + nt * 4 + 15) / 16 * 16, tgt_total = off_mon + (size_t)nmonths * 16;
    QACHK(hipMalloc(&b_tgt.p, tgt_total));
    char *dt = static_cast<char *>(b_tgt.p);
    int64_t *d_off = (int64_t *)(dt + off_off);
    int32_t *d_idx = (int32_t *)(dt + off_idx), *d_cnt = (int32_t *)(dt + off_cnt), *d_st = (int32_t *)(dt + off_st);
    QACHK(hipMemcpy(d_idx, target_idx, nt * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(dt + off_mon, mon.data(), (size_t)nmonths * 16, hipMemcpyHostToDevice));
    QaTimer tm, tm_fill;                                     // two pairs: the count pass is read after the fill pass
    QACHK(tm.init());
    QACHK(tm_fill.init());

    // ---- the radius lists: count, scan on the host, fill ---------------------------------------------------------
    const dim3 rgrid((unsigned)((ntarget + 3) / 4));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_qa_radius, rgrid, dim3(256), 0, nullptr, nstn, (const double *)d_lon, (const double *)d_lat, ntarget,
                       (const int32_t *)d_idx, 0, d_cnt, (const int64_t *)nullptr, (int32_t *)nullptr);
    QACHK(hipGetLastError());
    QACHK(hipEventRecord(tm.b, nullptr));                    // not stop_set(): the copy of the counts below waits for it
    std::vector<int32_t> cnt(nt), tst(nt);
    std::vector<int64_t> off(nt + 1);
    QACHK(hipMemcpy(cnt.data(), d_cnt, nt * 4, hipMemcpyDeviceToHost));
    off[0] = 0;
    for (size_t i = 0; i < nt; ++i) {                        // a list above the cap is not built: the target says so
        tst[i] = cnt[i] > TWXQA_MAX_RADIUS_NGH ? TWXQA_SP_NGH_CAP : TWXQA_SP_OK;
        off[i + 1] = off[i] + (tst[i] == TWXQA_SP_OK ? cnt[i] : 0);
    }
    QACHK(hipMemcpy(d_off, off.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_st, tst.data(), nt * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_csr.p, std::max<size_t>(4, (size_t)off[nt] * 4)));
    int32_t *d_csr = static_cast<int32_t *>(b_csr.p);
    float ms_fill = 0.0f;
    if (off[nt] > 0) {
        QACHK(tm_fill.start());
        hipLaunchKernelGGL(k_qa_radius, rgrid, dim3(256), 0, nullptr, nstn, (const double *)d_lon, (const double *)d_lat,
                           ntarget, (const int32_t *)d_idx, 1, d_cnt, (const int64_t *)d_off, d_csr);
        QACHK(hipGetLastError());
        QACHK(tm_fill.stop_set(&ms_fill));
    }
    float ms_count = 0.0f;
    QACHK(hipEventElapsedTime(&ms_count, tm.a, tm.b));

    // ---- the items ----------------------------------------------------------------------------------------------
    QACHK(hipMalloc(&b_obs.p, 2 * ns * nd * 4));
    float *d_tmin = static_cast<float *>(b_obs.p), *d_tmax = d_tmin + ns * nd;
    QACHK(hipMemcpy(d_tmin, tmin, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_tmax, tmax, ns * nd * 4, hipMemcpyHostToDevice));
    QACHK(hipMalloc(&b_flag.p, 2 * nt * nd));
    uint8_t *d_fmin = static_cast<uint8_t *>(b_flag.p), *d_fmax = d_fmin + nt * nd;
    QACHK(hipMemset(d_fmin, 0, 2 * nt * nd));
    double *d_est = nullptr;
    if (est) {                                               // all-ones bytes are a NaN: days without an estimate stay so
        QACHK(hipMalloc(&b_est.p, nt * 2 * nd * 8));
        d_est = static_cast<double *>(b_est.p);
        QACHK(hipMemset(d_est, 0xff, nt * 2 * nd * 8));
    }
    QACHK(hipMalloc(&b_item.p, nitems * 16));
    double *d_r = static_cast<double *>(b_item.p);
    int32_t *d_nv = (int32_t *)(d_r + nitems), *d_ist = d_nv + nitems;
    QACHK(tm.start());
    hipLaunchKernelGGL(k_spatial_regress, dim3((unsigned)nitems), dim3(64), 0, nullptr, ndays, nmonths, (const float *)d_tmin,
                       (const float *)d_tmax, (const int4 *)(dt + off_mon), (const int32_t *)d_idx, (const int32_t *)d_st,
                       (const int64_t *)d_off, (const int32_t *)d_csr, d_fmin, d_fmax, d_est, d_r, d_nv, d_ist);
    QACHK(hipGetLastError());
    float ms_items = 0.0f;
    QACHK(tm.stop_set(&ms_items));
    if (kernel_ms) { kernel_ms[0] = ms_count + ms_fill; kernel_ms[1] = ms_items; }
    QACHK(hipMemcpy(flag_tmin, d_fmin, nt * nd, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(flag_tmax, d_fmax, nt * nd, hipMemcpyDeviceToHost));
    if (est) QACHK(hipMemcpy(est, d_est, nt * 2 * nd * 8, hipMemcpyDeviceToHost));
    if (item_r) QACHK(hipMemcpy(item_r, d_r, nitems * 8, hipMemcpyDeviceToHost));
    if (item_nvalid) QACHK(hipMemcpy(item_nvalid, d_nv, nitems * 4, hipMemcpyDeviceToHost));
    if (item_status) QACHK(hipMemcpy(item_status, d_ist, nitems * 4, hipMemcpyDeviceToHost));
    return 0;
}
