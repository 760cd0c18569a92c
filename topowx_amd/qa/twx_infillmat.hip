// twx_infillmat.hip -- libtwxqa.so: the neighbour matrices of the infill family (step14 / step15 / step16): the first
// pass of _InfillMatrix (twx/infill/infill_normals.py:52-237), the widening loop of _InfillMatrix.infill (:324-343 with
// __extend_ngh_radius / __merge / __has_min_daily_nghs) and _shrink_matrix (:391-420), for all targets and day groups
// of one call (include/twx_qa.h, twxif_infill_matrix).  Its own translation unit; the helpers it shares with the
// other units of the library (the haversine, the wave sums, the buffer list, the event timer) are twx_qa_common.h's.
//
// An item is (target, day group).  The rings of a target -- (−1, 75], (75, 112.5], ... with an empty ring grown by
// 37.5 km until it holds a station -- depend on distances only, so every item of a target sees the same sequence of
// rings and consumes a prefix of it.  The host drives rounds: round r runs ring r for the targets that still have an
// unsatisfied item, and ends with one small copy of the items' done bytes.
//
// k_if_ring: one wavefront per active target.  Pass A: the nearest eligible station beyond the inner radius (none: the
// target is exhausted), from it the outer radius by the reference's own additions of 37.5.  Pass B: the stations of the
// ring into LDS, rank-sorted by distance (equal distances in table order).  LDS 12 bytes per ring station.  Both passes
// leave out the target itself and the one row of exclude_idx (twxxv_infill_matrix, step15: the full record of the
// station whose masked series is the target; -1 for twxif_infill_matrix).
//
// k_if_pair: one wavefront per (active target, ring station), all groups.  The host sorts the used days by group once
// (perm / goff), so a group is a run of that list and nothing is indexed by a run-time group number.  Per group, pass 1
// counts the neighbour's finite days (nlap), the days finite in both (nlap_stn) and sums the target over those; where
// nlap_stn reaches the target's threshold, pass 2 sums |p - o| and |p - mean| + |o - mean| (the rows come back from L2).
// A lane sums its days i = lane, lane + 64, ... in order and the 64 partial sums are combined by an xor butterfly: a
// fixed order, the same bits in every call.
//
// k_if_item: one workgroup of 256 per unsatisfied item.  Thread 0 scans the ring in distance order (acceptance, the
// best-short-record candidate of the first ring) and the first station that fails decides the item: a zero d1
// denominator at a station the reference would rank or weigh as a candidate (TWXIF_NUMERIC), or a full-record station
// that would be entry 257 of the list (TWXIF_NGH_CAP; at one station the denominator is looked at first); a kept
// candidate is appended after the scan and can only hit the cap; the ranked list, old and new, is rank-sorted by ioa
// descending (equal ioa: the larger distance first, then table order); a thread owns the days i = tid, tid + 256, ... of the item and
// finds the rank of each day's third finite column, nnghs is the block maximum; the shrink is the same walk with a
// per-day count (one byte per day in a global workspace, touched by its owning thread only) and a block-wide "any"
// per column.
// LDS of k_if_item, per workgroup: the ranked list 28 B x 256 (ioa, distance, row, nlap, nlap_stn), the ring
// 28 B x 256 (row, distance, nlap, nlap_stn, ioa), the sorted rows 4 B x 256, 1 KiB of reduction scratch = 16 KiB:
// the 8 workgroups that fill the 32 wave slots of a compute unit take 128 KiB of its 160 KiB.  A cap of 512 would
// take 31 KiB and leave room for 5.
//
// k_if_compact: the per-item lists (capacity 256 each) into the caller's CSR arrays.
// fp64 throughout on float32 observations widened exactly; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_series.h"

#define IF_CAP TWXQA_MAX_RADIUS_NGH
#define IF_IOA_DENOM0 (-2.0)                 // pair marker: the d1 denominator is 0 (d1 itself lies in [0, 1])
#define IF_RING_EXHAUSTED (-1)
#define IF_RING_OVERFLOW (-2)
#define IF_NOT_REACHED 0x7fffffff

__global__ __launch_bounds__(64) void k_if_ring(int64_t nstn, const double *__restrict__ lon,
                                                const double *__restrict__ lat, const uint8_t *__restrict__ elig,
                                                const int32_t *__restrict__ target_idx,
                                                const int32_t *__restrict__ exclude_idx, const int32_t *__restrict__ act_t,
                                                int first, double *__restrict__ cur_max, int32_t *__restrict__ ring_n,
                                                int32_t *__restrict__ ring_idx, double *__restrict__ ring_dist)
{
    __shared__ double ld[IF_CAP];
    __shared__ int32_t lj[IF_CAP];
    const int lane = threadIdx.x;
    const int64_t t = act_t[blockIdx.x];
    const int32_t self = target_idx[t], excl = exclude_idx[t];   // excl: -1 (no row has it) or the row twxxv_ leaves out
    const double lat1rad = lat[self] * QA_RADIAN, lon1rad = lon[self] * QA_RADIAN;
    const double cos1 = cos(lat1rad);
    const double rin = first ? -1.0 : cur_max[t];                // the reference's dists > min_dist, min_dist = -1
    // ---- pass A: the nearest eligible station beyond rin --------------------------------------------------------
    double dmin = __builtin_inf();
    for (int64_t j0 = 0; j0 < nstn; j0 += 64) {                  // uniform
        const int64_t j = j0 + lane;
        if (j < nstn && j != self && j != excl && elig[j]) {
            const double d = qa_dist_km(lat1rad, lon1rad, cos1, lat[j], lon[j]);
            if (d > rin && d < dmin) dmin = d;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) dmin = fmin(dmin, __shfl_xor(dmin, m, 64));
    if (!(dmin < __builtin_inf())) {                             // uniform: no station left (the reference loops forever)
        if (lane == 0) ring_n[t] = IF_RING_EXHAUSTED;
        return;
    }
    double rout = first ? TWXQA_NGH_RADIUS_KM : rin + TWXIF_RING_KM;
    while (!(dmin <= rout)) rout += TWXIF_RING_KM;   // infill_normals.py:124-126; dmin is finite
    // ---- pass B: the ring, in LDS ---------------------------------------------------------------------------------
    int32_t n = 0;
    for (int64_t j0 = 0; j0 < nstn; j0 += 64) {                  // uniform
        const int64_t j = j0 + lane;
        bool in = false;
        double d = 0.0;
        if (j < nstn && j != self && j != excl && elig[j]) {
            d = qa_dist_km(lat1rad, lon1rad, cos1, lat[j], lon[j]);
            in = d > rin && d <= rout;
        }
        const uint64_t b = __ballot(in);
        if (in) {
            const int k = n + __popcll(b & (((uint64_t)1 << lane) - 1));
            if (k < IF_CAP) { ld[k] = d; lj[k] = (int32_t)j; }
        }
        n += __popcll(b);
    }
    if (lane == 0) cur_max[t] = rout;
    if (n > IF_CAP) {                                            // uniform
        if (lane == 0) ring_n[t] = IF_RING_OVERFLOW;
        return;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {                         // rank sort: ascending distance, then table order
        const double di = ld[i];
        int rank = 0;
        for (int k = 0; k < n; ++k) {
            const double dk = ld[k];
            rank += (dk < di || (dk == di && k < i)) ? 1 : 0;
        }
        ring_idx[t * IF_CAP + rank] = lj[i];
        ring_dist[t * IF_CAP + rank] = di;
    }
    if (lane == 0) ring_n[t] = n;
}

__global__ __launch_bounds__(256) void k_if_pair(int64_t ndays, const float *__restrict__ obs,
                                                 const int32_t *__restrict__ target_idx,
                                                 const int32_t *__restrict__ act_t, int ngroups,
                                                 const int32_t *__restrict__ perm, const int32_t *__restrict__ goff,
                                                 const int32_t *__restrict__ thr_por, const uint8_t *__restrict__ it_done,
                                                 const int32_t *__restrict__ ring_n, const int32_t *__restrict__ ring_idx,
                                                 int32_t *__restrict__ p_nlap, int32_t *__restrict__ p_nst,
                                                 double *__restrict__ p_ioa)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = act_t[blockIdx.x];
    const int slot = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (slot >= ring_n[t]) return;                               // wave-uniform (also the exhausted / overflow marks)
    const float *__restrict__ o_row = obs + (int64_t)target_idx[t] * ndays;
    const float *__restrict__ p_row = obs + (int64_t)ring_idx[t * IF_CAP + slot] * ndays;
    for (int g = 0; g < ngroups; ++g) {                          // uniform
        const int64_t out = (t * IF_CAP + slot) * ngroups + g;
        if (it_done[t * ngroups + g]) continue;                  // uniform: nobody reads this group's result
        const int a = goff[g], b = goff[g + 1];
        int nlap = 0, nst = 0;
        double so = 0.0;
        for (int i = a + lane; i < b; i += 64) {
            const int d = perm[i];
            const float o = o_row[d], p = p_row[d];
            const bool fp = qa_finitef(p), fb = fp && qa_finitef(o);
            nlap += fp ? 1 : 0;
            nst += fb ? 1 : 0;
            if (fb) so = so + (double)o;
        }
        nlap = qa_wave_sum_i(nlap);
        nst = qa_wave_sum_i(nst);
        double ioa = __builtin_nan("");                          // not needed: below the target's threshold
        if (nst > 0 && nst >= thr_por[t * ngroups + g]) {        // uniform
            const double mean = qa_wave_sum(so) / (double)nst;      // np.mean of the overlap
            double num = 0.0, den = 0.0;
            for (int i = a + lane; i < b; i += 64) {
                const int d = perm[i];
                const float of = o_row[d], pf = p_row[d];
                if (qa_finitef(pf) && qa_finitef(of)) {
                    const double o = (double)of, p = (double)pf;
                    num = num + fabs(p - o);
                    den = den + (fabs(p - mean) + fabs(o - mean));
                }
            }
            num = qa_wave_sum(num);
            den = qa_wave_sum(den);
            ioa = den == 0.0 ? IF_IOA_DENOM0 : 1.0 - num / den;  // perf_metrics.py:59-62
        }
        if (lane == 0) { p_nlap[out] = nlap; p_nst[out] = nst; p_ioa[out] = ioa; }
    }
}

__global__ __launch_bounds__(256) void k_if_item(int64_t ndays, const float *__restrict__ obs, int ngroups,
                                                 const int32_t *__restrict__ act_item, const int32_t *__restrict__ perm,
                                                 const int32_t *__restrict__ goff, const int32_t *__restrict__ thr_all,
                                                 const int32_t *__restrict__ thr_por, int first, int min_nnghs,
                                                 const double *__restrict__ cur_max, const int32_t *__restrict__ ring_n,
                                                 const int32_t *__restrict__ ring_idx, const double *__restrict__ ring_dist,
                                                 const int32_t *__restrict__ p_nlap, const int32_t *__restrict__ p_nst,
                                                 const double *__restrict__ p_ioa, uint8_t *__restrict__ it_done,
                                                 int32_t *__restrict__ it_status, int32_t *__restrict__ it_nnghs,
                                                 double *__restrict__ it_maxdist, int32_t *__restrict__ it_n,
                                                 int32_t *__restrict__ l_idx, double *__restrict__ l_ioa,
                                                 double *__restrict__ l_dist, int32_t *__restrict__ l_nlap,
                                                 int32_t *__restrict__ l_nst, uint8_t *__restrict__ l_keep,
                                                 uint8_t *__restrict__ daycnt)
{
    __shared__ double s_ioa[IF_CAP], s_dist[IF_CAP], r_ioa[IF_CAP], r_dist[IF_CAP];
    __shared__ int32_t s_idx[IF_CAP], s_nlap[IF_CAP], s_nst[IF_CAP], r_idx[IF_CAP], r_nlap[IF_CAP], r_nst[IF_CAP];
    __shared__ int32_t s_sorted[IF_CAP];
    __shared__ int32_t red[256];
    __shared__ int32_t sh_n, sh_fail;
    const int tid = threadIdx.x;
    const int64_t item = act_item[blockIdx.x];
    const int64_t t = item / ngroups;
    const int g = (int)(item % ngroups);
    const int64_t base = item * IF_CAP;
    const int rn = ring_n[t];
    if (rn < 0) {                                                // uniform
        if (tid == 0) {
            it_done[item] = 1;
            if (rn == IF_RING_EXHAUSTED) it_status[item] = TWXIF_UNSATISFIED;    // the list stays as far as it got
            else { it_status[item] = TWXIF_NGH_CAP; it_n[item] = 0; it_maxdist[item] = cur_max[t]; }
        }
        return;
    }
    const int n0 = it_n[item];
    if (tid < n0) {
        s_ioa[tid] = l_ioa[base + tid]; s_dist[tid] = l_dist[base + tid]; s_idx[tid] = l_idx[base + tid];
        s_nlap[tid] = l_nlap[base + tid]; s_nst[tid] = l_nst[base + tid];
    }
    if (tid < rn) {
        const int64_t r = t * IF_CAP + tid;
        r_idx[tid] = ring_idx[r]; r_dist[tid] = ring_dist[r];
        r_nlap[tid] = p_nlap[r * ngroups + g]; r_nst[tid] = p_nst[r * ngroups + g]; r_ioa[tid] = p_ioa[r * ngroups + g];
    }
    __syncthreads();
    // ---- the scan of the ring in distance order (infill_normals.py:151-186) ---------------------------------------
    if (tid == 0) {
        const int ta = thr_all[g], tp = thr_por[item];
        int n = n0, fail = 0, cand = -1;
        double best = 0.0, maxioa = 0.0;
        for (int x = 0; x < rn; ++x) {
            if (r_nst[x] < tp) continue;
            const bool full = r_nlap[x] >= ta;
            if (!full && !first) continue;
            const double v = r_ioa[x];
            if (v == IF_IOA_DENOM0 || !(v == v)) { fail = TWXIF_NUMERIC; break; }
            if (full) {
                if (n >= IF_CAP) { fail = TWXIF_NGH_CAP; break; }
                s_ioa[n] = v; s_dist[n] = r_dist[x]; s_idx[n] = r_idx[x]; s_nlap[n] = r_nlap[x]; s_nst[n] = r_nst[x];
                ++n;
                maxioa = v > maxioa ? v : maxioa;
            } else if (v > best) {
                cand = x;
                best = v;
            }
        }
        if (!fail && cand >= 0 && !(best < maxioa) && !(best < TWXIF_BESTNGH_MIN_IOA)) {       // (:182-186; best >= every displaced candidate)
            if (n >= IF_CAP) fail = TWXIF_NGH_CAP;
            else {
                s_ioa[n] = best; s_dist[n] = r_dist[cand]; s_idx[n] = r_idx[cand]; s_nlap[n] = r_nlap[cand];
                s_nst[n] = r_nst[cand];
                ++n;
            }
        }
        sh_n = n;
        sh_fail = fail;
    }
    __syncthreads();
    if (sh_fail) {                                               // uniform
        if (tid == 0) { it_done[item] = 1; it_status[item] = sh_fail; it_n[item] = 0; it_maxdist[item] = cur_max[t]; }
        return;
    }
    const int n = sh_n;
    // ---- rank sort: ioa descending, equal ioa the larger distance first, then table order ---------------------------
    if (tid < n) {
        const double vi = s_ioa[tid], di = s_dist[tid];
        const int32_t ji = s_idx[tid];
        int rank = 0;
        for (int k = 0; k < n; ++k) {
            const double vk = s_ioa[k], dk = s_dist[k];
            rank += (vk > vi || (vk == vi && (dk > di || (dk == di && s_idx[k] < ji)))) ? 1 : 0;
        }
        s_sorted[rank] = ji;
        l_ioa[base + rank] = vi; l_dist[base + rank] = di; l_idx[base + rank] = ji;
        l_nlap[base + rank] = s_nlap[tid]; l_nst[base + rank] = s_nst[tid];
        l_keep[base + rank] = 0;
    }
    if (tid == 0) { it_n[item] = n; it_maxdist[item] = cur_max[t]; }
    __syncthreads();
    // ---- the selection loop (:324-343) in closed form ---------------------------------------------------------------
    int nn = it_nnghs[item];
    if (n < nn) return;                                          // uniform: the next ring
    const int a = goff[g], b = goff[g + 1];
    int m = 0;                                                   // the largest rank of a day's min_nnghs-th finite column
    for (int i = a + tid; i < b; i += 256) {
        const int64_t d = perm[i];
        int cnt = 0, c = 0;
        for (; c < n && cnt < min_nnghs; ++c) cnt += qa_finitef(obs[(int64_t)s_sorted[c] * ndays + d]) ? 1 : 0;
        const int pos = cnt >= min_nnghs ? c : IF_NOT_REACHED;
        m = pos > m ? pos : m;
    }
    red[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] > red[tid + s] ? red[tid] : red[tid + s];
        __syncthreads();
    }
    m = red[0];
    if (m > n) {                                                 // uniform: some day is short even with all n columns
        if (tid == 0) it_nnghs[item] = n + 1;
        return;
    }
    nn = m > nn ? m : nn;
    // ---- _shrink_matrix (:391-420) on the first nn columns ----------------------------------------------------------
    uint8_t *cnt_row = daycnt + t * ndays;                       // the item's days are its own: groups do not share days
    for (int c = 0; c < nn; ++c) {                               // uniform
        const float *col = obs + (int64_t)s_sorted[c] * ndays;
        int keep = 1;
        if (c >= min_nnghs) {
            int adds = 0;
            for (int i = a + tid; i < b; i += 256) {
                const int d = perm[i];
                adds |= (qa_finitef(col[d]) && cnt_row[d] < min_nnghs) ? 1 : 0;
            }
            keep = __syncthreads_or(adds);
        }
        if (keep) {
            for (int i = a + tid; i < b; i += 256) {
                const int d = perm[i];
                const int prev = c == 0 ? 0 : cnt_row[d];
                cnt_row[d] = (uint8_t)(prev + ((qa_finitef(col[d]) && prev < min_nnghs) ? 1 : 0));
            }
        }
        if (tid == 0) l_keep[base + c] = (uint8_t)keep;
    }
    if (tid == 0) { it_nnghs[item] = nn; it_status[item] = TWXIF_OK; it_done[item] = 1; }
}

__global__ __launch_bounds__(256) void k_if_compact(const int32_t *__restrict__ it_n, const int64_t *__restrict__ off,
                                                    const int32_t *__restrict__ l_idx, const double *__restrict__ l_ioa,
                                                    const double *__restrict__ l_dist, const int32_t *__restrict__ l_nlap,
                                                    const int32_t *__restrict__ l_nst, const uint8_t *__restrict__ l_keep,
                                                    int32_t *__restrict__ o_idx, double *__restrict__ o_ioa,
                                                    double *__restrict__ o_dist, int32_t *__restrict__ o_nlap,
                                                    int32_t *__restrict__ o_nst, uint8_t *__restrict__ o_keep)
{
    const int64_t item = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid >= it_n[item]) return;
    const int64_t src = item * IF_CAP + tid, dst = off[item] + tid;
    o_idx[dst] = l_idx[src]; o_ioa[dst] = l_ioa[src]; o_dist[dst] = l_dist[src];
    o_nlap[dst] = l_nlap[src]; o_nst[dst] = l_nst[src]; o_keep[dst] = l_keep[src];
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
namespace {

// the first index whose date is not the day after the one before it; -1: consecutive calendar days
int64_t if_first_gap(int64_t ndays, const int32_t *ymd)
{
    static const int mlen[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    int y = ymd[0] / 10000, mth = (ymd[0] / 100) % 100, day = ymd[0] % 100;
    if (ymd[0] < 10101 || mth < 1 || mth > 12 || day < 1 || day > mlen[mth - 1] + ((mth == 2 && qa_leap(y)) ? 1 : 0)) return 0;
    for (int64_t i = 0; i < ndays; ++i) {
        if (ymd[i] != y * 10000 + mth * 100 + day) return i;
        if (++day > mlen[mth - 1] + ((mth == 2 && qa_leap(y)) ? 1 : 0)) {
            day = 1;
            if (++mth > 12) { mth = 1; ++y; }
        }
    }
    return -1;
}

}  // namespace

// the driver of twxif_infill_matrix and twxxv_infill_matrix; exclude_idx: nullptr (no exclusion) or [ntarget]
static int if_matrix(const char *fn, int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                     const float *obs, const int32_t *ymd, const uint8_t *eligible, int64_t ntarget,
                     const int32_t *target_idx, const int32_t *exclude_idx, int32_t ngroups, const int8_t *group,
                     const int32_t *nthres_all, const int32_t *nthres_target_por, int32_t min_daily_nnghs,
                     int32_t *status, int32_t *nnghs, double *max_dist, int64_t *csr_off, int64_t csr_cap,
                     int32_t *ngh_idx, double *ngh_ioa, double *ngh_dist, int32_t *ngh_nlap, int32_t *ngh_nlap_stn,
                     uint8_t *keep, int32_t *nrounds, float *kernel_ms, char *errbuf, int errlen)
{
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || ndays < 1 || ntarget < 1 || nstn > INT32_MAX || ndays > INT32_MAX || ngroups < 1 ||
        ngroups > TWXIF_MAX_GROUPS || min_daily_nnghs < 1 || min_daily_nnghs > TWXIF_MAX_MIN_NNGHS ||
        ntarget * (int64_t)ngroups > INT32_MAX / 2) {
        snprintf(msg, sizeof msg, "%s: need nstn, ndays, ntarget >= 1, 1 <= ngroups <= %d and 1 <= min_daily_nnghs <= %d",
                 fn, TWXIF_MAX_GROUPS, TWXIF_MAX_MIN_NNGHS);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!lon || !lat || !obs || !ymd || !eligible || !target_idx || !group || !nthres_all || !nthres_target_por ||
        !status || !nnghs || !max_dist || !csr_off || !ngh_idx || !ngh_ioa || !ngh_dist || !ngh_nlap || !ngh_nlap_stn ||
        !keep || csr_cap < 0) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    const int64_t gap = if_first_gap(ndays, ymd);
    if (gap >= 0) {
        snprintf(msg, sizeof msg, "%s: ymd[%lld] = %d: the days are not consecutive calendar days", fn, (long long)gap,
                 (int)ymd[gap]);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t j = 0; j < nstn; ++j)
        if (!std::isfinite(lon[j]) || !std::isfinite(lat[j])) {
            snprintf(msg, sizeof msg, "%s: station %lld has a non-finite longitude / latitude", fn, (long long)j);
            return qa_fail(errbuf, errlen, msg);
        }
    for (int64_t t = 0; t < ntarget; ++t)
        if (target_idx[t] < 0 || target_idx[t] >= nstn) {
            snprintf(msg, sizeof msg, "%s: target index %d outside [0, %lld)", fn, (int)target_idx[t], (long long)nstn);
            return qa_fail(errbuf, errlen, msg);
        }
    for (int64_t t = 0; exclude_idx && t < ntarget; ++t)
        if (exclude_idx[t] < -1 || exclude_idx[t] >= nstn) {
            snprintf(msg, sizeof msg, "%s: exclude index %d outside -1 .. %lld", fn, (int)exclude_idx[t], (long long)nstn - 1);
            return qa_fail(errbuf, errlen, msg);
        }
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
    std::vector<int32_t> perm((size_t)goff[(size_t)ngroups]), fillpos(goff.begin(), goff.end() - 1);
    for (int64_t d = 0; d < ndays; ++d)
        if (group[d] >= 0) perm[(size_t)fillpos[(size_t)group[d]]++] = (int32_t)d;

    const int64_t ni = ntarget * ngroups;
    std::vector<uint8_t> done((size_t)ni, 0);
    std::vector<int32_t> h_status((size_t)ni, TWXIF_UNSATISFIED), h_nnghs((size_t)ni, min_daily_nnghs), h_n((size_t)ni, 0);
    std::vector<double> h_maxdist((size_t)ni, std::nan(""));
    for (int64_t i = 0; i < ni; ++i) {
        if (nthres_target_por[i] < 0 || nthres_all[i % ngroups] < 0) {
            snprintf(msg, sizeof msg, "%s: negative threshold of item %lld", fn, (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
        if (nthres_target_por[i] == 0) { done[(size_t)i] = 1; h_status[(size_t)i] = TWXIF_NO_TARGET_OBS; }
    }

    QACHK(hipSetDevice(device));
    const auto t_up = std::chrono::steady_clock::now();
    QaPool bufs;
    double *d_lon, *d_lat, *d_curmax, *d_rdist, *d_pioa, *d_maxdist, *d_lioa, *d_ldist;
    float *d_obs;
    uint8_t *d_elig, *d_done, *d_lkeep, *d_daycnt;
    int32_t *d_tidx, *d_excl, *d_actt, *d_acti, *d_perm, *d_goff, *d_thrall, *d_thrpor, *d_ringn, *d_ridx, *d_pnlap, *d_pnst,
        *d_status, *d_nnghs, *d_n, *d_lidx, *d_lnlap, *d_lnst;
    const size_t NS = (size_t)nstn, ND = (size_t)ndays, NT = (size_t)ntarget, NI = (size_t)ni, G = (size_t)ngroups;
    QAALLOC(bufs, d_lon, double, NS); QAALLOC(bufs, d_lat, double, NS); QAALLOC(bufs, d_elig, uint8_t, NS);
    QAALLOC(bufs, d_obs, float, NS * ND);
    QAALLOC(bufs, d_tidx, int32_t, NT); QAALLOC(bufs, d_excl, int32_t, NT); QAALLOC(bufs, d_actt, int32_t, NT);
    QAALLOC(bufs, d_acti, int32_t, NI);
    QAALLOC(bufs, d_perm, int32_t, perm.size()); QAALLOC(bufs, d_goff, int32_t, G + 1);
    QAALLOC(bufs, d_thrall, int32_t, G); QAALLOC(bufs, d_thrpor, int32_t, NI);
    QAALLOC(bufs, d_curmax, double, NT); QAALLOC(bufs, d_ringn, int32_t, NT);
    QAALLOC(bufs, d_ridx, int32_t, NT * IF_CAP); QAALLOC(bufs, d_rdist, double, NT * IF_CAP);
    QAALLOC(bufs, d_pnlap, int32_t, NT * IF_CAP * G); QAALLOC(bufs, d_pnst, int32_t, NT * IF_CAP * G);
    QAALLOC(bufs, d_pioa, double, NT * IF_CAP * G);
    QAALLOC(bufs, d_done, uint8_t, NI); QAALLOC(bufs, d_status, int32_t, NI); QAALLOC(bufs, d_nnghs, int32_t, NI);
    QAALLOC(bufs, d_maxdist, double, NI); QAALLOC(bufs, d_n, int32_t, NI);
    QAALLOC(bufs, d_lidx, int32_t, NI * IF_CAP); QAALLOC(bufs, d_lioa, double, NI * IF_CAP); QAALLOC(bufs, d_ldist, double, NI * IF_CAP);
    QAALLOC(bufs, d_lnlap, int32_t, NI * IF_CAP); QAALLOC(bufs, d_lnst, int32_t, NI * IF_CAP); QAALLOC(bufs, d_lkeep, uint8_t, NI * IF_CAP);
    QAALLOC(bufs, d_daycnt, uint8_t, NT * ND);
    QACHK(hipMemcpy(d_lon, lon, NS * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_lat, lat, NS * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_elig, eligible, NS, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_obs, obs, NS * ND * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_tidx, target_idx, NT * 4, hipMemcpyHostToDevice));
    if (exclude_idx) QACHK(hipMemcpy(d_excl, exclude_idx, NT * 4, hipMemcpyHostToDevice));
    else QACHK(hipMemset(d_excl, 0xff, NT * 4));                 // -1: no station has that row
    if (!perm.empty()) QACHK(hipMemcpy(d_perm, perm.data(), perm.size() * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_goff, goff.data(), (G + 1) * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_thrall, nthres_all, G * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_thrpor, nthres_target_por, NI * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_done, done.data(), NI, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_status, h_status.data(), NI * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_nnghs, h_nnghs.data(), NI * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(d_maxdist, h_maxdist.data(), NI * 8, hipMemcpyHostToDevice));
    QACHK(hipMemset(d_n, 0, NI * 4));
    QACHK(hipMemset(d_lkeep, 0, NI * IF_CAP));

    QaTimer tm;
    float ms[TWXIF_NTIMES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (kernel_ms) {
        QACHK(tm.init());
        QACHK(hipDeviceSynchronize());
        ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_up).count();
    }
    std::vector<int32_t> h_ringn((size_t)ntarget, 0);
    std::vector<int32_t> act_t, act_i;
    int rounds = 0;
    for (;; ++rounds) {
        act_t.clear();
        act_i.clear();
        for (int64_t t = 0; t < ntarget; ++t) {
            bool any = false;
            for (int g = 0; g < ngroups; ++g)
                if (!done[(size_t)(t * ngroups + g)]) { act_i.push_back((int32_t)(t * ngroups + g)); any = true; }
            if (any) act_t.push_back((int32_t)t);
        }
        if (act_t.empty()) break;
        if (rounds > nstn + 1) {                                 // every round takes a station of each active target, or ends it
            snprintf(msg, sizeof msg, "%s: internal error: %d rounds for %lld stations", fn, rounds, (long long)nstn);
            return qa_fail(errbuf, errlen, msg);
        }
        const int first = rounds == 0 ? 1 : 0;
        QACHK(hipMemcpy(d_actt, act_t.data(), act_t.size() * 4, hipMemcpyHostToDevice));
        QACHK(hipMemcpy(d_acti, act_i.data(), act_i.size() * 4, hipMemcpyHostToDevice));
        if (kernel_ms) QACHK(tm.start());
        hipLaunchKernelGGL(k_if_ring, dim3((unsigned)act_t.size()), dim3(64), 0, nullptr, nstn, (const double *)d_lon,
                           (const double *)d_lat, (const uint8_t *)d_elig, (const int32_t *)d_tidx,
                           (const int32_t *)d_excl, (const int32_t *)d_actt, first, d_curmax, d_ringn, d_ridx, d_rdist);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        // the pair grid is sized by the round's largest ring (about 26 stations on a real pool, not the cap of 256)
        QACHK(hipMemcpy(h_ringn.data(), d_ringn, NT * 4, hipMemcpyDeviceToHost));
        int ring_max = 0;
        for (int32_t t : act_t) ring_max = h_ringn[(size_t)t] > ring_max ? h_ringn[(size_t)t] : ring_max;
        const unsigned pair_rows = (unsigned)((ring_max + 3) / 4);
        if (kernel_ms) QACHK(tm.start());
        if (pair_rows > 0) {
            hipLaunchKernelGGL(k_if_pair, dim3((unsigned)act_t.size(), pair_rows), dim3(256), 0, nullptr, ndays,
                               (const float *)d_obs, (const int32_t *)d_tidx, (const int32_t *)d_actt, (int)ngroups,
                               (const int32_t *)d_perm, (const int32_t *)d_goff, (const int32_t *)d_thrpor,
                               (const uint8_t *)d_done, (const int32_t *)d_ringn, (const int32_t *)d_ridx, d_pnlap, d_pnst,
                               d_pioa);
        }
        QACHK(hipGetLastError());
        if (kernel_ms) { QACHK(tm.stop_add(&ms[1])); QACHK(tm.start()); }
        hipLaunchKernelGGL(k_if_item, dim3((unsigned)act_i.size()), dim3(256), 0, nullptr, ndays, (const float *)d_obs,
                           (int)ngroups, (const int32_t *)d_acti, (const int32_t *)d_perm, (const int32_t *)d_goff,
                           (const int32_t *)d_thrall, (const int32_t *)d_thrpor, first, (int)min_daily_nnghs,
                           (const double *)d_curmax, (const int32_t *)d_ringn, (const int32_t *)d_ridx,
                           (const double *)d_rdist, (const int32_t *)d_pnlap, (const int32_t *)d_pnst,
                           (const double *)d_pioa, d_done, d_status, d_nnghs, d_maxdist, d_n, d_lidx, d_lioa, d_ldist,
                           d_lnlap, d_lnst, d_lkeep, d_daycnt);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[2]));
        QACHK(hipMemcpy(done.data(), d_done, NI, hipMemcpyDeviceToHost));
    }
    QACHK(hipMemcpy(h_n.data(), d_n, NI * 4, hipMemcpyDeviceToHost));
    csr_off[0] = 0;
    for (int64_t i = 0; i < ni; ++i) {
        if (h_n[(size_t)i] < 0 || h_n[(size_t)i] > IF_CAP) {
            snprintf(msg, sizeof msg, "%s: internal error: list length %d of item %lld", fn, (int)h_n[(size_t)i], (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
        csr_off[i + 1] = csr_off[i] + h_n[(size_t)i];
    }
    const int64_t total = csr_off[ni];
    if (total > csr_cap) {
        snprintf(msg, sizeof msg, "%s: the ranked lists hold %lld entries, csr_cap is %lld (ntarget * ngroups * "
                 "TWXQA_MAX_RADIUS_NGH always suffices)", fn, (long long)total, (long long)csr_cap);
        return qa_fail(errbuf, errlen, msg);
    }
    const auto t_down = std::chrono::steady_clock::now();
    float compact_ms = 0.0f;
    if (total > 0) {
        int64_t *d_off;
        int32_t *o_idx, *o_nlap, *o_nst;
        double *o_ioa, *o_dist;
        uint8_t *o_keep;
        const size_t T = (size_t)total;
        QAALLOC(bufs, d_off, int64_t, NI + 1);
        QAALLOC(bufs, o_idx, int32_t, T); QAALLOC(bufs, o_nlap, int32_t, T); QAALLOC(bufs, o_nst, int32_t, T);
        QAALLOC(bufs, o_ioa, double, T); QAALLOC(bufs, o_dist, double, T); QAALLOC(bufs, o_keep, uint8_t, T);
        QACHK(hipMemcpy(d_off, csr_off, (NI + 1) * 8, hipMemcpyHostToDevice));
        if (kernel_ms) QACHK(tm.start());
        hipLaunchKernelGGL(k_if_compact, dim3((unsigned)ni), dim3(256), 0, nullptr, (const int32_t *)d_n,
                           (const int64_t *)d_off, (const int32_t *)d_lidx, (const double *)d_lioa,
                           (const double *)d_ldist, (const int32_t *)d_lnlap, (const int32_t *)d_lnst,
                           (const uint8_t *)d_lkeep, o_idx, o_ioa, o_dist, o_nlap, o_nst, o_keep);
        QACHK(hipGetLastError());
        if (kernel_ms) { QACHK(tm.stop_add(&ms[3])); compact_ms = ms[3]; }
        QACHK(hipMemcpy(ngh_idx, o_idx, T * 4, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(ngh_ioa, o_ioa, T * 8, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(ngh_dist, o_dist, T * 8, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(ngh_nlap, o_nlap, T * 4, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(ngh_nlap_stn, o_nst, T * 4, hipMemcpyDeviceToHost));
        QACHK(hipMemcpy(keep, o_keep, T, hipMemcpyDeviceToHost));
    }
    QACHK(hipMemcpy(status, d_status, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(nnghs, d_nnghs, NI * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(max_dist, d_maxdist, NI * 8, hipMemcpyDeviceToHost));
    if (nrounds) *nrounds = rounds;
    ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_down).count() - compact_ms;
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxif_infill_matrix(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                                   const float *obs, const int32_t *ymd, const uint8_t *eligible, int64_t ntarget,
                                   const int32_t *target_idx, int32_t ngroups, const int8_t *group,
                                   const int32_t *nthres_all, const int32_t *nthres_target_por, int32_t min_daily_nnghs,
                                   int32_t *status, int32_t *nnghs, double *max_dist, int64_t *csr_off, int64_t csr_cap,
                                   int32_t *ngh_idx, double *ngh_ioa, double *ngh_dist, int32_t *ngh_nlap,
                                   int32_t *ngh_nlap_stn, uint8_t *keep, int32_t *nrounds, float *kernel_ms, char *errbuf,
                                   int errlen)
{
    return if_matrix("twxif_infill_matrix", device, nstn, ndays, lon, lat, obs, ymd, eligible, ntarget, target_idx, nullptr,
                     ngroups, group, nthres_all, nthres_target_por, min_daily_nnghs, status, nnghs, max_dist, csr_off,
                     csr_cap, ngh_idx, ngh_ioa, ngh_dist, ngh_nlap, ngh_nlap_stn, keep, nrounds, kernel_ms, errbuf, errlen);
}

// step15: twxif_infill_matrix with one pool row per target that is never its neighbour (include/twx_qa.h)
extern "C" int twxxv_infill_matrix(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                                   const float *obs, const int32_t *ymd, const uint8_t *eligible, int64_t ntarget,
                                   const int32_t *target_idx, const int32_t *exclude_idx, int32_t ngroups,
                                   const int8_t *group, const int32_t *nthres_all, const int32_t *nthres_target_por,
                                   int32_t min_daily_nnghs, int32_t *status, int32_t *nnghs, double *max_dist,
                                   int64_t *csr_off, int64_t csr_cap, int32_t *ngh_idx, double *ngh_ioa, double *ngh_dist,
                                   int32_t *ngh_nlap, int32_t *ngh_nlap_stn, uint8_t *keep, int32_t *nrounds,
                                   float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxxv_infill_matrix";
    if (!exclude_idx) {
        if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s: null buffer", fn);
        return -1;
    }
    return if_matrix(fn, device, nstn, ndays, lon, lat, obs, ymd, eligible, ntarget, target_idx, exclude_idx, ngroups,
                     group, nthres_all, nthres_target_por, min_daily_nnghs, status, nnghs, max_dist, csr_off, csr_cap,
                     ngh_idx, ngh_ioa, ngh_dist, ngh_nlap, ngh_nlap_stn, keep, nrounds, kernel_ms, errbuf, errlen);
}
