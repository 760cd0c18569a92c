// twx_tzpoly.hip -- libtwxqa.so: step13's time-zone lookup, add_utc_offset over UtcOffset (twx/db/create_db_all_stations.py:
// 1333-1383, twx/db/stn_utc_offsets.py:43-117): for every station the first polygon that contains it, otherwise the nearest.
// The eighteenth translation unit of the library (include/twx_qa.h, twxtz_*).  The predicates are twx_tzpoly_pred.h, shared
// with a CPU program of the tests.
//
//   k_tz_count / k_tz_scatter   a thread per point over all bboxes: the (point, polygon) pairs whose closed bbox holds the
//                  point, and the work items they make (a pair of n edges is ceil(n / TWXTZ_CHUNK_EDGES) items), counted,
//                  scanned on the host (int64), then written point-major, polygons ascending, by the point's own thread.
//   k_tz_contain   a wavefront per item: the lanes stride the chunk's edges, one aligned 32-byte load each; the crossing and
//                  the uncertain lanes are balloted, the parity is the popcount's low bit.  A pair of several chunks is
//                  combined with an integer atomicXor (parity) / atomicOr (uncertain) on the pair's word: both commute, so
//                  the word does not depend on the order of arrival.
//   k_tz_pick      a thread per point: the lowest polygon among its inside pairs; uncertain pairs below it are appended to
//                  the uncertain list.  A point with neither is left TWXTZ_PENDING for the forced search.
//   k_tz_forced    a work-group per pending point over ALL edges: the lexicographic minimum of (d2, polygon) in float64 by
//                  a fixed tree (wavefront shuffles, then four partials in LDS), with the nearest d2 of another polygon and
//                  the lowest lower bound among ill-conditioned edges riding along, which decide `uncertain`.
// No float atomics; the uncertain list is appended with an integer counter and sorted by the host entry: two calls give
// the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"
#include "twx_tzpoly_pred.h"

namespace {

constexpr int TZ_BLOCK = 256;
constexpr double TZ_TIE_REL = 0x1p-40;                            // TWXTZ_TIE_REL

struct TzBest {                                                  // the forced search's running record
    double d2;                                                   // the minimum so far
    double other;                                                // the lowest d2 of a polygon other than poly
    double ill_lo;                                               // the lowest lower bound among ill-conditioned edges
    int32_t poly;
};

// (d2, poly) lexicographic; `other` stays the lowest d2 among polygons that are not the winner
__device__ __forceinline__ void tz_merge(TzBest &a, double d2, int32_t poly, double other, double ill_lo)
{
    if (poly >= 0) {
        if (a.poly < 0) {
            a.d2 = d2, a.poly = poly, a.other = other;
        } else if (poly == a.poly) {
            a.d2 = fmin(a.d2, d2);
            a.other = fmin(a.other, other);
        } else if (d2 < a.d2 || (d2 == a.d2 && poly < a.poly)) {
            a.other = fmin(a.d2, other);                         // the old winner is now another polygon
            a.d2 = d2, a.poly = poly;
        } else {
            a.other = fmin(a.other, d2);                         // other >= d2 needs no look
        }
    }
    a.ill_lo = fmin(a.ill_lo, ill_lo);
}

}  // namespace

__global__ __launch_bounds__(TZ_BLOCK) void k_tz_count(int64_t npt, const double *__restrict__ lon, const double *__restrict__ lat,
                                                       int32_t npoly, const int64_t *__restrict__ edge_off,
                                                       const double *__restrict__ bbox, int64_t *__restrict__ npair,
                                                       int64_t *__restrict__ nitem)
{
    const int64_t t = (int64_t)blockIdx.x * TZ_BLOCK + threadIdx.x;
    if (t >= npt) return;
    const double px = lon[t], py = lat[t];
    int64_t np = 0, ni = 0;
    if (isfinite(px) && isfinite(py))
        for (int32_t p = 0; p < npoly; ++p)
            if (tz_bbox_contains(bbox + 4 * (int64_t)p, px, py)) {
                ++np;
                ni += (edge_off[p + 1] - edge_off[p] + TWXTZ_CHUNK_EDGES - 1) / TWXTZ_CHUNK_EDGES;
            }
    npair[t] = np, nitem[t] = ni;
}

__global__ __launch_bounds__(TZ_BLOCK) void k_tz_scatter(int64_t npt, const double *__restrict__ lon, const double *__restrict__ lat,
                                                         int32_t npoly, const int64_t *__restrict__ edge_off,
                                                         const double *__restrict__ bbox, const int64_t *__restrict__ pair_off,
                                                         const int64_t *__restrict__ item_off, int32_t *__restrict__ pair_poly,
                                                         int64_t *__restrict__ item_pair, int32_t *__restrict__ item_chunk,
                                                         int32_t *__restrict__ item_pt)
{
    const int64_t t = (int64_t)blockIdx.x * TZ_BLOCK + threadIdx.x;
    if (t >= npt) return;
    const double px = lon[t], py = lat[t];
    int64_t kp = pair_off[t], ki = item_off[t];
    const int64_t endp = pair_off[t + 1], endi = item_off[t + 1];
    if (kp == endp) return;                                       // a non-finite point among them
    for (int32_t p = 0; p < npoly; ++p)
        if (tz_bbox_contains(bbox + 4 * (int64_t)p, px, py)) {
            const int32_t nc = (int32_t)((edge_off[p + 1] - edge_off[p] + TWXTZ_CHUNK_EDGES - 1) / TWXTZ_CHUNK_EDGES);
            if (kp >= endp || ki + nc > endi) return;             // cannot happen: the counts are of this very loop
            pair_poly[kp] = p;
            for (int32_t c = 0; c < nc; ++c, ++ki) item_pair[ki] = kp, item_chunk[ki] = c, item_pt[ki] = (int32_t)t;
            ++kp;
        }
}

__global__ __launch_bounds__(TZ_BLOCK) void k_tz_contain(int64_t nitem, const double *__restrict__ lon, const double *__restrict__ lat,
                                                         const int64_t *__restrict__ edge_off, const double4 *__restrict__ edges,
                                                         const int32_t *__restrict__ pair_poly, const int64_t *__restrict__ item_pair,
                                                         const int32_t *__restrict__ item_chunk, const int32_t *__restrict__ item_pt,
                                                         uint32_t *__restrict__ pair_word)
{
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * (TZ_BLOCK / 64) + (threadIdx.x >> 6);
    if (it >= nitem) return;                                      // the whole wavefront leaves
    const int64_t pair = item_pair[it];
    const int32_t poly = pair_poly[pair], pt = item_pt[it];
    const double px = lon[pt], py = lat[pt];
    const int64_t e0 = edge_off[poly] + (int64_t)item_chunk[it] * TWXTZ_CHUNK_EDGES;
    const int64_t e1 = min(e0 + (int64_t)TWXTZ_CHUNK_EDGES, edge_off[poly + 1]);
    int cross = 0, unc = 0;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const double4 g = edges[e];
        const int r = tz_edge_cross(g.x, g.y, g.z, g.w, px, py);
        cross ^= r & TZ_CROSS;
        unc |= r & TZ_CROSS_UNCERTAIN;
    }
    const unsigned long long bc = __ballot(cross != 0), bu = __ballot(unc != 0);
    if (lane == 0) {
        if (__popcll(bc) & 1) atomicXor(&pair_word[pair], 1u);
        if (bu) atomicOr(&pair_word[pair], 2u);
    }
}

__global__ __launch_bounds__(TZ_BLOCK) void k_tz_pick(int64_t npt, const double *__restrict__ lon, const double *__restrict__ lat,
                                                      const int64_t *__restrict__ pair_off, const int32_t *__restrict__ pair_poly,
                                                      const uint32_t *__restrict__ pair_word, int32_t *__restrict__ poly,
                                                      int32_t *__restrict__ status, double *__restrict__ dist2,
                                                      int32_t *__restrict__ unc, int64_t unc_cap, unsigned long long *__restrict__ nunc)
{
    const int64_t t = (int64_t)blockIdx.x * TZ_BLOCK + threadIdx.x;
    if (t >= npt) return;
    dist2[t] = 0.0;
    if (!isfinite(lon[t]) || !isfinite(lat[t])) {
        poly[t] = -1, status[t] = TWXTZ_BAD_POINT;
        return;
    }
    int32_t win = -1;
    bool any_unc = false;
    for (int64_t k = pair_off[t]; k < pair_off[t + 1]; ++k) {
        const uint32_t w = pair_word[k];
        if (w & 2u) {
            any_unc = true;
            const unsigned long long slot = atomicAdd(nunc, 1ull);
            if ((int64_t)slot < unc_cap) unc[2 * slot] = (int32_t)t, unc[2 * slot + 1] = pair_poly[k];
        } else if (w & 1u) {
            win = pair_poly[k];
            break;
        }
    }
    poly[t] = win;
    status[t] = any_unc ? TWXTZ_UNCERTAIN : win >= 0 ? TWXTZ_INSIDE : TWXTZ_PENDING;
}

__global__ __launch_bounds__(TZ_BLOCK) void k_tz_forced(const int32_t *__restrict__ pending, const double *__restrict__ lon,
                                                        const double *__restrict__ lat, int32_t npoly,
                                                        const int64_t *__restrict__ edge_off, const double4 *__restrict__ edges,
                                                        double max_force2, int32_t *__restrict__ poly, int32_t *__restrict__ status,
                                                        double *__restrict__ dist2, int32_t *__restrict__ unc, int64_t unc_cap,
                                                        unsigned long long *__restrict__ nunc)
{
    __shared__ TzBest part[TZ_BLOCK / 64];
    const int32_t pt = pending[blockIdx.x];
    const double px = lon[pt], py = lat[pt];
    TzBest best;
    best.d2 = INFINITY, best.other = INFINITY, best.ill_lo = INFINITY, best.poly = -1;
    int32_t p = 0;
    const int64_t nedge = edge_off[npoly];
    for (int64_t e = threadIdx.x; e < nedge; e += TZ_BLOCK) {
        while (e >= edge_off[p + 1]) ++p;                         // edges ascend with the polygons; empty ones are skipped
        const double4 g = edges[e];
        bool ill;
        double lo;
        const double d2 = tz_seg_d2(g.x, g.y, g.z, g.w, px, py, &ill, &lo);
        tz_merge(best, d2, p, INFINITY, ill ? lo : INFINITY);
    }
    for (int o = 32; o > 0; o >>= 1) {                            // a fixed tree: lane l takes lane l + o
        const double d2 = __shfl_down(best.d2, o), other = __shfl_down(best.other, o), ill = __shfl_down(best.ill_lo, o);
        const int32_t q = __shfl_down(best.poly, o);
        if ((threadIdx.x & 63) + o < 64) tz_merge(best, d2, q, other, ill);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < TZ_BLOCK / 64; ++w) tz_merge(best, part[w].d2, part[w].poly, part[w].other, part[w].ill_lo);
    const double tie = best.d2 + best.d2 * TZ_TIE_REL;
    bool uncertain = best.other <= tie || best.ill_lo <= tie;
    if (max_force2 < INFINITY && fabs(best.d2 - max_force2) <= max_force2 * TZ_TIE_REL) uncertain = true;
    dist2[pt] = best.d2;
    if (best.poly < 0) {                                          // no edge at all
        poly[pt] = -1, status[pt] = TWXTZ_NONE, dist2[pt] = INFINITY;
    } else if (uncertain) {
        poly[pt] = best.poly, status[pt] = TWXTZ_UNCERTAIN;
        const unsigned long long slot = atomicAdd(nunc, 1ull);
        if ((int64_t)slot < unc_cap) unc[2 * slot] = pt, unc[2 * slot + 1] = -1;
    } else if (best.d2 > max_force2) {
        poly[pt] = -1, status[pt] = TWXTZ_NONE;
    } else {
        poly[pt] = best.poly, status[pt] = TWXTZ_FORCED;
    }
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
namespace {

unsigned tz_grid(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int twxtz_locate(int device, int64_t npt, const double *lon, const double *lat, int64_t npoly, const int64_t *edge_off,
                            const double *bbox, const double *edges, double max_force_deg, int32_t *poly, int32_t *status,
                            double *dist2, int32_t *uncertain, int64_t uncertain_cap, int64_t *counts, float *timing_ms,
                            char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    char msg[320];
    if (!lon || !lat || !edge_off || !bbox || !poly || !status || !dist2 || !counts || (uncertain_cap > 0 && !uncertain))
        return qa_fail(errbuf, errlen, "twxtz_locate: null buffer");
    if (npt < 1 || npt > TWXTZ_MAX_POINTS || npoly < 1 || npoly > TWXTZ_MAX_POLY) {
        snprintf(msg, sizeof msg, "twxtz_locate: need 1 <= npt <= TWXTZ_MAX_POINTS = %d and 1 <= npoly <= TWXTZ_MAX_POLY = %d",
                 TWXTZ_MAX_POINTS, TWXTZ_MAX_POLY);
        return qa_fail(errbuf, errlen, msg);
    }
    if (uncertain_cap < 0 || uncertain_cap > TWXTZ_MAX_UNCERTAIN) {
        snprintf(msg, sizeof msg, "twxtz_locate: need 0 <= uncertain_cap <= TWXTZ_MAX_UNCERTAIN = %lld", (long long)TWXTZ_MAX_UNCERTAIN);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!(max_force_deg >= 0.0)) return qa_fail(errbuf, errlen, "twxtz_locate: max_force_deg must be >= 0 (infinity: no limit)");
    if (edge_off[0] != 0) return qa_fail(errbuf, errlen, "twxtz_locate: edge_off must start at 0");
    for (int64_t p = 0; p < npoly; ++p) {
        if (edge_off[p + 1] < edge_off[p]) {
            snprintf(msg, sizeof msg, "twxtz_locate: edge_off descends at polygon %lld", (long long)p);
            return qa_fail(errbuf, errlen, msg);
        }
        const double *bb = bbox + 4 * p;
        if (!(std::isfinite(bb[0]) && std::isfinite(bb[1]) && std::isfinite(bb[2]) && std::isfinite(bb[3]) && bb[0] <= bb[2] &&
              bb[1] <= bb[3])) {
            snprintf(msg, sizeof msg, "twxtz_locate: the bbox of polygon %lld is not finite or not ordered", (long long)p);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const int64_t nedge = edge_off[npoly];
    if (nedge < 1 || nedge > TWXTZ_MAX_EDGES || !edges) {
        snprintf(msg, sizeof msg, "twxtz_locate: need 1 <= edges <= TWXTZ_MAX_EDGES = %lld", (long long)TWXTZ_MAX_EDGES);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t e = 0; e < nedge; ++e) {
        const double *g = edges + 4 * e;
        if (!(std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]) && std::isfinite(g[3])) || (g[0] == g[2] && g[1] == g[3])) {
            snprintf(msg, sizeof msg, "twxtz_locate: edge %lld is not finite or has no length", (long long)e);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const double max_force2 = std::isinf(max_force_deg) ? INFINITY : max_force_deg * max_force_deg;

    float ms[TWXTZ_NPHASES];
    for (int i = 0; i < TWXTZ_NPHASES; ++i) ms[i] = 0.0f;
    for (int i = 0; i < TWXTZ_C_N; ++i) counts[i] = 0;
    QACHK(hipSetDevice(device));
    QaBuf b_lon, b_lat, b_off, b_bbox, b_edges, b_np, b_ni, b_poff, b_ioff, b_ppoly, b_ipair, b_ichunk, b_ipt, b_word, b_poly,
        b_status, b_d2, b_unc, b_nunc, b_pend;
    QaTimer tm;
    QACHK(tm.init());
    const size_t n = (size_t)npt;
    QACHK(hipMalloc(&b_lon.p, n * 8));
    QACHK(hipMalloc(&b_lat.p, n * 8));
    QACHK(hipMalloc(&b_off.p, ((size_t)npoly + 1) * 8));
    QACHK(hipMalloc(&b_bbox.p, (size_t)npoly * 32));
    QACHK(hipMalloc(&b_edges.p, (size_t)nedge * 32));
    QACHK(hipMalloc(&b_np.p, n * 8));
    QACHK(hipMalloc(&b_ni.p, n * 8));
    QACHK(hipMalloc(&b_poff.p, (n + 1) * 8));
    QACHK(hipMalloc(&b_ioff.p, (n + 1) * 8));
    QACHK(hipMalloc(&b_poly.p, n * 4));
    QACHK(hipMalloc(&b_status.p, n * 4));
    QACHK(hipMalloc(&b_d2.p, n * 8));
    QACHK(hipMalloc(&b_unc.p, (size_t)std::max<int64_t>(uncertain_cap, 1) * 8));
    QACHK(hipMalloc(&b_nunc.p, 8));
    QACHK(hipMemset(b_nunc.p, 0, 8));
    // ---- upload
    QACHK(tm.start());
    QACHK(hipMemcpy(b_lon.p, lon, n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_lat.p, lat, n * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_off.p, edge_off, ((size_t)npoly + 1) * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_bbox.p, bbox, (size_t)npoly * 32, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_edges.p, edges, (size_t)nedge * 32, hipMemcpyHostToDevice));
    QACHK(tm.stop_add(&ms[TWXTZ_T_UPLOAD]));
    const double *d_lon = static_cast<const double *>(b_lon.p), *d_lat = static_cast<const double *>(b_lat.p);
    const int64_t *d_off = static_cast<const int64_t *>(b_off.p);
    const double *d_bbox = static_cast<const double *>(b_bbox.p);
    const double4 *d_edges = static_cast<const double4 *>(b_edges.p);
    // ---- candidates: count, scan (host), scatter
    std::vector<int64_t> np(n), ni(n), poff(n + 1, 0), ioff(n + 1, 0);
    QACHK(tm.start());
    hipLaunchKernelGGL(k_tz_count, dim3(tz_grid(npt, TZ_BLOCK)), dim3(TZ_BLOCK), 0, nullptr, npt, d_lon, d_lat, (int32_t)npoly, d_off,
                       d_bbox, static_cast<int64_t *>(b_np.p), static_cast<int64_t *>(b_ni.p));
    QACHK(hipGetLastError());
    QACHK(hipMemcpy(np.data(), b_np.p, n * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(ni.data(), b_ni.p, n * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) poff[i + 1] = poff[i] + np[i], ioff[i + 1] = ioff[i] + ni[i];
    const int64_t npair = poff[n], nitem = ioff[n];
    if (nitem > TWXTZ_MAX_ITEMS) {
        snprintf(msg, sizeof msg, "twxtz_locate: %lld work items, more than TWXTZ_MAX_ITEMS = %lld: pass the points in parts",
                 (long long)nitem, (long long)TWXTZ_MAX_ITEMS);
        return qa_fail(errbuf, errlen, msg);
    }
    QACHK(hipMemcpy(b_poff.p, poff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_ioff.p, ioff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    if (npair > 0) {
        QACHK(hipMalloc(&b_ppoly.p, (size_t)npair * 4));
        QACHK(hipMalloc(&b_word.p, (size_t)npair * 4));
        QACHK(hipMalloc(&b_ipair.p, (size_t)nitem * 8));
        QACHK(hipMalloc(&b_ichunk.p, (size_t)nitem * 4));
        QACHK(hipMalloc(&b_ipt.p, (size_t)nitem * 4));
        QACHK(hipMemset(b_word.p, 0, (size_t)npair * 4));
        hipLaunchKernelGGL(k_tz_scatter, dim3(tz_grid(npt, TZ_BLOCK)), dim3(TZ_BLOCK), 0, nullptr, npt, d_lon, d_lat, (int32_t)npoly,
                           d_off, d_bbox, static_cast<const int64_t *>(b_poff.p), static_cast<const int64_t *>(b_ioff.p),
                           static_cast<int32_t *>(b_ppoly.p), static_cast<int64_t *>(b_ipair.p), static_cast<int32_t *>(b_ichunk.p),
                           static_cast<int32_t *>(b_ipt.p));
        QACHK(hipGetLastError());
    }
    QACHK(tm.stop_add(&ms[TWXTZ_T_CANDIDATES]));
    // ---- containment and the pick
    QACHK(tm.start());
    if (nitem > 0) {
        hipLaunchKernelGGL(k_tz_contain, dim3(tz_grid(nitem, TZ_BLOCK / 64)), dim3(TZ_BLOCK), 0, nullptr, nitem, d_lon, d_lat, d_off,
                           d_edges, static_cast<const int32_t *>(b_ppoly.p), static_cast<const int64_t *>(b_ipair.p),
                           static_cast<const int32_t *>(b_ichunk.p), static_cast<const int32_t *>(b_ipt.p),
                           static_cast<uint32_t *>(b_word.p));
        QACHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tz_pick, dim3(tz_grid(npt, TZ_BLOCK)), dim3(TZ_BLOCK), 0, nullptr, npt, d_lon, d_lat,
                       static_cast<const int64_t *>(b_poff.p), static_cast<const int32_t *>(b_ppoly.p),
                       static_cast<const uint32_t *>(b_word.p), static_cast<int32_t *>(b_poly.p), static_cast<int32_t *>(b_status.p),
                       static_cast<double *>(b_d2.p), static_cast<int32_t *>(b_unc.p), uncertain_cap,
                       static_cast<unsigned long long *>(b_nunc.p));
    QACHK(hipGetLastError());
    QACHK(hipMemcpy(status, b_status.p, n * 4, hipMemcpyDeviceToHost));
    QACHK(tm.stop_add(&ms[TWXTZ_T_CONTAIN]));
    // ---- the forced search of the points nothing contains
    std::vector<int32_t> pending;
    for (size_t i = 0; i < n; ++i)
        if (status[i] == TWXTZ_PENDING) pending.push_back((int32_t)i);
    QACHK(tm.start());
    if (!pending.empty()) {
        QACHK(hipMalloc(&b_pend.p, pending.size() * 4));
        QACHK(hipMemcpy(b_pend.p, pending.data(), pending.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_tz_forced, dim3((unsigned)pending.size()), dim3(TZ_BLOCK), 0, nullptr,
                           static_cast<const int32_t *>(b_pend.p), d_lon, d_lat, (int32_t)npoly, d_off, d_edges, max_force2,
                           static_cast<int32_t *>(b_poly.p), static_cast<int32_t *>(b_status.p), static_cast<double *>(b_d2.p),
                           static_cast<int32_t *>(b_unc.p), uncertain_cap, static_cast<unsigned long long *>(b_nunc.p));
        QACHK(hipGetLastError());
    }
    QACHK(tm.stop_add(&ms[TWXTZ_T_FORCED]));
    // ---- download
    unsigned long long nunc = 0;
    QACHK(tm.start());
    QACHK(hipMemcpy(poly, b_poly.p, n * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(status, b_status.p, n * 4, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(dist2, b_d2.p, n * 8, hipMemcpyDeviceToHost));
    QACHK(hipMemcpy(&nunc, b_nunc.p, 8, hipMemcpyDeviceToHost));
    const int64_t nkeep = std::min<int64_t>((int64_t)nunc, uncertain_cap);
    if (nkeep > 0) QACHK(hipMemcpy(uncertain, b_unc.p, (size_t)nkeep * 8, hipMemcpyDeviceToHost));
    QACHK(tm.stop_add(&ms[TWXTZ_T_DOWNLOAD]));
    if (nkeep > 0) {                                              // the order of arrival is not kept: (point, polygon) ascending
        std::vector<std::pair<int32_t, int32_t>> v((size_t)nkeep);
        for (int64_t k = 0; k < nkeep; ++k) v[(size_t)k] = {uncertain[2 * k], uncertain[2 * k + 1]};
        std::sort(v.begin(), v.end());
        for (int64_t k = 0; k < nkeep; ++k) uncertain[2 * k] = v[(size_t)k].first, uncertain[2 * k + 1] = v[(size_t)k].second;
    }
    counts[TWXTZ_C_PAIRS] = npair;
    counts[TWXTZ_C_ITEMS] = nitem;
    counts[TWXTZ_C_PENDING] = (int64_t)pending.size();
    counts[TWXTZ_C_UNCERTAIN] = (int64_t)nunc;
    if (timing_ms) memcpy(timing_ms, ms, sizeof ms);
    return (int64_t)nunc > uncertain_cap ? TWXTZ_OVERFLOW : 0;
}
