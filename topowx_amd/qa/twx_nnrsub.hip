// twx_nnrsub.hip -- libtwxqa.so: the North American reanalysis subsets of step12.  create_nnr_subset,
// create_nnr_subset_nolevel and create_thickness_nnr_subset (twx/db/reanalysis.py:45-305) for every product of one raw
// variable in one call: one upload of the raw slab feeds all of them.  The seventeenth translation unit of the library
// (include/twx_qa.h, twxns_*).  The index mapping is twx_nnrsub_map.h, shared with a CPU program of the tests.
//
// The host turns (rec_slot, rec_day) into day_rec [3][ndays], the record of each (slot, day) or -1, and refuses two records
// on one (slot, day) there.  The kernels then run over the OUTPUT, one launch per product:
//   k_nsub_tiled<T>  a thread per float4: row `row` of chunk (cy, cx) at (day, level), row fastest, then level, day, chunk --
//                  thread t stores the 16 bytes at 16 t, a wavefront 1024 contiguous bytes.  The four raw values are gathered
//                  through lat_idx / lon_idx (2 or 4 bytes each: the narrow side).  A day without a record, a row or a
//                  column past the subset's edge is fill: the prefill is folded in, and every byte of a chunk is determined.
//   k_nsub_plain<T>  a thread per element of [day][lev][lat][lon], 4-byte stores in order (the classic container's route).
// Every output element is written by exactly one thread.  The marks that matched are counted per product with a wavefront
// reduction and one integer atomicAdd per wavefront; nothing else is atomic.  All arithmetic is float32, one rounding per
// operation (-ffp-contract=off): u = f32(f32(x) * scale) + offset; u - f32(273.15); u_up - u_low.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_nnrsub_map.h"
#include "twx_qa.h"
#include "twx_qa_common.h"

namespace {

template <typename T>
struct NsMarks {
    T v[2];
    int32_t has[2];
};

struct NsArgs {
    NsShape s;
    NsProd p;
    float scale, offset;
    int32_t unpack;                                              // 0: scale 1, offset 0 -- the datum as it is
};

// One output value: *marked is raised if a raw datum it is made of equals a mark (the value is then the fill).
template <typename T>
__device__ __forceinline__ float ns_value(const T *__restrict__ raw, const NsArgs &a, const NsMarks<T> &m, int64_t rec, int32_t lev,
                                          int64_t y, int64_t x, bool *marked)
{
    const bool thick = a.p.kind == NS_KIND_THICK;
    const T d0 = raw[ns_raw_offset(a.s, rec, a.p.lev[thick ? 0 : lev], y, x)];
    bool hit = (m.has[0] && d0 == m.v[0]) || (m.has[1] && d0 == m.v[1]);
    float v = a.unpack ? (float)d0 * a.scale + a.offset : (float)d0;
    if (thick) {
        const T d1 = raw[ns_raw_offset(a.s, rec, a.p.lev[1], y, x)];
        hit = hit || (m.has[0] && d1 == m.v[0]) || (m.has[1] && d1 == m.v[1]);
        v = v - (a.unpack ? (float)d1 * a.scale + a.offset : (float)d1);
    }
    if (hit) {
        *marked = true;
        return TWXNS_FILL;
    }
    if (a.p.conv == TWXNS_CONV_K_TO_C) v = v - 273.15f;
    return v;
}

__device__ __forceinline__ void ns_count(uint32_t n, unsigned long long *__restrict__ nmarked)
{
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(nmarked, (unsigned long long)n);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void k_nsub_tiled(const T *__restrict__ raw, NsArgs a, NsMarks<T> m,
                                                  const int32_t *__restrict__ day_rec, const int32_t *__restrict__ lat_idx,
                                                  const int32_t *__restrict__ lon_idx, float *__restrict__ out,
                                                  unsigned long long *__restrict__ nmarked)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    NsCell c;
    uint32_t n = 0;
    if (ns_tiled_cell(a.s, a.p.nlev, t, &c)) {
        float v[4] = {TWXNS_FILL, TWXNS_FILL, TWXNS_FILL, TWXNS_FILL};
        const int64_t lat = c.cy * 4 + c.row;
        const int32_t rec = day_rec[c.day];
        if (rec >= 0 && lat < a.s.nlat_out) {
            const int64_t y = lat_idx[lat];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t lon = c.cx * 4 + k;
                if (lon < a.s.nlon_out) {
                    bool marked = false;
                    v[k] = ns_value(raw, a, m, (int64_t)rec, c.lev, y, (int64_t)lon_idx[lon], &marked);
                    n += marked ? 1u : 0u;
                }
            }
        }
        *reinterpret_cast<float4 *>(out + ns_tiled_offset(a.s, a.p.nlev, c)) = make_float4(v[0], v[1], v[2], v[3]);
    }
    ns_count(n, nmarked);
}

template <typename T>
__global__ __launch_bounds__(256) void k_nsub_plain(const T *__restrict__ raw, NsArgs a, NsMarks<T> m,
                                                  const int32_t *__restrict__ day_rec, const int32_t *__restrict__ lat_idx,
                                                  const int32_t *__restrict__ lon_idx, float *__restrict__ out,
                                                  unsigned long long *__restrict__ nmarked)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t day = 0, lat = 0, lon = 0;
    int32_t lev = 0;
    uint32_t n = 0;
    if (ns_plain_cell(a.s, a.p.nlev, t, &day, &lev, &lat, &lon)) {
        float v = TWXNS_FILL;
        const int32_t rec = day_rec[day];
        if (rec >= 0) {
            bool marked = false;
            v = ns_value(raw, a, m, (int64_t)rec, lev, (int64_t)lat_idx[lat], (int64_t)lon_idx[lon], &marked);
            n = marked ? 1u : 0u;
        }
        out[t] = v;
    }
    ns_count(n, nmarked);
}

// ---------------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------------
namespace {

bool ns_indices_ok(const int32_t *idx, int64_t n, int64_t bound)
{
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= bound) return false;
    return true;
}

template <typename T>
hipError_t ns_launch(int layout, const void *raw, const NsArgs &a, const void *marks, const int32_t *has_mark,
                     const int32_t *day_rec, const int32_t *lat_idx, const int32_t *lon_idx, float *out,
                     unsigned long long *nmarked)
{
    NsMarks<T> m;
    memcpy(m.v, marks, 2 * sizeof(T));
    m.has[0] = has_mark[0] != 0;
    m.has[1] = has_mark[1] != 0;
    const int64_t nthr = layout == TWXNS_TILED ? ns_tiled_size(a.s, a.p.nlev) / 4 : ns_plain_size(a.s, a.p.nlev);
    const dim3 grid((unsigned)((nthr + 255) / 256));
    if (layout == TWXNS_TILED)
        hipLaunchKernelGGL(k_nsub_tiled<T>, grid, dim3(256), 0, nullptr, static_cast<const T *>(raw), a, m, day_rec, lat_idx, lon_idx,
                           out, nmarked);
    else
        hipLaunchKernelGGL(k_nsub_plain<T>, grid, dim3(256), 0, nullptr, static_cast<const T *>(raw), a, m, day_rec, lat_idx, lon_idx,
                           out, nmarked);
    return hipGetLastError();
}

}  // namespace

extern "C" int twxns_subset(int device, int dtype, const void *raw, int64_t nrec, int64_t nl, int64_t ny, int64_t nx, float scale,
                            float offset, const void *marks, const int32_t *has_mark, const int32_t *rec_slot,
                            const int32_t *rec_day, int64_t ndays, int64_t nlat_out, const int32_t *lat_idx, int64_t nlon_out,
                            const int32_t *lon_idx, int64_t nprod, const int32_t *prod, int layout, float *const *out,
                            int64_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    if (errbuf && errlen > 0) errbuf[0] = 0;
    char msg[320];
    if (dtype != TWXNS_I16 && dtype != TWXNS_F32)
        return qa_fail(errbuf, errlen, "twxns_subset: dtype must be TWXNS_I16 or TWXNS_F32");
    if (layout != TWXNS_TILED && layout != TWXNS_PLAIN)
        return qa_fail(errbuf, errlen, "twxns_subset: layout must be TWXNS_TILED or TWXNS_PLAIN");
    if (!raw || !marks || !has_mark || !rec_slot || !rec_day || !lat_idx || !lon_idx || !prod || !out || !counts)
        return qa_fail(errbuf, errlen, "twxns_subset: null buffer");
    if (nrec < 1 || nl < 1 || ny < 1 || nx < 1 || nrec > INT32_MAX || nl > INT32_MAX || ny > INT32_MAX || nx > INT32_MAX ||
        (double)nrec * (double)nl * (double)ny * (double)nx > (double)TWXNS_MAX_RAW) {
        snprintf(msg, sizeof msg, "twxns_subset: need a raw slab [nrec][nl][ny][nx] of 1 .. TWXNS_MAX_RAW = %lld values",
                 (long long)TWXNS_MAX_RAW);
        return qa_fail(errbuf, errlen, msg);
    }
    if (ndays < 1 || ndays > TWXNS_MAX_DAYS || nlat_out < 1 || nlat_out > TWXNS_MAX_SIDE || nlon_out < 1 ||
        nlon_out > TWXNS_MAX_SIDE) {
        snprintf(msg, sizeof msg, "twxns_subset: need 1 <= ndays <= TWXNS_MAX_DAYS = %d and 1 <= nlat_out, nlon_out <= "
                                  "TWXNS_MAX_SIDE = %d", TWXNS_MAX_DAYS, TWXNS_MAX_SIDE);
        return qa_fail(errbuf, errlen, msg);
    }
    if (nprod < 1 || nprod > TWXNS_MAX_PROD) {
        snprintf(msg, sizeof msg, "twxns_subset: need 1 <= nprod <= TWXNS_MAX_PROD = %d", TWXNS_MAX_PROD);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!ns_indices_ok(lat_idx, nlat_out, ny)) return qa_fail(errbuf, errlen, "twxns_subset: a lat_idx entry is out of range 0 .. ny - 1");
    if (!ns_indices_ok(lon_idx, nlon_out, nx)) return qa_fail(errbuf, errlen, "twxns_subset: a lon_idx entry is out of range 0 .. nx - 1");
    NsShape s;
    s.nrec = nrec, s.nl = nl, s.ny = ny, s.nx = nx, s.ndays = ndays, s.nlat_out = nlat_out, s.nlon_out = nlon_out;
    std::vector<NsProd> prods((size_t)nprod);
    std::vector<int64_t> off((size_t)nprod + 1, 0);                // floats; every product starts on a multiple of 4
    for (int64_t p = 0; p < nprod; ++p) {
        const int32_t *d = prod + p * TWXNS_PD_WORDS;
        NsProd &q = prods[(size_t)p];
        memset(&q, 0, sizeof q);
        if (d[TWXNS_PD_SLOT] < 0 || d[TWXNS_PD_SLOT] > 2) {
            snprintf(msg, sizeof msg, "twxns_subset: product %lld: the slot must be 0, 1 or 2", (long long)p);
            return qa_fail(errbuf, errlen, msg);
        }
        if (d[TWXNS_PD_CONV] != TWXNS_CONV_NONE && d[TWXNS_PD_CONV] != TWXNS_CONV_K_TO_C) {
            snprintf(msg, sizeof msg, "twxns_subset: product %lld: unknown conversion %d", (long long)p, (int)d[TWXNS_PD_CONV]);
            return qa_fail(errbuf, errlen, msg);
        }
        q.conv = d[TWXNS_PD_CONV];
        int nidx = 0;
        if (d[TWXNS_PD_KIND] == TWXNS_KIND_LEVELS) {
            if (d[TWXNS_PD_NLEV] < 1 || d[TWXNS_PD_NLEV] > TWXNS_MAX_LEV) {
                snprintf(msg, sizeof msg, "twxns_subset: product %lld: need 1 <= nlev_out <= TWXNS_MAX_LEV = %d, got %d",
                         (long long)p, TWXNS_MAX_LEV, (int)d[TWXNS_PD_NLEV]);
                return qa_fail(errbuf, errlen, msg);
            }
            q.kind = NS_KIND_LEVELS, q.nlev = nidx = d[TWXNS_PD_NLEV];
        } else if (d[TWXNS_PD_KIND] == TWXNS_KIND_THICK) {
            q.kind = NS_KIND_THICK, q.nlev = 1, nidx = 2;
            if (d[TWXNS_PD_LEV0] == d[TWXNS_PD_LEV0 + 1]) {
                snprintf(msg, sizeof msg, "twxns_subset: product %lld: a thickness needs two different levels, got index %d twice",
                         (long long)p, (int)d[TWXNS_PD_LEV0]);
                return qa_fail(errbuf, errlen, msg);
            }
        } else {
            snprintf(msg, sizeof msg, "twxns_subset: product %lld: the kind must be TWXNS_KIND_LEVELS or TWXNS_KIND_THICK", (long long)p);
            return qa_fail(errbuf, errlen, msg);
        }
        for (int k = 0; k < nidx; ++k) {
            q.lev[k] = d[TWXNS_PD_LEV0 + k];
            if (q.lev[k] < 0 || q.lev[k] >= nl) {
                snprintf(msg, sizeof msg, "twxns_subset: product %lld: level index %d is out of range 0 .. nl - 1 = %lld", (long long)p,
                         (int)q.lev[k], (long long)(nl - 1));
                return qa_fail(errbuf, errlen, msg);
            }
        }
        if (!out[p]) return qa_fail(errbuf, errlen, "twxns_subset: null output buffer");
        const int64_t n = layout == TWXNS_TILED ? ns_tiled_size(s, q.nlev) : ns_plain_size(s, q.nlev);
        if (n > TWXNS_MAX_OUT) {
            snprintf(msg, sizeof msg, "twxns_subset: product %lld has %lld values, more than TWXNS_MAX_OUT = %lld", (long long)p,
                     (long long)n, (long long)TWXNS_MAX_OUT);
            return qa_fail(errbuf, errlen, msg);
        }
        off[(size_t)p + 1] = off[(size_t)p] + (n + 3) / 4 * 4;
    }
    std::vector<int32_t> day_rec(3 * (size_t)ndays, -1);
    int64_t got[3] = {0, 0, 0};
    for (int64_t r = 0; r < nrec; ++r) {
        if (rec_slot[r] < -1 || rec_slot[r] > 2 || rec_day[r] < -1 || rec_day[r] >= ndays) {
            snprintf(msg, sizeof msg, "twxns_subset: record %lld: slot %d, day %d (need -1 .. 2 and -1 .. ndays - 1)", (long long)r,
                     (int)rec_slot[r], (int)rec_day[r]);
            return qa_fail(errbuf, errlen, msg);
        }
        if (rec_slot[r] < 0 || rec_day[r] < 0) continue;
        int32_t &e = day_rec[(size_t)rec_slot[r] * (size_t)ndays + (size_t)rec_day[r]];
        if (e >= 0) {
            snprintf(msg, sizeof msg, "twxns_subset: records %d and %lld both map to slot %d, day %d", (int)e, (long long)r,
                     (int)rec_slot[r], (int)rec_day[r]);
            return qa_fail(errbuf, errlen, msg);
        }
        e = (int32_t)r;
        ++got[rec_slot[r]];
    }

    const size_t esize = dtype == TWXNS_I16 ? 2 : 4;
    const size_t raw_bytes = (size_t)nrec * (size_t)nl * (size_t)ny * (size_t)nx * esize;
    float ms[TWXNS_NKERNELS];
    for (int i = 0; i < TWXNS_NKERNELS; ++i) ms[i] = 0.0f;
    QACHK(hipSetDevice(device));
    QaBuf b_raw, b_rec, b_lat, b_lon, b_out, b_cnt;
    QaTimer tm;
    QACHK(tm.init());
    QACHK(hipMalloc(&b_raw.p, raw_bytes));
    QACHK(hipMalloc(&b_rec.p, day_rec.size() * 4));
    QACHK(hipMalloc(&b_lat.p, (size_t)nlat_out * 4));
    QACHK(hipMalloc(&b_lon.p, (size_t)nlon_out * 4));
    QACHK(hipMalloc(&b_out.p, (size_t)off[(size_t)nprod] * 4));
    QACHK(hipMalloc(&b_cnt.p, (size_t)nprod * 8));
    QACHK(hipMemset(b_cnt.p, 0, (size_t)nprod * 8));
    QACHK(tm.start());
    QACHK(hipMemcpy(b_raw.p, raw, raw_bytes, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_rec.p, day_rec.data(), day_rec.size() * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_lat.p, lat_idx, (size_t)nlat_out * 4, hipMemcpyHostToDevice));
    QACHK(hipMemcpy(b_lon.p, lon_idx, (size_t)nlon_out * 4, hipMemcpyHostToDevice));
    QACHK(tm.stop_set(&ms[0]));
    QACHK(tm.start());
    for (int64_t p = 0; p < nprod; ++p) {
        NsArgs a;
        a.s = s, a.p = prods[(size_t)p], a.scale = scale, a.offset = offset;
        a.unpack = !(scale == 1.0f && offset == 0.0f);
        const int32_t *d_rec = static_cast<const int32_t *>(b_rec.p) + (size_t)prod[p * TWXNS_PD_WORDS + TWXNS_PD_SLOT] * (size_t)ndays;
        float *d_out = static_cast<float *>(b_out.p) + off[(size_t)p];
        unsigned long long *d_cnt = static_cast<unsigned long long *>(b_cnt.p) + p;
        const int32_t *d_lat = static_cast<const int32_t *>(b_lat.p), *d_lon = static_cast<const int32_t *>(b_lon.p);
        if (dtype == TWXNS_I16) QACHK(ns_launch<int16_t>(layout, b_raw.p, a, marks, has_mark, d_rec, d_lat, d_lon, d_out, d_cnt));
        else QACHK(ns_launch<float>(layout, b_raw.p, a, marks, has_mark, d_rec, d_lat, d_lon, d_out, d_cnt));
    }
    QACHK(tm.stop_set(&ms[1]));
    std::vector<unsigned long long> nmarked((size_t)nprod, 0);
    QACHK(tm.start());
    for (int64_t p = 0; p < nprod; ++p) {
        const int64_t n = layout == TWXNS_TILED ? ns_tiled_size(s, prods[(size_t)p].nlev) : ns_plain_size(s, prods[(size_t)p].nlev);
        QACHK(hipMemcpy(out[p], static_cast<const float *>(b_out.p) + off[(size_t)p], (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    QACHK(hipMemcpy(nmarked.data(), b_cnt.p, (size_t)nprod * 8, hipMemcpyDeviceToHost));
    QACHK(tm.stop_set(&ms[2]));
    for (int64_t p = 0; p < nprod; ++p) {
        const int64_t g = got[prod[p * TWXNS_PD_WORDS + TWXNS_PD_SLOT]];
        counts[p * TWXNS_C_N + TWXNS_C_DAYS] = g;
        counts[p * TWXNS_C_N + TWXNS_C_MARKED] = (int64_t)nmarked[(size_t)p];
        counts[p * TWXNS_C_N + TWXNS_C_UNWRITTEN] = ndays - g;
    }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
