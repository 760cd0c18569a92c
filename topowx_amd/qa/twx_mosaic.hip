// twx_mosaic.hip -- libtwxqa.so: the daily and monthly mosaics of step26 / step27 (twx/interp/tiling.py:567-780, 1169-1219)
// assembled in device memory and deflated there into the chunk bytes of their HDF5 datasets.  The nineteenth translation unit
// of the library (include/twx_qa.h, twxmo_*).  The host arithmetic is twx_mosaic_host.h, shared with a CPU program of the tests.
//
// A mosaic object holds an image int16 [max_days][Yp][Xp] (Y, X rounded up to whole chunks; the padding holds the fill value,
// which is what libhdf5 puts into the unused part of an edge chunk and lets the coder's gather run without bounds tests), a
// second image [12][Yp][Xp] for the monthly means, and the coder's workspace.
//
//   k_mo_clear     fills layers with TWX_FILL_I2, 16-byte stores
//   k_mo_place     a wavefront per row of a slab [nd][ty][tx]: the widest unit (16, 8, 4 or 2 bytes) at which the row's source
//                  and destination agree is loaded and stored aligned, the values before the first and after the last unit one
//                  by one.  Slabs come up through two pinned staging buffers on a copy stream: the upload of slab t + 1 runs
//                  under the placement of slab t.
//   the coder      the kernels of topowx_amd/csrc/twx_deflate.h AS THEY ARE.  A mosaic chunk is (1, cy, cx): the image
//                  [nd][Yp][Xp] is handed to them as ONE layer of nd * Yp rows, so chunk (row r, column c) of day d is chunk
//                  (d * ncy + r) * ncx + c of that layer -- stream d * nchunk + ch, the order of the file -- and the day never
//                  enters the kernels: the day is folded into the chunk index on the host side of DfArgs.  One Huffman code per
//                  call, from segment 0 of every chunk of every day (TWX_DF_SAMPLE = 16 >= the segments of a mosaic chunk).
//   k_mo_compact   a work-group per stream: its bytes from the slot to their scanned offset in one packed block (aligned
//                  4-byte loads and stores; source words are funnel-shifted to the destination's alignment), copied out in one
//                  transfer
//   k_agg          topowx_amd/csrc/twx_agg.h as it is, on the resident image: ncell = Yp * Xp, twelve groups
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "twx.h"
#include "twx_qa.h"
#include "twx_mosaic_host.h"
#include "../csrc/twx_device.h"

namespace {                                 // (the coder's and the aggregation's kernels get internal linkage in this library)
#include "../csrc/twx_deflate.h"
#include "../csrc/twx_agg.h"

static_assert(TWXMO_DF_SEG == TWX_DF_SEG && TWXMO_DF_STORED == TWX_DF_STORED && TWXMO_DF_THREADS == TWX_DF_THREADS &&
              TWXMO_DF_NSYM == TWX_DF_NSYM, "twx_mosaic_host.h restates the coder's constants");
static_assert(TWXMO_NGROUPS == 7, "timing groups");

constexpr int MO_BLOCK = 256;
constexpr int MO_MAX_BLOCKS = 8192;

template <int W> struct MoVec { int16_t v[W]; };

__global__ __launch_bounds__(MO_BLOCK) void k_mo_clear(int16_t *__restrict__ img, int64_t n)
{
    typedef MoVec<8> __attribute__((aligned(16))) vec_t;
    vec_t f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f.v[e] = TWX_FILL_I2;
    const int64_t nv = n / 8, stride = (int64_t)gridDim.x * MO_BLOCK;
    vec_t *o = reinterpret_cast<vec_t *>(img);                                 // (the image is 256-byte aligned)
    for (int64_t i = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; i < nv; i += stride) o[i] = f;
    if (blockIdx.x == 0 && threadIdx.x < n - nv * 8) img[nv * 8 + threadIdx.x] = TWX_FILL_I2;
}

template <int W>
__device__ __forceinline__ void mo_copy_row(const int16_t *__restrict__ s, int16_t *__restrict__ d, int n, int lane)
{
    typedef MoVec<W> __attribute__((aligned(2 * W))) vec_t;
    const int head = mo_copy_head((uint64_t)reinterpret_cast<uintptr_t>(d) / 2, W, n);     // (< 8 <= 64 lanes)
    if (lane < head) d[lane] = s[lane];
    const int nv = (n - head) / W;
    for (int j = lane; j < nv; j += 64)
        *reinterpret_cast<vec_t *>(d + head + j * W) = *reinterpret_cast<const vec_t *>(s + head + j * W);
    const int t0 = head + nv * W;
    if (lane < n - t0) d[t0 + lane] = s[t0 + lane];                                          // (< W <= 8 values)
}

// src [nd][ty][tx] -> img[(d * Yp + y0 + r) * Xp + x0 ..]; the host has checked that the slab lies inside the image
__global__ __launch_bounds__(MO_BLOCK) void k_mo_place(const int16_t *__restrict__ src, int16_t *__restrict__ img, int64_t nrow, int ty,
                                                       int tx, int y0, int x0, int64_t Yp, int64_t Xp)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * (MO_BLOCK / 64);
    for (int64_t row = (int64_t)blockIdx.x * (MO_BLOCK / 64) + (threadIdx.x >> 6); row < nrow; row += stride) {
        const int64_t d = row / ty;
        const int r = (int)(row - d * ty);
        const int16_t *s = src + row * tx;
        int16_t *o = img + (d * Yp + y0 + r) * Xp + x0;
        // wave-uniform: every lane of the wave copies the same row
        const int w = mo_copy_width((uint64_t)reinterpret_cast<uintptr_t>(s) / 2, (uint64_t)reinterpret_cast<uintptr_t>(o) / 2);
        if (w == 8) mo_copy_row<8>(s, o, tx, lane);
        else if (w == 4) mo_copy_row<4>(s, o, tx, lane);
        else if (w == 2) mo_copy_row<2>(s, o, tx, lane);
        else mo_copy_row<1>(s, o, tx, lane);
    }
}

// stream k: chunk_bytes[k] bytes from slot k to packed + offset[k]
__global__ __launch_bounds__(MO_BLOCK) void k_mo_compact(const uint8_t *__restrict__ slots, int64_t slot_bytes,
                                                         const int64_t *__restrict__ offset, uint8_t *__restrict__ packed)
{
    const int64_t k = blockIdx.x;
    const int64_t o = offset[k];
    const int n = (int)(offset[k + 1] - o);
    const uint8_t *s = slots + k * slot_bytes;                                 // (256-byte aligned)
    uint8_t *d = packed + o;
    int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 3u)) & 3u);
    if (head > n) head = n;
    const int t = threadIdx.x;
    if (t < head) d[t] = s[t];
    const int nw = (n - head) / 4;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s);
    uint32_t *dw = reinterpret_cast<uint32_t *>(d + head);
    const unsigned sh = 8u * (unsigned)head;                                   // destination word j = source bytes head + 4 j ..
    for (int j = t; j < nw; j += MO_BLOCK) {
        const uint32_t lo = sw[j];
        // (the word after the stream's last lies inside the slot or the 256 bytes allocated behind the last slot)
        dw[j] = sh ? (lo >> sh) | (sw[j + 1] << (32u - sh)) : lo;
    }
    const int t0 = head + nw * 4;
    if (t < n - t0) d[t0 + t] = s[t0 + t];
}

struct EvP { hipEvent_t a = nullptr, b = nullptr; };

}  // namespace

struct twxmo_mosaic {
    int device = 0;
    MoDims d{};
    std::string err;
    hipStream_t s_comp = nullptr, s_copy = nullptr;
    int16_t *img = nullptr, *mimg = nullptr;
    uint8_t *slots = nullptr;
    char *small = nullptr;
    int32_t *agg_dev = nullptr;                    // [13 + max_days] group starts, day indices
    uint8_t *packed = nullptr; size_t packed_cap = 0;
    uint8_t *h_packed = nullptr; size_t h_packed_cap = 0;       // pinned: the compacted streams of the last twxmo_deflate
    int64_t *h_sizes = nullptr, *h_off = nullptr;   // pinned [layers * nchunk], [layers * nchunk + 1]
    // the coder's workspace inside `small`
    uint32_t *seg_bytes = nullptr, *seg_off = nullptr, *adl = nullptr, *hist = nullptr;
    uint16_t *piece_bits = nullptr;
    int64_t *chunk_bytes = nullptr, *d_off = nullptr;
    DfTable *table = nullptr;
    // slabs: two pinned host buffers and their device images
    int16_t *h_stage[2] = {nullptr, nullptr}, *d_stage[2] = {nullptr, nullptr};
    size_t stage_cap = 0;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};
    int next_stage = 0;
    // timing
    EvP ev[TWXMO_NGROUPS];
    bool ev_set[TWXMO_NGROUPS] = {};
    float acc[TWXMO_NGROUPS] = {};                  // earlier runs of a group since the last twxmo_clear
    std::vector<EvP> place_ev;
    size_t place_used = 0;
    float place_acc = 0.f;
    int64_t pinned_bytes = 0, device_bytes = 0;
};

namespace {

int mo_fail(twxmo_mosaic *m, const char *what, hipError_t e = hipSuccess)
{
    if (m) {
        m->err = what;
        if (e != hipSuccess) { m->err += ": "; m->err += hipGetErrorString(e); }
    }
    return -1;
}

#define MOCHK(call)                                                          \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return mo_fail(m, #call, e_);                  \
    } while (0)

template <class T> T *mo_carve(char *&cur, int64_t count)
{
    T *r = reinterpret_cast<T *>(cur);
    cur += mo_round256(count * (int64_t)sizeof(T));
    return r;
}

struct MoScope {                                   // events around a group of launches on the compute stream
    twxmo_mosaic *m; int g;
    MoScope(twxmo_mosaic *m_, int g_) : m(m_), g(g_)
    {
        if (!m->ev[g].a) { (void)hipEventCreate(&m->ev[g].a); (void)hipEventCreate(&m->ev[g].b); }
        if (m->ev_set[g]) {                        // the group ran before: its time is kept, the pair is used again
            float ms = 0.f;
            if (hipEventSynchronize(m->ev[g].b) == hipSuccess && hipEventElapsedTime(&ms, m->ev[g].a, m->ev[g].b) == hipSuccess)
                m->acc[g] += ms;
            m->ev_set[g] = false;
        }
        (void)hipEventRecord(m->ev[g].a, m->s_comp);
    }
    ~MoScope() { (void)hipEventRecord(m->ev[g].b, m->s_comp); m->ev_set[g] = true; }
};

int mo_fold_place(twxmo_mosaic *m)                 // the placement kernels' event pairs -> place_acc (synchronises)
{
    for (size_t i = 0; i < m->place_used; ++i) {
        float ms = 0.f;
        MOCHK(hipEventSynchronize(m->place_ev[i].b));
        MOCHK(hipEventElapsedTime(&ms, m->place_ev[i].a, m->place_ev[i].b));
        m->place_acc += ms;
    }
    m->place_used = 0;
    return 0;
}

int mo_stage_reserve(twxmo_mosaic *m, size_t bytes)
{
    if (bytes <= m->stage_cap) return 0;
    MOCHK(hipStreamSynchronize(m->s_copy));
    MOCHK(hipStreamSynchronize(m->s_comp));
    const size_t want = (bytes + bytes / 8 + 4095) / 4096 * 4096;
    for (int k = 0; k < 2; ++k) {
        if (m->h_stage[k]) (void)hipHostFree(m->h_stage[k]);
        if (m->d_stage[k]) (void)hipFree(m->d_stage[k]);
        m->h_stage[k] = nullptr; m->d_stage[k] = nullptr; m->stage_used[k] = false;
    }
    m->pinned_bytes -= 2 * (int64_t)m->stage_cap; m->device_bytes -= 2 * (int64_t)m->stage_cap;
    m->stage_cap = 0;
    for (int k = 0; k < 2; ++k) {
        MOCHK(hipHostMalloc((void **)&m->h_stage[k], want, hipHostMallocDefault));
        MOCHK(hipMalloc((void **)&m->d_stage[k], want));
    }
    m->stage_cap = want;
    m->pinned_bytes += 2 * (int64_t)want; m->device_bytes += 2 * (int64_t)want;
    return 0;
}

void mo_release(twxmo_mosaic *m)
{
    (void)hipSetDevice(m->device);
    if (m->s_comp) (void)hipStreamSynchronize(m->s_comp);
    if (m->s_copy) (void)hipStreamSynchronize(m->s_copy);
    for (void *p : {(void *)m->img, (void *)m->mimg, (void *)m->slots, (void *)m->small, (void *)m->agg_dev, (void *)m->packed,
                    (void *)m->d_stage[0], (void *)m->d_stage[1]})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)m->h_packed, (void *)m->h_sizes, (void *)m->h_off, (void *)m->h_stage[0], (void *)m->h_stage[1]})
        if (p) (void)hipHostFree(p);
    for (int k = 0; k < 2; ++k) {
        if (m->ev_up[k]) (void)hipEventDestroy(m->ev_up[k]);
        if (m->ev_free[k]) (void)hipEventDestroy(m->ev_free[k]);
    }
    for (EvP &e : m->ev) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
    for (EvP &e : m->place_ev) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
    if (m->s_comp) (void)hipStreamDestroy(m->s_comp);
    if (m->s_copy) (void)hipStreamDestroy(m->s_copy);
    delete m;
}

void mo_err(char *errbuf, int errlen, const std::string &s)
{
    if (errbuf && errlen > 0) std::snprintf(errbuf, (size_t)errlen, "%s", s.c_str());
}

}  // namespace

extern "C" int twxmo_sizes(int64_t max_days, int32_t Y, int32_t X, int32_t chunk_y, int32_t chunk_x, int64_t *sizes, char *errbuf,
                           int errlen)
{
    MoDims d;
    const char *bad = mo_dims(max_days, Y, X, chunk_y, chunk_x, (int64_t)sizeof(DfTable), &d);
    if (bad || !sizes) { mo_err(errbuf, errlen, std::string("twxmo_sizes: ") + (bad ? bad : "sizes is NULL")); return -1; }
    if (d.slot_bytes != df_slot_bytes(d.N) || d.nseg != df_nseg(d.N) || d.lo_bytes != df_lo_bytes(d.N)) {
        mo_err(errbuf, errlen, "twxmo_sizes: the slot arithmetic disagrees with the coder's");
        return -1;
    }
    sizes[TWXMO_S_YP] = d.Yp; sizes[TWXMO_S_XP] = d.Xp; sizes[TWXMO_S_NCHUNK] = d.nchunk; sizes[TWXMO_S_NSEG] = d.nseg;
    sizes[TWXMO_S_SLOT_BYTES] = d.slot_bytes; sizes[TWXMO_S_DEVICE_BYTES] = d.device_bytes;
    sizes[TWXMO_S_PINNED_BYTES] = mo_round256(d.layers * d.nchunk * 8) + mo_round256((d.layers * d.nchunk + 1) * 8);
    sizes[TWXMO_S_VEC] = d.vec;
    return 0;
}

extern "C" int twxmo_create(int device, int64_t max_days, int32_t Y, int32_t X, int32_t chunk_y, int32_t chunk_x, twxmo_mosaic **out,
                            char *errbuf, int errlen)
{
    int64_t sz[TWXMO_S_N];
    if (!out) { mo_err(errbuf, errlen, "twxmo_create: out is NULL"); return -1; }
    *out = nullptr;
    if (twxmo_sizes(max_days, Y, X, chunk_y, chunk_x, sz, errbuf, errlen)) return -1;
    twxmo_mosaic *m = new (std::nothrow) twxmo_mosaic();
    if (!m) { mo_err(errbuf, errlen, "twxmo_create: out of host memory"); return -1; }
    m->device = device;
    (void)mo_dims(max_days, Y, X, chunk_y, chunk_x, (int64_t)sizeof(DfTable), &m->d);
    const MoDims &d = m->d;
    auto body = [&]() -> int {
        MOCHK(hipSetDevice(device));
        size_t free_b = 0, total_b = 0;
        MOCHK(hipMemGetInfo(&free_b, &total_b));
        // the packed block of a call is allocated when its size is known; at worst it is as large as the slots
        const int64_t need = d.device_bytes + (int64_t)(64 << 20);
        if (need > (int64_t)free_b) {
            char msg[256];
            std::snprintf(msg, sizeof msg, "twxmo_create: %lld days of %d x %d need %.2f GB of device memory, %.2f GB are free: "
                          "ask for fewer days", (long long)max_days, Y, X, need / 1e9, free_b / 1e9);
            return mo_fail(m, msg);
        }
        MOCHK(hipStreamCreateWithFlags(&m->s_comp, hipStreamNonBlocking));
        MOCHK(hipStreamCreateWithFlags(&m->s_copy, hipStreamNonBlocking));
        MOCHK(hipMalloc((void **)&m->img, (size_t)d.image_bytes));
        MOCHK(hipMalloc((void **)&m->mimg, (size_t)d.mthly_bytes));
        MOCHK(hipMalloc((void **)&m->slots, (size_t)d.slots_bytes));
        MOCHK(hipMalloc((void **)&m->small, (size_t)d.small_bytes));
        MOCHK(hipMalloc((void **)&m->agg_dev, (size_t)(TWXMO_MONTHS + 1 + d.max_days) * 4));
        m->device_bytes = d.device_bytes + (TWXMO_MONTHS + 1 + d.max_days) * 4;
        const int64_t nslot = d.layers * d.nchunk, per = nslot * d.nseg;
        char *cur = m->small;
        m->seg_bytes = mo_carve<uint32_t>(cur, per);
        m->seg_off = mo_carve<uint32_t>(cur, per);
        m->adl = mo_carve<uint32_t>(cur, per * 4);
        m->piece_bits = mo_carve<uint16_t>(cur, per * TWX_DF_THREADS);
        m->chunk_bytes = mo_carve<int64_t>(cur, nslot);
        m->d_off = mo_carve<int64_t>(cur, nslot + 1);
        m->hist = mo_carve<uint32_t>(cur, TWX_DF_NSYM);
        m->table = reinterpret_cast<DfTable *>(cur);
        cur += mo_round256((int64_t)sizeof(DfTable));
        if (cur - m->small != d.small_bytes) return mo_fail(m, "twxmo_create: workspace arithmetic");
        MOCHK(hipHostMalloc((void **)&m->h_sizes, (size_t)mo_round256(nslot * 8), hipHostMallocDefault));
        MOCHK(hipHostMalloc((void **)&m->h_off, (size_t)mo_round256((nslot + 1) * 8), hipHostMallocDefault));
        m->pinned_bytes = sz[TWXMO_S_PINNED_BYTES];
        for (int k = 0; k < 2; ++k) {
            MOCHK(hipEventCreateWithFlags(&m->ev_up[k], hipEventDisableTiming));
            MOCHK(hipEventCreateWithFlags(&m->ev_free[k], hipEventDisableTiming));
        }
        return 0;
    };
    if (body()) {
        mo_err(errbuf, errlen, m->err);
        mo_release(m);
        return -1;
    }
    *out = m;
    return 0;
}

extern "C" void twxmo_destroy(twxmo_mosaic *m)
{
    if (m) mo_release(m);
}

extern "C" const char *twxmo_last_error(const twxmo_mosaic *m) { return m ? m->err.c_str() : "no mosaic"; }

extern "C" int twxmo_clear(twxmo_mosaic *m, int64_t ndays)
{
    if (!m) return -1;
    m->err.clear();
    if (ndays < 1 || ndays > m->d.max_days) return mo_fail(m, "twxmo_clear: ndays outside 1 .. max_days");
    MOCHK(hipSetDevice(m->device));
    if (mo_fold_place(m)) return -1;
    m->place_acc = 0.f;
    for (bool &b : m->ev_set) b = false;
    for (float &f : m->acc) f = 0.f;
    const int64_t n = ndays * m->d.Yp * m->d.Xp;
    const int64_t nb = (n / 8 + MO_BLOCK - 1) / MO_BLOCK;
    MoScope ev(m, TWXMO_T_CLEAR);
    hipLaunchKernelGGL(k_mo_clear, dim3((unsigned)(nb < 1 ? 1 : nb > MO_MAX_BLOCKS ? MO_MAX_BLOCKS : nb)), dim3(MO_BLOCK), 0, m->s_comp,
                       m->img, n);
    MOCHK(hipGetLastError());
    return 0;
}

extern "C" int twxmo_staging(twxmo_mosaic *m, int64_t bytes, void **ptr)
{
    if (!m) return -1;
    m->err.clear();
    if (bytes < 1 || !ptr) return mo_fail(m, "twxmo_staging: bad arguments");
    MOCHK(hipSetDevice(m->device));
    if (mo_stage_reserve(m, (size_t)bytes)) return -1;
    const int k = m->next_stage;
    if (m->stage_used[k]) MOCHK(hipEventSynchronize(m->ev_free[k]));           // the placement that read its image is done
    *ptr = m->h_stage[k];
    return 0;
}

extern "C" int twxmo_place(twxmo_mosaic *m, const int16_t *src, int64_t nd, int32_t ty, int32_t tx, int32_t y0, int32_t x0)
{
    if (!m) return -1;
    m->err.clear();
    if (!src) return mo_fail(m, "twxmo_place: src is NULL");
    const char *bad = mo_check_place(m->d, nd, ty, tx, y0, x0);
    if (bad) { m->err = std::string("twxmo_place: ") + bad; return -1; }
    MOCHK(hipSetDevice(m->device));
    const size_t bytes = (size_t)nd * ty * tx * 2;
    const bool own = m->stage_cap && src == m->h_stage[m->next_stage];         // the caller filled twxmo_staging's buffer
    if (!own && mo_stage_reserve(m, bytes)) return -1;
    if (own && bytes > m->stage_cap) return mo_fail(m, "twxmo_place: the slab is larger than the staging buffer asked for");
    const int k = m->next_stage;
    if (m->stage_used[k]) MOCHK(hipEventSynchronize(m->ev_free[k]));
    if (!own) std::memcpy(m->h_stage[k], src, bytes);
    MOCHK(hipMemcpyAsync(m->d_stage[k], m->h_stage[k], bytes, hipMemcpyHostToDevice, m->s_copy));
    MOCHK(hipEventRecord(m->ev_up[k], m->s_copy));
    MOCHK(hipStreamWaitEvent(m->s_comp, m->ev_up[k], 0));
    if (m->place_used >= 1024 && mo_fold_place(m)) return -1;
    if (m->place_used == m->place_ev.size()) {
        EvP e;
        MOCHK(hipEventCreate(&e.a)); MOCHK(hipEventCreate(&e.b));
        m->place_ev.push_back(e);
    }
    EvP &e = m->place_ev[m->place_used++];
    const int64_t nrow = nd * ty, nb = (nrow + MO_BLOCK / 64 - 1) / (MO_BLOCK / 64);
    MOCHK(hipEventRecord(e.a, m->s_comp));
    hipLaunchKernelGGL(k_mo_place, dim3((unsigned)(nb > MO_MAX_BLOCKS ? MO_MAX_BLOCKS : nb)), dim3(MO_BLOCK), 0, m->s_comp,
                       (const int16_t *)m->d_stage[k], m->img, nrow, (int)ty, (int)tx, (int)y0, (int)x0, (int64_t)m->d.Yp, (int64_t)m->d.Xp);
    MOCHK(hipEventRecord(e.b, m->s_comp));
    MOCHK(hipEventRecord(m->ev_free[k], m->s_comp));
    MOCHK(hipGetLastError());
    m->stage_used[k] = true;
    m->next_stage = k ^ 1;
    return 0;
}

extern "C" int twxmo_download(twxmo_mosaic *m, int which, int64_t nlayers, int16_t *dst)
{
    if (!m) return -1;
    m->err.clear();
    const int64_t cap = which == TWXMO_MONTHLY ? TWXMO_MONTHS : m->d.max_days;
    if ((which != TWXMO_DAILY && which != TWXMO_MONTHLY) || nlayers < 1 || nlayers > cap || !dst)
        return mo_fail(m, "twxmo_download: bad arguments");
    MOCHK(hipSetDevice(m->device));
    MOCHK(hipStreamSynchronize(m->s_comp));
    MOCHK(hipMemcpy(dst, which == TWXMO_MONTHLY ? m->mimg : m->img, (size_t)nlayers * m->d.Yp * m->d.Xp * 2, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int twxmo_monthly(twxmo_mosaic *m, int64_t ndays, const int32_t *day_month)
{
    if (!m) return -1;
    m->err.clear();
    if (ndays < 1 || ndays > m->d.max_days || !day_month) return mo_fail(m, "twxmo_monthly: bad arguments");
    std::vector<int32_t> g((size_t)(TWXMO_MONTHS + 1 + ndays), 0);
    for (int64_t i = 0; i < ndays; ++i) {
        if (day_month[i] < 1 || day_month[i] > 12) return mo_fail(m, "twxmo_monthly: month outside 1..12");
        g[(size_t)day_month[i]]++;                                             // (counts at [month]: the scan makes them starts)
    }
    for (int k = 1; k <= TWXMO_MONTHS; ++k) g[(size_t)k] += g[(size_t)k - 1];
    std::vector<int32_t> fillp(g.begin(), g.begin() + TWXMO_MONTHS);
    for (int64_t i = 0; i < ndays; ++i) g[(size_t)(TWXMO_MONTHS + 1 + fillp[(size_t)day_month[i] - 1]++)] = (int32_t)i;
    MOCHK(hipSetDevice(m->device));
    MOCHK(hipStreamSynchronize(m->s_comp));                                    // (agg_dev may still be read by an earlier call)
    MOCHK(hipMemcpy(m->agg_dev, g.data(), g.size() * 4, hipMemcpyHostToDevice));
    AggAxis ax{};
    ax.ng = TWXMO_MONTHS; ax.nyr = 1; ax.nmth = TWXMO_MONTHS; ax.gstart = m->agg_dev; ax.gday = m->agg_dev + TWXMO_MONTHS + 1;
    const int64_t ncell = (int64_t)m->d.Yp * m->d.Xp;
    MoScope ev(m, TWXMO_T_AGGREGATE);
    // (both images are 256-byte aligned: the widest loads whose rows stay aligned depend on ncell alone)
    if (ncell % 8 == 0) launch_agg<int16_t, 8>(m->img, ncell, ax, nullptr, m->mimg, nullptr, m->s_comp);
    else if (ncell % 4 == 0) launch_agg<int16_t, 4>(m->img, ncell, ax, nullptr, m->mimg, nullptr, m->s_comp);
    else launch_agg<int16_t, 1>(m->img, ncell, ax, nullptr, m->mimg, nullptr, m->s_comp);
    MOCHK(hipGetLastError());
    return 0;
}

extern "C" int twxmo_deflate(twxmo_mosaic *m, int which, int64_t nlayers, twxmo_streams *out)
{
    if (!m) return -1;
    m->err.clear();
    const MoDims &d = m->d;
    const int64_t cap = which == TWXMO_MONTHLY ? TWXMO_MONTHS : d.max_days;
    if ((which != TWXMO_DAILY && which != TWXMO_MONTHLY) || nlayers < 1 || nlayers > cap || !out)
        return mo_fail(m, "twxmo_deflate: bad arguments");
    MOCHK(hipSetDevice(m->device));
    const int64_t n = nlayers * d.nchunk;                                      // (<= layers * nchunk <= the grid's x dimension)
    DfArgs a{};
    a.daily = reinterpret_cast<const uint16_t *>(which == TWXMO_MONTHLY ? m->mimg : m->img);
    a.out = m->slots;
    a.seg_bytes = m->seg_bytes; a.seg_off = m->seg_off; a.adl = m->adl; a.piece_bits = m->piece_bits;
    a.chunk_bytes = m->chunk_bytes; a.hist = m->hist; a.table = m->table;
    a.N = d.N; a.slot_bytes = d.slot_bytes; a.lo_bytes = d.lo_bytes;
    a.Y = (int32_t)(nlayers * d.Yp);                                           // the layers as ONE layer of nlayers * Yp rows
    a.X = d.Xp; a.cy = d.cy; a.cx = d.cx; a.ncx = d.ncx; a.nseg = d.nseg;
    const dim3 grid((unsigned)n, (unsigned)d.nseg), sgrid((unsigned)n, (unsigned)((d.nseg + TWX_DF_SAMPLE - 1) / TWX_DF_SAMPLE));
    const dim3 th(TWX_DF_THREADS);
    {
        MoScope ev(m, TWXMO_T_HIST);
        MOCHK(hipMemsetAsync(a.hist, 0, TWX_DF_NSYM * 4, m->s_comp));
        if (d.vec == 2) hipLaunchKernelGGL(k_deflate_hist<2>, sgrid, th, 0, m->s_comp, a);
        else hipLaunchKernelGGL(k_deflate_hist<1>, sgrid, th, 0, m->s_comp, a);
        hipLaunchKernelGGL(k_deflate_table, dim3(1), th, 0, m->s_comp, (const uint32_t *)a.hist, a.table, (const uint32_t *)a.hist, a.table);
    }
    {
        MoScope ev(m, TWXMO_T_COUNT);
        if (d.vec == 2) hipLaunchKernelGGL(k_deflate_count<2>, grid, th, 0, m->s_comp, a);
        else hipLaunchKernelGGL(k_deflate_count<1>, grid, th, 0, m->s_comp, a);
        hipLaunchKernelGGL(k_deflate_scan, dim3((unsigned)n), th, 0, m->s_comp, a);
    }
    {
        MoScope ev(m, TWXMO_T_EMIT);
        if (d.vec == 2) hipLaunchKernelGGL(k_deflate_emit<2>, grid, th, 0, m->s_comp, a);
        else hipLaunchKernelGGL(k_deflate_emit<1>, grid, th, 0, m->s_comp, a);
    }
    MOCHK(hipGetLastError());
    // the sizes are final after the scan: they come down while the emission runs behind them on the compute stream
    MOCHK(hipMemcpyAsync(m->h_sizes, m->chunk_bytes, (size_t)n * 8, hipMemcpyDeviceToHost, m->s_comp));
    MOCHK(hipStreamSynchronize(m->s_comp));
    const char *bad = mo_offsets(m->h_sizes, n, d.slot_bytes, m->h_off);
    if (bad) { m->err = std::string("twxmo_deflate: ") + bad + " (device fault?)"; return -1; }
    const size_t total = (size_t)m->h_off[n];
    if (total > m->packed_cap) {
        if (m->packed) (void)hipFree(m->packed);
        m->packed = nullptr; m->device_bytes -= (int64_t)m->packed_cap; m->packed_cap = 0;
        const size_t want = (total + total / 8 + 4095) / 4096 * 4096;
        MOCHK(hipMalloc((void **)&m->packed, want));
        m->packed_cap = want; m->device_bytes += (int64_t)want;
    }
    if (total > m->h_packed_cap) {
        if (m->h_packed) (void)hipHostFree(m->h_packed);
        m->h_packed = nullptr; m->pinned_bytes -= (int64_t)m->h_packed_cap; m->h_packed_cap = 0;
        const size_t want = (total + total / 8 + 4095) / 4096 * 4096;
        MOCHK(hipHostMalloc((void **)&m->h_packed, want, hipHostMallocDefault));
        m->h_packed_cap = want; m->pinned_bytes += (int64_t)want;
    }
    MOCHK(hipMemcpyAsync(m->d_off, m->h_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, m->s_comp));
    {
        MoScope ev(m, TWXMO_T_COMPACT);
        hipLaunchKernelGGL(k_mo_compact, dim3((unsigned)n), dim3(MO_BLOCK), 0, m->s_comp, (const uint8_t *)m->slots, d.slot_bytes,
                           (const int64_t *)m->d_off, m->packed);
    }
    MOCHK(hipGetLastError());
    MOCHK(hipMemcpyAsync(m->h_packed, m->packed, total, hipMemcpyDeviceToHost, m->s_comp));
    MOCHK(hipStreamSynchronize(m->s_comp));
    out->data = m->h_packed; out->offset = m->h_off; out->nstreams = n; out->nchunk = d.nchunk;
    out->chunk_y = d.cy; out->chunk_x = d.cx; out->slot_bytes = d.slot_bytes;
    return 0;
}

extern "C" int twxmo_timing(twxmo_mosaic *m, float *kernel_ms, int64_t *device_bytes, int64_t *pinned_bytes)
{
    if (!m) return -1;
    m->err.clear();
    MOCHK(hipSetDevice(m->device));
    if (mo_fold_place(m)) return -1;
    if (kernel_ms) {
        for (int g = 0; g < TWXMO_NGROUPS; ++g) {
            kernel_ms[g] = 0.f;
            if (g == TWXMO_T_PLACE) { kernel_ms[g] = m->place_acc; continue; }
            kernel_ms[g] = m->acc[g];
            if (!m->ev_set[g]) continue;
            float ms = 0.f;
            MOCHK(hipEventSynchronize(m->ev[g].b));
            MOCHK(hipEventElapsedTime(&ms, m->ev[g].a, m->ev[g].b));
            kernel_ms[g] += ms;
        }
    }
    if (device_bytes) *device_bytes = m->device_bytes;
    if (pinned_bytes) *pinned_bytes = m->pinned_bytes;
    return 0;
}
