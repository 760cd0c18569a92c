// The host scaffold and the small helpers that the units of libtwxqa.so share (every topowx_amd/qa/twx_*.hip but
// twx_mosaic.hip, whose errors and events belong to a persistent object).  Internal: a quoted include finds it next to
// the units.  Everything has internal linkage, so each unit gets its own copy and the library exports none of it.
//
// The macros return from the enclosing function: they need `char *errbuf, int errlen` in scope.
#ifndef TWX_QA_COMMON_H
#define TWX_QA_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <vector>

namespace {

// The message of a failed entry: `what`, and the runtime's text of `e` after it where there is one.  Always -1.
inline int qa_fail(char *errbuf, int errlen, const char *what, hipError_t e = hipSuccess)
{
    if (errbuf && errlen > 0) {
        if (e != hipSuccess) snprintf(errbuf, (size_t)errlen, "%s: %s", what, hipGetErrorString(e));
        else snprintf(errbuf, (size_t)errlen, "%s", what);
    }
    return -1;
}

struct QaBuf {                                                   // one device allocation; the unit calls hipMalloc(&p, ..)
    void *p = nullptr;
    ~QaBuf() { if (p) (void)hipFree(p); }
};

struct QaPool {                                                  // every device allocation of a call, freed together
    std::vector<void *> p;
    ~QaPool() { for (void *x : p) if (x) (void)hipFree(x); }
    hipError_t get(void **out, size_t bytes)                     // an empty array still gets a pointer a kernel may be handed
    {
        hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
};

struct QaTimer {                                                 // HIP-event time of work on the null stream
    hipEvent_t a = nullptr, b = nullptr;
    ~QaTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t init() { hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
    hipError_t start() { return hipEventRecord(a, nullptr); }
    hipError_t stop_set(float *ms)                               // *ms = the milliseconds since start()
    {
        hipError_t e = hipEventRecord(b, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(ms, a, b);
        return e;
    }
    hipError_t stop_add(float *acc)                              // *acc += the milliseconds since start()
    {
        float ms = 0.0f;
        hipError_t e = hipEventRecord(b, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
        *acc += ms;
        return e;
    }
};

inline float qa_since(std::chrono::steady_clock::time_point t)   // host milliseconds since t
{
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
}

inline int64_t qa_days_from_civil(int64_t y, int mth, int day)   // days since 1970-01-01, proleptic Gregorian
{
    y -= mth <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const int64_t yoe = y - era * 400;
    const int64_t doy = (153 * (mth + (mth > 2 ? -3 : 9)) + 2) / 5 + day - 1;
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

inline bool qa_leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }

#ifdef __HIPCC__

#define QA_RADIAN 0.017453292519943295       // util_geo.py:21
#define QA_EARTH_KM 6371.009                 // util_geo.py:22

// Haversine distance in km from a point given in radians (cos1 = cos(lat1rad), hoisted) to one given in degrees.
__device__ __forceinline__ double qa_dist_km(double lat1rad, double lon1rad, double cos1, double lat2, double lon2)
{
    const double lat2rad = lat2 * QA_RADIAN, lon2rad = lon2 * QA_RADIAN;
    const double s1 = sin((lat1rad - lat2rad) / 2.0), s2 = sin((lon1rad - lon2rad) / 2.0);
    const double a = s1 * s1 + (cos1 * cos(lat2rad)) * (s2 * s2);
    return QA_EARTH_KM * (2.0 * asin(sqrt(a)));
}

// xor-butterfly reductions over the 64 lanes of a wave: every lane gets the result, summed in the same order.
__device__ __forceinline__ double qa_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ int qa_wave_sum_i(int v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double qa_wave_max(double v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

#endif  // __HIPCC__

}  // namespace

#define QACHK(call)                                                                     \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) return qa_fail(errbuf, errlen, #call, e_);                \
    } while (0)
#define QAALLOC(pool, ptr, type, count) QACHK((pool).get((void **)&(ptr), (size_t)(count) * sizeof(type)))
#define QAUP(dst, src, type, count) QACHK(hipMemcpy((dst), (src), (size_t)(count) * sizeof(type), hipMemcpyHostToDevice))
#define QADOWN(dst, src, type, count) QACHK(hipMemcpy((dst), (src), (size_t)(count) * sizeof(type), hipMemcpyDeviceToHost))
// the same, but an empty array is not copied (its host pointer may be null)
#define QAUP_NZ(dst, src, type, count)                                                  \
    do {                                                                                \
        if ((count) > 0) QAUP(dst, src, type, count);                                   \
    } while (0)
#define QADOWN_NZ(dst, src, type, count)                                                \
    do {                                                                                \
        if ((count) > 0) QADOWN(dst, src, type, count);                                 \
    } while (0)

#endif  // TWX_QA_COMMON_H
