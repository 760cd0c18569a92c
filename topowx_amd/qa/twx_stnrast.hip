// twx_stnrast.hip -- libtwxqa.so: raster values at stations (add_stn_raster_values and _find_nn_data,
// twx/infill/post_infill.py:248-352 and :443-510, of scripts/step19_add_raster_predictors.py) and the front of step20
// (find_dup_stns, post_infill.py:193-246, and the "no good station has a missing value" check of
// scripts/step20_add_bad_stn_flag.py:102-112), as include/twx_qa.h states them (twxrv_sample, twxrv_nearest_data,
// twxrv_dup_classes, twxrv_col_count).  Its own translation unit; the buffer list and the event timer it shares with
// the other units are twx_qa_common.h's.
//
// k_rv_sample: one thread per station, a gather of at most five cells.  mpl_toolkits.basemap.interp is restated with the
// expressions of k_sample (topowx_amd/csrc/twx_sample.h); the raster is read north-up, so the row of interp's flipped copy
// is rows - 1 - yi.
// k_rv_ring: one wavefront per station.  Ring r has 8 r + 2 slots in the reference's order (top row left to right, left
// column top to bottom, bottom row right to left without its last cell, right column bottom to top without its last cell;
// two corners are met twice, as in the reference).  Lane l takes the slots l, l + 64, ...; the (distance, slot) minimum is
// reduced by a butterfly, so a tie goes to the earlier slot.  The loop ends at the first ring with a data cell or at the
// cap max(rows, cols); a second pass over that ring gives the nearest data cell that is not the winner's cell.
// k_rv_dup: all pairs, the keys lat * F and lon * F of 256 stations a tile staged in LDS.
// k_rv_colcount: a workgroup of 256 is 64 columns x 4 day slices of a [days][stations] block, station fastest, so a
// wavefront reads 64 consecutive stations of one day; the slices meet in LDS and an integer atomic adds the workgroup's
// count: exact in any order, two calls give the same bytes.
// Every cell index is tested against the raster before it is read; every loop is bounded by the ring cap, by the tile or
// by the days of a workgroup; nothing waits on another workgroup.  fp64 throughout; built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "twx_qa.h"
#include "twx_qa_common.h"

#define RV_THREADS 256
#define RV_RADIAN 0.017453292519943295       // RADIAN_CONVERSION_FACTOR, twx/utils/util_geo.py:21
#define RV_EARTH_KM 6371.009                 // AVG_EARTH_RADIUS_KM
#define RV_NO_SLOT 0x7fffffff
#define RV_COLS_PER_GROUP 64                 // columns of a workgroup of k_rv_colcount
#define RV_SLICES (RV_THREADS / RV_COLS_PER_GROUP)
#define RV_DAYS_PER_GROUP 512                // days of a workgroup of k_rv_colcount
#define RV_FLT_MAX 3.402823466e+38f

namespace {

struct RvGrid {
    int rows, cols;
    double g0, g1, g3, g5;                   // geo_t without its rotation terms (both 0)
    double x0, x1, ylo, yhi;                 // centres of the first and last cells: interp's checkbounds
    double min_x, max_x, min_y, max_y;       // outer edges: is_inbounds
    int has_band;                            // the band has a no-data value (a NaN one masks nothing: NaN == NaN is false)
    double band_ndata;
};

template <typename T>
__device__ __forceinline__ bool rv_cell(const T *__restrict__ data, const RvGrid &g, int yi, int xi, double *v)
{
    // interp's datain[yi, xi] on the flipped copy; false: masked.  0 <= yi < rows and 0 <= xi < cols by the clips
    *v = (double)data[(int64_t)(g.rows - 1 - yi) * g.cols + xi];
    return !(g.has_band && *v == g.band_ndata);
}

// abs(int(f)) clipped to 0 .. n - 1 (get_row_col with check_bounds=False); an f beyond int64 clips as its abs does
__device__ __forceinline__ int rv_offset(double f, int n)
{
    if (!(fabs(f) < 2147483648.0)) return n - 1;
    int64_t c = (int64_t)f;
    if (c < 0) c = -c;
    return c >= n ? n - 1 : (int)c;
}

__device__ __forceinline__ double rv_grt_circle_dist(double lon1, double lat1, double lon2, double lat2)
{
    const double lat1r = lat1 * RV_RADIAN, lat2r = lat2 * RV_RADIAN, lon1r = lon1 * RV_RADIAN, lon2r = lon2 * RV_RADIAN;
    const double dlat = lat1r - lat2r, dlon = lon1r - lon2r;
    const double s1 = sin(dlat / 2.0), s2 = sin(dlon / 2.0);
    const double ca = 2.0 * asin(sqrt(s1 * s1 + cos(lat1r) * cos(lat2r) * (s2 * s2)));
    return RV_EARTH_KM * ca;
}

// get_coord(row, col) with the rotation terms 0 (their products are the +0.0 the reference adds)
__device__ __forceinline__ double rv_x(const RvGrid &g, int col) { return (g.g0 + (double)col * g.g1 + 0.0) + g.g1 / 2.0; }
__device__ __forceinline__ double rv_y(const RvGrid &g, int row) { return (g.g3 + 0.0 + (double)row * g.g5) + g.g5 / 2.0; }

__device__ __forceinline__ bool rv_less(double d, int s, double bd, int bs) { return d < bd || (d == bd && s < bs); }

}  // namespace

template <typename T>
__global__ __launch_bounds__(RV_THREADS) void k_rv_sample(const T *__restrict__ data, RvGrid g, int64_t nstn,
                                                          const double *__restrict__ qlon, const double *__restrict__ qlat,
                                                          int method, int revert_nn, int force, double ndata,
                                                          double *__restrict__ val, int32_t *__restrict__ status,
                                                          int32_t *__restrict__ row, int32_t *__restrict__ col)
{
    const int64_t i = (int64_t)blockIdx.x * RV_THREADS + threadIdx.x;
    if (i >= nstn) return;
    const double lon = qlon[i], lat = qlat[i];
    const bool outside = (lon < g.x0) || (lon > g.x1) || (lat < g.ylo) || (lat > g.yhi);
    double xc = (double)(g.cols - 1) * (lon - g.x0) / (g.x1 - g.x0);
    double yc = (double)(g.rows - 1) * (lat - g.ylo) / (g.yhi - g.ylo);
    xc = fmin(fmax(xc, 0.0), (double)(g.cols - 1));
    yc = fmin(fmax(yc, 0.0), (double)(g.rows - 1));
    const int xn = (int)rint(xc), yn = (int)rint(yc);            // np.around: half to even
    double v = 0.0;
    bool have = false;
    int st = TWXRV_OK;
    if (!outside) {
        if (method == 1) {
            const int xi = (int)xc, yi = (int)yc;
            const int xip = min(xi + 1, g.cols - 1), yip = min(yi + 1, g.rows - 1);
            const double dx = xc - (double)(float)xi, dy = yc - (double)(float)yi;
            double a, b, c, d;
            const bool ma = rv_cell(data, g, yi, xi, &a), mb = rv_cell(data, g, yip, xip, &b);
            const bool mc = rv_cell(data, g, yip, xi, &c), md = rv_cell(data, g, yi, xip, &d);
            if (ma && mb && mc && md) {
                v = (1. - dx) * (1. - dy) * a + dx * dy * b + (1. - dx) * dy * c + dx * (1. - dy) * d;
                have = true;
            }
        } else {
            have = rv_cell(data, g, yn, xn, &v);
        }
    }
    if (!have) {
        const bool inb = lon >= g.min_x && lon <= g.max_x && lat >= g.min_y && lat <= g.max_y;
        if ((inb && (method == 0 || revert_nn)) || force) {      // checkbounds=False, order=0: the clipped nearest cell
            have = rv_cell(data, g, yn, xn, &v);
            if (have) st = TWXRV_NEAREST;
        }
    }
    if (!have) {
        st = force ? TWXRV_NEEDS_FORCE : TWXRV_NODATA;
        v = ndata;
    }
    val[i] = v;
    status[i] = st;
    row[i] = rv_offset((lat - g.g3) / g.g5, g.rows);
    col[i] = rv_offset((lon - g.g0) / g.g1, g.cols);
}

// the cell of slot s of ring r around (y, x), and whether the reference's tests let it be a candidate
__device__ __forceinline__ bool rv_slot(const RvGrid &g, int y, int x, int r, int s, int *rr, int *cc)
{
    const int lcol = x - r, rcol = x + r, trow = y - r, brow = y + r;
    if (s < 2 * r + 1) { *rr = trow; *cc = lcol + s; }
    else if (s < 4 * r + 2) { *rr = trow + (s - (2 * r + 1)); *cc = lcol; }
    else if (s < 6 * r + 2) { *rr = brow; *cc = rcol - (s - (4 * r + 2)); }
    else { *rr = brow - (s - (6 * r + 2)); *cc = rcol; }
    return *rr > 0 && *rr < g.rows && *cc > 0 && *cc < g.cols;   // the reference's strict > 0: never row 0 or column 0
}

template <typename T>
__global__ __launch_bounds__(64) void k_rv_ring(const T *__restrict__ data, RvGrid g, double ndata, int rmax,
                                                const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                double *__restrict__ val, double *__restrict__ dist,
                                                int32_t *__restrict__ ring, int32_t *__restrict__ winner,
                                                double *__restrict__ dist2, int32_t *__restrict__ status)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int y = row[p], x = col[p];                            // 0 <= y < rows, 0 <= x < cols (checked by the entry)
    const double pt_lat = rv_y(g, y), pt_lon = rv_x(g, x);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double bd = inf;
    int bs = RV_NO_SLOT, r = 1;
    for (; r <= rmax; ++r) {
        const int nslots = 8 * r + 2;
        for (int s = lane; s < nslots; s += 64) {
            int rr, cc;
            if (!rv_slot(g, y, x, r, s, &rr, &cc)) continue;
            if ((double)data[(int64_t)rr * g.cols + cc] == ndata) continue;
            const double d = rv_grt_circle_dist(pt_lon, pt_lat, rv_x(g, cc), rv_y(g, rr));
            if (rv_less(d, s, bd, bs)) { bd = d; bs = s; }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const double od = __shfl_xor(bd, m, 64);
            const int os = __shfl_xor(bs, m, 64);
            if (rv_less(od, os, bd, bs)) { bd = od; bs = os; }
        }
        if (bs != RV_NO_SLOT) break;                             // uniform: every lane holds the same minimum
    }
    if (bs == RV_NO_SLOT) {
        if (lane == 0) {
            val[p] = ndata; dist[p] = inf; ring[p] = 0; winner[p] = -1; dist2[p] = inf;
            status[p] = TWXRV_NO_DATA_ANYWHERE;
        }
        return;
    }
    int wr, wc;
    (void)rv_slot(g, y, x, r, bs, &wr, &wc);
    double d2 = inf;                                             // the nearest data cell of the ring that is another cell
    const int nslots = 8 * r + 2;
    for (int s = lane; s < nslots; s += 64) {
        int rr, cc;
        if (!rv_slot(g, y, x, r, s, &rr, &cc)) continue;
        if (rr == wr && cc == wc) continue;
        if ((double)data[(int64_t)rr * g.cols + cc] == ndata) continue;
        const double d = rv_grt_circle_dist(pt_lon, pt_lat, rv_x(g, cc), rv_y(g, rr));
        if (d < d2) d2 = d;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) d2 = fmin(d2, __shfl_xor(d2, m, 64));
    if (lane == 0) {
        val[p] = (double)data[(int64_t)wr * g.cols + wc];
        dist[p] = bd; ring[p] = r; winner[p] = bs; dist2[p] = d2;
        status[p] = TWXRV_OK;
    }
}

__global__ __launch_bounds__(RV_THREADS) void k_rv_dup(int n, const double *__restrict__ lon, const double *__restrict__ lat,
                                                       int32_t *__restrict__ cls, int32_t *__restrict__ size)
{
    __shared__ double t_lon[RV_THREADS], t_lat[RV_THREADS];
    const int k = threadIdx.x, i = blockIdx.x * RV_THREADS + k;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double my_lon = i < n ? lon[i] * RV_RADIAN : nan, my_lat = i < n ? lat[i] * RV_RADIAN : nan;
    int first = RV_NO_SLOT, cnt = 0;
    for (int j0 = 0; j0 < n; j0 += RV_THREADS) {
        const int j = j0 + k;
        __syncthreads();                                         // the tile before has been read
        t_lon[k] = j < n ? lon[j] * RV_RADIAN : nan;
        t_lat[k] = j < n ? lat[j] * RV_RADIAN : nan;
        __syncthreads();
        const int m = n - j0 < RV_THREADS ? n - j0 : RV_THREADS;
        for (int q = 0; q < m; ++q) {                            // every lane reads the same word: a broadcast
            if (t_lat[q] == my_lat && t_lon[q] == my_lon) {
                ++cnt;
                if (j0 + q < first) first = j0 + q;
            }
        }
    }
    if (i < n) {
        cls[i] = cnt > 0 ? first : i;                            // a NaN coordinate equals nothing, itself included
        size[i] = cnt > 0 ? cnt : 1;
    }
}

// KIND 0: the sum of an int8 column without the days that equal fill (a NaN fill: every day counts); KIND 1: the days of a
// float32 column that are non-finite or equal to fill.  data: the batch's days, [nd][nstn]; cols null: column ci is station ci
template <int KIND>
__global__ __launch_bounds__(RV_THREADS) void k_rv_colcount(const void *__restrict__ data, int nd, int64_t nstn, float fill,
                                                            int64_t ncol, const int32_t *__restrict__ cols,
                                                            int32_t *__restrict__ out)
{
    __shared__ int lds[RV_THREADS];
    const int k = threadIdx.x, cl = k & (RV_COLS_PER_GROUP - 1), sl = k / RV_COLS_PER_GROUP;
    const int64_t ci = (int64_t)blockIdx.x * RV_COLS_PER_GROUP + cl;
    const int d0 = blockIdx.y * RV_DAYS_PER_GROUP;
    const int d1 = d0 + RV_DAYS_PER_GROUP < nd ? d0 + RV_DAYS_PER_GROUP : nd;
    const int ifill = fill == fill ? (int)fill : 256;            // 256: no int8 equals it
    int sum = 0;
    if (ci < ncol) {
        const int64_t c = cols ? (int64_t)cols[ci] : ci;         // 0 <= c < nstn (checked by the entry)
        for (int d = d0 + sl; d < d1; d += RV_SLICES) {
            if (KIND == 0) {
                const int v = (int)((const int8_t *)data)[(int64_t)d * nstn + c];
                if (v != ifill) sum += v;
            } else {
                const float v = ((const float *)data)[(int64_t)d * nstn + c];
                if (!(fabsf(v) <= RV_FLT_MAX) || v == fill) ++sum;
            }
        }
    }
    lds[k] = sum;
    __syncthreads();
    if (sl == 0 && ci < ncol) {
#pragma unroll
        for (int s = 1; s < RV_SLICES; ++s) sum += lds[s * RV_COLS_PER_GROUP + cl];
        if (sum != 0) atomicAdd(&out[ci], sum);
    }
}

namespace {

// the grid of a north-up geographic raster; a message if it is refused
const char *rv_grid(int64_t rows, int64_t cols, const double *geo_t, int has_band, double band_ndata, RvGrid *g)
{
    if (rows < 2 || cols < 2) return "the raster must be at least 2 x 2 (interp needs two cell centres on each axis)";
    if (rows > TWXRV_MAX_EXTENT || cols > TWXRV_MAX_EXTENT) return "the raster has more rows or columns than TWXRV_MAX_EXTENT";
    if (!geo_t) return "null buffer";
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(geo_t[k])) return "geo_t must be finite";
    if (geo_t[2] != 0.0 || geo_t[4] != 0.0) return "a rotated raster is refused (geo_t[2] and geo_t[4] must be 0)";
    if (!(geo_t[1] > 0.0) || !(geo_t[5] < 0.0)) return "the raster must be north-up (geo_t[1] > 0, geo_t[5] < 0)";
    g->rows = (int)rows; g->cols = (int)cols;
    g->g0 = geo_t[0]; g->g1 = geo_t[1]; g->g3 = geo_t[3]; g->g5 = geo_t[5];
    // get_coord_grid_1d: ulX, urX = get_coord(0, cols - 1)[1], ulY, llY = get_coord(rows - 1, 0)[0]; linspace keeps both ends
    g->x0 = geo_t[0] + geo_t[1] / 2.0;
    g->x1 = (geo_t[0] + (double)(cols - 1) * geo_t[1] + 0.0) + geo_t[1] / 2.0;
    g->yhi = geo_t[3] + geo_t[5] / 2.0;
    g->ylo = (geo_t[3] + 0.0 + (double)(rows - 1) * geo_t[5]) + geo_t[5] / 2.0;
    g->min_x = geo_t[0];
    g->max_x = g->min_x + (double)cols * geo_t[1];
    g->max_y = geo_t[3];
    g->min_y = g->max_y - ((double)(-rows) * geo_t[5]);
    if (!(g->x1 > g->x0) || !(g->yhi > g->ylo)) return "the cell centres do not ascend (a cell size below the coordinates' precision)";
    g->has_band = has_band ? 1 : 0;
    g->band_ndata = band_ndata;
    return nullptr;
}

}  // namespace

extern "C" int twxrv_sample(int device, int64_t rows, int64_t cols, int32_t dtype, const void *data, const double *geo_t,
                            int32_t has_band_ndata, double band_ndata, double ndata, int64_t nstn, const double *lon,
                            const double *lat, int32_t extract_method, int32_t revert_nn, int32_t force_data_value,
                            double *value, int32_t *status, int32_t *row, int32_t *col, float *kernel_ms, char *errbuf,
                            int errlen)
{
    const char *fn = "twxrv_sample";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    RvGrid g;
    if (const char *why = rv_grid(rows, cols, geo_t, has_band_ndata, band_ndata, &g)) {
        snprintf(msg, sizeof msg, "%s: %s", fn, why);
        return qa_fail(errbuf, errlen, msg);
    }
    if (dtype != TWXRV_F32 && dtype != TWXRV_F64) {
        snprintf(msg, sizeof msg, "%s: dtype must be TWXRV_F32 or TWXRV_F64", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (extract_method != 0 && extract_method != 1) {
        snprintf(msg, sizeof msg, "%s: extract_method must be 0 (nearest) or 1 (bilinear)", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (nstn < 1 || nstn > INT32_MAX / 2) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nstn <= %d", fn, INT32_MAX / 2);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!data || !lon || !lat || !value || !status || !row || !col) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t i = 0; i < nstn; ++i) {
        if (!std::isfinite(lon[i]) || !std::isfinite(lat[i])) {
            snprintf(msg, sizeof msg, "%s: station %lld has a non-finite coordinate", fn, (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const size_t NC = (size_t)rows * (size_t)cols, NS = (size_t)nstn, esz = dtype == TWXRV_F32 ? 4 : 8;

    QACHK(hipSetDevice(device));
    QaPool bufs;
    void *d_data;
    double *d_lon, *d_lat, *d_val;
    int32_t *d_st, *d_row, *d_col;
    float ms[TWXRV_NTIMES] = {0.0f, 0.0f, 0.0f};
    const auto t_up = std::chrono::steady_clock::now();
    QACHK(bufs.get(&d_data, NC * esz));
    QAALLOC(bufs, d_lon, double, NS); QAALLOC(bufs, d_lat, double, NS); QAALLOC(bufs, d_val, double, NS);
    QAALLOC(bufs, d_st, int32_t, NS); QAALLOC(bufs, d_row, int32_t, NS); QAALLOC(bufs, d_col, int32_t, NS);
    QACHK(hipMemcpy(d_data, data, NC * esz, hipMemcpyHostToDevice));
    QAUP(d_lon, lon, double, NS); QAUP(d_lat, lat, double, NS);
    QaTimer tm;
    if (kernel_ms) { QACHK(tm.init()); QACHK(hipDeviceSynchronize()); ms[1] = qa_since(t_up); QACHK(tm.start()); }
    const dim3 grid((unsigned)((NS + RV_THREADS - 1) / RV_THREADS)), block(RV_THREADS);
    if (dtype == TWXRV_F32)
        hipLaunchKernelGGL(k_rv_sample<float>, grid, block, 0, nullptr, (const float *)d_data, g, nstn, (const double *)d_lon,
                           (const double *)d_lat, (int)extract_method, (int)revert_nn, (int)force_data_value, ndata, d_val,
                           d_st, d_row, d_col);
    else
        hipLaunchKernelGGL(k_rv_sample<double>, grid, block, 0, nullptr, (const double *)d_data, g, nstn,
                           (const double *)d_lon, (const double *)d_lat, (int)extract_method, (int)revert_nn,
                           (int)force_data_value, ndata, d_val, d_st, d_row, d_col);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(value, d_val, double, NS); QADOWN(status, d_st, int32_t, NS);
    QADOWN(row, d_row, int32_t, NS); QADOWN(col, d_col, int32_t, NS);
    ms[2] = qa_since(t_down);
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxrv_nearest_data(int device, int64_t rows, int64_t cols, int32_t dtype, const void *data,
                                  const double *geo_t, double ndata, int64_t npts, const int32_t *row, const int32_t *col,
                                  double *value, double *dist, int32_t *ring, int32_t *winner, double *runner_up,
                                  int32_t *status, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxrv_nearest_data";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    RvGrid g;
    if (const char *why = rv_grid(rows, cols, geo_t, 0, 0.0, &g)) {
        snprintf(msg, sizeof msg, "%s: %s", fn, why);
        return qa_fail(errbuf, errlen, msg);
    }
    if (dtype != TWXRV_F32 && dtype != TWXRV_F64) {
        snprintf(msg, sizeof msg, "%s: dtype must be TWXRV_F32 or TWXRV_F64", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (npts < 1 || npts > INT32_MAX / 2) {
        snprintf(msg, sizeof msg, "%s: need 1 <= npts <= %d", fn, INT32_MAX / 2);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!data || !row || !col || !value || !dist || !ring || !winner || !runner_up || !status) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    for (int64_t i = 0; i < npts; ++i) {
        if (row[i] < 0 || row[i] >= rows || col[i] < 0 || col[i] >= cols) {
            snprintf(msg, sizeof msg, "%s: point %lld starts outside the raster", fn, (long long)i);
            return qa_fail(errbuf, errlen, msg);
        }
    }
    const size_t NC = (size_t)rows * (size_t)cols, NP = (size_t)npts, esz = dtype == TWXRV_F32 ? 4 : 8;
    const int rmax = (int)(rows > cols ? rows : cols);

    QACHK(hipSetDevice(device));
    QaPool bufs;
    void *d_data;
    double *d_val, *d_dist, *d_d2;
    int32_t *d_row, *d_col, *d_ring, *d_win, *d_st;
    float ms[TWXRV_NTIMES] = {0.0f, 0.0f, 0.0f};
    const auto t_up = std::chrono::steady_clock::now();
    QACHK(bufs.get(&d_data, NC * esz));
    QAALLOC(bufs, d_val, double, NP); QAALLOC(bufs, d_dist, double, NP); QAALLOC(bufs, d_d2, double, NP);
    QAALLOC(bufs, d_row, int32_t, NP); QAALLOC(bufs, d_col, int32_t, NP); QAALLOC(bufs, d_ring, int32_t, NP);
    QAALLOC(bufs, d_win, int32_t, NP); QAALLOC(bufs, d_st, int32_t, NP);
    QACHK(hipMemcpy(d_data, data, NC * esz, hipMemcpyHostToDevice));
    QAUP(d_row, row, int32_t, NP); QAUP(d_col, col, int32_t, NP);
    QaTimer tm;
    if (kernel_ms) { QACHK(tm.init()); QACHK(hipDeviceSynchronize()); ms[1] = qa_since(t_up); QACHK(tm.start()); }
    if (dtype == TWXRV_F32)
        hipLaunchKernelGGL(k_rv_ring<float>, dim3((unsigned)NP), dim3(64), 0, nullptr, (const float *)d_data, g, ndata, rmax,
                           (const int32_t *)d_row, (const int32_t *)d_col, d_val, d_dist, d_ring, d_win, d_d2, d_st);
    else
        hipLaunchKernelGGL(k_rv_ring<double>, dim3((unsigned)NP), dim3(64), 0, nullptr, (const double *)d_data, g, ndata, rmax,
                           (const int32_t *)d_row, (const int32_t *)d_col, d_val, d_dist, d_ring, d_win, d_d2, d_st);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(value, d_val, double, NP); QADOWN(dist, d_dist, double, NP); QADOWN(runner_up, d_d2, double, NP);
    QADOWN(ring, d_ring, int32_t, NP); QADOWN(winner, d_win, int32_t, NP); QADOWN(status, d_st, int32_t, NP);
    ms[2] = qa_since(t_down);
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxrv_dup_classes(int device, int64_t nstn, const double *lon, const double *lat, int32_t *cls,
                                 int32_t *size, float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxrv_dup_classes";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (nstn < 1 || nstn > TWXRV_MAX_DUP_STNS) {
        snprintf(msg, sizeof msg, "%s: need 1 <= nstn <= %d", fn, TWXRV_MAX_DUP_STNS);
        return qa_fail(errbuf, errlen, msg);
    }
    if (!lon || !lat || !cls || !size) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    const size_t NS = (size_t)nstn;
    QACHK(hipSetDevice(device));
    QaPool bufs;
    double *d_lon, *d_lat;
    int32_t *d_cls, *d_size;
    float ms[TWXRV_NTIMES] = {0.0f, 0.0f, 0.0f};
    const auto t_up = std::chrono::steady_clock::now();
    QAALLOC(bufs, d_lon, double, NS); QAALLOC(bufs, d_lat, double, NS);
    QAALLOC(bufs, d_cls, int32_t, NS); QAALLOC(bufs, d_size, int32_t, NS);
    QAUP(d_lon, lon, double, NS); QAUP(d_lat, lat, double, NS);
    QaTimer tm;
    if (kernel_ms) { QACHK(tm.init()); QACHK(hipDeviceSynchronize()); ms[1] = qa_since(t_up); QACHK(tm.start()); }
    hipLaunchKernelGGL(k_rv_dup, dim3((unsigned)((NS + RV_THREADS - 1) / RV_THREADS)), dim3(RV_THREADS), 0, nullptr, (int)nstn,
                       (const double *)d_lon, (const double *)d_lat, d_cls, d_size);
    QACHK(hipGetLastError());
    if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(cls, d_cls, int32_t, NS); QADOWN(size, d_size, int32_t, NS);
    ms[2] = qa_since(t_down);
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}

extern "C" int twxrv_col_count(int device, int64_t ndays, int64_t nstn, int32_t kind, const void *data, float fill,
                               int64_t ncol, const int32_t *cols, int64_t workspace_bytes, int32_t *out, int32_t *counts,
                               float *kernel_ms, char *errbuf, int errlen)
{
    const char *fn = "twxrv_col_count";
    char msg[256];
    if (errbuf && errlen > 0) errbuf[0] = 0;
    if (counts) { counts[0] = 0; counts[1] = 0; }
    if (kernel_ms) memset(kernel_ms, 0, TWXRV_NTIMES * sizeof(float));
    if (ndays < 1 || ndays > TWXSC_MAX_DAYS || nstn < 1 || nstn > INT32_MAX / 2) {
        snprintf(msg, sizeof msg, "%s: need 1 <= ndays <= %d and 1 <= nstn <= %d", fn, TWXSC_MAX_DAYS, INT32_MAX / 2);
        return qa_fail(errbuf, errlen, msg);
    }
    if (kind != TWXRV_COUNT_I8_SUM && kind != TWXRV_COUNT_F32_MISSING) {
        snprintf(msg, sizeof msg, "%s: kind must be TWXRV_COUNT_I8_SUM or TWXRV_COUNT_F32_MISSING", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (ncol < 0 || ncol > INT32_MAX / 2 || (!cols && ncol != nstn)) {
        snprintf(msg, sizeof msg, "%s: need 0 <= ncol <= %d, and ncol = nstn without a column list", fn, INT32_MAX / 2);
        return qa_fail(errbuf, errlen, msg);
    }
    if (kind == TWXRV_COUNT_I8_SUM && fill == fill && !(fill >= -128.0f && fill <= 127.0f && fill == (float)(int)fill)) {
        snprintf(msg, sizeof msg, "%s: the fill of an int8 variable must be NaN (none) or an integer in -128 .. 127", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (ncol == 0) return 0;                                     // an empty list: nothing to count, no device work
    if (!data || !out) {
        snprintf(msg, sizeof msg, "%s: null buffer", fn);
        return qa_fail(errbuf, errlen, msg);
    }
    if (cols) {
        for (int64_t i = 0; i < ncol; ++i) {
            if (cols[i] < 0 || cols[i] >= nstn) {
                snprintf(msg, sizeof msg, "%s: column %lld of the list is outside 0 .. nstn - 1", fn, (long long)i);
                return qa_fail(errbuf, errlen, msg);
            }
        }
    }
    if (workspace_bytes <= 0) workspace_bytes = TWXSC_WORKSPACE_BYTES;
    const size_t esz = kind == TWXRV_COUNT_I8_SUM ? 1 : 4, NST = (size_t)nstn, NCOL = (size_t)ncol;
    int64_t per = workspace_bytes / (int64_t)(NST * esz);       // days of a batch: as many as fit the budget, at least one
    if (per < 1) per = 1;
    if (per > ndays) per = ndays;

    QACHK(hipSetDevice(device));
    QaPool bufs;
    void *w_data;
    int32_t *d_cols = nullptr, *d_out;
    float ms[TWXRV_NTIMES] = {0.0f, 0.0f, 0.0f};
    const auto t_alloc = std::chrono::steady_clock::now();
    QACHK(bufs.get(&w_data, (size_t)per * NST * esz));
    QAALLOC(bufs, d_out, int32_t, NCOL);
    QACHK(hipMemset(d_out, 0, NCOL * sizeof(int32_t)));
    if (cols) { QAALLOC(bufs, d_cols, int32_t, NCOL); QAUP(d_cols, cols, int32_t, NCOL); }
    QaTimer tm;
    if (kernel_ms) { QACHK(tm.init()); QACHK(hipDeviceSynchronize()); ms[1] = qa_since(t_alloc); }
    int nbatches = 0;
    for (int64_t first = 0; first < ndays; first += per) {       // runs of days that fit the budget
        const int64_t nd = ndays - first < per ? ndays - first : per;
        const auto t_up = std::chrono::steady_clock::now();
        QACHK(hipMemcpy(w_data, (const char *)data + (size_t)first * NST * esz, (size_t)nd * NST * esz, hipMemcpyHostToDevice));
        ++nbatches;
        if (kernel_ms) { QACHK(hipDeviceSynchronize()); ms[1] += qa_since(t_up); QACHK(tm.start()); }
        const dim3 grid((unsigned)((NCOL + RV_COLS_PER_GROUP - 1) / RV_COLS_PER_GROUP),
                        (unsigned)((nd + RV_DAYS_PER_GROUP - 1) / RV_DAYS_PER_GROUP));
        if (kind == TWXRV_COUNT_I8_SUM)
            hipLaunchKernelGGL(k_rv_colcount<0>, grid, dim3(RV_THREADS), 0, nullptr, (const void *)w_data, (int)nd, nstn, fill,
                               ncol, (const int32_t *)d_cols, d_out);
        else
            hipLaunchKernelGGL(k_rv_colcount<1>, grid, dim3(RV_THREADS), 0, nullptr, (const void *)w_data, (int)nd, nstn, fill,
                               ncol, (const int32_t *)d_cols, d_out);
        QACHK(hipGetLastError());
        if (kernel_ms) QACHK(tm.stop_add(&ms[0]));
        else QACHK(hipDeviceSynchronize());                      // the next batch overwrites the days
    }
    const auto t_down = std::chrono::steady_clock::now();
    QADOWN(out, d_out, int32_t, NCOL);
    ms[2] = qa_since(t_down);
    if (counts) { counts[0] = nbatches; counts[1] = nbatches; }
    if (kernel_ms) memcpy(kernel_ms, ms, sizeof ms);
    return 0;
}
