// devmath_probe.hip -- evaluates the kriging and variogram kernels' own device math (twx_uk.h, twx_vario.h) on arguments read
// from a file, for tests/test_gpu_devmath.py, which compares the results with high-precision references:
//
//   devmath_probe exp  N in out   in: N doubles x            out: 2N doubles: exp_neg_f64(x) with the table in global memory
//                                                              (twx_exp2_tab), then with the table staged in LDS (exp_tab_stage)
//   devmath_probe dist N in out   in: N x 8 doubles          out: 2N doubles: ellip_pair_f64, then ellip_pair_fast (widened)
//                                 (sin, cos of half lat, sin, cos of half lon) of both points, as twx_set_stations forms them;
//                                 cos(lat) is formed on the device from the half angles, as the kernels form it
//   devmath_probe vdist N in out  in: N x 8 doubles (as dist) out: 2N doubles: ellip_pair_vario (the semivariogram's pair distance,
//                                                              twx_vario.h), then ellip_pair_f64 on the same pair
//   devmath_probe vmath N in out  in: N doubles x            out: 2N doubles: rcp_nr1(x), then sqrt_nr(x) (twx_vario.h)
//
// Exit status 0 only if every HIP call succeeded and the output file was written in full.
#include "twx_vario.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHK(x)                                                                                          \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) {                                                                         \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));          \
            return 2;                                                                                   \
        }                                                                                               \
    } while (0)

__global__ __launch_bounds__(256) void k_exp(const double *x, int64_t n, double *out_g, double *out_l)
{
    __shared__ double s_tab[TWX_EXP_TAB_N];
    exp_tab_stage<256>(s_tab, threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    out_g[i] = exp_neg_f64(v, twx_exp2_tab);
    out_l[i] = exp_neg_f64(v, s_tab);
}

__global__ __launch_bounds__(256) void k_dist(const double *tg, int64_t n, double *out_f64, double *out_fast)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *q = tg + i * 8;
    const double a[5] = {q[0], q[1], q[2], q[3], fma(q[1], q[1], -(q[0] * q[0]))};
    const double b[5] = {q[4], q[5], q[6], q[7], fma(q[5], q[5], -(q[4] * q[4]))};
    out_f64[i] = ellip_pair_f64(a, b);
    out_fast[i] = (double)ellip_pair_fast(a[0], a[1], a[2], a[3], a[4], b[0], b[1], b[2], b[3], b[4]);
}

__global__ __launch_bounds__(256) void k_vdist(const double *tg, int64_t n, double *out_vario, double *out_f64)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *q = tg + i * 8;
    const double a[5] = {q[0], q[1], q[2], q[3], fma(q[1], q[1], -(q[0] * q[0]))};
    const double b[5] = {q[4], q[5], q[6], q[7], fma(q[5], q[5], -(q[4] * q[4]))};
    out_vario[i] = ellip_pair_vario(a, b);
    out_f64[i] = ellip_pair_f64(a, b);
}

__global__ __launch_bounds__(256) void k_vmath(const double *x, int64_t n, double *out_rcp, double *out_sqrt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    out_rcp[i] = rcp_nr1(v);
    out_sqrt[i] = sqrt_nr(v);
}

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s exp|dist|vdist|vmath N in out\n", argv[0]);
        return 1;
    }
    const bool is_exp = strcmp(argv[1], "exp") == 0, is_dist = strcmp(argv[1], "dist") == 0;
    const bool is_vdist = strcmp(argv[1], "vdist") == 0, is_vmath = strcmp(argv[1], "vmath") == 0;
    if (!is_exp && !is_dist && !is_vdist && !is_vmath) {
        fprintf(stderr, "unknown mode %s\n", argv[1]);
        return 1;
    }
    const int64_t n = atoll(argv[2]);
    if (n <= 0 || n > (int64_t)1 << 26) {
        fprintf(stderr, "bad N %s\n", argv[2]);
        return 1;
    }
    const size_t nin = (size_t)n * (is_exp || is_vmath ? 1 : 8), nout = (size_t)n * 2;
    std::vector<double> in(nin), out(nout);
    FILE *f = fopen(argv[3], "rb");
    if (!f || fread(in.data(), 8, nin, f) != nin) {
        fprintf(stderr, "cannot read %zu doubles from %s\n", nin, argv[3]);
        return 1;
    }
    fclose(f);
    double *d_in = nullptr, *d_out = nullptr;
    CHK(hipMalloc(&d_in, nin * 8));
    CHK(hipMalloc(&d_out, nout * 8));
    CHK(hipMemcpy(d_in, in.data(), nin * 8, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((n + 255) / 256));
    if (is_exp)
        hipLaunchKernelGGL(k_exp, grid, dim3(256), 0, nullptr, d_in, n, d_out, d_out + n);
    else if (is_vdist)
        hipLaunchKernelGGL(k_vdist, grid, dim3(256), 0, nullptr, d_in, n, d_out, d_out + n);
    else if (is_vmath)
        hipLaunchKernelGGL(k_vmath, grid, dim3(256), 0, nullptr, d_in, n, d_out, d_out + n);
    else
        hipLaunchKernelGGL(k_dist, grid, dim3(256), 0, nullptr, d_in, n, d_out, d_out + n);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(out.data(), d_out, nout * 8, hipMemcpyDeviceToHost));
    CHK(hipFree(d_in));
    CHK(hipFree(d_out));
    f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), 8, nout, f) != nout || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[4]);
        return 1;
    }
    return 0;
}
