/*
 * twx_qa.h -- C ABI of libtwxqa.so: station quality checks that run before the
 * interpolation stages (gfx950).  A library of its own, next to libtwxhip.so:
 * nothing here touches the kriging / daily kernels or their context.
 *
 * Conventions (as include/twx.h)
 *   - every function returns 0 = ok or -1 = call-level failure (bad arguments,
 *     HIP errors); the message goes to errbuf (errlen bytes, NUL-terminated).
 *   - per-item failures are not call failures: they are reported in status[]
 *     with the TWX_CELL_* numbers of include/twx.h.
 *   - all buffers are host memory owned by the caller; a call is synchronous.
 */
#ifndef TWX_QA_H
#define TWX_QA_H
#include <stdint.h>

#include "twx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWXQA_NTARGET 13     /* 12 monthly normals + the annual one */
#define TWXQA_PT_STRIDE 29   /* doubles per left-out station: lon, lat, elev, lst[13], norm[13] */
#define TWXQA_MAX_K 159      /* largest neighbourhood (twx_knn's limit) */

/* per-(station, target) status */
#define TWXQA_OK TWX_CELL_OK                      /* err holds prediction - observation (NaN if the
                                                     left-out station's own predictor / normal is NaN) */
#define TWXQA_FEW_STATIONS TWX_CELL_FEW_STATIONS  /* passed through from knn_status */
#define TWXQA_SINGULAR TWX_CELL_NUMERIC           /* the WLS system has no Cholesky factorisation; err = NaN */

/*
 * Leave-one-out weighted least squares of XvalOutlier.run_xval_stn
 * (twx/interp/optimize.py:113-153): for left-out station p and target t
 * (months 1..12, then the annual mean), fit
 *     norm_t ~ 1 + lst_t + elevation + longitude + latitude
 * over the k neighbours idx[p][:] with WLS weights wgt[p][:] and return the
 * prediction at p minus p's own norm_t.  A neighbour with a non-finite predictor
 * or normal for target t is left out of that fit (patsy's missing='drop').
 *
 * nstn                      pool size (the good stations the neighbours index)
 * lon, lat, elev [nstn]     pool predictors
 * lst13, norm13  [13][nstn] pool monthly columns, row 12 = annual means
 * pt   [npts][29]           left-out stations (TWXQA_PT_STRIDE layout)
 * idx, wgt [npts][k]        neighbours (0 <= idx < nstn) and weights, as twx_knn gives them
 * knn_status [npts]         twx_knn's status: rows with a non-zero status are not fitted
 * err, status [npts][13]    outputs
 * kernel_ms (optional)      device time of the fit kernel
 */
int twxqa_outlier_wls(int device, int64_t nstn, const double *lon, const double *lat, const double *elev,
                      const double *lst13, const double *norm13, int64_t npts, const double *pt, int32_t k,
                      const int32_t *idx, const double *wgt, const int32_t *knn_status, double *err,
                      int32_t *status, float *kernel_ms, char *errbuf, int errlen);

#ifdef __cplusplus
}
#endif
#endif
