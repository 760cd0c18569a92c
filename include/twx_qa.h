/*
 * twx_qa.h -- C ABI of libtwxqa.so: station quality checks that run before the
 * interpolation stages (gfx950).  A library of its own, next to libtwxhip.so:
 * nothing here touches the kriging / daily kernels or their context.
 *
 * Conventions (as include/twx.h)
 *   - every function returns 0 = ok or -1 = call-level failure (bad arguments,
 *     HIP errors); the message goes to errbuf (errlen bytes, NUL-terminated).
 *   - per-item failures are not call failures: they are reported in status[]
 *     with the TWX_CELL_* numbers of include/twx.h where one applies (the
 *     spatial check adds two of its own, TWXQA_SP_FEW_DAYS / _FEW_VALID).
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

/* ---- step08's spatial regression check (_qa_spatial_regress, twx/qa/qa_temp.py:688-738, 858-1015) ---- */
#define TWXQA_NGH_RADIUS_KM 75.0        /* NGH_RADIUS, qa_temp.py:66 */
#define TWXQA_MIN_DAYS_MTH_WINDOW 40    /* qa_temp.py:71 */
#define TWXQA_MIN_NGHS 3                /* qa_temp.py:72 */
#define TWXQA_MAX_NGHS 7                /* qa_temp.py:73 */
/* Largest radius neighbourhood a target may have.  A library limit without a reference counterpart: a wavefront keeps
 * the (weight, slope, intercept, column) of every valid neighbour in LDS, 34 bytes each; 256 of them leave room for 18
 * waves in the 160 KiB of a compute unit.  A target above it gets TWXQA_SP_NGH_CAP on all of its items, never a
 * truncated list. */
#define TWXQA_MAX_RADIUS_NGH 256

/* per-(target, variable, year-month) item status */
#define TWXQA_SP_OK TWX_CELL_OK                   /* checked (flags or none; r below 0.8 is ok and flags nothing) */
#define TWXQA_SP_FEW_NGHS TWX_CELL_FEW_STATIONS   /* fewer than 3 stations within 75 km of the target */
#define TWXQA_SP_DEGENERATE TWX_CELL_NUMERIC      /* see below */
#define TWXQA_SP_NGH_CAP TWX_CELL_CAND_OVERFLOW   /* more than TWXQA_MAX_RADIUS_NGH stations within 75 km */
#define TWXQA_SP_FEW_DAYS 16                      /* fewer than 40 finite target days in the window */
#define TWXQA_SP_FEW_VALID 17                     /* fewer than 3 neighbours with a model for this window */

/*
 * The number of (year, month) items of a day axis: the calendar months from that of ymd[0] to that of
 * ymd[ndays - 1]; -1 on bad arguments.  (A month of the first or last year outside that span holds no day of the
 * series.  Its window may still reach into the series -- one that ends on Feb 20 lies inside March's window of
 * Feb 14 to Apr 15 -- but flags go to a month's own days only, so such a month flags nothing in the reference either.)
 */
int twxqa_spatial_nmonths(int64_t ndays, const int32_t *ymd);

/*
 * For every target station, variable (0 = tmin, 1 = tmax) and (year, month): the window is the month plus 15 days on
 * either side; every station within 75 km (haversine, util_geo.py:24-40; the target left out by index; ascending
 * table order) whose finite days overlap the target's finite window days on >= 40 days, with more than one distinct
 * value on either side, gets an index-of-agreement weight (perf_metrics.py:59-62) and the model of
 * linregress(neighbour, target); each finite window day is estimated from the (up to) 7 heaviest neighbours that have
 * a finite value on that day of the series or the one before / after it (the one nearest the observation; the first
 * of previous, own, next on a tie), a day with fewer than 3 has no estimate; if Pearson's r of estimates against
 * observations over the window is >= 0.8, a day of the month is flagged where |obs - est| >= 8.0 and that residual
 * lies >= 4.0 population standard deviations from the mean window residual.
 * Arithmetic is fp64 on the float32 observations widened exactly (NaN = missing).
 *
 * Deviation from the reference: an item with fewer than two estimated window days, a zero standard deviation of
 * the window residuals or a non-finite r is TWXQA_SP_DEGENERATE and flags nothing.  The reference raises there
 * (pearsonr on one point; a division by zero under step08's np.seterr), which drops ALL of that station's QA, or
 * its result depends on the scipy version (r of a constant series).
 *
 * lon, lat [nstn]            finite
 * tmin, tmax [nstn][ndays]   station-major observations
 * ymd [ndays]                consecutive calendar days, YYYYMMDD
 * target_idx [ntarget]       0 <= index < nstn
 * flag_tmin, flag_tmax [ntarget][ndays]   out: 1 = flagged, 0 = not
 * est (optional) [ntarget][2][ndays]      out: the estimate of each day within its own month's item, NaN if none
 * item_r, item_nvalid, item_status (each optional) [ntarget][2][nmonths]   out: r (NaN if not computed), the number
 *                            of valid neighbours, TWXQA_SP_*
 * kernel_ms (optional) [2]   device time of the radius kernel (both passes) and of the item kernel
 * Call-level failures: non-consecutive days, an index out of range, a non-finite longitude / latitude.
 */
int twxqa_spatial_regress(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                          const float *tmin, const float *tmax, const int32_t *ymd, int64_t ntarget,
                          const int32_t *target_idx, uint8_t *flag_tmin, uint8_t *flag_tmax, double *est,
                          double *item_r, int32_t *item_nvalid, int32_t *item_status, float *kernel_ms,
                          char *errbuf, int errlen);

/* ---- the rest of step08's spatial stage (run_qa_spatial_only, qa_temp.py:218-258): day-of-year normals, the
 * corroboration check (_qa_spatial_corrob, :740-813, 1017-1082) and _qa_mega_inconsist (:815-840) ---- */
#define TWXQA_ANOMALY_CUTOFF 10.0       /* ANOMALY_CUTOFF, qa_temp.py:70 */
#define TWXQA_MIN_NORM_VALUES 100       /* MIN_NORM_VALUES, qa_temp.py:84 */
#define TWXQA_NORM_ROWS 731             /* the 365-row table (dates of 2003), then the 366-row table (dates of 2004) */
/* Most values a row of the normals may draw on: 15 calendar dates per year the series touches, so 136 years.  A
 * library limit without a reference counterpart: a workgroup of 4 waves sorts a row's values in LDS, 4 bytes each plus
 * 2 KiB of reduction scratch; at 2048 values that is 10 KiB, and the 8 workgroups that fill the 32 wave slots of a
 * compute unit take 80 KiB of its 160 KiB.  4096 values (18 KiB, 144 KiB for 8 workgroups) would leave a compute
 * unit no LDS to share with any other kernel; 8192 would halve the waves in flight.  A series that touches more
 * years fails the call with a message, never a truncated window. */
#define TWXQA_MAX_NORM_VALUES 2048

/*
 * The two day-of-year tables of each series (_get_norms_md_masks / _build_mean_norms / _biweight_mean,
 * qa_temp.py:1111-1130, 1171-1184, 1215-1228).  Row x of the 365-row table takes every finite day of the series whose
 * (month, day) is one of the 15 dates from 7 days before to 7 days after day x of 2003 (windows wrap the year end;
 * Feb 29 is in none of them); the 366-row table likewise with the dates of 2004.  Fewer than 100 values: NaN.  Else
 * M = median (the mean of the two middle values of an even count), MAD = median |X - M|; MAD == 0: the plain mean;
 * else u = (X - M) / (7.5 MAD), |u| >= 1 set to 1, row = M + sum (X - M)(1 - u^2)^2 / sum (1 - u^2)^2.  Both medians
 * are exact.  fp64 on float32 values widened exactly; the sums run over the sorted values.
 *
 * series [nseries][ndays]   float32, NaN (or any non-finite value) = missing
 * ymd [ndays]               consecutive calendar days, YYYYMMDD
 * norms [nseries][731]      out: rows 0..364 the 365-row table, rows 365..730 the 366-row table
 * kernel_ms (optional) [1]  device time of the kernel
 * Call-level failures: non-consecutive days; a series that touches more than TWXQA_MAX_NORM_VALUES / 15 years.
 */
int twxqa_doy_norms(int device, int64_t nseries, int64_t ndays, const float *series, const int32_t *ymd,
                    double *norms, float *kernel_ms, char *errbuf, int errlen);

/*
 * run_qa_spatial_only for all targets in one call: the regression check (twxqa_spatial_regress, above) -> its flagged
 * days removed from the target -> normals -> the corroboration check -> its flagged days removed -> the
 * mega-inconsistency check.
 *
 * Corroboration: the neighbours are the stations within 75 km, the target left out by index, in ascending distance
 * (equal distances in table order); fewer than 3: nothing is flagged.  The normals of a neighbour come from the pool's
 * observations as they are, those of the target from its series without the regression check's days.  For each
 * variable and day x except the first and last of the series: anom = |obs[x] - target normal of x's day of year, table
 * by x's own year|; NaN: no flag.  The day is tested if at least 3 neighbours have a finite observation on each of
 * x - 1, x, x + 1; per such day the first 7 neighbours with a finite |obs - own normal| (row and table from that
 * day's own date) give up to 21 anomalies, and x is flagged if every one differs from anom by >= 10.0 -- also if
 * there is none (no neighbour has a normal: the reference's empty-list case, kept).
 * Mega-inconsistency, per calendar month over all years on the series after both removals: finite Tmin above the
 * month's highest Tmax and finite Tmax below the month's lowest Tmin; a month empty on either side is skipped.
 *
 * Inputs as twxqa_spatial_regress.
 * flag_tmin, flag_tmax [ntarget][ndays]  out: the reference's numbers: 1 ok, 2 missing (NaN), 16 regression,
 *                            17 corroboration, 18 mega-inconsistency; a later check writes only where the flag is 1
 * norms (optional) [ntarget][2][731]     out: the target tables (variable 0 = tmin), 365 rows then 366 rows
 * status (optional) [ntarget]            out: TWXQA_SP_OK, TWXQA_SP_FEW_NGHS (fewer than 3 neighbours: no spatial
 *                            flags) or TWXQA_SP_NGH_CAP (more than TWXQA_MAX_RADIUS_NGH: no spatial flags either);
 *                            the mega-inconsistency check runs for every target
 * kernel_ms (optional) [6]   device time: regression radius passes, regression items, distance-ordered radius lists,
 *                            normals, corroboration, mega-inconsistency + final flags
 * Call-level failures: those of twxqa_spatial_regress and of twxqa_doy_norms.
 */
int twxqa_spatial_only(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat,
                       const float *tmin, const float *tmax, const int32_t *ymd, int64_t ntarget,
                       const int32_t *target_idx, uint8_t *flag_tmin, uint8_t *flag_tmax, double *norms,
                       int32_t *status, float *kernel_ms, char *errbuf, int errlen);

/* ---- step08's first run: the non-spatial checks (run_qa_non_spatial, qa_temp.py:172-216) ---- */
/* Most values the gap check may sort for one calendar month: 31 per year the series touches, so 132 years.  A library
 * limit without a reference counterpart: a workgroup of 4 waves sorts the month's values in LDS, 4 bytes each; at 4096
 * values that is 16 KiB, and the 8 workgroups that fill the 32 wave slots of a compute unit take 128 KiB of its
 * 160 KiB.  8192 values (32 KiB) would leave room for 5 workgroups.  The day-of-year rows of the outlier check are
 * bounded by TWXQA_MAX_NORM_VALUES (136 years), so this cap is the one a long axis meets first.  A series that touches
 * more years fails the call with a message, never a truncated month. */
#define TWXQA_MAX_GAP_VALUES 4096
#define TWXQA_NS_NKERNELS 8             /* kernel groups timed by the entry below */

/*
 * run_qa_non_spatial for nstn stations in one call; every station is checked on its own.  The checks run in the
 * reference's order, each on the series without the observations every earlier check flagged; a check writes its number
 * only where the flag is still 1; all decisions of one check are taken on the same snapshot.  In execution order:
 *    2 missing: NaN.   3 naught: both variables round to -17.8 at one decimal (rintf(v * 10) / 10 in float32), or both
 *   are 0.0.   4 duplicate year: per variable, two years of the axis with a value each whose first min(len, len) days
 *   on the axis are all ==, by position.   6 duplicate months of one year, by position over the shorter; the month
 *   NUMBER equal to (distinct months on the axis) - 1 is never the first of a pair (the reference's loop, kept: on a
 *   12-month axis November and December are never compared).   5 the same calendar month of two years, by position.
 *    7 a (year, month) with >= 10 days of Tmin == Tmax: the whole month, both variables.   8 below -89.4 or above 57.7
 *   (float32).   9 a run of >= 20 equal values among the non-missing ones, ended by a different value (a run that
 *   reaches the end of the series is not flagged: kept).   10 gap: per calendar month over all years, the sorted values,
 *   numpy's float32 median; walking up from the median the first step >= 10.0 (float32 subtraction) gives a bound and
 *   every value of the month >= it is flagged, likewise downwards; a step across the median of an even count is never
 *   looked at (kept).   15 outlier: |(v - mean) / std| >= 6.0 against the day-of-year row of the day's own year (365- or
 *   366-row table, windows and minimum count of the normals above); a row holds the biweight mean and the biweight
 *   standard deviation sqrt(n sum (X - M)^2 (1 - u^2)^4) / |sum (1 - u^2)(1 - 5 u^2)|, or the plain mean and std(ddof = 1)
 *   when MAD == 0; fp64 on the values widened exactly, both medians exact.   11 Tmin > Tmax: both.   13 spike / dip:
 *   |cur - prev| >= 25 and |cur - next| >= 25 (float32) on adjacent days of the axis.   12 lagged range: day x with the
 *   window x - 1 .. x + 1 clipped to the axis, a value of each variable somewhere in it: Tmax[x] >= warmest Tmin of the
 *   window + 40 flags Tmax[x] and the whole window of Tmin; Tmin[x] <= coldest Tmax - 40 flags Tmin[x] and the whole
 *   window of Tmax; compared in fp64 on the widened values.   18 mega-inconsistency as in the spatial stage above.
 *
 * Deviation from the reference: a row of >= 100 identical values has standard deviation 0; here it flags nothing (0 / 0);
 * the reference divides by zero, which under step08's np.seterr drops all of that station's QA.
 *
 * tmin, tmax [nstn][ndays]   station-major float32, NaN = missing; not modified
 * ymd [ndays]                consecutive calendar days, YYYYMMDD; need not start or end at a year boundary
 * flag_tmin, flag_tmax [nstn][ndays]   out: the reference's numbers 1 .. 13, 15, 18
 * norms (optional) [nstn][2][731][2]   out: mean and standard deviation of each row as the outlier check used them
 *                            (variable 0 = tmin; the 365-row table, then the 366-row table; NaN: fewer than 100 values)
 * kernel_ms (optional) [TWXQA_NS_NKERNELS]   device time: missing + naught, duplicates + impossible values, streaks,
 *                            gaps, day-of-year rows, outliers + Tmin > Tmax, spike + lagged range, mega-inconsistency
 * Call-level failures: non-consecutive days; a series that touches more than TWXQA_MAX_GAP_VALUES / 31 years (or more
 * than TWXQA_MAX_NORM_VALUES / 15): the message names the macro.
 */
int twxqa_non_spatial(int device, int64_t nstn, int64_t ndays, const float *tmin, const float *tmax,
                      const int32_t *ymd, uint8_t *flag_tmin, uint8_t *flag_tmax, double *norms, float *kernel_ms,
                      char *errbuf, int errlen);

/* ---- the neighbour matrices of the infill family (step14 / step15 / step16): _InfillMatrix.__init__, the widening
 * loop of _InfillMatrix.infill and _shrink_matrix (twx/infill/infill_normals.py:52-237, 239-299, 324-343, 391-420) ---- */
#define TWXIF_RING_KM 37.5              /* MAX_DISTANCE / 2: the width of every ring after the first (75 km) */
#define TWXIF_MIN_POR_OVERLAP (2.0 / 3.0)   /* MIN_POR_OVERLAP */
#define TWXIF_BESTNGH_MIN_IOA 0.7       /* infill_normals.py:184 */
#define TWXIF_MAX_COLS_NORM_IMPUTE 31   /* MAX_COLS_NORM_IMPUTE: the target's column and at most 30 stations */
#define TWXIF_MAX_GROUPS 12             /* day groups of one call (step14: the calendar months) */
#define TWXIF_MAX_MIN_NNGHS 16          /* largest min_daily_nnghs (the reference's default is 3) */
#define TWXIF_NKERNELS 4                /* kernel groups timed by the entry below */
#define TWXIF_NTIMES 6                  /* entries of kernel_ms: the kernel groups, then two host-clock figures */
/* The ring of a target and the ranked list of an item hold at most TWXQA_MAX_RADIUS_NGH (256) stations.  A library limit
 * without a reference counterpart: the item kernel keeps the ranked list (28 bytes per station), the ring with its pair
 * results (28 bytes) and the sorted rows (4 bytes) in LDS, plus 1 KiB of reduction scratch: 16 KiB per workgroup of 4
 * waves at 256, and the 8 workgroups that fill the 32 wave slots of a compute unit take 128 KiB of its 160 KiB; 512
 * would take 31 KiB and leave room for 5 workgroups.  An item above it gets TWXIF_NGH_CAP and an empty list, never a
 * truncated one. */

/* per-(target, group) item status */
#define TWXIF_OK TWX_CELL_OK                      /* every day of the item has min_daily_nnghs neighbour observations */
#define TWXIF_NUMERIC TWX_CELL_NUMERIC            /* a pair the reference would rank has a d1 denominator of 0 (it raises
                                                     under step14's np.seterr); the list is empty */
#define TWXIF_NGH_CAP TWX_CELL_CAND_OVERFLOW      /* a ring or the ranked list above TWXQA_MAX_RADIUS_NGH; the list is empty */
#define TWXIF_NO_TARGET_OBS 18                    /* the target has no finite day in the item (nthres_target_por == 0); the
                                                     reference takes the mean of an empty slice and loses the station */
#define TWXIF_UNSATISFIED 19                      /* no eligible station is left beyond max_dist and some day still has
                                                     fewer observations (the reference loops forever, :124-126); the ranked
                                                     list as far as it got, keep all 0, nnghs as the loop left it */

/*
 * For every target and day group g (an item; its days are those with group[day] == g):
 *   1. ring 1 is the eligible stations (the target left out by index) with haversine distance (util_geo.py:24-40, fp64)
 *      in [0, 75] km; an empty ring's outer radius grows by 37.5 km until it holds a station, and the grown radius is the
 *      item's max_dist.  Stations are taken in ascending distance, equal distances in table order.
 *   2. a ring station with nlap (its finite days of the item) >= nthres_all and nlap_stn (days finite in both series) >=
 *      nthres_target_por is ranked with ioa = d1(o = target, p = neighbour) over the overlap (perf_metrics.py:59-62).  In
 *      ring 1 only, a station that misses nthres_all but reaches nthres_target_por is the best-neighbour candidate if its
 *      ioa is strictly above every earlier candidate's (and 0); the last candidate is ranked only if no ranked station of
 *      the ring has a larger ioa and its ioa is >= 0.7.
 *   3. the ranked stations are ordered by ioa descending, over all rings taken so far (equal ioa: the larger distance
 *      first, then table order; the reference's order is undefined there).
 *   4. nnghs starts at min_daily_nnghs.  While fewer than nnghs stations are ranked, the next ring (max_dist,
 *      max_dist + 37.5] is taken (grown likewise); else while some day of the item has fewer than min_daily_nnghs finite
 *      values among the first nnghs ranked stations, nnghs grows by one.  nnghs is never reset.
 *   5. of the first nnghs ranked stations the first min_daily_nnghs are kept, a later one only if it has a finite value
 *      on a day with fewer than min_daily_nnghs finite values among the stations kept before it (_shrink_matrix).
 * fp64 on the float32 observations widened exactly; every sum runs in a fixed order: two calls give the same bytes.
 * Not done here: the reanalysis columns, the cut to TWXIF_MAX_COLS_NORM_IMPUTE columns (the caller's, on keep), em.norm.
 *
 * lon, lat [nstn]            finite
 * obs [nstn][ndays]          station-major float32 of one variable, NaN (any non-finite value) = missing
 * ymd [ndays]                consecutive calendar days, YYYYMMDD
 * eligible [nstn]            the reference's stns_mask: 0 = never a neighbour
 * target_idx [ntarget]       0 <= index < nstn
 * group [ndays]              -1 (day not used) or 0 .. ngroups - 1, ngroups <= TWXIF_MAX_GROUPS
 * nthres_all [ngroups], nthres_target_por [ntarget][ngroups]
 *                            np.round(2 / 3 * days of the item) and np.round(2 / 3 * finite target days of the item), the
 *                            caller's (infill_normals.py:110-115); nthres_target_por == 0 marks a target without a finite
 *                            day (round(2 / 3 n) >= 1 for n >= 1)
 * status, nnghs [ntarget][ngroups], max_dist [ntarget][ngroups]       out; for an item that did not end TWXIF_OK nnghs is
 *                            what the loop had reached and max_dist the last ring taken (NaN: none)
 * csr_off [ntarget * ngroups + 1]   out: the ranked list of item i is csr_off[i] .. csr_off[i + 1]
 * ngh_idx, ngh_ioa, ngh_dist, ngh_nlap, ngh_nlap_stn, keep [csr_cap]   out: pool row, ioa, distance, nlap, nlap_stn, and 1
 *                            where the station is among the first nnghs and survived the shrink (status TWXIF_OK only);
 *                            ntarget * ngroups * TWXQA_MAX_RADIUS_NGH entries always suffice, fewer fail the call if the
 *                            lists need more
 * nrounds (optional)         out: the rings the host ran (the largest number any item took, + 1 if some item ended
 *                            unsatisfied)
 * kernel_ms (optional) [TWXIF_NTIMES]   device time over all rounds: rings, pairs, items, the CSR gather; then host-clock
 *                            milliseconds of the allocations and copies to the device before the first round, and of
 *                            the copies back after the last (the gather kernel left out)
 * Failure order within a ring: the stations are scanned in ascending distance and the first that fails decides the item:
 * a zero d1 denominator at a station that would be ranked or weighed as a candidate (TWXIF_NUMERIC), or a station that
 * would be entry TWXQA_MAX_RADIUS_NGH + 1 of the list (TWXIF_NGH_CAP); at one station the denominator is looked at first.
 * A ring above the cap is TWXIF_NGH_CAP before any of its stations is looked at.
 * Call-level failures: non-consecutive days, an index out of range, a group value outside -1 .. ngroups - 1, a non-finite
 * longitude / latitude.
 */
int twxif_infill_matrix(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat, const float *obs,
                        const int32_t *ymd, const uint8_t *eligible, int64_t ntarget, const int32_t *target_idx,
                        int32_t ngroups, const int8_t *group, const int32_t *nthres_all,
                        const int32_t *nthres_target_por, int32_t min_daily_nnghs, int32_t *status, int32_t *nnghs,
                        double *max_dist, int64_t *csr_off, int64_t csr_cap, int32_t *ngh_idx, double *ngh_ioa,
                        double *ngh_dist, int32_t *ngh_nlap, int32_t *ngh_nlap_stn, uint8_t *keep, int32_t *nrounds,
                        float *kernel_ms, char *errbuf, int errlen);

/* ---- the mean / variance estimator of step14: infill_mu_sigma of twx/infill/rpy/norm_infill.R (prelim.norm, em.norm,
 * getparam.norm; the reference keeps mu[1] and sigma[1, 1]), restated from Schafer (1997, section 5.3) and norm's
 * documented defaults.  Neither R nor norm can be run against it: the divisor of prelim.norm's column scaling and whether
 * the stopping rule is absolute or relative are not fixed by the reference tree; both move the iteration at which EM
 * stops, not the fixed point it approaches (DESIGN.md section 17 gives the size of that). ---- */
#define TWXEM_MAX_COLS TWXIF_MAX_COLS_NORM_IMPUTE   /* columns of an item: the target, its stations, its extra columns */
#define TWXEM_MAX_ROWS 8192             /* rows (days) of an item: k_em_prep sorts the rows of an item in LDS, 8 bytes each;
                                           the longest axis the other caps admit has 31 days x 136 years = 4216 */
#define TWXEM_RUN_ROWS 128              /* a stretch of equal missingness patterns is cut into runs of at most this */
#define TWXEM_DEFAULT_CRITERION 1e-4            /* em.norm's default criterion */
#define TWXEM_DEFAULT_MAXITS 1000               /* em.norm's default maxits */
#define TWXEM_ITERS_PER_LAUNCH 16       /* default: iterations of one launch of k_em_iter */
#define TWXEM_WORKSPACE_BYTES (256ll << 20)   /* default budget of the per-batch device workspace */
#define TWXEM_NKERNELS 2                /* kernel groups timed: k_em_prep, k_em_iter */
#define TWXEM_NTIMES 4                  /* entries of kernel_ms: the kernel groups, then two host-clock figures */
/* LDS per workgroup.  k_em_prep (256 threads): the sort keys 8 B x TWXEM_MAX_ROWS = 64 KiB + cnt / xbar / sdv 3 x 32 x 8 B
 * = 64.8 KiB: two workgroups fit a compute unit's 160 KiB.  k_em_iter (256 threads, 4 wavefronts): theta 32 x 32 x 8 B =
 * 8 KiB + one swept copy W per wavefront 4 x 8 KiB (reused for the partial T) + one completed row per wavefront
 * 4 x 256 B + xbar / sdv / reduction 0.6 KiB = 41.6 KiB: three workgroups fit.  Both are below 80 KiB.
 * Workspace per item of a batch: the row permutation and the run starts (8 bytes per row), theta (8 KiB), xbar / sdv
 * (512 B); the matrix is gathered again from obs in every iteration, no standardised copy is kept. */

/* per-item status */
#define TWXEM_OK TWX_CELL_OK                      /* converged: delta <= criterion */
#define TWXEM_NUMERIC TWX_CELL_NUMERIC            /* a sweep pivot <= 0 or not finite (R would return NaN / Inf); NaN results */
#define TWXEM_MAXITS 20                   /* maxits iterations without convergence: the last iterate is returned,
                                                     as em.norm does silently */
#define TWXEM_NO_MATRIX 21                        /* item_matrix_status was not TWXIF_OK: nothing computed, NaN */
#define TWXEM_EMPTY_COLUMN 22                     /* a column without a finite value on the item's days; NaN */
#define TWXEM_ROW_CAP 23                          /* more rows than TWXEM_MAX_ROWS; NaN, never an estimate from fewer rows */

/*
 * For every item (a target, a day group, its station columns, optionally one set of extra columns), X [n, P]: column 0
 * the target's observations on the days of the group, then the stations of its CSR list in order, then the columns of
 * its extra set; a non-finite value is missing.
 *   1. per column over its finite values: cnt, xbar = sum / cnt, sdv = sqrt((sum x^2 - (sum x)^2 / cnt) / cnt), 0 -> 1;
 *      z = (x - xbar) / sdv.
 *   2. theta, symmetric (P + 1) x (P + 1): theta[0][0] = -1, theta[0][j] = mu_j = 0, theta[j][k] = sigma_jk = I.
 *   3. an iteration: the rows grouped by their 32-bit mask of finite columns (equal masks keep day order), T = 0; per
 *      pattern with observed set O and missing set M: W = a fresh copy of theta swept on every k in O in ascending k
 *      (pivot d = W[k][k], r = 1 / d, c = W[:, k]: W -= (c c') r, W[:, k] = W[k, :] = c r, W[k][k] = -r); per row zhat = z on
 *      O and W[0][m] + sum over o in O (ascending) of W[o][m] z_o on m in M; T[0][j] += zhat_j, T[j][k] += zhat_j zhat_k, and
 *      W[j][k] for j, k in M (added once per run as rows x W[j][k]).  A row with nothing observed is a pattern like any
 *      other.  mu = T[0][.] / n, sigma = T / n - mu mu'; delta = the largest absolute change of an element of theta.
 *   4. stop at delta <= criterion or after maxits iterations.
 *   5. mean = mu_0 sdv_0 + xbar_0, variance = sigma_00 sdv_0^2.
 * iters counts completed iterations.  Every sum has a fixed order and no float atomics are used: two calls give the same
 * bytes, whatever iters_per_launch and workspace_bytes.
 *
 * obs [nstn][ndays]          station-major float32 of one variable, NaN (any non-finite value) = missing
 * group [ndays]              -1 (day not used) or 0 .. ngroups - 1
 * item_target, item_group [nitem]   the target's row of obs and the day group
 * item_matrix_status (optional) [nitem]   the item's status from twxif_infill_matrix; not TWXIF_OK: TWXEM_NO_MATRIX
 * col_off [nitem + 1], col_idx   CSR of each item's station columns (rows of obs), in order
 * set_group, set_ncol [nset], set_vals   extra-column sets: set s holds set_ncol[s] float64 columns over the days of group
 *                            set_group[s] in day order, column after column, the sets one after the other
 * item_set [nitem]           the item's set (of the item's own group) or -1; sets are shared between items; may be NULL
 *                            when nset == 0
 * criterion, maxits          > 0
 * iters_per_launch, workspace_bytes   <= 0: TWXEM_ITERS_PER_LAUNCH, TWXEM_WORKSPACE_BYTES.  A launch of k_em_iter runs at
 *                            most iters_per_launch iterations of the unfinished items of a batch; a batch is a run of
 *                            consecutive items whose workspace fits the budget (at least one item)
 * mean, variance, iters, delta, status [nitem]   out; delta is the last iteration's; NaN unless TWXEM_OK or
 *                            TWXEM_MAXITS
 * mu [nitem][31], sigma [nitem][31][31] (optional, both or neither)   out: all of mu and sigma on the original scale, NaN
 *                            beyond the item's columns
 * counts (optional) [2]      out: launches of k_em_iter, batches
 * kernel_ms (optional) [TWXEM_NTIMES]   device time of k_em_prep and of k_em_iter over all launches; then host-clock
 *                            milliseconds of the allocations and copies in, and of the copies back
 * Call-level failures (the message names the macro): an item with more than TWXEM_MAX_COLS columns in all; a target,
 * column, group or set index out of range; a set of another group than the item's; criterion or maxits not positive.
 */
int twxem_mean_variance(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t ngroups, const int8_t *group,
                        int64_t nitem, const int32_t *item_target, const int32_t *item_group,
                        const int32_t *item_matrix_status, const int64_t *col_off, const int32_t *col_idx, int64_t nset,
                        const int32_t *set_group, const int32_t *set_ncol, const double *set_vals, const int32_t *item_set,
                        double criterion, int32_t maxits, int32_t iters_per_launch, int64_t workspace_bytes, double *mean,
                        double *variance, int32_t *iters, double *delta, int32_t *status, double *mu, double *sigma,
                        int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/* ---- the estimator of step16: pca(method = 'ppca') of pcaMethods as twx/infill/rpy/pca_infill.R calls it, restated: EM
 * for probabilistic PCA with missing values (Tipping and Bishop 1999; Verbeek's ppca_mv, which pcaMethods follows).  Neither
 * R nor pcaMethods can be run against it.  Deviation: the start C0 is an ARGUMENT (R's rnorm stream under set.seed(4324)
 * cannot be reproduced); the facade passes np.random.RandomState(4324).standard_normal(D * d), column-major.  C0 moves
 * the iteration at which EM stops, not the fixed point (DESIGN.md section 18 gives the size of that). ---- */
#define TWXPP_MAX_COLS 64               /* columns of an item: one lane of a wavefront per column */
#define TWXPP_MAX_PCS 32                /* components of a fit */
#define TWXPP_MAX_ROWS 8192             /* rows (days) of an item; the longest axis the other caps admit has 4216 */
#define TWXPP_DEFAULT_THRESHOLD 1e-5            /* pca_infill.R: THRESHOLD */
#define TWXPP_DEFAULT_MAXITS 1000               /* pcaMethods' maxIterations */
#define TWXPP_ITERS_PER_LAUNCH 32       /* default: iterations of one launch of k_pp_iter */
#define TWXPP_WORKSPACE_BYTES (256ll << 20)   /* default budget of the per-batch device workspace */
#define TWXPP_NKERNELS 2                /* kernel groups timed: k_pp_prep, k_pp_iter */
#define TWXPP_NTIMES 4                  /* entries of kernel_ms: the kernel groups, then two host-clock figures */
/* The caps are library limits without a reference counterpart.  LDS per workgroup of k_pp_iter (256 threads, 4
 * wavefronts): C and Ye'X (which becomes the new C) 2 x 64 x 33 x 8 B = 33 KiB (row stride 33: lane j walks row j), S, Sx,
 * CtC and the inverse scratch 4 x 32 x 32 x 8 B = 32 KiB, per wavefront one row of Ye and three d-vectors 4 x 1.25 KiB,
 * reduction scratch 1.1 KiB: 71.3 KiB, two workgroups fit a compute unit's 160 KiB.  k_pp_prep: 32 KiB.  Workspace per
 * item of a batch: X twice (2 x N x d x 8 B), C (16.5 KiB), M and three scalars; the matrix is gathered again from obs in
 * every pass, no filled copy is kept. */

/* per-item status */
#define TWXPP_OK TWX_CELL_OK                      /* stopped at rel < threshold with count > 5 */
#define TWXPP_NUMERIC TWX_CELL_NUMERIC            /* a pivot of an inverse <= 0 or not finite, ss <= 0 or not finite, or a
                                                     column of C without norm in the orthonormalisation; NaN results */
#define TWXPP_MAXITS 20                           /* count passed maxits: the last iterate is returned (pcaMethods warns) */
#define TWXPP_NO_MATRIX 21                        /* item_matrix_status was not TWXIF_OK: nothing computed, NaN */
#define TWXPP_EMPTY_COLUMN 22                     /* a column without a finite standardised value; NaN */
#define TWXPP_ROW_CAP 23                          /* more rows than TWXPP_MAX_ROWS; NaN, never a fit from fewer rows */
#define TWXPP_COL_CAP 24                          /* more columns than TWXPP_MAX_COLS; NaN */
#define TWXPP_PCS_CAP 25                          /* more components than TWXPP_MAX_PCS; NaN */

/*
 * For every item: Y [N, D], column 0 the target's observations on the days of the group, then the stations of its CSR
 * list, then the columns of its extra set, each (value - norm_j) / std_j; a non-finite result is missing.  d = item_npcs.
 *   set-up    hidden = the missing positions, missing their count.  M_j = the mean of column j over its observed values;
 *             Ye = Y - M with the hidden positions 0; C = C0 [D, d]; CtC = C'C; X = (Ye C) CtC^-1;
 *             ss = sum over the observed positions of (X C' - Ye)^2 / (N D - missing); count = 1, old = infinity.
 *   iterate   Sx = (I + CtC / ss)^-1, ss_old = ss; Ye[hidden] = (X C')[hidden]; X = ((Ye C) Sx) / ss; S = X'X;
 *             C = (Ye'X) (S + N Sx)^-1; CtC = C'C;
 *             ss = (sum (C X' - Ye')^2 + N sum(CtC o Sx) + missing ss_old) / (N D);
 *             objective = N (D log ss + tr Sx - log det Sx) + tr S - missing log ss_old;
 *             rel = |1 - objective / old|, old = objective, count += 1;
 *             stop when rel < threshold and count > 5 (TWXPP_OK), else when count > maxits (TWXPP_MAXITS, the last iterate).
 *   after     Q = the columns of C orthonormalised in order (modified Gram-Schmidt, every column against the earlier ones
 *             twice); T = Ye Q with Ye holding its last fill; cov = (T'T - s s' / N) / (N - 1), s the column sums of T;
 *             V = the eigenvectors of cov, eigenvalues descending (cyclic Jacobi); C = Q V; X = Ye C.
 *   out       R2cum[i] = 1 - sum_obs (Ye - X[:, :i] C[:, :i]')^2 / sum_obs Ye^2, i = 1 .. d;
 *             fit = (X C[0, :]' + M_0) std_0 + norm_0: the reference keeps only column 0 of fitted().
 * An inverse is Gauss-Jordan without pivoting, the pivot row divided by the pivot; log det Sx is minus the sum of the logs
 * of the pivots of I + CtC / ss.  iters = count - 1.  Every sum has a fixed order and no float atomics are used: two calls
 * give the same bytes, whatever iters_per_launch and workspace_bytes.
 *
 * obs, group, item_target, item_group, item_matrix_status, col_off, col_idx, nset .. item_set   as twxem_mean_variance
 *                            takes them (a set may hold any number of columns)
 * item_npcs [nitem]          d of the item
 * norms, stds                per item its D values, the items one after the other (an item without a matrix has 1 column)
 * c0                         per item D x d values, column after column, the items one after the other; an item whose
 *                            item_matrix_status is not TWXIF_OK has none
 * threshold, maxits          > 0
 * iters_per_launch, workspace_bytes   <= 0: TWXPP_ITERS_PER_LAUNCH, TWXPP_WORKSPACE_BYTES
 * fit                        out: per item its N values in day order, the items one after the other; NaN unless TWXPP_OK
 *                            or TWXPP_MAXITS
 * r2cum [nitem][32], iters, rel, status [nitem]   out; rel is the last iteration's
 * c_out [nitem][64][32], m_out [nitem][64] (optional, each)   out: the rotated C and M, NaN beyond the item's D and d
 * counts (optional) [2]      out: launches of k_pp_iter, batches
 * kernel_ms (optional) [TWXPP_NTIMES]   device time of k_pp_prep and of k_pp_iter over all launches; then host-clock
 *                            milliseconds of the allocations and copies in, and of the copies back
 * An item above a cap gets TWXPP_ROW_CAP / TWXPP_COL_CAP / TWXPP_PCS_CAP (looked at in this order) and NaN.
 * Call-level failures: an item with a matrix and d < 1, d > D or N <= d; a target, column, group or set index out of range;
 * a set of another group than the item's; threshold or maxits not positive.
 */
int twxpp_ppca_fit(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t ngroups, const int8_t *group,
                   int64_t nitem, const int32_t *item_target, const int32_t *item_group,
                   const int32_t *item_matrix_status, const int32_t *item_npcs, const int64_t *col_off,
                   const int32_t *col_idx, int64_t nset, const int32_t *set_group, const int32_t *set_ncol,
                   const double *set_vals, const int32_t *item_set, const double *norms, const double *stds,
                   const double *c0, double threshold, int32_t maxits, int32_t iters_per_launch, int64_t workspace_bytes,
                   double *fit, double *r2cum, int32_t *iters, double *rel, int32_t *status, double *c_out, double *m_out,
                   int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/* ---- the check of step16's fits: _is_nonoptimal_infill (twx/infill/infill_daily.py:563-595) with hasVarChgPt
 * (twx/infill/rpy/pca_infill.R:306-310: cpt.var(vals, penalty = "Asymptotic", pen.value = sig) of R's changepoint with the
 * package defaults: at most one change, normal likelihood, mean unknown), restated: neither R nor the package's text can be
 * read or run against it.  Deviations: the range tau = 2 .. N - 2 is the package's of the reference's time as recalled
 * (later versions differ at the ends); the decision is cpt_stat >= pen; a NaN penalty (N too small for the asymptotic
 * formula, where R stops with an error) means "no change point"; a fit with a non-finite value gets the status
 * TWXCK_NOT_FITTED where R would raise. ---- */
#define TWXCK_MAX_ROWS 8192             /* rows of an item: the cap of TWXPP_MAX_ROWS */
#define TWXCK_DEFAULT_MAE_MAX 2.0               /* infill_daily.py:578 */
#define TWXCK_DEFAULT_R2_MIN 0.7
#define TWXCK_DEFAULT_IMPOSSIBLE_HIGH 57.7      /* infill_daily.py:584 */
#define TWXCK_DEFAULT_IMPOSSIBLE_LOW (-89.4)
#define TWXCK_VAR_FLOOR 1e-10           /* what a segment variance <= 0 is replaced by */
#define TWXCK_WORKSPACE_BYTES (256ll << 20)   /* default budget of the per-batch device copies of fit and obs */
#define TWXCK_NTIMES 3                  /* entries of kernel_ms: k_ck_check, then two host-clock figures */

/* bits of reasons */
#define TWXCK_LOW_PERF 1                /* mae > mae_max or r2 < r2_min (a NaN compares false, as in the reference) */
#define TWXCK_IMPOSSIBLE 2              /* nimpossible > 0 */
#define TWXCK_VAR_CHGPT 4               /* a variance change point */
#define TWXCK_UNFITTED 8                /* nothing to judge: status TWXCK_NOT_FITTED or TWXCK_ROW_CAP */

/* per-item status */
#define TWXCK_OK TWX_CELL_OK                      /* checked */
#define TWXCK_NOT_FITTED 26                       /* a non-finite value in fit: nothing computed; mae, r2, cpt_stat NaN, the
                                                     counts and cpt_tau 0, reasons = TWXCK_UNFITTED */
#define TWXCK_FEW_ROWS 27                         /* N < 4 (the package refuses such data): no change point, cpt_stat NaN,
                                                     cpt_tau 0; the other diagnostics are computed */
#define TWXCK_ROW_CAP 28                          /* N > TWXCK_MAX_ROWS: as TWXCK_NOT_FITTED, fit and obs are not read */

/*
 * For every item: fit [N] (degrees C) and obs [N] (NaN, any non-finite value, = missing) on the same days, N = off[i + 1] -
 * off[i]; V = the rows with a finite obs.
 *   performance   nobs = |V|; mae = sum_V |fit - obs| / nobs; xbar = sum_V obs / nobs, ybar = sum_V fit / nobs;
 *                 ssxm = sum_V (obs - xbar)^2, ssym = sum_V (fit - ybar)^2, ssxym = sum_V (obs - xbar)(fit - ybar) (the means
 *                 first, then the centred sums: two passes); r = ssxym / sqrt(ssxm ssym) clipped to [-1, 1], r = 0 when ssxm
 *                 or ssym is 0 (scipy.stats.linregress of the reference's time); r2 = r r.  nobs = 0: mae = r2 = NaN.
 *   impossible    nimpossible = the count of fit > impossible_high plus the count of fit < impossible_low, over all N rows.
 *   change point  mu = sum fit / N; y2[t] = sum over i <= t of (fit_i - mu)^2, t = 1 .. N; null = N log(y2[N] / N); for
 *                 tau = 2 .. N - 2: s1 = y2[tau] / tau, sn = (y2[N] - y2[tau]) / (N - tau), each replaced by TWXCK_VAR_FLOOR
 *                 if <= 0, tmp(tau) = tau log s1 + (N - tau) log sn.  cpt_tau = the FIRST tau of the smallest tmp (a NaN
 *                 tmp is never the smallest; all NaN: cpt_tau = 0, cpt_stat = NaN); cpt_stat = null - tmp(cpt_tau).  There
 *                 is a change point iff pen is not NaN and cpt_stat >= pen.  A constant series has null = -infinity and
 *                 every tmp equal: cpt_tau = 2, cpt_stat = -infinity, no change point.
 *   reasons       the TWXCK_* bits above.
 * The kernel (one workgroup of 256 per item, thread k owns the rows k c .. k c + c - 1, c = ceil(N / 256)) sums every
 * thread's rows in row order, the 64 lanes of a wavefront in a butterfly, the four wavefronts in order; y2[tau] is the
 * exclusive scan of the 256 chunk sums (shuffle-up inside a wavefront, the wavefront totals added in order) plus the
 * thread's own partial sum, y2[N] the scan's total.  That order is fixed and there are no float atomics: two calls give the
 * same bytes, whatever workspace_bytes.  The arg-min compares (tmp, tau) lexicographically.
 *
 * off [nitem + 1]            non-decreasing from 0: item i owns fit / obs [off[i], off[i + 1])
 * fit, obs                   float64, the items one after the other
 * pen [nitem]                the penalty of each item (the binding's cpt_penalty(N, sig)); NaN: no change point
 * mae_max, r2_min, impossible_high, impossible_low   finite; the reference's are the TWXCK_DEFAULT_* above
 * workspace_bytes            <= 0: TWXCK_WORKSPACE_BYTES.  A batch is a run of consecutive items whose fit and obs (16 B a
 *                            row) fit the budget (at least one item)
 * nobs, mae, r2, nimpossible, cpt_stat, cpt_tau, reasons, status [nitem]   out
 * counts (optional) [2]      out: launches of k_ck_check, batches (equal)
 * kernel_ms (optional) [TWXCK_NTIMES]   device time of k_ck_check over all launches; then host-clock milliseconds of the
 *                            allocations and copies in, and of the copies back
 * Call-level failures: nitem < 1, a null buffer, off not non-decreasing from 0, a non-finite scalar.
 */
int twxck_infill_check(int device, int64_t nitem, const int64_t *off, const double *fit, const double *obs,
                       const double *pen, double mae_max, double r2_min, double impossible_high, double impossible_low,
                       int64_t workspace_bytes, int32_t *nobs, double *mae, double *r2, int32_t *nimpossible,
                       double *cpt_stat, int32_t *cpt_tau, int32_t *reasons, int32_t *status, int32_t *counts,
                       float *kernel_ms, char *errbuf, int errlen);

/* ---- step15, the cross-validation of the infill (twx/infill/xval_infill.py, scripts/step15_mpi_xval_infill.py): which
 * observations of a station are hidden from its own infill, the neighbour matrices of a target that must not see its own
 * full record, and the comparison of the infilled series with the hidden observations.  The chain between them is
 * twxem_mean_variance, twxpp_ppca_fit and twxck_infill_check as they are: the masked series of a cross-validation station
 * travels as a row APPENDED to the pool (same longitude / latitude, never eligible), the target is that row, and the
 * station's own row is the one excluded from its neighbours, so every other target still sees the full record. ---- */
#define TWXXV_NGROUPS 12                /* day groups of twxxv_score (the calendar months) */
#define TWXXV_NSCORES 13                /* entries per series of n / bias / mae: the groups, then the whole series */

/*
 * XvalInfill.__init__ (:73-86) in closed form.  For target row t = obs[target_idx[t]]: day d is HELD iff its value is
 * finite and, when nkeep > 0, at least nkeep finite days of the row lie after d (the reference keeps
 * np.nonzero(fin)[0][-nkeep:]).  nkeep == 0 holds nothing ([-0:] is the whole list: the reference's quirk, kept); a row
 * with at most nkeep finite days holds nothing.  Any non-finite value is missing.  nkeep is the caller's
 * int(np.round(ntrain_yrs * 365.25)), rounded half to even.
 *
 * obs [nstn][ndays]          station-major float32; only the targets' rows are copied to the device
 * target_idx [ntarget]       0 <= index < nstn
 * held [ntarget][ndays]      out: 1 = held
 * train_obs [ntarget][ndays] out: the row with the held days NaN (0x7fc00000), every other value bit for bit
 * nheld, nfinite [ntarget]   out: held days, finite days of the row
 * kernel_ms (optional) [1]   device time of k_xv_holdout
 * Call-level failures: nstn, ndays or ntarget < 1, nkeep < 0, a null buffer, an index out of range.
 */
int twxxv_holdout(int device, int64_t nstn, int64_t ndays, const float *obs, int64_t ntarget, const int32_t *target_idx,
                  int32_t nkeep, uint8_t *held, float *train_obs, int32_t *nheld, int32_t *nfinite, float *kernel_ms,
                  char *errbuf, int errlen);

/*
 * twxif_infill_matrix (same driver, same kernels, same outputs) with exclude_idx [ntarget]: a row of the pool that is never
 * a neighbour of that target, or -1.  With every entry -1 the outputs are twxif_infill_matrix's byte for byte; with row x
 * excluded they are those of a call in which eligible[x] is 0 for that target alone.
 * Call-level failures: twxif_infill_matrix's, and an exclude_idx outside -1 .. nstn - 1.
 */
int twxxv_infill_matrix(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat, const float *obs,
                        const int32_t *ymd, const uint8_t *eligible, int64_t ntarget, const int32_t *target_idx,
                        const int32_t *exclude_idx, int32_t ngroups, const int8_t *group, const int32_t *nthres_all,
                        const int32_t *nthres_target_por, int32_t min_daily_nnghs, int32_t *status, int32_t *nnghs,
                        double *max_dist, int64_t *csr_off, int64_t csr_cap, int32_t *ngh_idx, double *ngh_ioa,
                        double *ngh_dist, int32_t *ngh_nlap, int32_t *ngh_nlap_stn, uint8_t *keep, int32_t *nrounds,
                        float *kernel_ms, char *errbuf, int errlen);

/*
 * run_xval:153-154 and the writer's np.ma arithmetic (step15:127-134).  A day of series s is SCORED iff held[s][d] != 0
 * and infill[s][d] is finite.  Over the scored days of the series, and over those of each group g (group[d] == g):
 *   n, bias = sum(infill - obs) / n, mae = sum |infill - obs| / n     (n == 0: NaN)
 * fp64 on the float32 observations widened exactly.  One workgroup of 256 per series, one pass: thread i adds its days i,
 * i + 256, ... in ascending order to thirteen accumulators of its own, and for each of them the 256 partial sums meet in
 * a halving tree; no float atomics: two calls give the same bytes.
 *
 * infill [nseries][ndays]    float64, NaN = not fitted
 * obs [nseries][ndays]       float32; finite wherever held is set (what twxxv_holdout gives)
 * held [nseries][ndays]      0 / not 0
 * group [ndays]              -1 (in no group) or 0 .. TWXXV_NGROUPS - 1; shared by the series
 * n, bias, mae [nseries][TWXXV_NSCORES]   out: entries 0 .. 11 the groups, entry 12 the whole series
 * obs_out, infill_out [nseries][ndays]    out, float32: the value on the scored days, NaN elsewhere (what step15 stores)
 * kernel_ms (optional) [1]   device time of k_xv_score
 * Call-level failures: nseries or ndays < 1, a null buffer, a group value outside -1 .. 11.
 */
int twxxv_score(int device, int64_t nseries, int64_t ndays, const double *infill, const float *obs, const uint8_t *held,
                const int8_t *group, int32_t *n, double *bias, double *mae, float *obs_out, float *infill_out,
                float *kernel_ms, char *errbuf, int errlen);

/* ---- step17 and step18, from the infilled database to the serially-complete one: the choice between "observations +
 * infill" and "all model" per station with the scrub of what is still missing (create_serially_complete_db,
 * twx/infill/post_infill.py:106-149), the 1981-2010 monthly normals (add_monthly_normals :354-402 with
 * TairAggregate.daily_to_mthly / daily_to_mthly_norms, twx/utils/util_tair.py:67-158), and the check of a suspect station's
 * WHOLE series (has_bad_infill, scripts/step17_find_bad_infill_stns.py:40-68).  The change-point test is the restated one of
 * the twxck_infill_check block above, same caveat. ---- */
#define TWXSC_MAX_DAYS 1048576          /* days of a series (2^20); the reference's axis has 25 203 */
#define TWXSC_MAX_GROUPS 1536           /* (year, month) groups of the normals: 128 years; one double of LDS each */
#define TWXSC_DEFAULT_RUN_THRESHOLD 1826        /* USE_ALL_INFILL_THRESHOLD = np.round(365.25 * 5.0), post_infill.py:39 */
#define TWXSC_DEFAULT_MAX_MISS 9                /* util_tair.py:67,109 */
#define TWXSC_WORKSPACE_BYTES (256ll << 20)   /* default budget of the per-batch device copies of the series */
#define TWXSC_NTIMES 4                  /* entries of kernel_ms, see the entries */

/*
 * For every series s (station-major rows of ndays days):
 *   infilled day  flag != 0 (the reference's .astype(np.bool): the int8 fill -127 of a station that failed the infill counts)
 *   max_run       the longest run of consecutive infilled days (_runs_of_ones_array), 0 if there is none
 *   all_infill    max_run >= run_threshold
 *   source row    tair_infilled if all_infill, else tair
 *   flag_out      all 1 if all_infill, else flag != 0 as 0 / 1
 *   missing       a source value that is non-finite or compares equal to fill (netCDF4's masking plus the reference's
 *                 ~np.isfinite scrub); serial holds fill there and the source value bit for bit elsewhere; nmissing counts
 *                 the missing days
 *   normals       from serial.  Group g = 12 (year - start_norm_yr) + month - 1 owns the contiguous days group_first[g] ..
 *                 group_first[g] + group_ndays[g] - 1 (group_ndays[g] = 0: no such day on the axis).  n_miss = its missing
 *                 days; mean_g = (the sum of its non-missing values IN DAY ORDER) / their count.  The group is masked if it
 *                 has no day, no non-missing day, or max_miss >= 0 and n_miss > max_miss.  norm[m] = (the sum of the
 *                 unmasked mean_g, g = m mod 12, IN YEAR ORDER) / their number, which is norm_nmths[m]; none unmasked: NaN
 *                 and 0.  fp64 on the float32 values widened exactly.
 * tair_infilled and flag may be null together: the source row is tair as it is, max_run = 0, all_infill = 0, and serial and
 * flag_out may then be null too (normals only; flag_out, if given, is all 0).  group_first may be null: no normals.
 * One workgroup of 256 per series.  k_sc_select: thread k reduces its contiguous flags k c .. k c + c - 1, c = ceil(ndays /
 * 256), to (length, longest prefix run, longest suffix run, longest run), an associative monoid joined in order across the
 * 64 lanes and the four wavefronts (integers: any tree gives the same answer); then the select-and-write pass.  k_sc_norms
 * (the batch still on the device): one thread per group adds its days in day order, one thread per month adds its years in
 * year order.  No float atomics, nothing waits on another workgroup: two calls give the same bytes, whatever workspace_bytes.
 *
 * tair [nseries][ndays]      float32: the infilled database's <var>
 * tair_infilled [nseries][ndays], flag [nseries][ndays]   float32 and int8, or both null
 * run_threshold              the binding's int(np.round(365.25 * 5.0)) = TWXSC_DEFAULT_RUN_THRESHOLD
 * fill                       finite; the float32 netCDF fill is 9.96921e36
 * ngroups, group_first, group_ndays [ngroups]   ngroups a multiple of 12 in 12 .. TWXSC_MAX_GROUPS; the groups with days
 *                            ascending and disjoint
 * max_miss                   negative: no threshold (the reference's None)
 * workspace_bytes            <= 0: TWXSC_WORKSPACE_BYTES.  A batch is a run of consecutive series whose device rows (4 B a
 *                            day for tair, 5 for tair_infilled and flag, 4 for serial, 1 for flag_out) fit (at least one)
 * serial [nseries][ndays], flag_out [nseries][ndays]   out, float32 and int8
 * max_run, nmissing [nseries], all_infill [nseries]    out, int32 and uint8
 * norm [nseries][12], norm_nmths [nseries][12]         out, float64 and int32 (not written without groups)
 * counts (optional) [2]      out: kernel launches, batches
 * kernel_ms (optional) [TWXSC_NTIMES]   device time of k_sc_select and of k_sc_norms over all launches; then host-clock
 *                            milliseconds of the allocations and copies in, and of the copies back
 * Call-level failures: nseries or ndays < 1, ndays > TWXSC_MAX_DAYS, exactly one of tair_infilled / flag null, a null buffer,
 * ngroups not a multiple of 12 in range, a group outside the axis or not after the groups before it, a non-finite fill.
 */
int twxsc_serial_complete(int device, int64_t nseries, int64_t ndays, const float *tair, const float *tair_infilled,
                          const int8_t *flag, int32_t run_threshold, float fill, int32_t ngroups, const int32_t *group_first,
                          const int32_t *group_ndays, int32_t max_miss, int64_t workspace_bytes, float *serial,
                          int8_t *flag_out, int32_t *max_run, int32_t *nmissing, uint8_t *all_infill, double *norm,
                          int32_t *norm_nmths, int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/*
 * step17's has_bad_infill of every series (all of N = ndays rows), with the TWXCK_* reason bits and statuses as they are:
 *   missing       a value that is non-finite or compares equal to fill.  A series with one gets nmissing = their count,
 *                 status TWXCK_NOT_FITTED, reasons TWXCK_UNFITTED, nimpossible = cpt_tau = 0, cpt_stat NaN (R would raise
 *                 there, and step17 calls the station bad).
 *   otherwise     nmissing = 0, and nimpossible, cpt_stat, cpt_tau and the bits TWXCK_IMPOSSIBLE / TWXCK_VAR_CHGPT are the
 *                 "impossible" and "change point" paragraphs of the twxck_infill_check block with fit := the series widened
 *                 to float64 and N = ndays, WITHOUT the cap of TWXCK_MAX_ROWS; ndays < 4: TWXCK_FEW_ROWS.
 * The kernel is k_ck_check's shape and order of summation (thread k owns the rows k c .. k c + c - 1, c = ceil(N / 256), about
 * 99 at 25 203 days; the chunk is read again from global memory, never held in registers or LDS), so on a series both
 * entries accept the two give the same bytes.
 *
 * series [nseries][ndays]    float32
 * fill                       finite
 * pen                        the penalty of every series (the binding's cpt_penalty(ndays, sig)); NaN: no change point
 * impossible_high, impossible_low   finite; step17's world records are TWXCK_DEFAULT_IMPOSSIBLE_HIGH / _LOW
 * workspace_bytes            <= 0: TWXSC_WORKSPACE_BYTES; a batch is a run of series whose rows (4 B a day) fit
 * nimpossible, nmissing, cpt_stat, cpt_tau, reasons, status [nseries]   out
 * counts (optional) [2]      out: launches of k_sc_series, batches (equal)
 * kernel_ms (optional) [TWXSC_NTIMES]   device time of k_sc_series; 0; host-clock milliseconds of the allocations and
 *                            copies in, and of the copies back
 * Call-level failures: nseries or ndays < 1, ndays > TWXSC_MAX_DAYS, a null buffer, a non-finite fill or bound.
 */
int twxsc_series_check(int device, int64_t nseries, int64_t ndays, const float *series, float fill, double pen,
                       double impossible_high, double impossible_low, int64_t workspace_bytes, int32_t *nimpossible,
                       int32_t *nmissing, double *cpt_stat, int32_t *cpt_tau, int32_t *reasons, int32_t *status,
                       int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/* ---- the reanalysis columns of the infill family (step14 / step15 / step16): pca_svd(A, True, True) of
 * twx/utils/pca.py:26-76 on the matrix NNRNghData.get_nngh_matrix returns (twx/db/reanalysis.py:372-432), cut as
 * _InfillMatrix.infill cuts it (twx/infill/infill_normals.py:347-356), for every (column set, day group) item of one call.
 * The route differs from the reference's: the eigen-decomposition of the Gram matrix of the standardised columns instead of
 * LAPACK's SVD of the matrix.  The sign of a component is LAPACK's there and fixed by a rule here; the estimate does not
 * depend on it.  DESIGN.md section 22 gives the measured distance between the two routes. ---- */
#define TWXNR_MAX_COLS 64               /* columns of a set; the reference's shape is 4 cells x 8 variable / level columns */
#define TWXNR_MAX_CUTS 4                /* thresholds of one call (the reference uses 0.99, and 0.90 in chk_perf's ladder) */
#define TWXNR_MAX_SWEEPS 30             /* Jacobi sweeps before TWXNR_NOCONV */
#define TWXNR_NKERNELS 3                /* kernel groups timed: k_nr_gram, k_nr_eig, k_nr_scores */
#define TWXNR_NTIMES 5                  /* entries of kernel_ms: the kernel groups, then two host-clock figures */
/* LDS per workgroup.  k_nr_gram (256 threads): a tile of 64 days x 64 columns at a row stride of 65 doubles = 33 280 B,
 * mean and sd 2 x 64 x 8 B = 1 024 B, the column verdicts 64 x 4 B = 256 B: 34 560 B, four workgroups fit a compute unit's
 * 160 KiB.  k_nr_eig (64 threads): the Gram matrix and the rotation accumulator, 2 x P x P x 8 B for the largest P of the
 * call: 65 536 B at the cap, 16 384 B at P = 32.  k_nr_scores (256 threads): the loadings 64 x 64 x 8 B = 32 768 B, mean and
 * sd 1 024 B: 33 792 B.  Nothing row-sized lives in LDS: there is no row cap. */

/* per-item status */
#define TWXNR_OK TWX_CELL_OK                      /* decomposed */
#define TWXNR_NOCONV 29                           /* the off-diagonal norm is still above eps x trace after
                                                     TWXNR_MAX_SWEEPS sweeps: the last iterate is returned, no scores */
#define TWXNR_NONFINITE 30                        /* a non-finite value in a column on a day of the group (the reference
                                                     returns NaN scores); bad_col names the first such column */
#define TWXNR_CONSTANT 31                         /* a column of zero variance on the days of the group (the reference
                                                     divides by zero); bad_col names the first such column */
#define TWXNR_FEW_ROWS 32                         /* fewer than 2 days in the group: nothing computed */

/*
 * For every set s (P = set_off[s + 1] - set_off[s] columns of cols, in order) and day group g (its days are those with
 * group[day] == g, n of them, in day order), item = s * ngroups + g:
 *   1. per column: mean = sum / n, sd = sqrt(sum (x - mean)^2 / (n - 1)) (the mean first, then the centred sum), z = (x -
 *      mean) / sd.  A non-finite value: TWXNR_NONFINITE; else sd == 0: TWXNR_CONSTANT.
 *   2. G = Z'Z / (n - 1), every entry one sum over the days in ascending order: symmetric to the bit.
 *   3. the eigen-decomposition of G by cyclic Jacobi (round-robin pair order, see twx_nnr.hip), until the off-diagonal
 *      norm is <= eps x trace (eps = 2^-52).  Eigenvalues descending, equal ones by index; a component's loadings are
 *      signed so that the one of largest magnitude (the first of equal ones) is positive.
 *   4. var_explain[k] = lambda_k / (lambda_0 + lambda_1 + .. in this order); ncomp[v] = 1 + the first k at which
 *      var_explain[0] + .. + var_explain[k] (added in order) >= max_var[v]; P if no k does.  With n < P the trailing
 *      eigenvalues are ~0 (possibly below 0 by rounding) and the cut is unchanged.
 *   5. the scores of the first max over v of ncomp[v] components: score[r][k] = sum over j (ascending) of z[r][j] x
 *      loadings[k][j].
 * fp64 on the float32 values widened exactly; every sum has a fixed order and no float atomics are used: two calls give
 * the same bytes.
 *
 * cols [ncol][ndays]         float32, column-major: a column's days are contiguous.  A column may belong to several sets
 * set_off [nset + 1], set_col   CSR of the sets' columns (0 <= set_col < ncol), 1 <= P <= TWXNR_MAX_COLS
 * group [ndays]              -1 (day in no group) or 0 .. ngroups - 1, ngroups <= TWXIF_MAX_GROUPS
 * max_var [nthr]             in (0, 1), nthr <= TWXNR_MAX_CUTS
 * status, bad_col, sweeps [nitem], ncomp [nitem][nthr]   out; bad_col = -1 unless the status names a column; ncomp = 0
 *                            for an item that was not decomposed
 * mean, sd, var_explain, eigval   out, packed: item (s, g) owns the P entries from ngroups x set_off[s] + g x P
 * loadings                   out, packed: item (s, g) owns P x P entries from ngroups x (sum of P^2 of the sets before s) +
 *                            g x P^2, component k the row k P .. k P + P - 1.  The packed entries of an item that was not
 *                            decomposed are NaN (mean and sd are written before a column is judged)
 * score_off [nitem + 1], scores   out: the scores of item i are (score_off[i + 1] - score_off[i]) / n columns of n days,
 *                            column after column; an item whose status is not TWXNR_OK has none.  score_cap entries must
 *                            suffice: the call fails if they do not (sum over the items of n x P always does)
 * kernel_ms (optional) [TWXNR_NTIMES]   device time of k_nr_gram, k_nr_eig, k_nr_scores; then host-clock milliseconds of
 *                            the allocations and copies in, and of the copies back
 * Call-level failures, all before any device work: ndays, ncol or nset < 1, a null buffer, ngroups outside 1 ..
 * TWXIF_MAX_GROUPS, nthr outside 1 .. TWXNR_MAX_CUTS, a max_var outside (0, 1), set_off not from 0, a set with no column or
 * more than TWXNR_MAX_COLS, a set_col out of range, a group value outside -1 .. ngroups - 1.
 */
int twxnr_components(int device, int64_t ndays, int64_t ncol, const float *cols, int64_t nset, const int64_t *set_off,
                     const int32_t *set_col, int32_t ngroups, const int8_t *group, int32_t nthr, const double *max_var,
                     int32_t *status, int32_t *bad_col, int32_t *ncomp, int32_t *sweeps, double *mean, double *sd,
                     double *var_explain, double *eigval, double *loadings, int64_t *score_off, int64_t score_cap,
                     double *scores, float *kernel_ms, char *errbuf, int errlen);

/* ---- step05 and step09 to step11, from the flagged database to the homogenised one: the observation counts of
 * add_obs_cnt (twx/db/create_db_all_stations.py:1414-1416), the monthly means of add_monthly_means (:1312-1329 with
 * TairAggregate.daily_to_mthly, twx/utils/util_tair.py:67-104), the time-of-observation shift of Tmax (_tobs_shift_tmax,
 * twx/homog/tobs.py:243-264) and the daily homogenisation from PHA's monthly output (HomogDaily.homog_stn,
 * twx/homog/pha.py:242-290).  PHA itself is an external program and is not part of this library.  A record is station-major,
 * [nstn][ndays] float32 with NaN for "no value"; year-months are runs of consecutive days mth_first[g] .. mth_first[g] +
 * mth_ndays[g] - 1 with 1 <= mth_ndays[g] <= 31 and mth_first[g + 1] = mth_first[g] + mth_ndays[g] (a record may start or
 * end inside a month; days before the first or after the last month belong to none). ---- */
#define TWXHM_MAX_MONTHS 16384          /* year-months of a record */
#define TWXHM_MTHS_PER_GROUP 128        /* months one workgroup of k_hm_means stages in LDS: at most 3 968 days */
#define TWXHM_DEFAULT_MAX_MISS 9        /* add_monthly_means' max_miss */
#define TWXHM_PHA_MISSING (-9999)       /* PHA's missing monthly value */
#define TWXHM_NTIMES 4                  /* entries of kernel_ms: two kernel figures, then two host-clock figures */
/* LDS of k_hm_means (128 threads): 3 968 + 8 floats = 15 904 B (the stretch is read from the 16-byte boundary below its
 * first day to the one above its last).  The other kernels use a few integers. */

/* per-station status of twxhm_homog_daily */
#define TWXHM_OK TWX_CELL_OK
#define TWXHM_NO_ADJ 33                 /* a month needs the adjustment list and the station has none (the reference dies
                                           on an IndexError there) */
#define TWXHM_OVERLAP 34                /* a month lies in more than one adjustment interval (the reference raises) */

/*
 * cnt[s][m - 1] = the number of days d in first_day .. last_day (inclusive day indices) with day_month[d] == m and obs[s][d]
 * finite.  obs is the raw variable with its fill value as NaN; quality flags are NOT applied (the reference counts ds[elem]).
 * One workgroup of 256 per station; integer counts, joined by a shuffle tree and through LDS.
 *
 * obs [nstn][ndays]          float32
 * day_month [ndays]          int8, 1 .. 12
 * workspace_bytes            <= 0: TWXSC_WORKSPACE_BYTES; a batch is a run of stations whose rows (4 B a day) fit, at least one
 * cnt [nstn][12]             out, int32
 * counts (optional) [2]      out: kernel launches, batches
 * kernel_ms (optional) [TWXHM_NTIMES]   device time of k_hm_cnt; 0; host-clock milliseconds of the allocations and copies
 *                            in, and of the copies back (the same layout in every entry below)
 * Call-level failures: nstn or ndays < 1, ndays > TWXSC_MAX_DAYS, a null buffer, a window outside the axis or empty, a
 * day_month outside 1 .. 12.
 */
int twxhm_obs_cnt(int device, int64_t nstn, int64_t ndays, const float *obs, const int8_t *day_month, int64_t first_day,
                  int64_t last_day, int64_t workspace_bytes, int32_t *cnt, int32_t *counts, float *kernel_ms, char *errbuf,
                  int errlen);

/*
 * For every station s and month g: mth_miss = the number of non-finite days of the month; mth_mean = (float32)(sum / n),
 * n the number of finite days and sum the fp64 sum IN DAY ORDER of the month's days with a non-finite day counted as +0.0
 * and the first day's value (or +0.0) as the start -- numpy's masked sum over the day axis, to the sign of a zero.  NaN if
 * n = 0, or max_miss >= 0 and mth_miss > max_miss.  obs holds NaN on flagged and on missing days.
 * k_hm_means: a workgroup of 128 owns TWXHM_MTHS_PER_GROUP consecutive months of one station, loads their days into LDS
 * with 16-byte loads from the aligned boundary below (the last, partial vector of a batch by scalar loads), then lane g adds
 * month g's days from LDS in day order.  No atomics: two calls give the same bytes.
 *
 * nmth, mth_first, mth_ndays [nmth]   1 <= nmth <= TWXHM_MAX_MONTHS, as the block comment states
 * max_miss                   negative: no threshold
 * workspace_bytes            as above
 * mth_mean [nstn][nmth], mth_miss [nstn][nmth]   out, float32 and int16
 * Call-level failures: as above, and a month list that is empty, too long, not consecutive or outside the axis.
 */
int twxhm_monthly_means(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t nmth, const int32_t *mth_first,
                        const int32_t *mth_ndays, int32_t max_miss, int64_t workspace_bytes, float *mth_mean,
                        int16_t *mth_miss, int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/*
 * Per station, am[d] = tobs[d] > 0 && tobs[d] < 1100 (a morning observation; NaN is none), ok[d] = !am[d] &&
 * finite(tmax[d]), S = {d > 0 : am[d] && !ok[d - 1]}, nshift = |S|.
 *   |S| > 1    out[d] = tmax[d + 1] if d + 1 is in S; else tmax[d] if ok[d]; else NaN (0x7fc00000).  d + 1 in S implies
 *              !ok[d], so the cases do not collide.
 *   |S| <= 1   out = tmax, bit for bit.  THE REFERENCE'S QUIRK, KEPT: it tests idx_shift.size > 1, so a station with
 *              exactly one morning observation to shift keeps it on its day, and keeps its other morning values too.
 * One workgroup of 256 per station: the count (integers, any tree), then the element-wise pass.
 *
 * tmax, tobs [nstn][ndays]   float32, NaN = none
 * workspace_bytes            as above; 12 B a day
 * out [nstn][ndays], nshift [nstn]   out, float32 and int32
 * Call-level failures: nstn or ndays < 1, ndays > TWXSC_MAX_DAYS, a null buffer.
 */
int twxhm_tobs_shift(int device, int64_t nstn, int64_t ndays, const float *tmax, const float *tobs, int64_t workspace_bytes,
                     float *out, int32_t *nshift, int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/*
 * HomogDaily.homog_stn for every station.  Per station s and month g, with round2(x) = rint(x * 100) / 100 in fp64 (numpy's
 * round(x, 2)):
 *   m = round2((double)mth_mean), masked if mth_mean is NaN;  h = round2((double)pha / 100), masked if pha ==
 *   TWXHM_PHA_MISSING.
 *   both present       m != h: delta = h - m, and the month counts in nchanged (the reference's dif_cnt); m == h: untouched.
 *   h present, m masked, mth_miss < mth_ndays   with the station's adjustments a = adj_off[s] .. adj_off[s + 1] - 1, sorted
 *                      by adj_ymd_start: none: TWXHM_NO_ADJ; mth_ymd[g] < adj_ymd_start[first]: delta = -adj[first]; else
 *                      by the number of intervals with adj_ymd_start <= mth_ymd[g] <= adj_ymd_end (inclusive): 0: delta =
 *                      +0.0, WHICH IS ADDED (-0.0 + 0.0 changes a bit; the reference adds it); 1: delta = -adj of it; more:
 *                      TWXHM_OVERLAP.  Then delta = round2(delta).
 *   otherwise          untouched.
 * delta[s][g] is NaN for an untouched month.  out[s][d] = (float)((double)obs[s][d] + delta[s][g]) on the days of a touched
 * month, obs[s][d] bit for bit elsewhere.  A station whose status is not TWXHM_OK has its delta and out rows NaN and
 * nchanged 0; its neighbours are unaffected.
 * k_hm_delta: one workgroup of 256 per station, a thread per month, the status and the count joined as integers.
 * k_hm_apply: the batch's rows as one flat array, 16-byte loads and stores of four days a thread (the buffers are aligned,
 * so every vector is; a row boundary may fall inside one) and a scalar tail of the batch; plain vector stores.
 *
 * obs [nstn][ndays]          float32
 * mth_mean, mth_miss, pha [nstn][nmth]   float32, int16, int32 hundredths
 * mth_ymd [nmth]             yyyymmdd of a month's first day
 * adj_off [nstn + 1], adj_ymd_start, adj_ymd_end, adj   CSR of the adjustment list, int64, int32, int32, float64
 * workspace_bytes            as above; 8 B a day
 * delta [nstn][nmth], out [nstn][ndays], status [nstn], nchanged [nstn]   out, float64, float32, int32, int32
 * kernel_ms                  device time of k_hm_delta, of k_hm_apply over all batches, then the host-clock figures
 * Call-level failures, all before any launch: the above, adj_off not ascending from 0, a station's adj_ymd_start not sorted.
 */
int twxhm_homog_daily(int device, int64_t nstn, int64_t ndays, const float *obs, int32_t nmth, const float *mth_mean,
                      const int16_t *mth_miss, const int32_t *pha, const int32_t *mth_ymd, const int32_t *mth_first,
                      const int32_t *mth_ndays, const int64_t *adj_off, const int32_t *adj_ymd_start,
                      const int32_t *adj_ymd_end, const double *adj, int64_t workspace_bytes, double *delta, float *out,
                      int32_t *status, int32_t *nchanged, int32_t *counts, float *kernel_ms, char *errbuf, int errlen);

/* ---- step19 and the front of step20: raster values at the stations of a serially-complete database
 * (add_stn_raster_values with _find_nn_data, twx/infill/post_infill.py:248-352 and :443-510), the duplicate stations of
 * find_dup_stns (:193-246) and the column counts that find_dup_stns and step20's final check
 * (scripts/step20_add_bad_stn_flag.py:102-112) take from the file.  A raster is [rows][cols], north-up, float32 or float64
 * (an integer raster is converted by the caller to whichever holds it exactly), with GDAL's geo_t = (left edge, cell width
 * > 0, 0, top edge, 0, cell height < 0) in the stations' own geographic coordinates: the reference's osr transformation is
 * an identity that is required here and not performed, and a rotated raster is refused.  At least 2 x 2:
 * mpl_toolkits.basemap.interp, which the sampling restates as k_sample does, needs two cell centres on each axis.  The
 * BAND's no-data value is what read_as_array masks; ndata (a_rast.ndata) is what is written for "no value" and what
 * _find_nn_data compares with.  The two are separate inputs: step19 reassigns ndata on the mask raster. ---- */
#define TWXRV_F32 0                     /* dtype of a raster */
#define TWXRV_F64 1
#define TWXRV_MAX_EXTENT 134217727      /* rows and columns of a raster: the 8 r + 2 slots of the last ring fit an int32 */
#define TWXRV_MAX_DUP_STNS 1048576      /* stations of twxrv_dup_classes (all pairs) */
#define TWXRV_COUNT_I8_SUM 0            /* kind of twxrv_col_count */
#define TWXRV_COUNT_F32_MISSING 1
#define TWXRV_NTIMES 3                  /* entries of kernel_ms: the kernel; host-clock milliseconds of the allocations and
                                           copies in, and of the copies back */
#define TWXRV_TIE_REL 1e-9              /* the caller decides a ring again on the host when the runner-up lies this close */
/* LDS: k_rv_dup 4 096 B (the keys of a tile of 256 stations), k_rv_colcount 1 024 B; the others none. */

/* per-station status of twxrv_sample and twxrv_nearest_data */
#define TWXRV_OK TWX_CELL_OK            /* twxrv_sample: the value of extract_method; twxrv_nearest_data: a data cell found */
#define TWXRV_NEAREST 35                /* the value of the clipped nearest cell (the checkbounds=False, order=0 call) */
#define TWXRV_NODATA 36                 /* no value and force_data_value is off: value = ndata */
#define TWXRV_NEEDS_FORCE 37            /* no value and force_data_value is on: the station goes to twxrv_nearest_data */
#define TWXRV_NO_DATA_ANYWHERE 38       /* twxrv_nearest_data: no ring up to max(rows, cols) holds a data cell the
                                           reference's tests admit (the reference loops forever) */

/*
 * Per station, in the reference's order, with x0, x1 (ylo, yhi) the centres of the first and last columns (rows) as
 * get_coord_grid_1d gives them, xc = clip((cols - 1) (lon - x0) / (x1 - x0), 0, cols - 1) and yc likewise from the south:
 *   1. if x0 <= lon <= x1 and ylo <= lat <= yhi (checkbounds=True; outside, interp raises and the value is missing):
 *      extract_method 1: the bilinear value of the cells (yi, xi), (yi + 1, xi + 1), (yi + 1, xi), (yi, xi + 1), upper
 *      indices clipped, xi = int(xc), weights from xc - float32(xi) as interp computes them; missing if any of the four
 *      cells equals the band's no-data value.  extract_method 0: the cell (around(yc), around(xc)), half to even.
 *   2. if missing and ((is_inbounds(lon, lat), outer edges, and (extract_method 0 or revert_nn)) or force_data_value): the
 *      cell (around(yc), around(xc)) of the clipped coordinates; status TWXRV_NEAREST if it has a value.
 *   3. if still missing: TWXRV_NEEDS_FORCE with force_data_value, else TWXRV_NODATA; value = ndata.
 * row, col: get_row_col(lon, lat, check_bounds=False) = clip(abs(int((lat - geo_t[3]) / geo_t[5])), 0, rows - 1) and the
 * same of the columns: a station west or north of the raster is mirrored into it by the abs() -- the reference's quirk,
 * kept, because _find_nn_data starts there.
 *
 * data [rows][cols]          float32 (TWXRV_F32) or float64 (TWXRV_F64)
 * geo_t [6]
 * has_band_ndata, band_ndata the band's no-data value, if it has one
 * lon, lat [nstn]            finite
 * value [nstn], status [nstn], row [nstn], col [nstn]   out: float64, int32 (TWXRV_*), int32, int32
 * kernel_ms (optional) [TWXRV_NTIMES]
 * Call-level failures, all before any device work: a raster below 2 x 2 or above TWXRV_MAX_EXTENT, a geo_t that is
 * non-finite, rotated or not north-up, an unknown dtype or extract_method, nstn < 1, a null buffer, a non-finite coordinate.
 */
int twxrv_sample(int device, int64_t rows, int64_t cols, int32_t dtype, const void *data, const double *geo_t,
                 int32_t has_band_ndata, double band_ndata, double ndata, int64_t nstn, const double *lon, const double *lat,
                 int32_t extract_method, int32_t revert_nn, int32_t force_data_value, double *value, int32_t *status,
                 int32_t *row, int32_t *col, float *kernel_ms, char *errbuf, int errlen);

/*
 * _find_nn_data for every point (row, col): rings r = 1, 2, ... of 8 r + 2 slots in the reference's order -- slots 0 ..
 * 2 r the top row y - r from column x - r to x + r; 2 r + 1 .. 4 r + 1 the left column x - r from row y - r to y + r;
 * 4 r + 2 .. 6 r + 1 the bottom row y + r from column x + r down to x - r + 1; 6 r + 2 .. 8 r + 1 the right column x + r
 * from row y + r down to y - r + 1.  A slot is a candidate if 0 < row < rows and 0 < col < cols (THE REFERENCE'S STRICT
 * > 0, KEPT: row 0 and column 0 never are) and its cell != ndata.  The search stops at the FIRST ring with a candidate
 * (kept too: the answer is the nearest cell of that ring, not of the raster).  dist = grt_circle_dist between the centres
 * (get_coord) of the starting cell and of the candidate in fp64; the winner is the candidate of least (dist, slot): an
 * exact tie goes to the earlier slot, which the reference's argsort does not define.  runner_up = the least dist of the
 * ring's candidates in ANOTHER cell than the winner's (+Inf if none): the device's sin / cos / asin are not numpy's, so the
 * caller decides a point again with numpy's when runner_up - dist <= TWXRV_TIE_REL x runner_up.
 * k_rv_ring: one wavefront per point.
 *
 * row, col [npts]            the start: 0 <= row < rows, 0 <= col < cols
 * value, dist, runner_up [npts]   out, float64 (kilometres)
 * ring, winner, status [npts]     out, int32: r, the winner's slot, TWXRV_OK or TWXRV_NO_DATA_ANYWHERE (value = ndata,
 *                            dist = runner_up = +Inf, ring 0, winner -1)
 * Call-level failures: as twxrv_sample's of the raster, npts < 1, a null buffer, a start outside the raster.
 */
int twxrv_nearest_data(int device, int64_t rows, int64_t cols, int32_t dtype, const void *data, const double *geo_t,
                       double ndata, int64_t npts, const int32_t *row, const int32_t *col, double *value, double *dist,
                       int32_t *ring, int32_t *winner, double *runner_up, int32_t *status, float *kernel_ms, char *errbuf,
                       int errlen);

/*
 * The location classes of find_dup_stns.  grt_circle_dist(a, b) == 0 exactly when lat_a F == lat_b F and lon_a F == lon_b F
 * in fp64, F = 0.017453292519943295: the squares and the sum of non-negative terms cannot cancel and the asin of a
 * non-zero argument is non-zero (coordinates within 1e-150 of each other AND of 0, where the square underflows, excepted).
 * Raw coordinates one ulp apart can have equal products, so the products are what is compared: one multiplication, no
 * transcendental, bit-exact under -ffp-contract=off.  cls[i] = the smallest j whose key equals i's, size[i] = the number of
 * such j.  A NaN coordinate equals nothing: cls[i] = i, size[i] = 1.
 * k_rv_dup: all pairs, the keys of 256 stations a tile through LDS.
 *
 * lon, lat [nstn]            1 <= nstn <= TWXRV_MAX_DUP_STNS
 * cls [nstn], size [nstn]    out, int32
 */
int twxrv_dup_classes(int device, int64_t nstn, const double *lon, const double *lat, int32_t *cls, int32_t *size,
                      float *kernel_ms, char *errbuf, int errlen);

/*
 * Column counts of a variable in the file's own layout, [ndays][nstn] with the station fastest (no transpose is taken).
 *   TWXRV_COUNT_I8_SUM        data int8 (flag_infilled): out[i] = the sum over the days of column cols[i] that do not equal
 *                             fill (netCDF4 masks them and numpy's sum skips a masked day); a NaN fill: every day counts
 *   TWXRV_COUNT_F32_MISSING   data float32: out[i] = the number of days of column cols[i] that are non-finite or equal fill
 * cols may repeat and need not be sorted; null with ncol = nstn: every column in order.  ncol = 0 returns at once.
 * Integer results: exact in any order, two calls give the same bytes whatever workspace_bytes.
 *
 * workspace_bytes            <= 0: TWXSC_WORKSPACE_BYTES; a batch is a run of days whose rows fit, at least one
 * out [ncol]                 int32
 * counts (optional) [2]      out: kernel launches, batches
 * Call-level failures: ndays < 1 or > TWXSC_MAX_DAYS, nstn < 1, an unknown kind, an int8 fill that is neither NaN nor an
 * integer in -128 .. 127, ncol < 0, no list and ncol != nstn, a null buffer, a column outside 0 .. nstn - 1.
 */
int twxrv_col_count(int device, int64_t ndays, int64_t nstn, int32_t kind, const void *data, float fill, int64_t ncol,
                    const int32_t *cols, int64_t workspace_bytes, int32_t *out, int32_t *counts, float *kernel_ms,
                    char *errbuf, int errlen);

/* ---- the quality assurance of daily precipitation (twx/qa/qa_prcp.py, Durre et al. 2010): the non-spatial chain
 * run_qa_non_spatial (:135-176) and the two checks the reference defines but leaves commented out of it, _qa_streak
 * (:379-407) and _qa_frequent (:409-445); twx_prcpqa.hip.  The spatial corroboration check that completes run_qa_all and
 * run_qa_spatial_only is twxpc_spatial_corrob below; out of scope: _qa_yr_clim_outlier.  These entries have no per-item status: every failure is call-level (a number after
 * TWXRV_NO_DATA_ANYWHERE = 38 is the next free one). ---- */
#define TWXPQ_PCTILE_ROWS 366           /* the dates of 2004 (DATES_366) */
#define TWXPQ_PCTILE_COLS 5             /* the 30th, 50th, 70th, 90th and 95th percentile */
#define TWXPQ_MIN_PERCENTILE_VALUES 20  /* MIN_PERCENTILE_VALUES: a row with fewer values is NaN */
/* Values of one row of the percentile table: the values > 0 on 29 month-days over all years, sorted in LDS by one
 * workgroup.  4096 float32 are 16 KiB: 8 workgroups of 4 waves fill a compute unit's 32 wave slots with 128 KiB of its
 * 160 KiB.  29 per year: 141 years.  A longer series fails the call, never a truncated window.  (The chain's gap check
 * sorts 31 slots per year under TWXQA_MAX_GAP_VALUES: 132 years, the cap a chain call meets first.) */
#define TWXPQ_MAX_WINDOW_VALUES 4096
#define TWXPQ_NKERNELS 7                /* kernel groups timed by twxpq_non_spatial */

/*
 * run_qa_non_spatial(prcp, tavg, days) for nstn stations in one call; every station is checked on its own.  The checks run
 * in the reference's order, each on the series without the observations every earlier one flagged (_update_obs_flags:
 * flagged days become NaN, a number is written only where the flag is still 1); all decisions of one check are taken on
 * the same snapshot.  "Wet" below: a finite value > 0 that is still in the series.  In execution order:
 *    2 missing: NaN.
 *    4 duplicate year: two years of the axis with >= 3 wet values each whose first min(len, len) days on the axis are all
 *   ==, by position (one NaN in the overlap: no duplicate).   6 duplicate months of one year, by position over the shorter,
 *   >= 3 wet values each; the month NUMBER equal to (distinct months on the axis) - 1 is never the first of a pair (the
 *   reference's loop, kept: on a 12-month axis November and December are never compared; on a March - September axis June
 *   is never the first).   5 the same calendar month of two years, likewise.
 *    8 impossible: < 0 or > 182.88f, compared in float32 (float32(182.88) itself is not flagged, its successor is).
 *    9 streak (only with streak != 0): on the sequence of wet values -- zeros and NaN are skipped and break no run -- every
 *   maximal run of >= 20 equal values that a different value ends; the last run of the series is never flagged (kept).
 *   19 frequent value (only with frequent != 0): for every start x of that sequence the window x .. x + 9 (shorter at the
 *   end) and every value v in it with c occurrences there: flagged when c >= 9 and v >= the 30th percentile of the row of
 *   each of its days, or c >= 8 against the 50th, c >= 7 against the 70th, c >= 5 against the 90th (the reference's elif
 *   chain: a tier with a NaN percentile or a smaller v falls through to the next); fp64 comparison; the table is that of
 *   15 below, built from the series as it stands at this point.
 *   10 gap: per calendar month over all years the sorted wet values; the first float32 difference of neighbours that is
 *   >= 30.0f gives the bound (the upper value) and every wet value of the month >= it is flagged.
 *   15 outlier: the table [366][5] of _build_percentiles: row r holds the five percentiles of all wet values whose
 *   month-day lies within 14 days of the r-th date of 2004 (29 month-days, wrapping over the year end; 29 February is in
 *   the windows of rows 45 .. 73 only), NaN below 20 values; numpy's linear interpolation in fp64 on the values widened
 *   exactly: virtual index (n - 1) q, g its fraction, a + (b - a) g below g = 0.5 and b - (b - a)(1 - g) from 0.5 on.  A wet
 *   value is flagged when (double)v >= m * p95[row], m = 5 where tavg < 0 (a NaN tavg: 9), row = yday - 1 of the day's OWN
 *   year (kept: from 1 March of a common year that is the row of the calendar day before).
 *
 * Deviation from the reference: numpy subtracts b - a in the series' own precision, so its table on a float32 series can
 * differ from this one by one float32 rounding of that difference (relative 6e-8 of the result).
 *
 * prcp, tavg [nstn][ndays]   station-major float32, NaN = missing (tavg may be all NaN); not modified
 * ymd [ndays]                consecutive calendar days, YYYYMMDD; need not start or end at a year boundary
 * streak, frequent           0: the reference's chain; non-zero: with check 9 / check 19
 * flag [nstn][ndays]         out: 1, 2, 4, 5, 6, 8, 9, 10, 15, 19
 * pctiles (optional) [nstn][366][5]   out: the table as check 15 used it
 * kernel_ms (optional) [TWXPQ_NKERNELS]   device time: missing; duplicates + impossible values; streaks; frequent values
 *                            with their table; gaps; the table; outliers (0 for a check that did not run)
 * Call-level failures: non-consecutive days; a series that touches more than TWXPQ_MAX_WINDOW_VALUES / 29 years or more
 * than TWXQA_MAX_GAP_VALUES / 31: the message names the macro; no device work is done.  Integer atomics only count or
 * take a minimum; no floating-point atomics: two calls give the same bytes.
 */
int twxpq_non_spatial(int device, int64_t nstn, int64_t ndays, const float *prcp, const float *tavg, const int32_t *ymd,
                      int32_t streak, int32_t frequent, uint8_t *flag, double *pctiles, float *kernel_ms, char *errbuf,
                      int errlen);

/*
 * _build_percentiles(vals, days, DATES_366) alone: the table above of every series as it is given (NaN = missing).
 * k_pq_pctiles: one workgroup per (station, row) compacts the window into LDS, sorts it there and reads five pairs of ranks.
 *
 * vals [nstn][ndays]         station-major float32
 * pctiles [nstn][366][5]     out
 * kernel_ms (optional) [1]   device time of the table
 * Call-level failures: non-consecutive days; more than TWXPQ_MAX_WINDOW_VALUES / 29 years.
 */
int twxpq_percentiles(int device, int64_t nstn, int64_t ndays, const float *vals, const int32_t *ymd, double *pctiles,
                      float *kernel_ms, char *errbuf, int errlen);

/* ---- the spatial corroboration check of the precipitation QA, _qa_spatial_corrob / _get_spatial_corrob_flag
 * (twx/qa/qa_prcp.py:614-664, 683-782; flag 17); twx_prcpcorrob.hip.  With it run_qa_spatial_only (:178-215: missing, then
 * this check) and run_qa_all (:87-133: the non-spatial chain, then this check) are complete.  Out of scope:
 * _qa_yr_clim_outlier, which the reference never calls.  Per-target statuses are the TWXQA_SP_* numbers of the temperature
 * checks. ---- */
#define TWXPC_NKERNELS 4                /* kernel groups timed by twxpc_spatial_corrob */

/*
 * _qa_spatial_corrob for ntarget stations of a pool in one call.  A target's series is "flags == 1 ? pool value : NaN" (what
 * the checks before left); a NEIGHBOUR's observations are the pool's values as they are.  The neighbours are the stations
 * within TWXQA_NGH_RADIUS_KM (75 km, k_radius_dist's arithmetic), self excluded, in ascending distance, equal distances in
 * table order; fewer than 3: nothing is flagged.  "pors" counts: a station has 366 rows, row r holds its finite values > 0
 * whose month-day lies within 14 days of the r-th date of 2004 (the windows of the percentile table above); a row has a
 * percentile basis when it holds MORE than TWXPQ_MIN_PERCENTILE_VALUES (20) values.  A target's rows come from its series,
 * a neighbour's from the pool.
 *
 * Day x is tested unless it is the first or last day of the axis or its value is NaN:
 *   1. on each of x - 1, x, x + 1 at least 3 neighbours (of all) have a finite observation, else no flag;
 *   2. of the first 7 finite observations of each of the three days in distance order (up to 21 values): a value above their
 *      maximum has abs_dif = value - max, one below their minimum abs_dif = min - value, any other is not flagged;
 *   3. thres = 26.924 cm unless the target's row yday(x) - 1 (of the day's OWN year: from 1 March of a common year the row
 *      of the calendar day before) has a basis AND on each of the three days at least 3 of the finite neighbours have a
 *      basis at that day's own row (31 December and 1 January use different rows).  Then
 *      pctile = scipy.stats.percentileofscore(target row, value), kind "rank": with left = #(a < v), right = #(a <= v),
 *      (left + right + (left < right)) * (50.0 / n); pctile_dif = the distance of pctile above the maximum or below the
 *      minimum of THE OBSERVATIONS IN CM OF ALL FINITE NEIGHBOURS ON THE THREE DAYS (the reference's line 760, kept: not
 *      capped at 7, not percentiles: a percentile is compared with centimetres; the neighbours' own percentiles are never
 *      used), 0 inside; thres = 26.924 if pctile_dif == 0, else (-45.72 * ln(pctile_dif) + 269.24) / 10 -- above 26.924
 *      where pctile_dif < 1;
 *   4. flagged (17) when abs_dif > thres.
 * All in fp64 on float32 values widened exactly; ln is the device library's (1 ulp).
 *
 * lon, lat [nstn]            degrees
 * prcp [nstn][ndays]         station-major float32, NaN = missing; not modified
 * ymd [ndays]                consecutive calendar days, YYYYMMDD
 * target_idx [ntarget]       rows of the pool
 * flags [ntarget][ndays]     in / out: 17 is written where the day is flagged and the flag is 1; nothing else changes
 * status (optional) [ntarget]   TWXQA_SP_OK, TWXQA_SP_FEW_NGHS (fewer than 3 within 75 km) or TWXQA_SP_NGH_CAP (more than
 *                            TWXQA_MAX_RADIUS_NGH: no flags)
 * abs_dif, pctile, thres (optional) [ntarget][ndays]   float64, NaN where the day did not reach step 2 / 3 (pctile is NaN
 *                            where thres is 26.924 for want of a basis)
 * kernel_ms (optional) [TWXPC_NKERNELS]   device time: neighbour lists; row counts; the walk; rank + threshold + flags
 * Call-level failures, before any device work: non-consecutive days; more than TWXPQ_MAX_WINDOW_VALUES / 29 years; a
 * target index outside 0 .. nstn - 1.  Integer atomics only count; no floating-point atomics: two calls give the same
 * bytes.
 */
int twxpc_spatial_corrob(int device, int64_t nstn, int64_t ndays, const double *lon, const double *lat, const float *prcp,
                         const int32_t *ymd, int64_t ntarget, const int32_t *target_idx, uint8_t *flags, int32_t *status,
                         double *abs_dif, double *pctile, double *thres, float *kernel_ms, char *errbuf, int errlen);

/*
 * The sizes of _build_pors' rows alone (:675-681): counts [nstn][366] uint16 of every series as it is given.
 * kernel_ms (optional) [1].  Call-level failures: non-consecutive days; more than TWXPQ_MAX_WINDOW_VALUES / 29 years.
 */
int twxpc_pors_counts(int device, int64_t nstn, int64_t ndays, const float *vals, const int32_t *ymd, uint16_t *counts,
                      float *kernel_ms, char *errbuf, int errlen);

/* ---- the GHCN-Daily ingest of step04: InsertGhcn.parse_stn_obs (twx/db/create_db_all_stations.py:1042-1103) for a batch
 * of .dly files, and create_tobs_db (twx/homog/tobs.py:121-157) for a batch of by-year CSV files; twx_ghcn.hip.  Both see
 * one byte buffer of files laid end to end: file_off [nfiles + 1] int64 from 0 to nbytes.  A last line without a newline is
 * a line; lines never span files.  Out of scope: InsertSnotel, downloading (InsertRaws: include/twx_raws.h; add_utc_offset: twxtz_*). ---- */
#define TWXGH_NKERNELS 4                /* kernel groups timed: fill; line index; claim pass; write pass */
#define TWXGH_MAX_BYTES ((int64_t)2147483584)   /* of one call's buffer: a line's position + 1 is a uint32 */
#define TWXGH_MAX_CELLS ((int64_t)1 << 31)      /* 3 nrows ndays of a .dly call, nstn nwin of a by-year call */
#define TWXGH_FB_WORDS 8                /* uint32 words of a fallback entry */
#define TWXGH_NO_BAD_HEADER 0xffffffffu
#define TWXGH_DC_LINES 0                /* counts of twxgh_parse_dly: entries of the line index (with the dropped ones) */
#define TWXGH_DC_VALUES 1               /*   day fields that gave a value (duplicates counted each time) */
#define TWXGH_DC_FALLBACK 2             /*   fields only Python's float() can decide (may exceed fallback_cap) */
#define TWXGH_DC_N 3
#define TWXGH_TC_VALUES 0               /* counts of twxgh_parse_tobs: lines that gave a value in the window */
#define TWXGH_TC_OUTSIDE 1              /*   selected lines of a known station whose date is no day of the period */
#define TWXGH_TC_OTHER_WINDOW 2         /*   ... whose date is a day of the period outside the window */
#define TWXGH_TC_BAD 3                  /*   ... whose date or value int() would not take as [+-]?digits (may exceed bad_cap) */
#define TWXGH_TC_N 4                    /* counts [TWXGH_TC_N + 1]: the last entry is the line index's size */

/*
 * parse_stn_obs of nfiles .dly files in one call.  File f writes row file_col[f] (distinct, 0 .. nrows - 1) of
 * val, qflag [3][nrows][ndays] (TMIN, TMAX, PRCP; float32 pre-set to -9999, uint8 pre-set to 0), ndays the days from
 * min_ymd to max_ymd.  Per line: int(line[11:15]), int(line[15:17]), line[17:21] one of the three elements (other lines
 * are skipped whole); per day field, in the reference's order: a valid date, inside the period, the value field
 * line[21 + 8 (d - 1) : 26 + 8 (d - 1)] clipped to the line's end.  A value is canonical if, stripped of Python's
 * whitespace, it is [+-]?[0-9]+: -9999 stays, PRCP is v / 100.0, temperatures v / 10.0 in fp64, rounded once to float32;
 * the flag is byte 27 + 8 (d - 1) if inside the line, whitespace = 0.  An empty value is skipped.  Any other text is listed:
 * fallback [fallback_cap][TWXGH_FB_WORDS] = file, line position in the file, line length, day field 0 .. 30, element, the
 * position + 1 in the buffer of the canonical line that won the field's (row, day, element) (0: none), the day's index,
 * the line's position in the buffer; sorted by position then day.  When several lines give a (day, element) the LAST one
 * whose field was not skipped wins (value and flag, -9999 included): integer atomicMax of the position, no result depends
 * on scheduling.  bad_header [nfiles]: the position in the file of the first line whose year or month is not canonical (an
 * empty line is one), TWXGH_NO_BAD_HEADER if none; such lines write nothing.  counts [TWXGH_DC_N].
 * kernel_ms (optional) [TWXGH_NKERNELS].  Every argument is checked before anything touches the device.
 */
int twxgh_parse_dly(int device, const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off,
                    const int32_t *file_col, int64_t nrows, int32_t min_ymd, int32_t max_ymd, int64_t ndays, float *val,
                    uint8_t *qflag, uint32_t *bad_header, uint32_t *fallback, int64_t fallback_cap, int64_t *counts,
                    float *kernel_ms, char *errbuf, int errlen);

/*
 * create_tobs_db on nfiles by-year CSV files (ID(11),YYYYMMDD(8),ELEM(4),value,m,q,s,HHMM), in buffer order.  The filter of
 * create_tobs_file (tobs.py:61-62) restated: the element field equals element (four characters), the id starts with US / CA
 * / MX, the last character is a digit, the line does not end in 2400.  ids [nstn][11]: the sorted station ids without
 * their GHCN_ prefix; an unknown station is skipped.  Day = int(line[12:20]); value = int() of the last five
 * characters of the line as grep prints it, newline included: the last four of its text.  tobs [nstn][nwin] int16, IN and OUT: the days win0 .. win0 + nwin - 1 of the period; only
 * the entries a line gives are changed, the last line winning as in twxgh_parse_dly.  One deviation: a date that is no day
 * of the period is skipped and counted (the reference dies with IndexError).  bad [bad_cap][2]: file and position of the
 * lines whose date or value is not [+-]?[0-9]+ or does not fit int16, sorted.  counts [TWXGH_TC_N + 1].
 */
int twxgh_parse_tobs(int device, const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off, int64_t nstn,
                     const uint8_t *ids, const char *element, int32_t min_ymd, int32_t max_ymd, int64_t win0, int64_t nwin,
                     int16_t *tobs, uint32_t *bad, int64_t bad_cap, int64_t *counts, float *kernel_ms, char *errbuf,
                     int errlen);

/* Page-locked host memory for the file buffer (NULL on failure), and its release. */
void *twxgh_host_alloc(int64_t nbytes);
void twxgh_host_free(void *p);

/* ---- the North American reanalysis subsets of step12: create_nnr_subset, create_nnr_subset_nolevel and
 * create_thickness_nnr_subset (twx/db/reanalysis.py:45-305) for every product of one raw variable in one call;
 * twx_nnrsub.hip.  Out of scope: downloading, deflate of the subsets (step13's time-zone lookup: twxtz_*). ---- */
#define TWXNS_NKERNELS 3                /* groups timed: upload; the subset kernels (one launch per product); download */
#define TWXNS_I16 0                     /* dtype of the raw slab: packed short */
#define TWXNS_F32 1                     /*   float */
#define TWXNS_TILED 0                   /* layout: chunk-major [cy][cx][day][lev][4][4], edge chunks padded with the fill */
#define TWXNS_PLAIN 1                   /*   [day][lev][lat][lon] */
#define TWXNS_CONV_NONE 0
#define TWXNS_CONV_K_TO_C 1             /* u - f32(273.15) */
#define TWXNS_KIND_LEVELS 0             /* a product of nlev_out >= 1 level indices */
#define TWXNS_KIND_THICK 1              /*   the difference of two levels: u[idx_up] - u[idx_low] */
#define TWXNS_FILL 9.969209968386869e36f   /* netCDF4.default_fillvals['f4'] */
#define TWXNS_MAX_LEV 32                /* level indices of a product (the reanalysis has 17 levels) */
#define TWXNS_MAX_PROD 64               /* products of a call */
#define TWXNS_MAX_DAYS (1 << 20)        /* days of the period (2870 years) */
#define TWXNS_MAX_SIDE 4096             /* nlat_out, nlon_out */
#define TWXNS_MAX_RAW ((int64_t)1 << 32)   /* values of the raw slab: 8 GiB of short, 16 GiB of float */
#define TWXNS_MAX_OUT ((int64_t)1 << 31)   /* values of one product, padding included: 8 GiB */
#define TWXNS_PD_SLOT 0                 /* words of a product descriptor: the slot, 0 / 1 / 2 = 12z / 18z / 24z */
#define TWXNS_PD_KIND 1                 /*   TWXNS_KIND_* */
#define TWXNS_PD_CONV 2                 /*   TWXNS_CONV_* */
#define TWXNS_PD_NLEV 3                 /*   nlev_out of TWXNS_KIND_LEVELS (ignored for a thickness: its output has one level) */
#define TWXNS_PD_LEV0 4                 /*   the level indices from here on; a thickness: idx_up, idx_low */
#define TWXNS_PD_WORDS (TWXNS_PD_LEV0 + TWXNS_MAX_LEV)
#define TWXNS_C_DAYS 0                  /* counts of a product: days that received a record */
#define TWXNS_C_MARKED 1                /*   values written as fill because a raw datum equalled a mark */
#define TWXNS_C_UNWRITTEN 2             /*   days of the period left unwritten (all fill) */
#define TWXNS_C_N 3

/*
 * All years of one raw variable, every product made of it.  Stateless.
 * raw [nrec][nl][ny][nx]     int16 (TWXNS_I16) or float32 (TWXNS_F32); nl = 1 for a variable without levels.  The caller may
 *                            have cut the slab to the levels and rows in use: the entry only sees index lists.
 * scale, offset              u = f32(f32(x) * scale) + offset, two roundings.  scale 1 with offset 0 leaves the datum as it
 *                            is (a float -0 stays -0): what to pass for a variable without packing attributes.
 * marks [2], has_mark [2]    missing_value and _FillValue in the raw dtype, and whether each exists.  A datum that EQUALS a
 *                            present mark (floats by value: NaN equals nothing) gives the fill; a thickness is fill if either
 *                            level is marked.
 * rec_slot, rec_day [nrec]   0 / 1 / 2 or -1 (a record nobody uses); the output day 0 .. ndays - 1 or -1 (outside the period)
 * lat_idx [nlat_out], lon_idx [nlon_out]   raw rows / columns of the output's; any order, repeats allowed
 * prod [nprod][TWXNS_PD_WORDS]   the product descriptors (TWXNS_PD_*); Kelvin to Celsius is u - f32(273.15), after the
 *                            difference of a thickness
 * out [nprod]                host buffers of float32: TWXNS_TILED ceil(nlat_out / 4) ceil(nlon_out / 4) ndays nlev 16 values,
 *                            TWXNS_PLAIN ndays nlev nlat_out nlon_out.  A day without a record is TWXNS_FILL, and so is the
 *                            padding of an edge chunk: every byte is determined.
 * counts [nprod][TWXNS_C_N]  int64
 * kernel_ms (optional) [TWXNS_NKERNELS]
 * Every output element is written by exactly one thread; the only atomics are integer additions to the mark counts: two
 * calls give the same bytes.  Every argument is checked before anything touches the device: a dtype or layout flag, sizes
 * beyond the TWXNS_MAX_* limits, an index outside the slab, nlev_out < 1, a thickness of one level twice, and two records
 * that map to the same (slot, day) -- refused, naming both.
 */
int twxns_subset(int device, int dtype, const void *raw, int64_t nrec, int64_t nl, int64_t ny, int64_t nx, float scale,
                 float offset, const void *marks, const int32_t *has_mark, const int32_t *rec_slot, const int32_t *rec_day,
                 int64_t ndays, int64_t nlat_out, const int32_t *lat_idx, int64_t nlon_out, const int32_t *lon_idx,
                 int64_t nprod, const int32_t *prod, int layout, float *const *out, int64_t *counts, float *kernel_ms,
                 char *errbuf, int errlen);

/* ---- step13's time-zone lookup: add_utc_offset over UtcOffset (twx/db/create_db_all_stations.py:1333-1383,
 * twx/db/stn_utc_offsets.py:43-117), tzwhere's tzNameAt(lat, lon, forceTZ=True) restated: the first polygon that contains
 * the point, otherwise the nearest; twx_tzpoly.hip, the predicates in twx_tzpoly_pred.h.  Out of scope: the zone names and
 * their offsets (Python), the Geonames client. ---- */
#define TWXTZ_NPHASES 5                 /* groups timed */
#define TWXTZ_T_UPLOAD 0
#define TWXTZ_T_CANDIDATES 1            /*   count, the host's scan, scatter */
#define TWXTZ_T_CONTAIN 2               /*   containment and the pick */
#define TWXTZ_T_FORCED 3
#define TWXTZ_T_DOWNLOAD 4
#define TWXTZ_INSIDE 0                  /* status of a point: poly contains it (the lowest index that does) */
#define TWXTZ_FORCED 1                  /*   nothing contains it; poly is the nearest within max_force_deg */
#define TWXTZ_NONE 2                    /*   nothing contains it and nothing lies within max_force_deg; poly = -1 */
#define TWXTZ_BAD_POINT 3               /*   lon or lat is not finite; poly = -1, no device work */
#define TWXTZ_UNCERTAIN 4               /*   float64 could not decide it: the uncertain list says what to decide again */
#define TWXTZ_PENDING 5                 /*   internal: waits for the forced search; never returned */
#define TWXTZ_OVERFLOW 1                /* return value: the uncertain list was too small; counts say how many it needs */
#define TWXTZ_CHUNK_EDGES 2048          /* edges of one work item of the containment kernel */
#define TWXTZ_MAX_POINTS (1 << 30)
#define TWXTZ_MAX_POLY (1 << 24)
#define TWXTZ_MAX_EDGES ((int64_t)1 << 31)
#define TWXTZ_MAX_ITEMS ((int64_t)1 << 31)     /* (pair, chunk) items of a call */
#define TWXTZ_MAX_UNCERTAIN ((int64_t)1 << 28)
#define TWXTZ_C_PAIRS 0                 /* counts: (point, polygon) pairs whose bbox holds the point */
#define TWXTZ_C_ITEMS 1                 /*   work items they made */
#define TWXTZ_C_PENDING 2               /*   points that went to the forced search */
#define TWXTZ_C_UNCERTAIN 3             /*   entries the uncertain list needs */
#define TWXTZ_C_N 4

/*
 * One call for all points.  Stateless.
 * lon, lat [npt]              float64 degrees, as written: nothing wraps at +-180
 * edge_off [npoly + 1]        int64, ascending from 0: polygon p owns edges edge_off[p] .. edge_off[p + 1] - 1 (all its rings;
 *                             the even-odd rule over them makes the holes)
 * bbox [npoly][4]             xmin, ymin, xmax, ymax, closed
 * edges [nedge][4]            x1, y1, x2, y2, none of zero length
 * max_force_deg               a point that nothing contains takes the nearest polygon if sqrt(d2) <= max_force_deg (infinity:
 *                             always); d2 is the squared distance in degrees to the nearest edge, (d2, polygon) lexicographic
 * poly, status [npt] int32, dist2 [npt] float64 (0 unless forced; of TWXTZ_NONE the distance found)
 * uncertain [uncertain_cap][2]  int32 (point, polygon) sorted: pairs whose crossing parity float64 cannot certify (Shewchuk's
 *                             static filter of orient2d) and that lie below the point's first inside polygon; (point, -1): a forced
 *                             point with a second polygon within a relative 2^-40 of the nearest, an ill-conditioned distance,
 *                             or a distance that close to max_force_deg.  Their points carry TWXTZ_UNCERTAIN and a provisional
 *                             poly; the caller decides them exactly.
 * counts [TWXTZ_C_N] int64; timing_ms (optional) [TWXTZ_NPHASES]
 * Returns 0, TWXTZ_OVERFLOW (everything but the list is valid; call again with counts[TWXTZ_C_UNCERTAIN] entries), or -1
 * with errbuf.  Integer atomics only (XOR / OR of a pair's parity word, the list's counter); the list is sorted before it is
 * returned: two calls give the same bytes.  Every argument is checked before anything touches the device.
 */
int twxtz_locate(int device, int64_t npt, const double *lon, const double *lat, int64_t npoly, const int64_t *edge_off,
                 const double *bbox, const double *edges, double max_force_deg, int32_t *poly, int32_t *status, double *dist2,
                 int32_t *uncertain, int64_t uncertain_cap, int64_t *counts, float *timing_ms, char *errbuf, int errlen);

/* ---- step26 / step27: the daily and monthly mosaics with their chunks deflated on the device (twx_mosaic.hip; the host
 * arithmetic in twx_mosaic_host.h).  TileMosaic.create_dly_ann_mosaics (twx/interp/tiling.py:567-780) and write_ds_mthly
 * (:1169-1219) store int16 variables with zlib=True in chunks (1, 325, 700) (tiling.py:718-720, 892-894, 1035): THESE are the
 * files the reference deflates -- the daily and normals mosaics and the monthly files.  Its tile files are NOT deflated
 * (tiling.py:442-444).  A year of the mosaic is assembled in device memory from tile slabs, deflated there into one zlib stream
 * per (day, chunk row, chunk column) that H5Dwrite_chunk appends as it is, and the monthly means come from the same resident
 * year.
 *
 * The streams are those of topowx_amd/csrc/twx_deflate.h for a chunk whose time extent is one day: 78 01; the low bytes of the
 * N = chunk_y * chunk_x values, element order (row, column), in ceil(N / 65535) stored blocks; the high bytes in
 * dynamic-Huffman blocks of 16 384 input bytes, or stored where that is shorter; 01 00 00 FF FF; Adler-32 of the shuffled
 * chunk.  ONE Huffman code per twxmo_deflate call, from the tokens of the first block of every chunk of every day of the call.
 * oracle/deflate_oracle.py restates them byte for byte: the image [nd][Yp][Xp] as one layer of nd * Yp rows is a tile of
 * (1, chunk_y, chunk_x) chunks.  Out of scope: inflating, a time extent other than 1, the normals mosaic. ---- */
typedef struct twxmo_mosaic twxmo_mosaic;
#define TWXMO_DAILY 0                   /* which image: int16 [max_days][Yp][Xp] */
#define TWXMO_MONTHLY 1                 /*   int16 [12][Yp][Xp], written by twxmo_monthly */
#define TWXMO_NGROUPS 7                 /* kernel groups timed */
#define TWXMO_T_CLEAR 0
#define TWXMO_T_PLACE 1                 /*   summed over the twxmo_place calls since the last twxmo_clear */
#define TWXMO_T_HIST 2                  /*   token counts and the Huffman code */
#define TWXMO_T_COUNT 3                 /*   block sizes, low planes, the per-chunk scan */
#define TWXMO_T_EMIT 4
#define TWXMO_T_COMPACT 5
#define TWXMO_T_AGGREGATE 6
#define TWXMO_S_YP 0                    /* twxmo_sizes: Y, X rounded up to whole chunks */
#define TWXMO_S_XP 1
#define TWXMO_S_NCHUNK 2                /*   chunks per layer */
#define TWXMO_S_NSEG 3                  /*   high-plane blocks per chunk */
#define TWXMO_S_SLOT_BYTES 4            /*   the longest stream of a chunk, rounded to 256 */
#define TWXMO_S_DEVICE_BYTES 5          /*   device memory twxmo_create allocates (images, slots, workspace) */
#define TWXMO_S_PINNED_BYTES 6          /*   pinned host memory twxmo_create allocates */
#define TWXMO_S_VEC 7                   /*   2: chunk_x and Xp even, the coder loads two values at once; else 1 */
#define TWXMO_S_N 8

typedef struct twxmo_streams {
    const uint8_t *data;                /* the streams one after the other (pinned; valid until the next twxmo_deflate) */
    const int64_t *offset;              /* [nstreams + 1] byte offsets into data */
    int64_t nstreams;                   /* layers * nchunk, in (layer, chunk row, chunk column) order */
    int64_t slot_bytes;                 /* no stream is longer */
    int32_t nchunk, chunk_y, chunk_x, reserved;
} twxmo_streams;

/* The sizes of an object with these arguments, without a device: sizes [TWXMO_S_N].  -1 with errbuf when the arguments are
 * refused: max_days < 1, a chunk larger than the mosaic, a slot of 2^32 bytes or more, more chunks than a grid's x dimension. */
int twxmo_sizes(int64_t max_days, int32_t Y, int32_t X, int32_t chunk_y, int32_t chunk_x, int64_t *sizes, char *errbuf, int errlen);

/* Allocates the images, max(max_days, 12) * nchunk slots and the coder's workspace on `device`.  Refuses, naming both numbers,
 * when hipMemGetInfo says that it does not fit: the caller asks for fewer days.  The arguments are checked first. */
int twxmo_create(int device, int64_t max_days, int32_t Y, int32_t X, int32_t chunk_y, int32_t chunk_x, twxmo_mosaic **out,
                 char *errbuf, int errlen);
void twxmo_destroy(twxmo_mosaic *m);
const char *twxmo_last_error(const twxmo_mosaic *m);

/* Every later call returns 0 or -1 (twxmo_last_error has the text) and checks its arguments before it touches the device.
 * twxmo_clear: layers 0 .. ndays - 1 of the daily image, padding included, hold TWX_FILL_I2; the timings start again. */
int twxmo_clear(twxmo_mosaic *m, int64_t ndays);

/* src int16 [nd][ty][tx] (host) is written at row y0, column x0 of layers 0 .. nd - 1.  A slab with any part outside Y x X (the
 * padding is outside) is refused, not clipped.  Slabs are placed in call order: where two overlap, the later one wins.  The
 * call returns once src has been copied to a staging buffer; the upload of the next slab runs under this one's placement.
 * twxmo_staging hands out the staging buffer the NEXT twxmo_place will use (at least `bytes` long), so that a reader can fill
 * it in place: pass that pointer as src. */
int twxmo_place(twxmo_mosaic *m, const int16_t *src, int64_t nd, int32_t ty, int32_t tx, int32_t y0, int32_t x0);
int twxmo_staging(twxmo_mosaic *m, int64_t bytes, void **ptr);

/* The twelve monthly means of layers 0 .. ndays - 1 (day_month [ndays], 1..12) into the monthly image: twx_aggregate's kernel
 * and its mthly_i16 output (np.ma.round(mean, 2) packed with scale_factor float32(0.01); a month without valid days is
 * TWX_FILL_I2) on ncell = Yp * Xp. */
int twxmo_monthly(twxmo_mosaic *m, int64_t ndays, const int32_t *day_month);

/* Deflates layers 0 .. nlayers - 1 of image `which` (TWXMO_MONTHLY: nlayers <= 12).  Synchronous. */
int twxmo_deflate(twxmo_mosaic *m, int which, int64_t nlayers, twxmo_streams *out);

/* Debug / tests: layers 0 .. nlayers - 1 of image `which`, padded, int16 [nlayers][Yp][Xp]. */
int twxmo_download(twxmo_mosaic *m, int which, int64_t nlayers, int16_t *dst);

/* kernel_ms [TWXMO_NGROUPS] (HIP events; synchronises; every group summed over its runs since the last twxmo_clear), the device and the
 * pinned host bytes the object holds now.  Any pointer may be NULL. */
int twxmo_timing(twxmo_mosaic *m, float *kernel_ms, int64_t *device_bytes, int64_t *pinned_bytes);

#ifdef __cplusplus
}
#endif
#endif
