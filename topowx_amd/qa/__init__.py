"""Station quality checks that run before the interpolation stages (libtwxqa.so, include/twx_qa.h).

``qa_temp`` holds step08's checks of the daily Tmin / Tmax observations: the non-spatial chain of its first run and
the spatial checks of its second (regression, corroboration, mega-inconsistency); the kernel sources of the library
(``twx_outlier.hip``, ``twx_spatial.hip``, ``twx_corrob.hip``, ``twx_nonspatial.hip``) live next to it.
"""
from .qa_temp import (ANOMALY_CUTOFF, GHCN_TO_TWX_FLAGS_MAP, MAX_NGHS, MIN_DAYS_MTH_WINDOW, MIN_NGHS, MIN_NORM_VALUES,
                      NGH_CORR, NGH_RADIUS, NGH_RESID_CUTOFF, NGH_RESID_STD_CUTOFF, NON_SPATIAL_FLAGS, QA_CLIM_OUTLIER,
                      QA_DUP_MONTH, QA_DUP_WITHIN_MONTH, QA_DUP_YEAR, QA_DUP_YEAR_MONTH, QA_GAP, QA_IMPOSS_VALUE,
                      QA_INTERNAL_INCONSIST, QA_LAGRANGE_INCONSIST, QA_MEGA_INCONSIST, QA_MISSING, QA_NAUGHT, QA_OK,
                      QA_SPATIAL_CORROB, QA_SPATIAL_REGRESS, QA_SPIKE_DIP, QA_STREAK, TWX_TO_GHCN_FLAGS_MAP, StationObsPool,
                      doy_norms, qa_spatial_regress, run_qa_non_spatial, run_qa_spatial_only)

__all__ = ["StationObsPool", "qa_spatial_regress", "run_qa_spatial_only", "doy_norms", "QA_OK", "QA_MISSING",
           "QA_SPATIAL_REGRESS", "QA_SPATIAL_CORROB", "QA_MEGA_INCONSIST", "NGH_RADIUS", "NGH_CORR", "NGH_RESID_CUTOFF",
           "NGH_RESID_STD_CUTOFF", "MIN_DAYS_MTH_WINDOW", "MIN_NGHS", "MAX_NGHS", "ANOMALY_CUTOFF", "MIN_NORM_VALUES",
           "TWX_TO_GHCN_FLAGS_MAP", "GHCN_TO_TWX_FLAGS_MAP", "run_qa_non_spatial", "NON_SPATIAL_FLAGS", "QA_NAUGHT",
           "QA_DUP_YEAR", "QA_DUP_MONTH", "QA_DUP_YEAR_MONTH", "QA_DUP_WITHIN_MONTH", "QA_IMPOSS_VALUE", "QA_STREAK", "QA_GAP",
           "QA_INTERNAL_INCONSIST", "QA_LAGRANGE_INCONSIST", "QA_SPIKE_DIP", "QA_CLIM_OUTLIER"]
