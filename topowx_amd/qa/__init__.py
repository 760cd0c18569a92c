"""Station quality checks that run before the interpolation stages (libtwxqa.so, include/twx_qa.h).

``qa_temp`` holds step08's checks of the daily Tmin / Tmax observations: the non-spatial chain of its first run and
the spatial checks of its second (regression, corroboration, mega-inconsistency); the kernel sources of the library
(``twx_outlier.hip``, ``twx_spatial.hip``, ``twx_corrob.hip``, ``twx_nonspatial.hip``) live next to it.

``qa_prcp`` holds the non-spatial chain of the precipitation QA (``twx_prcpqa.hip``).  Its ``run_qa_non_spatial`` shares
its name with the temperature one, as in the reference: call it as ``qa_prcp.run_qa_non_spatial`` or by the alias
``run_qa_non_spatial_prcp``; the names that do not collide are re-exported here.
"""
from . import qa_prcp
from .qa_prcp import (GAP_THRES, MIN_PERCENTILE_VALUES, PRCP_GHCN_TO_TWX_FLAGS_MAP, PRCP_MAX_VALUE, PRCP_MIN_VALUE,
                      PRCP_NON_SPATIAL_FLAGS, PRCP_TWX_TO_GHCN_FLAGS_MAP, QA_FREQUENT, QA_YR_CLIM_OUTLIER, STREAK_LEN,
                      PrcpObsPool, build_percentiles, load_prcp_pool)
from .qa_prcp import run_qa_non_spatial as run_qa_non_spatial_prcp
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
           "QA_INTERNAL_INCONSIST", "QA_LAGRANGE_INCONSIST", "QA_SPIKE_DIP", "QA_CLIM_OUTLIER",
           "qa_prcp", "run_qa_non_spatial_prcp", "build_percentiles", "load_prcp_pool", "PrcpObsPool", "PRCP_NON_SPATIAL_FLAGS",
           "QA_FREQUENT", "QA_YR_CLIM_OUTLIER", "PRCP_MIN_VALUE", "PRCP_MAX_VALUE", "STREAK_LEN", "GAP_THRES",
           "MIN_PERCENTILE_VALUES", "PRCP_TWX_TO_GHCN_FLAGS_MAP", "PRCP_GHCN_TO_TWX_FLAGS_MAP"]
