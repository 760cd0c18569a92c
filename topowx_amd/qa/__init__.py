"""Station quality checks that run before the interpolation stages (libtwxqa.so, include/twx_qa.h).

``qa_temp`` holds step08's spatial regression check of the daily Tmin / Tmax observations; the kernel sources of the
library (``twx_outlier.hip``, ``twx_spatial.hip``) live next to it.
"""
from .qa_temp import (MAX_NGHS, MIN_DAYS_MTH_WINDOW, MIN_NGHS, NGH_CORR, NGH_RADIUS, NGH_RESID_CUTOFF,
                      NGH_RESID_STD_CUTOFF, QA_MISSING, QA_OK, QA_SPATIAL_REGRESS, TWX_TO_GHCN_FLAGS_MAP, StationObsPool,
                      qa_spatial_regress)

__all__ = ["StationObsPool", "qa_spatial_regress", "QA_OK", "QA_MISSING", "QA_SPATIAL_REGRESS", "NGH_RADIUS", "NGH_CORR",
           "NGH_RESID_CUTOFF", "NGH_RESID_STD_CUTOFF", "MIN_DAYS_MTH_WINDOW", "MIN_NGHS", "MAX_NGHS",
           "TWX_TO_GHCN_FLAGS_MAP"]
