"""The infill family of the reference (``twx.infill``: step14 / step15 / step16) on the GPU.  So far: the neighbour
matrices every infill worker starts from (``infill_matrix``; libtwxqa.so's ``twxif_infill_matrix``, kernel source
``topowx_amd/qa/twx_infillmat.hip``) and step14's estimate of mean and variance from them (``infill_normals``;
``twxem_mean_variance``, ``topowx_amd/qa/twx_emnorm.hip``), and step16's daily infill: the batched PPCA of the matrices
with its component search (``infill_daily``; ``twxpp_ppca_fit``, ``topowx_amd/qa/twx_ppca.hip``) and, with ``chk_perf``, the
reference's check of every fit and its retry ladder (``RetryLadder``; ``twxck_infill_check``,
``topowx_amd/qa/twx_infillchk.hip``); and step15's cross-validation of that chain (``xval_infill``: ``XvalInfill``;
``twxxv_holdout`` / ``twxxv_infill_matrix`` / ``twxxv_score``, ``topowx_amd/qa/twx_xvalinfill.hip``); and what follows the
infill (``post_infill``: the infilled database, step17's check of whole series and step18's serially-complete database
with its monthly normals; ``twxsc_serial_complete`` / ``twxsc_series_check``, ``topowx_amd/qa/twx_serial.hip``; step19's
raster values at the stations and step20's duplicate stations; ``twxrv_*``, ``topowx_amd/qa/twx_stnrast.hip``).
"""
from .infill_daily import (PP_STATUS, InfillDaily, PcSearch, RetryLadder, add_npcs, assemble_daily_columns, daily_items, first_npcs,
                           infill_daily, infill_daily_obs, item_matrix)
from .infill_matrix import (ITEM_STATUS, MAX_COLS_NORM_IMPUTE, MAX_DISTANCE, MIN_DAILY_NGHBRS, MIN_POR_OVERLAP, InfillMatrices,
                            InfillMatrix, build_infill_matrices, item_thresholds)
from .infill_normals import (EM_STATUS, NNGH_NNR, InfillEstimates, assemble_columns, estimate_mean_variance,
                             infill_mean_variance, nnr_components)
from .post_infill import (SERIAL_DB_VARIABLES, USE_ALL_INFILL_THRESHOLD, SerialComplete, add_monthly_normals,
                          add_stn_raster_values, create_serially_complete_db, find_bad_infill_stns, find_dup_stns,
                          get_bad_infill_stnids, suspect_infill_stnids, write_bad_stns_csv, write_infill_db)
from .xval_infill import XvalInfill, XvalInfillParams, XvalInfillResult

__all__ = ["build_infill_matrices", "InfillMatrices", "InfillMatrix", "item_thresholds", "ITEM_STATUS", "MAX_DISTANCE",
           "MIN_POR_OVERLAP", "MIN_DAILY_NGHBRS", "MAX_COLS_NORM_IMPUTE", "assemble_columns", "nnr_components",
           "estimate_mean_variance", "infill_mean_variance", "InfillEstimates", "EM_STATUS", "NNGH_NNR", "infill_daily",
           "infill_daily_obs", "InfillDaily", "PcSearch", "assemble_daily_columns", "daily_items", "item_matrix", "first_npcs",
           "add_npcs", "PP_STATUS", "RetryLadder", "XvalInfill", "XvalInfillParams", "XvalInfillResult", "write_infill_db",
           "get_bad_infill_stnids", "suspect_infill_stnids", "find_bad_infill_stns", "write_bad_stns_csv",
           "create_serially_complete_db", "add_monthly_normals", "SerialComplete", "SERIAL_DB_VARIABLES",
           "USE_ALL_INFILL_THRESHOLD", "add_stn_raster_values", "find_dup_stns"]
