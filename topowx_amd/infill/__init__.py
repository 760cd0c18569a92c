"""The infill family of the reference (``twx.infill``: step14 / step15 / step16) on the GPU.  So far: the neighbour
matrices every infill worker starts from (``infill_matrix``; libtwxqa.so's ``twxif_infill_matrix``, kernel source
``topowx_amd/qa/twx_infillmat.hip``).  The estimators that consume the matrix are not part of it yet.
"""
from .infill_matrix import (ITEM_STATUS, MAX_COLS_NORM_IMPUTE, MAX_DISTANCE, MIN_DAILY_NGHBRS, MIN_POR_OVERLAP, InfillMatrices,
                            InfillMatrix, build_infill_matrices, item_thresholds)

__all__ = ["build_infill_matrices", "InfillMatrices", "InfillMatrix", "item_thresholds", "ITEM_STATUS", "MAX_DISTANCE",
           "MIN_POR_OVERLAP", "MIN_DAILY_NGHBRS", "MAX_COLS_NORM_IMPUTE"]
