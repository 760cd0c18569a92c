"""The homogenisation family of the reference (``twx.homog``: step09 / step11) around the external PHA program: the
time-of-observation shift of Tmax (``tobs``; libtwxqa.so's ``twxhm_tobs_shift``), the text files PHA reads and writes and the
daily homogenisation from its monthly output (``pha``; ``twxhm_homog_daily``), kernel source ``topowx_amd/qa/twx_homog.hip``.
PHA itself is not part of this package: it is unpacked, built and run by hand between ``step11 --setup`` and ``--apply``.
"""
from .pha import (HomogDaily, create_homog_db, format_stnid, get_pha_adj_csv, load_input_not_stnlist, parse_pha_adj, pha_paths,
                  read_pha_monthly, write_input_station_data, write_metadata_file, write_stn_list, write_stn_obs_files)
from .tobs import create_tobs_adjusted_db, tobs_shift_tmax

__all__ = ["tobs_shift_tmax", "create_tobs_adjusted_db", "HomogDaily", "create_homog_db", "format_stnid", "write_stn_list",
           "write_stn_obs_files", "write_metadata_file", "write_input_station_data", "parse_pha_adj", "read_pha_monthly",
           "load_input_not_stnlist", "get_pha_adj_csv", "pha_paths"]
