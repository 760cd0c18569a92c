"""topowx_amd: MI355X-native moving-window regression-kriging / GWR interpolator.

Drop-in for the ``twx.interp`` hot path of jaredwo/topowx.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "NNRNghData":                 # the reanalysis reader (topowx_amd.reanalysis), imported at first use
        from .reanalysis import NNRNghData
        return NNRNghData
    if name in ("UtcOffset", "add_utc_offset", "load_tz_polygons"):     # step13's time-zone lookup (topowx_amd.utc_offsets)
        from . import utc_offsets
        return getattr(utc_offsets, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
