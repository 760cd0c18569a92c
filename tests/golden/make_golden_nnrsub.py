"""Generate tests/golden/golden_nnrsub_v1.npz by EXECUTING the year loops of the reference's three subset functions on the
seeded yearly files of tests/nnrsub_cases.py, for the 21 products of step12.  Needs the reference checkout
(``make_golden.REF``); the tests only read the fixture.

    python tests/golden/make_golden_nnrsub.py

Executed (read at run time, nothing of the text is stored), each under a function header of ours:
  * twx/db/reanalysis.py:37 and :41-42 (``UTC_TIMES``, the bounds);
  * :83-92 and :102-129 (``create_nnr_subset``: the masks, the year loop without its ``print``);
  * :171-179 and :189-216 (``create_nnr_subset_nolevel``);
  * :253-265 and :274-303 (``create_thickness_nnr_subset``);
  * scripts/step12_process_reanalysis_data.py:40 (``k_to_c``), for the assertion below.
They run on stand-ins of ours for ``Dataset``, ``num2date``, ``get_ymd_array``, ``A_DAY`` and ``ds_out``: neither netCDF4
nor cftime is installed here.  The ``Dataset`` stand-in does what netCDF4-python does to a variable: orthogonal indexing
with boolean masks and integers, a masked array whose mask is set where a stored value equals ``missing_value`` or
``_FillValue``, and ``data * scale_factor + add_offset`` with float32 attribute scalars.  The ``ds_out`` stand-in writes
the fill under a mask and counts days and masked values.

The np.ma trap (measured on numpy 2.2.6): ``masked_float32_array - 273.15`` comes back float64, where a plain float32 array
stays float32 -- as both kinds did under the reference's numpy 1.x, the result the subsets in use were made with.  So the
maker passes ``lambda k: k - np.float32(273.15)`` as ``conv_func`` and asserts that step12's own lambda (executed) gives
the same bits on the unmasked arrays.

The fixture holds, per product: the sha256 of the executed array, its three counts (days written, values masked, days left
unwritten), a few hundred sampled values with their flat indices, its shape; and the checksum of the inputs.
"""
import datetime as dt
import hashlib
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nnrsub_cases as NC  # noqa: E402

OUT = os.path.join(HERE, "golden_nnrsub_v1.npz")
NSAMPLE = 300


class _RawVar(object):
    """A packed variable as netCDF4-python presents it (auto mask and scale on)."""

    def __init__(self, a, pack, marks):
        self.a, self.pack, self.marks = a, pack, marks

    def __getitem__(self, key):
        a = self.a
        for ax in reversed(range(len(key))):                      # orthogonal: each axis on its own
            k = key[ax]
            if isinstance(k, (int, np.integer)):
                a = np.take(a, int(k), axis=ax)
            elif isinstance(k, slice):
                a = a[(slice(None),) * ax + (k,)]
            else:
                a = np.compress(np.asarray(k, bool), a, axis=ax)
        mask = np.zeros(a.shape, bool)
        for m in self.marks:
            if m is not None:
                mask |= a == a.dtype.type(m)
        if self.pack is not None:
            a = a * np.float32(self.pack[0]) + np.float32(self.pack[1])
        return np.ma.array(a, mask=mask)


class _Coord(object):
    def __init__(self, a, units=None):
        self.a = a
        if units is not None:
            self.units = units

    def __getitem__(self, key):
        return np.array(self.a[key])


class Dataset(object):
    def __init__(self, path):
        var, year = os.path.basename(path).split(".")[:2]
        _, pack, mv, fv, has_level, _ = NC.VARS[var]
        self.variables = {var: _RawVar(NC.year_raw(var, int(year)), pack, (mv, fv)), "lon": _Coord(NC.LONS), "lat": _Coord(NC.LATS),
                          "time": _Coord(NC.year_times(int(year)), NC.UNITS)}
        if has_level:
            self.variables["level"] = _Coord(NC.LEVELS)

    def close(self):
        pass


def num2date(times, units):
    assert units == NC.UNITS
    return np.array([NC.EPOCH + dt.timedelta(hours=float(h)) for h in times], dtype=object)


def get_ymd_array(dates):
    return np.array([d.year * 10000 + d.month * 100 + d.day for d in dates], np.int64)


class _OutVar(object):
    def __init__(self, shape):
        self.a = np.full(shape, NC.FILL_F4, np.float32)
        self.days = self.masked = 0

    def __setitem__(self, key, value):
        day_mask = key[0]
        assert all(k == slice(None) for k in key[1:])
        assert value.dtype == np.float32, value.dtype
        self.days += int(day_mask.sum())
        self.masked += int(np.ma.getmaskarray(value).sum())
        self.a[day_mask] = np.ma.filled(value, NC.FILL_F4)


class _OutDs(object):
    def __init__(self, name, shape):
        self.variables = {name: _OutVar(shape)}

    def sync(self):
        pass


def load_reference():
    import make_golden as mg
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    ns = dict(np=np, os=os, Dataset=Dataset, num2date=num2date, get_ymd_array=get_ymd_array, A_DAY=dt.timedelta(days=1), YMD="YMD")
    exec(compile(mg._slice("twx/db/reanalysis.py", 37, 37) + mg._slice("twx/db/reanalysis.py", 41, 42), "reanalysis.py", "exec"), ns)
    heads = (("subset", "path_nnr, ds_out, yrs, days, varname_in, varname_out, levels_subset, utc_time, conv_func", (83, 92), (102, 129)),
             ("nolevel", "path_nnr, ds_out, yrs, days, varname_in, varname_out, utc_time, conv_func, suffix=''", (171, 179), (189, 216)),
             ("thick", "path_nnr, ds_out, yrs, days, level_up, level_low, utc_time", (253, 265), (274, 303)))
    for name, args, a, b in heads:
        src = "def %s(%s):\n" % (name, args) + mg._slice("twx/db/reanalysis.py", *a) + mg._slice("twx/db/reanalysis.py", *b)
        exec(compile(src, "reanalysis.py:%s" % name, "exec"), ns)
    script = {}
    exec(compile(mg._slice("scripts/step12_process_reanalysis_data.py", 40, 40).strip() + "\n", "step12.py", "exec"), script)
    return ns, script["k_to_c"]


def main():
    ns, k_to_c_script = load_reference()
    days = NC.days()
    yrs = np.unique(days["YEAR"])
    assert tuple(yrs) == NC.YEARS
    k_to_c = lambda k: k - np.float32(273.15)  # noqa: E731
    no_conv = lambda x: x  # noqa: E731
    # the trap, and that the script's own lambda gives these bits on unmasked arrays
    plain = (NC.year_raw("air", 2000)[:50] * np.float32(NC.PACKS[0][0]) + np.float32(NC.PACKS[0][1]))
    assert plain.dtype == np.float32 and k_to_c_script(plain).dtype == np.float32
    assert k_to_c_script(plain).tobytes() == k_to_c(plain).tobytes()
    print("masked float32 - 273.15 is %s on numpy %s" % (k_to_c_script(np.ma.array(plain, mask=plain > 400)).dtype, np.__version__))
    nlat, nlon = 6, 7
    out = dict(input_sha=np.array(NC.checksum()), names=[])
    rng = np.random.default_rng(12)
    for raw_var, products in NC.PRODUCTS:
        for p in products:
            nlev = len(p["levels"]) if p.get("levels") is not None else 1
            shape = (days.size, nlev, nlat, nlon) if p.get("levels") is not None else (days.size, nlat, nlon)
            ds_out = _OutDs(p["varname_out"], shape)
            if p.get("thick") is not None:
                ns["thick"]("", ds_out, yrs, days, p["thick"][0], p["thick"][1], p["utc_time"])
            elif p.get("levels") is not None:
                ns["subset"]("", ds_out, yrs, days, raw_var, p["varname_out"], np.array(p["levels"]), p["utc_time"],
                             k_to_c if p.get("conv") == "k_to_c" else no_conv)
            else:
                ns["nolevel"]("", ds_out, yrs, days, raw_var, p["varname_out"], p["utc_time"], no_conv)
            v = ds_out.variables[p["varname_out"]]
            a = np.ascontiguousarray(v.a)
            flat = a.ravel()
            fills = np.nonzero(flat == NC.FILL_F4)[0]
            idx = np.unique(np.concatenate([rng.integers(0, flat.size, NSAMPLE - 100), rng.choice(fills, min(100, fills.size), False)]))
            key = p["fname"][:-3]
            out["names"].append(key)
            out[key + "/sha"] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
            out[key + "/counts"] = np.array([v.days, v.masked, days.size - v.days], np.int64)
            out[key + "/shape"] = np.array(a.shape, np.int64)
            out[key + "/idx"], out[key + "/val"] = idx.astype(np.int64), flat[idx]
            print("%-14s %s days %d masked %d unwritten %d" % (key, a.shape, v.days, v.masked, days.size - v.days))
    out["names"] = np.array(out["names"])
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes, %d products" % (OUT, os.path.getsize(OUT), len(out["names"])))


if __name__ == "__main__":
    main()
