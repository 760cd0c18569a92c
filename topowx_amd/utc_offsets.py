"""Step13: the UTC offset of every station by a point-in-polygon lookup of time-zone polygons on the GPU.

The reference's ``add_utc_offset`` (twx/db/create_db_all_stations.py:1333-1383) over ``UtcOffset``
(twx/db/stn_utc_offsets.py:43-117) asks ``tzwhere(shapely=True, forceTZ=True).tzNameAt(lat, lon)`` once per station.
Neither tzwhere nor shapely nor their polygon file can be executed here, so the lookup is RESTATED:

* the first polygon, in file order, that contains the point by the even-odd rule over all its rings' edges; an edge
  straddles when ``(y1 > py) != (y2 > py)`` and crosses when ``det * (y2 - y1) > 0`` with ``det = (x2 - x1) * (py - y1) -
  (px - x1) * (y2 - y1)``; ``det == 0`` is no crossing;
* otherwise the polygon of the nearest edge, ``(d2, polygon index)`` lexicographic, if it lies within ``max_force_deg``
  degrees;
* the zone's offset on 2009-01-01 in hours, as the reference computes it.

libtwxqa's ``twxtz_locate`` evaluates this in float64 for all points in one call and names every (point, polygon) pair
and every forced point that float64 cannot certify; those are decided again here with ``fractions.Fraction`` on the float64
coordinates, so the result of every point is the exact evaluation of the rule.  Nothing here reaches a network: there is
no Geonames client.
"""
import datetime as _dt
import json
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from . import _qalib

__all__ = ["load_tz_polygons", "TzPolygons", "TzResult", "UtcOffset", "add_utc_offset", "UTC_OFFSET"]

UTC_OFFSET = "utc_offset"                 # twx.db.UTC_OFFSET
A_DATE = _dt.datetime(2009, 1, 1)         # stn_utc_offsets.py:70
EPS = 2.0 ** -53

TzPolygons = namedtuple("TzPolygons", "edges edge_off bbox zone names")
TzResult = namedtuple("TzResult", "offset zone poly status dist_deg")


def _ring_edges(ring, fi):
    try:
        a = np.array([(c[0], c[1]) for c in ring], np.float64).reshape(-1, 2)
    except (TypeError, ValueError, IndexError):
        raise ValueError("feature %d: a ring is not a list of [lon, lat] positions" % fi)
    if not np.isfinite(a).all():
        raise ValueError("feature %d: a coordinate is not finite" % fi)
    if len(a) > 1 and (a[0] == a[-1]).all():
        a = a[:-1]
    if len(set(map(tuple, a))) < 3:
        raise ValueError("feature %d: a ring has fewer than 3 distinct vertices" % fi)
    e = np.hstack([a, np.roll(a, -1, axis=0)])
    return e[(e[:, 0] != e[:, 2]) | (e[:, 1] != e[:, 3])], a


def load_tz_polygons(path, holes=True):
    """Time-zone polygons of a GeoJSON ``FeatureCollection``: ``tz_world.json`` as tzwhere ships it (``properties.TZID``,
    ``Polygon``) or timezone-boundary-builder's ``combined.json`` (``properties.tzid``, ``Polygon`` / ``MultiPolygon``).

    Every part of a ``MultiPolygon`` is a polygon entry of its own with the feature's zone; entries keep file order
    (features, then parts).  The edges of all rings of a part form one edge list, and the even-odd rule over it makes the
    interior rings holes; ``holes=False`` drops the interior rings.  That holes count restates what tzwhere with shapely is
    believed to do (shapely polygons built with their interiors); it has NOT been verified against tzwhere, which is not
    available here.  A ring may repeat its first vertex or not; zero-length edges are dropped.  Longitudes are taken as
    written: nothing wraps at +-180, a polygon that crosses the antimeridian must be cut there by the file.

    Returns ``TzPolygons``: ``edges`` [nedge, 4] float64 (x1, y1, x2, y2), ``edge_off`` [npoly + 1] int64, ``bbox``
    [npoly, 4] (xmin, ymin, xmax, ymax: minima and maxima of the coordinates, exact), ``zone`` [npoly] int32 into ``names``.
    ``ValueError`` names the feature of a ring with fewer than 3 distinct vertices, a non-finite coordinate, a missing zone
    property or a geometry of another type."""
    with open(path) as fh:
        try:
            doc = json.load(fh)
        except ValueError as e:
            raise ValueError("%s is not JSON: %s" % (path, e))
    if not isinstance(doc, dict) or doc.get("type") != "FeatureCollection" or not isinstance(doc.get("features"), list):
        raise ValueError("%s is not a GeoJSON FeatureCollection" % path)
    names, index, zone, edges, off, bbox = [], {}, [], [], [0], []
    for fi, f in enumerate(doc["features"]):
        props = (f.get("properties") if isinstance(f, dict) else None) or {}
        name = props.get("TZID", props.get("tzid"))
        if not isinstance(name, str) or not name:
            raise ValueError("feature %d has no zone property (TZID / tzid)" % fi)
        geom = f.get("geometry") or {}
        if geom.get("type") == "Polygon":
            parts = [geom.get("coordinates")]
        elif geom.get("type") == "MultiPolygon":
            parts = geom.get("coordinates")
        else:
            raise ValueError("feature %d: geometry type %r is neither Polygon nor MultiPolygon" % (fi, geom.get("type")))
        if not isinstance(parts, list) or not parts:
            raise ValueError("feature %d has no coordinates" % fi)
        for part in parts:
            if not isinstance(part, list) or not part:
                raise ValueError("feature %d: a polygon without rings" % fi)
            got = [_ring_edges(ring, fi) for ring in (part if holes else part[:1])]
            e = np.vstack([g[0] for g in got])
            v = np.vstack([g[1] for g in got])
            edges.append(e)
            off.append(off[-1] + len(e))
            bbox.append((v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()))
            zone.append(index.setdefault(name, len(index)))
            if zone[-1] == len(names):
                names.append(name)
    if not zone:
        raise ValueError("%s holds no polygon" % path)
    return TzPolygons(np.ascontiguousarray(np.vstack(edges)), np.array(off, np.int64), np.array(bbox, np.float64).reshape(-1, 4),
                      np.array(zone, np.int32), names)


# ---- the exact rule, for what float64 could not certify ----
def _exact_contains(e, px, py):
    """The even-odd rule of one polygon's edges ``e`` [n, 4] at (px, py), exact: float comparisons find the straddling
    edges (they are exact), rationals the sign of det."""
    odd = False
    fx, fy = Fraction(px), Fraction(py)
    for x1, y1, x2, y2 in e[(e[:, 1] > py) != (e[:, 3] > py)].tolist():
        x1, y1, x2, y2 = Fraction(x1), Fraction(y1), Fraction(x2), Fraction(y2)
        det = (x2 - x1) * (fy - y1) - (fx - x1) * (y2 - y1)
        if det * (y2 - y1) > 0:
            odd = not odd
    return odd


def _exact_d2(x1, y1, x2, y2, px, py):
    x1, y1, x2, y2, px, py = (Fraction(v) for v in (x1, y1, x2, y2, px, py))
    dx, dy, wx, wy = x2 - x1, y2 - y1, px - x1, py - y1
    dot, len2 = wx * dx + wy * dy, dx * dx + dy * dy
    if dot <= 0:
        return wx * wx + wy * wy
    if dot >= len2:
        return (px - x2) ** 2 + (py - y2) ** 2
    det = dx * wy - wx * dy
    return det * det / len2


def _d2_bounds(e, px, py):
    """(lo, hi) [n]: float64 bounds that enclose the exact squared distance from (px, py) to every edge of ``e``."""
    with np.errstate(all="ignore"):
        dx, dy, wx, wy = e[:, 2] - e[:, 0], e[:, 3] - e[:, 1], px - e[:, 0], py - e[:, 1]
        ux, uy = px - e[:, 2], py - e[:, 3]
        dot1, dot2, len2 = wx * dx + wy * dy, ux * dx + uy * dy, dx * dx + dy * dy
        far = dot1 + dot2 > 0.0
        a, b = dx * np.where(far, uy, wy), np.where(far, ux, wx) * dy
        det, s = np.abs(a - b), np.abs(a) + np.abs(b)
        beta = 4.0 * EPS * s
        lo_i = np.maximum(det - beta, 0.0) ** 2 / len2
        hi_i = (det + beta) ** 2 / len2
        end1, end2 = wx * wx + wy * wy, ux * ux + uy * uy
        v = np.where(dot1 <= 0.0, end1, np.where(dot2 >= 0.0, end2, 0.0))
        inner = (dot1 > 0.0) & (dot2 < 0.0)
        lo = np.where(inner, lo_i, v) * (1.0 - 2.0 ** -45)
        hi = np.where(inner, np.minimum(hi_i, np.minimum(end1, end2)), v) * (1.0 + 2.0 ** -45)
        bad = ~np.isfinite(lo) | ~np.isfinite(hi)                 # overflow somewhere: let the rationals look
        lo[bad], hi[bad] = 0.0, np.inf
        tiny = ~(hi >= 2.0 ** -900)                               # squares that have lost bits to underflow, zero included
        lo[tiny], hi[tiny] = 0.0, 2.0 ** -890
    return lo, hi


def _exact_nearest(tz, px, py, hint=-1):
    """(exact minimum squared distance as a Fraction, the lowest polygon index that attains it).  Float64 bounds discard
    the polygons and edges that cannot attain it; ``hint``: a polygon believed near, which gives the first upper bound."""
    upper = np.inf
    if hint >= 0 and tz.edge_off[hint + 1] > tz.edge_off[hint]:
        upper = _d2_bounds(tz.edges[tz.edge_off[hint]:tz.edge_off[hint + 1]], px, py)[1].min()
    bb = tz.bbox
    gx = np.maximum(np.maximum(bb[:, 0] - px, px - bb[:, 2]), 0.0)
    gy = np.maximum(np.maximum(bb[:, 1] - py, py - bb[:, 3]), 0.0)
    with np.errstate(all="ignore"):
        blo = (gx * gx + gy * gy) * (1.0 - 2.0 ** -45)
    polys = np.nonzero(~(blo > upper) & (np.diff(tz.edge_off) > 0))[0]
    idx = np.concatenate([np.arange(tz.edge_off[p], tz.edge_off[p + 1]) for p in polys]) if polys.size else np.zeros(0, np.int64)
    if idx.size == 0:
        return None, -1
    lo, hi = _d2_bounds(tz.edges[idx], px, py)
    keep = idx[lo <= hi.min()]
    owner = np.searchsorted(tz.edge_off, keep, side="right") - 1
    best, who = None, -1
    for k, p in zip(keep.tolist(), owner.tolist()):
        d2 = _exact_d2(*tz.edges[k].tolist(), px, py)
        if best is None or d2 < best or (d2 == best and p < who):
            best, who = d2, p
    return best, who


class UtcOffset(object):
    """``UtcOffset`` (stn_utc_offsets.py:43-117) over a polygon file instead of tzwhere's own.

    ``tz_polygons``: the path of a GeoJSON file (``load_tz_polygons``) or a ``TzPolygons``.  ``tz_offsets`` is built as the
    reference builds it, ``tz.utcoffset(datetime(2009, 1, 1)).total_seconds() / 3600.0`` per zone name of the file, with
    ``pytz`` if it can be imported and ``zoneinfo`` otherwise.  Deviations: the name ``uninhabited`` maps to ``ndata`` (the
    reference leaves it out of the table and would raise ``KeyError`` for a point inside such a polygon); a name the
    library does not know raises ``ValueError`` here, at construction; there is no Geonames client.
    ``max_force_deg``: how far the nearest polygon of a point that nothing contains may lie (``None``: any distance) -- a
    restated choice that stands in for tzwhere's one-degree shortcut bins."""

    def __init__(self, tz_polygons, ndata=-32767, max_force_deg=1.0, holes=True, device=0):
        self.tz = tz_polygons if isinstance(tz_polygons, TzPolygons) else load_tz_polygons(tz_polygons, holes=holes)
        self.ndata, self.max_force_deg, self.device = ndata, max_force_deg, device
        if max_force_deg is not None and not float(max_force_deg) >= 0.0:
            raise ValueError("max_force_deg must be >= 0 or None")
        self.tz_offsets = {}
        zone_of = _zone_factory()
        for name in self.tz.names:
            if name == "uninhabited":
                self.tz_offsets[name] = ndata
                continue
            try:
                a_tz = zone_of(name)
            except Exception:
                raise ValueError("unknown time zone name %r in the polygon file" % name)
            self.tz_offsets[name] = a_tz.utcoffset(A_DATE).total_seconds() / 3600.0
        self.last_report = None

    def get_utc_offset(self, lon, lat):
        """The UTC offset of one point in hours, ``ndata`` if it cannot be determined (a batch of one)."""
        return self.get_utc_offsets([lon], [lat]).offset[0]

    def get_utc_offsets(self, lons, lats, uncertain_cap=4096):
        """``TzResult`` of arrays over the points: ``offset`` (float hours, ``ndata`` where undetermined), ``zone`` (names,
        ``None`` where no polygon was found), ``poly`` (index into the file's polygon entries, -1 for none), ``status``
        (``_qalib.TZ_INSIDE`` / ``TZ_FORCED`` / ``TZ_NONE`` / ``TZ_BAD_POINT``) and ``dist_deg`` (0 inside, the distance to
        the nearest polygon otherwise, NaN for a bad point).  ``last_report`` holds the counts, the device's phase times
        and the number of items settled on the host."""
        import time
        lons, lats = np.ascontiguousarray(lons, np.float64).ravel(), np.ascontiguousarray(lats, np.float64).ravel()
        if lons.shape != lats.shape:
            raise ValueError("lons / lats must have one length")
        tz, tm = self.tz, {}
        if lons.size == 0:
            self.last_report = dict(npoints=0, settled=0)
            return TzResult(np.zeros(0), np.zeros(0, object), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
        poly, status, d2, unc, counts = _qalib.tz_locate(lons, lats, tz.edge_off, tz.bbox, tz.edges, self.max_force_deg,
                                                         uncertain_cap, self.device, tm)
        t0 = time.perf_counter()
        settled = self._settle(lons, lats, poly, status, d2, unc)
        tm["tz_settle_ms"] = (time.perf_counter() - t0) * 1e3
        if (status == _qalib.TZ_UNCERTAIN).any() or (status == _qalib.TZ_PENDING).any():
            raise _qalib.QaError("twxtz_locate left a point undecided that its uncertain list does not name")
        dist = np.sqrt(d2)
        dist[status == _qalib.TZ_BAD_POINT] = np.nan
        zone = np.array([tz.names[tz.zone[p]] if p >= 0 else None for p in poly.tolist()], object)
        offset = np.array([self.tz_offsets[z] if z is not None else self.ndata for z in zone.tolist()], np.float64)
        self.last_report = dict(npoints=int(lons.size), npoly=int(tz.zone.size), nedge=int(tz.edges.shape[0]),
                                pairs=int(counts[_qalib.TZ_C_PAIRS]), items=int(counts[_qalib.TZ_C_ITEMS]),
                                forced_points=int(counts[_qalib.TZ_C_PENDING]), uncertain=int(unc.shape[0]), settled=settled,
                                inside=int((status == _qalib.TZ_INSIDE).sum()), forced=int((status == _qalib.TZ_FORCED).sum()),
                                none=int((status == _qalib.TZ_NONE).sum()), bad_points=int((status == _qalib.TZ_BAD_POINT).sum()),
                                **tm)
        return TzResult(offset, zone, poly, status, dist)

    def _settle(self, lons, lats, poly, status, d2, unc):
        """Decide every entry of the uncertain list exactly, in place; returns the number of entries."""
        tz = self.tz
        by_pt = {}
        for pt, p in unc.tolist():
            by_pt.setdefault(pt, []).append(p)
        for pt, ps in by_pt.items():
            px, py = float(lons[pt]), float(lats[pt])
            forced_hint = poly[pt] if ps == [-1] else -1
            if ps != [-1]:                                        # pairs below the first certain inside polygon, ascending
                win = -1
                for p in sorted(q for q in ps if q >= 0):
                    if _exact_contains(tz.edges[tz.edge_off[p]:tz.edge_off[p + 1]], px, py):
                        win = p
                        break
                if win < 0:
                    win = int(poly[pt])                           # the device's own first certain inside polygon, if any
                if win >= 0:
                    poly[pt], status[pt], d2[pt] = win, _qalib.TZ_INSIDE, 0.0
                    continue
            best, who = _exact_nearest(tz, px, py, int(forced_hint))
            if best is None:
                poly[pt], status[pt], d2[pt] = -1, _qalib.TZ_NONE, np.inf
                continue
            d2[pt] = float(best)
            far = self.max_force_deg is not None and best > Fraction(float(self.max_force_deg)) ** 2
            poly[pt], status[pt] = (-1, _qalib.TZ_NONE) if far else (who, _qalib.TZ_FORCED)
        return int(unc.shape[0])


def _zone_factory():
    try:
        import pytz
        return pytz.timezone
    except ImportError:
        import zoneinfo
        return zoneinfo.ZoneInfo


def add_utc_offset(ds_path, tz_polygons, ndata=None, max_force_deg=1.0, holes=True, device=0, dry_run=False):
    """``add_utc_offset`` (create_db_all_stations.py:1333-1383): the station variable ``utc_offset`` (``i2``, long name
    ``utc_offset``, units ``""``) of a station database in either container, from the stations' longitude / latitude.

    Where an offset was found it is written as ``np.float64(offset).astype('i2')``, which truncates toward zero: -3.5
    (America/St_Johns) is stored as -3, as the reference's assignment of -3.5 to an ``i2`` variable stores it.  Elsewhere
    the fill value stays and the reference's line "Error: Couldn't determine UTC offset for: <id>" is printed.
    ``dry_run``: look up and report, write nothing.  Returns the report: ``UtcOffset.last_report`` with ``ids``,
    ``utc_offset`` (the int16 values, ``ndata`` where undetermined), ``offset``, ``zone``, ``poly``, ``status`` and
    ``dist_deg`` per station."""
    from . import ncio
    from .stationdb import LAT, LON, STN_ID, StationSerialDataDb
    ndata = ncio.DEFAULT_FILLS["i2"] if ndata is None else ndata
    utc = UtcOffset(tz_polygons, ndata, max_force_deg, holes, device)
    stnda = StationSerialDataDb(ds_path, None, mode="r" if dry_run else "r+")
    try:
        print("Starting to get station UTC offset data...")
        res = utc.get_utc_offsets(stnda.stns[LON], stnda.stns[LAT])
        found = res.offset != ndata
        stored = np.full(res.offset.size, ndata, np.int16)
        stored[found] = np.float64(res.offset[found]).astype("i2")
        for sid in stnda.stns[STN_ID][~found]:
            print("Error: Couldn't determine UTC offset for: %s" % sid)
        if not dry_run:
            var_utc = stnda.add_stn_variable(UTC_OFFSET, UTC_OFFSET, "", "i2")
            if found.any():
                var_utc[found] = stored[found]
            stnda.ds.sync()
    finally:
        stnda.close()
    return dict(utc.last_report, ids=np.array(stnda.stns[STN_ID]), utc_offset=stored, offset=res.offset,
                zone=np.array(["" if z is None else z for z in res.zone]), poly=res.poly, status=res.status, dist_deg=res.dist_deg,
                written=not dry_run)
