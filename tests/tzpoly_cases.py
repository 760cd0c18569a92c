"""Seeded generators of time-zone polygon sets and points for the tests of step13 (tests/test_tzpoly_host.py,
tests/test_gpu_tzpoly.py) and for its timing (tests/tools/gpu_tz_timing.py).  Nothing here comes from a real polygon file.

A *feature* is ``(zone name, [part, ...])``, a part ``[ring, ...]`` (exterior first), a ring a list of ``(lon, lat)``.
"""
import json
import math

import numpy as np

# zones whose offsets on 2009-01-01 lie in the -4 .. -8 h that the reanalysis reader knows, and two that pin quirks
ZONES = ("America/Denver", "America/Los_Angeles", "America/Chicago", "America/New_York", "America/Halifax", "America/Phoenix")
CHUNK = 2048                              # TWXTZ_CHUNK_EDGES
EDGE_COUNTS = (3, 4, 63, 64, 65, 127, 128, 129, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
POLY_COUNTS = (1, 2, 64, 65)
POINT_COUNTS = (1, 63, 64, 65, 257)


def ngon(cx, cy, r, n, seed, jitter=0.35):
    """A star-shaped ring of exactly n distinct vertices about (cx, cy): sorted random angles, radii r (1 +- jitter)."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2.0 * math.pi, n))
    while np.unique(ang).size != n:
        ang = np.sort(rng.uniform(0.0, 2.0 * math.pi, n))
    rad = r * (1.0 + jitter * rng.uniform(-1.0, 1.0, n))
    return [(float(cx + a * math.cos(t)), float(cy + a * math.sin(t))) for a, t in zip(rad, ang)]


def rect(x0, y0, x1, y1):
    return [(float(x0), float(y0)), (float(x1), float(y0)), (float(x1), float(y1)), (float(x0), float(y1))]


def write_geojson(path, features, form="tz_world", close=True):
    """``form``: 'tz_world' (TZID, Polygon only: a feature per part) or 'combined' (tzid, MultiPolygon where a feature has
    several parts).  ``close``: repeat each ring's first vertex, as GeoJSON asks; False leaves the rings open."""
    def ring_out(r):
        r = [list(p) for p in r]
        return r + [r[0]] if close else r
    out = []
    for name, parts in features:
        coords = [[ring_out(r) for r in part] for part in parts]
        if form == "tz_world":
            out += [{"type": "Feature", "properties": {"TZID": name}, "geometry": {"type": "Polygon", "coordinates": c}} for c in coords]
        elif len(coords) == 1:
            out.append({"type": "Feature", "properties": {"tzid": name}, "geometry": {"type": "Polygon", "coordinates": coords[0]}})
        else:
            out.append({"type": "Feature", "properties": {"tzid": name}, "geometry": {"type": "MultiPolygon", "coordinates": coords}})
    with open(path, "w") as fh:
        json.dump({"type": "FeatureCollection", "features": out}, fh)
    return path


def box_points(n, box, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(box[0], box[2], n), rng.uniform(box[1], box[3], n)


def grid_features(npoly, seed, nedge=(5, 12)):
    """npoly small star polygons on a lattice of pitch 2, radius about 1.2: neighbours overlap, gaps stay between them."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(npoly)))
    feats = []
    for k in range(npoly):
        n = int(rng.integers(nedge[0], nedge[1] + 1))
        feats.append((ZONES[k % len(ZONES)], [[ngon(-110.0 + 2.0 * (k % side), 35.0 + 2.0 * (k // side), 1.2, n, seed * 1000 + k)]]))
    return feats, (-112.5, 32.5, -110.0 + 2.0 * side + 0.5, 35.0 + 2.0 * side + 0.5)


def adversarial_points(edges, bbox):
    """Points that sit on what the rule is sharp about, from the polygons' own coordinates: every vertex; the midpoints of
    edges (float64 rounds some and not others); points with py equal to a vertex's y; points collinear with a horizontal
    edge left and right of it; the four nextafter neighbours of every vertex; the corners of the bboxes."""
    e = np.asarray(edges, np.float64)
    xs, ys = [], []
    vx, vy = e[:, 0], e[:, 1]
    xs += vx.tolist()
    ys += vy.tolist()
    xs += ((e[:, 0] + e[:, 2]) / 2.0).tolist()
    ys += ((e[:, 1] + e[:, 3]) / 2.0).tolist()
    xs += (vx + 0.37).tolist() + (vx - 0.41).tolist()
    ys += vy.tolist() * 2
    hor = e[e[:, 1] == e[:, 3]]
    for x1, y, x2, _ in hor.tolist():
        lo, hi = min(x1, x2), max(x1, x2)
        xs += [lo - 0.25, hi + 0.25, (lo + hi) / 2.0]
        ys += [y, y, y]
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        xs += (np.nextafter(vx, sx * np.inf) if sx else vx).tolist()
        ys += (np.nextafter(vy, sy * np.inf) if sy else vy).tolist()
    for b in np.asarray(bbox, np.float64).tolist():
        xs += [b[0], b[2], b[0], b[2]]
        ys += [b[1], b[1], b[3], b[3]]
    return np.array(xs, np.float64), np.array(ys, np.float64)


# ---- the timing's polygon set: a lattice of cells with fractal-roughened shared boundaries ----
def _roughen(p, q, depth, rng, amp=0.18):
    """The polyline from p to q by midpoint displacement: 2 ** depth segments, end points kept."""
    pts = np.array([p, q], np.float64)
    for _ in range(depth):
        mid = (pts[:-1] + pts[1:]) / 2.0
        d = pts[1:] - pts[:-1]
        mid += amp * rng.uniform(-1.0, 1.0, (len(mid), 1)) * np.stack([-d[:, 1], d[:, 0]], axis=1)
        out = np.empty((len(pts) + len(mid), 2))
        out[0::2], out[1::2] = pts, mid
        pts = out
    return pts


def fractal_zones(seed=13, ncx=64, ncy=52, depth=7, box=(-170.0, 10.0, -50.0, 85.0), zone_cells=3, drop=0.1):
    """(edges, edge_off, bbox, zone, names) as ``load_tz_polygons`` returns them, made directly: ncx x ncy cells over
    ``box`` whose corner nodes are jittered and whose sides are midpoint-displacement polylines of 2 ** depth segments,
    each shared by the two cells it separates; a zone is a block of zone_cells x zone_cells cells; a share ``drop`` of the
    cells is left out (water).  The defaults give about 3.0e3 parts of 512 edges, 1.5e6 edges, about 400 zones."""
    from topowx_amd.utc_offsets import TzPolygons
    rng = np.random.default_rng(seed)
    gx, gy = np.linspace(box[0], box[2], ncx + 1), np.linspace(box[1], box[3], ncy + 1)
    px, py = (gx[1] - gx[0]), (gy[1] - gy[0])
    node = np.stack(np.meshgrid(gx, gy, indexing="ij"), axis=-1) + rng.uniform(-0.2, 0.2, (ncx + 1, ncy + 1, 2)) * (px, py)
    hor = [[_roughen(node[i, j], node[i + 1, j], depth, rng) for j in range(ncy + 1)] for i in range(ncx)]
    ver = [[_roughen(node[i, j], node[i, j + 1], depth, rng) for j in range(ncy)] for i in range(ncx + 1)]
    keep = rng.uniform(size=(ncx, ncy)) >= drop
    edges, off, bbox, zone, names, index = [], [0], [], [], [], {}
    for i in range(ncx):
        for j in range(ncy):
            if not keep[i, j]:
                continue
            ring = np.vstack([hor[i][j][:-1], ver[i + 1][j][:-1], hor[i][j + 1][::-1][:-1], ver[i][j][::-1][:-1]])
            e = np.hstack([ring, np.roll(ring, -1, axis=0)])
            e = e[(e[:, 0] != e[:, 2]) | (e[:, 1] != e[:, 3])]
            edges.append(e)
            off.append(off[-1] + len(e))
            bbox.append((ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max()))
            name = "zone_%d_%d" % (i // zone_cells, j // zone_cells)
            zone.append(index.setdefault(name, len(index)))
            if zone[-1] == len(names):
                names.append(name)
    return TzPolygons(np.ascontiguousarray(np.vstack(edges)), np.array(off, np.int64), np.array(bbox, np.float64),
                      np.array(zone, np.int32), names)
