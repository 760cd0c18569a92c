"""The oracle of step13's time-zone lookup (topowx_amd/utc_offsets.py, topowx_amd/qa/twx_tzpoly.hip): the rule of DESIGN.md
section 29 in exact arithmetic on the float64 coordinates.  Pure Python.

* ``crosses`` / ``contains``: the even-odd rule.  An edge straddles when ``(y1 > py) != (y2 > py)``, a straddling edge
  crosses when ``det * (y2 - y1) > 0`` with ``det = (x2 - x1) (py - y1) - (px - x1) (y2 - y1)``; ``det == 0`` is no crossing.
* ``seg_d2``: the exact squared distance to a segment, the projection clamped to the ends (a ``Fraction``).
* ``locate``: the first polygon that contains the point, otherwise the polygon of the nearest edge with the lowest index
  among exact ties, ``NONE`` beyond ``max_force_deg``, ``BAD_POINT`` for a non-finite coordinate.

``Exact`` does the same for many points on integers: every float64 is a dyadic rational, so all coordinates of a case
times one power of two are integers, and the rule's signs and comparisons need no division.  ``tests/test_tzpoly_host.py``
holds the two routes against each other.
"""
import math
from fractions import Fraction

import numpy as np

INSIDE, FORCED, NONE, BAD_POINT = 0, 1, 2, 3


def crosses(x1, y1, x2, y2, px, py):
    if (y1 > py) == (y2 > py):
        return False
    x1, y1, x2, y2, px, py = (Fraction(v) for v in (x1, y1, x2, y2, px, py))
    det = (x2 - x1) * (py - y1) - (px - x1) * (y2 - y1)
    return det * (y2 - y1) > 0


def contains(edges, px, py):
    odd = False
    for e in edges:
        if crosses(e[0], e[1], e[2], e[3], px, py):
            odd = not odd
    return odd


def seg_d2(x1, y1, x2, y2, px, py):
    x1, y1, x2, y2, px, py = (Fraction(v) for v in (x1, y1, x2, y2, px, py))
    dx, dy, wx, wy = x2 - x1, y2 - y1, px - x1, py - y1
    dot, len2 = wx * dx + wy * dy, dx * dx + dy * dy
    if dot <= 0:
        return wx * wx + wy * wy
    if dot >= len2:
        return (px - x2) ** 2 + (py - y2) ** 2
    det = dx * wy - wx * dy
    return det * det / len2


def locate(edges, edge_off, px, py, max_force_deg=1.0):
    """(poly, status, d2 as a Fraction or None) of one point, with Fractions throughout."""
    if not (math.isfinite(px) and math.isfinite(py)):
        return -1, BAD_POINT, None
    npoly = len(edge_off) - 1
    for p in range(npoly):
        if contains(edges[edge_off[p]:edge_off[p + 1]], px, py):
            return p, INSIDE, Fraction(0)
    best, who = None, -1
    for p in range(npoly):
        for e in edges[edge_off[p]:edge_off[p + 1]]:
            d2 = seg_d2(e[0], e[1], e[2], e[3], px, py)
            if best is None or d2 < best:                         # polygons ascend: a tie keeps the lower index
                best, who = d2, p
    if best is None:
        return -1, NONE, None
    if max_force_deg is not None and best > Fraction(float(max_force_deg)) ** 2:
        return -1, NONE, best
    return who, FORCED, best


class Exact(object):
    """The same rule on integers for the polygons ``edges`` [n, 4], ``edge_off`` and many points."""

    def __init__(self, edges, edge_off):
        self.edges = np.ascontiguousarray(edges, np.float64).reshape(-1, 4)
        self.off = [int(v) for v in edge_off]
        self.owner = (np.searchsorted(np.asarray(edge_off), np.arange(len(self.edges)), side="right") - 1).tolist()
        rows = [[Fraction(v) for v in row] for row in self.edges.tolist()]
        self.den = max([1] + [v.denominator for row in rows for v in row])       # powers of two: the largest is a common multiple
        self.iedges = [tuple(int(v * self.den) for v in row) for row in rows]

    def locate_all(self, lons, lats, max_force_deg=1.0):
        """(poly [n], status [n], d2 [n] Fractions or None)."""
        poly, status, d2s = [], [], []
        for px, py in zip(np.asarray(lons, np.float64).tolist(), np.asarray(lats, np.float64).tolist()):
            p, s, d = self._one(px, py, max_force_deg)
            poly.append(p), status.append(s), d2s.append(d)
        return np.array(poly, np.int32), np.array(status, np.int32), d2s

    def _one(self, px, py, max_force_deg):
        if not (math.isfinite(px) and math.isfinite(py)):
            return -1, BAD_POINT, None
        e = self.edges
        fx, fy = Fraction(px), Fraction(py)
        den = max(self.den, fx.denominator, fy.denominator)
        ipx, ipy, f = int(fx * den), int(fy * den), den // self.den
        # inside: only straddling edges can cross, and the comparison that finds them is exact in float64
        parity = {}
        for k in np.nonzero((e[:, 1] > py) != (e[:, 3] > py))[0].tolist():
            x1, y1, x2, y2 = (v * f for v in self.iedges[k])
            det = (x2 - x1) * (ipy - y1) - (ipx - x1) * (y2 - y1)
            if det * (y2 - y1) > 0:
                parity[self.owner[k]] = not parity.get(self.owner[k], False)
        inside = sorted(p for p, odd in parity.items() if odd)
        if inside:
            return inside[0], INSIDE, Fraction(0)
        bn, bd, who = None, 1, -1                                  # the minimum as bn / bd (in units of 1 / den^2)
        for k, row in enumerate(self.iedges):
            x1, y1, x2, y2 = row if f == 1 else (v * f for v in row)
            dx, dy, wx, wy = x2 - x1, y2 - y1, ipx - x1, ipy - y1
            dot, len2 = wx * dx + wy * dy, dx * dx + dy * dy
            if dot <= 0:
                n, d = wx * wx + wy * wy, 1
            elif dot >= len2:
                n, d = (ipx - x2) ** 2 + (ipy - y2) ** 2, 1
            else:
                det = dx * wy - wx * dy
                n, d = det * det, len2
            if bn is None or n * bd < bn * d:                      # edges ascend with the polygons: a tie keeps the lower index
                bn, bd, who = n, d, self.owner[k]
        if bn is None:
            return -1, NONE, None
        best = Fraction(bn, bd * den * den)
        if max_force_deg is not None and best > Fraction(float(max_force_deg)) ** 2:
            return -1, NONE, best
        return who, FORCED, best
