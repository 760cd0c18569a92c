// twx_tzpoly_pred.h -- the predicates of twx_tzpoly.hip (step13's point-in-polygon lookup), shared with a CPU program of the
// tests (tests/tools/tzpoly_hostcheck.cpp): the closed bbox test, the crossing test of one edge with its static error
// filter, and the squared point-segment distance with its conditioning.  Plain C++, no device call; every operation is
// rounded on its own (the build sets -ffp-contract=off, and nothing here is written so that contraction could change it
// silently: the CPU program is built with the same flag).
#ifndef TWX_TZPOLY_PRED_H
#define TWX_TZPOLY_PRED_H
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TZ_HD __host__ __device__ __forceinline__
#else
#define TZ_HD inline
#endif

#define TZ_CROSS 1                            // bits of tz_edge_cross: the edge crosses the ray of the point
#define TZ_CROSS_UNCERTAIN 2                  //   the sign of det is not certain in float64: the pair is decided on the host
#define TZ_EPS 0x1p-53
// Shewchuk's static filter of orient2d (ccwerrboundA): |det| >= (3 + 16 eps) eps (|a| + |b|) makes the sign of det certain
#define TZ_CCW_ERRBOUND ((3.0 + 16.0 * TZ_EPS) * TZ_EPS)
// the filter's proof assumes no underflow: below this |a| + |b| the edge is uncertain whatever det is
#define TZ_UNDERFLOW_GUARD 0x1p-960
// tz_seg_d2: an interior foot whose (|a| + |b|) / |det| exceeds this is ill-conditioned (the point is that much nearer to
// the edge's line than to its ends); its d2 is then only a candidate for the host
#define TZ_D2_COND 8.0
// relative error of a well-conditioned d2, in units of 2^-53, by the count of rounded operations below: det carries
// (3 + 16 eps) eps (|a| + |b|) <= 3.01 TZ_D2_COND |det| eps, squared twice that and one rounding (49.2); len2 has two
// differences (each squared: 4), two squares and a sum (3); the quotient one more: 57.2, stated as 60.  The two end cases
// (two differences squared, two squares, a sum: 7) lie far below.
#define TZ_D2_RELERR_ULPS 60.0

// closed on all four sides; bb = xmin, ymin, xmax, ymax, copied from the coordinates
TZ_HD bool tz_bbox_contains(const double *bb, double px, double py)
{
    return px >= bb[0] && px <= bb[2] && py >= bb[1] && py <= bb[3];
}

// The even-odd rule's test of one edge against the ray from (px, py) towards +x.  An edge straddles when (y1 > py) !=
// (y2 > py): a vertex on the ray belongs to the lower half.  A straddling edge crosses when det (y2 - y1) > 0, det = (x2 - x1)
// (py - y1) - (px - x1) (y2 - y1); det == 0 (the point on the edge) is no crossing.  Returns TZ_CROSS and / or
// TZ_CROSS_UNCERTAIN; with the latter the crossing bit means nothing.
TZ_HD int tz_edge_cross(double x1, double y1, double x2, double y2, double px, double py)
{
    if ((y1 > py) == (y2 > py)) return 0;
    const double dy = y2 - y1;
    const double a = (x2 - x1) * (py - y1);
    const double b = (px - x1) * dy;
    const double det = a - b;
    const double s = fabs(a) + fabs(b);
    if (!(fabs(det) >= TZ_CCW_ERRBOUND * s) || !(s >= TZ_UNDERFLOW_GUARD)) {
        if (a == 0.0 && b == 0.0 && (x2 == x1 || py == y1) && px == x1) return 0;      // both products are exact zeros
        return TZ_CROSS_UNCERTAIN;
    }
    return (det > 0.0) == (dy > 0.0) ? TZ_CROSS : 0;
}

// Squared distance from (px, py) to the segment, the projection clamped to the ends.  *ill: the foot is interior and the
// cross product ill-conditioned (TZ_D2_COND); the value is then still an approximation and *lo a lower bound of the true
// one.  Otherwise *lo = the value.  A zero-length edge never reaches this (len2 > 0).
TZ_HD double tz_seg_d2(double x1, double y1, double x2, double y2, double px, double py, bool *ill, double *lo)
{
    const double dx = x2 - x1, dy = y2 - y1, wx = px - x1, wy = py - y1, ux = px - x2, uy = py - y2;
    // each end's test uses the vector from THAT end, so that a point next to an end is judged by small, exact differences:
    // a wrong sign then needs the foot within a few eps |w| of the end, where the two formulas agree to eps^2
    const double dot1 = wx * dx + wy * dy, dot2 = ux * dx + uy * dy;
    *ill = false;
    double d2;
    if (dot1 <= 0.0) {
        d2 = wx * wx + wy * wy;
    } else if (dot2 >= 0.0) {
        d2 = ux * ux + uy * uy;
    } else {
        const double len2 = dx * dx + dy * dy;
        const bool far = dot1 + dot2 > 0.0;                        // the foot lies beyond the middle: take the cross product from end 2
        const double a = dx * (far ? uy : wy), b = (far ? ux : wx) * dy;
        const double det = a - b;
        const double s = fabs(a) + fabs(b);
        d2 = det * det / len2;
        if (!(fabs(det) * TZ_D2_COND >= s)) {
            *ill = true;
            const double m = fabs(det) - 4.0 * TZ_EPS * s;
            *lo = m > 0.0 ? m * m / len2 * (1.0 - 16.0 * TZ_EPS) : 0.0;
            return d2;
        }
    }
    if (!(d2 >= TZ_UNDERFLOW_GUARD)) {                            // squares this small have lost bits, zero included: the host looks
        *ill = true;
        *lo = 0.0;
        return d2;
    }
    *lo = d2;
    return d2;
}

#endif
