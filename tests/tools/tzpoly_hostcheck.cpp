// tzpoly_hostcheck -- the predicates of twx_tzpoly.hip (twx_tzpoly_pred.h) on the CPU, as a program of its own, built by
// tests/test_tzpoly_host.py with -fsanitize=address,undefined and -ffp-contract=off.
//
//   tzpoly_hostcheck CASEFILE
//
// CASEFILE: "NEDGE NPOLY NPT", then NEDGE lines "x1 y1 x2 y2", NPOLY + 1 offsets, NPOLY lines "xmin ymin xmax ymax", NPT
// lines "px py"; numbers as C hexadecimal floats, so nothing is rounded on the way.  For every (point, edge) it prints
// "E pt edge bits ill d2 lo" (bits of tz_edge_cross; d2, *ill and *lo of tz_seg_d2), and for every (point, polygon) whose
// closed bbox holds the point "P pt poly parity uncertain", walking the edges through the offsets as the kernels do, in
// buffers of exactly the stated sizes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "twx_tzpoly_pred.h"

static bool rd(FILE *f, double *v)
{
    char tok[128];
    if (fscanf(f, "%127s", tok) != 1) return false;
    char *end = nullptr;
    *v = strtod(tok, &end);
    return end && *end == 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: tzpoly_hostcheck CASEFILE\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "tzpoly_hostcheck: cannot open %s\n", argv[1]); return 2; }
    long long ne = 0, npoly = 0, npt = 0;
    if (fscanf(f, "%lld %lld %lld", &ne, &npoly, &npt) != 3 || ne < 1 || npoly < 1 || npt < 1) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<double> edges((size_t)ne * 4), bbox((size_t)npoly * 4), pts((size_t)npt * 2);
    std::vector<long long> off((size_t)npoly + 1);
    for (size_t i = 0; i < edges.size(); ++i)
        if (!rd(f, &edges[i])) { fprintf(stderr, "bad edge\n"); return 2; }
    for (size_t i = 0; i < off.size(); ++i)
        if (fscanf(f, "%lld", &off[i]) != 1) { fprintf(stderr, "bad offset\n"); return 2; }
    for (size_t i = 0; i < bbox.size(); ++i)
        if (!rd(f, &bbox[i])) { fprintf(stderr, "bad bbox\n"); return 2; }
    for (size_t i = 0; i < pts.size(); ++i)
        if (!rd(f, &pts[i])) { fprintf(stderr, "bad point\n"); return 2; }
    fclose(f);
    if (off[0] != 0 || off[(size_t)npoly] != ne) { fprintf(stderr, "offsets do not span the edges\n"); return 2; }
    for (long long p = 0; p < npt; ++p) {
        const double px = pts.at((size_t)p * 2), py = pts.at((size_t)p * 2 + 1);
        for (long long e = 0; e < ne; ++e) {
            const double *g = &edges.at((size_t)e * 4);
            bool ill = false;
            double lo = 0.0;
            const int bits = tz_edge_cross(g[0], g[1], g[2], g[3], px, py);
            const double d2 = tz_seg_d2(g[0], g[1], g[2], g[3], px, py, &ill, &lo);
            printf("E %lld %lld %d %d %a %a\n", p, e, bits, ill ? 1 : 0, d2, lo);
        }
        for (long long q = 0; q < npoly; ++q) {
            if (!tz_bbox_contains(&bbox.at((size_t)q * 4), px, py)) continue;
            int cross = 0, unc = 0;
            for (long long e = off.at((size_t)q); e < off.at((size_t)q + 1); ++e) {
                const double *g = &edges.at((size_t)e * 4);
                const int r = tz_edge_cross(g[0], g[1], g[2], g[3], px, py);
                cross ^= r & TZ_CROSS;
                unc |= r & TZ_CROSS_UNCERTAIN;
            }
            printf("P %lld %lld %d %d\n", p, q, cross, unc ? 1 : 0);
        }
    }
    return 0;
}
