"""The device math the kriging kernels rest on (twx_uk.h), evaluated by the library's own functions on the GPU
(tests/tools/devmath_probe.hip, run as a child process) and compared with high-precision references:

* exp_neg_f64 (table of 2^(j/256) + degree-4 polynomial: every element of the fp64 covariance build) against long-double
  exp, with the table in global memory and staged in LDS (the kernels use both);
* ellip_pair_f64 (fp64 covariance build, tie guard) and ellip_pair_fast (fp32 tail: default build, k_stn_nn's routing
  bound) against the 40-digit arbiter (oracle/arbiter.py) on station half-angle sines / cosines formed as
  twx_set_stations forms them;
* ellip_pair_vario (twx_vario.h: the semivariogram's pair distance on the hardware reciprocal / reciprocal square root)
  against the same arbiter and against ellip_pair_f64 on the same inputs, and its Newton helpers rcp_nr1 / sqrt_nr
  against long-double 1 / x and sqrt(x).

The compile-only test runs without a GPU, so a header change that breaks the probe shows up on a CPU box."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "devmath_probe.hip")
LN2_256 = np.log(np.longdouble(2)) / 256


def _compile(out_dir):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = os.path.join(str(out_dir), "devmath_probe")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "topowx_amd", "csrc"), SRC, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_devmath_probe_compiles(tmp_path):
    """CPU: the probe (the device functions exactly as the kernels include them) cross-compiles for gfx950."""
    exe = _compile(tmp_path)
    assert os.path.getsize(exe) > 0


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("devmath"))


def _run(exe, tmp_path, mode, arr, n):
    src, dst = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.ascontiguousarray(arr, np.float64).tofile(src)
    r = subprocess.run([exe, mode, str(n), src, dst], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        print(r.stderr)
        pytest.fail("devmath_probe %s exited with %d: %s" % (mode, r.returncode, r.stderr[-2000:]))
    out = np.fromfile(dst, np.float64)
    assert out.size == 2 * n
    return out[:n], out[n:]


def _exp_arguments():
    rng = np.random.default_rng(11)
    parts = [rng.uniform(-708.0, 0.0, 400000),                              # the whole normal range
             -10.0 ** rng.uniform(-30.0, 0.0, 150000),                      # dense near 0 (1 - x rounds to 1 below 2^-54)
             np.array([-5e-324, -2.2250738585072014e-308, -1e-300, -1e-200, -2.0 ** -53, -2.0 ** -54]),
             -708.0 + rng.uniform(0.0, 0.5, 10000),                         # the low end (2^-1022 at x = -708.396)
             rng.uniform(-745.2, -708.4, 20000),                            # subnormal results (and 0 below -745.13)
             rng.uniform(-800.0, -745.2, 2000)]
    # table-index boundaries: k = rint(x 256 / ln 2) changes at (j + 1/2) ln 2 / 256, the table entry is exact at j ln 2 / 256;
    # both, and 1 .. 2 ulps to either side
    j = rng.integers(0, int(708 * 256 / math.log(2)), 40000).astype(np.longdouble)
    for off in (0.0, 0.5):
        b = (-(j + off) * LN2_256).astype(np.float64)
        b = b[b >= -708.0]
        lo1, hi1 = np.nextafter(b, -np.inf), np.nextafter(b, 0.0)
        parts += [b, lo1, hi1, np.nextafter(lo1, -np.inf), np.nextafter(hi1, 0.0)]
    return np.concatenate(parts)


@pytest.mark.gpu
def test_exp_neg_f64_against_long_double(probe, tmp_path):
    """exp_neg_f64 against long-double exp on ~1e6 arguments: <= 1.5 ulp wherever the result is normal (the comment's
    figure is 1.33), within one subnormal unit below that, exactly 1 at +-0, exactly 0 at -inf, NaN and below -800;
    the LDS-staged table gives the same bits as the global one.  Measured on gfx950: max 1.331 ulp (normal range);
    0.977 subnormal units (a final scaling rounded to nearest would stay within 0.5: harmless for covariances, which
    are psill times this, but the bar is the full unit)."""
    x = _exp_arguments()
    special = np.array([0.0, -0.0, -np.inf, np.nan, -800.0, -800.5, -1e3, -1e300, -np.finfo(np.float64).max])
    allx = np.concatenate([x, special])
    g, l = _run(probe, tmp_path, "exp", allx, allx.size)
    assert np.array_equal(g.view(np.uint64), l.view(np.uint64)), "LDS and global tables differ"
    gs = g[x.size:]
    assert gs[0] == 1.0 and gs[1] == 1.0, gs[:2]
    assert np.all(gs[2:] == 0.0) and not np.any(np.signbit(gs[2:])), gs[2:]
    g = g[:x.size]
    ref = np.exp(x.astype(np.longdouble))
    err = np.abs(g.astype(np.longdouble) - ref)
    normal = ref >= np.longdouble(2.0) ** -1022
    assert normal.sum() > 900000
    _, e = np.frexp(ref[normal])
    ulp = np.ldexp(np.longdouble(1), e - 53)                                # ulp of the binade of the exact value
    ulps = (err[normal] / ulp).astype(np.float64)
    worst = float(ulps.max())
    i = int(np.argmax(ulps))
    assert worst <= 1.5, (worst, float(x[normal][i]))
    sub = ~normal
    assert sub.sum() > 10000
    sub_err = float((err[sub] / np.longdouble(2.0) ** -1074).max())
    assert sub_err <= 1.0, sub_err
    print("exp_neg_f64: max %.3f ulp (normal), %.3f subnormal units" % (worst, sub_err))


def _trig(lon, lat):
    r = 3.14159265358979323846 / 180.0                                       # the constant and operation order of twx_set_stations
    return (math.sin(lat * r / 2.0), math.cos(lat * r / 2.0), math.sin(lon * r / 2.0), math.cos(lon * r / 2.0))


def _dest(lon, lat, c, th):
    """The point at central angle c (sphere) and bearing th from (lon, lat), degrees; longitude wrapped to [-180, 180)."""
    p1, l1 = math.radians(lat), math.radians(lon)
    p2 = math.asin(math.sin(p1) * math.cos(c) + math.cos(p1) * math.sin(c) * math.cos(th))
    l2 = l1 + math.atan2(math.sin(th) * math.sin(c) * math.cos(p1), math.cos(c) - math.sin(p1) * math.sin(p2))
    return (math.degrees(l2) + 180.0) % 360.0 - 180.0, math.degrees(p2)


def _sd(a, b):
    """S = sin^2 of half the central angle, from the half-angle values, in fp64 (the branch variable of both functions)."""
    sG, sL = a[0] * b[1] - a[1] * b[0], a[2] * b[3] - a[3] * b[2]
    return sG * sG + (a[1] * a[1] - a[0] * a[0]) * (b[1] * b[1] - b[0] * b[0]) * sL * sL


def _pairs():
    rng = np.random.default_rng(12)
    pairs = []                                                                # (lon1, lat1, lon2, lat2, kind)
    for _ in range(12000):                                                    # 10 m .. 3000 km, latitudes -60 .. 80
        lon, lat = rng.uniform(-180, 180), rng.uniform(-60, 80)
        c = 10.0 ** rng.uniform(-2, math.log10(3000.0)) / 6371.0
        pairs.append((lon, lat) + _dest(lon, lat, c, rng.uniform(0, 2 * math.pi)) + ("sep",))
    for th, kind in ((4e-3, "f64_switch"), (0.01, "fast_switch")):           # both sides of each near / far switch
        for _ in range(3000):
            lon, lat = rng.uniform(-180, 180), rng.uniform(-60, 80)
            eps = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-12, -2)
            c = 2 * math.asin(math.sqrt(th * (1 + eps)))
            pairs.append((lon, lat) + _dest(lon, lat, c, rng.uniform(0, 2 * math.pi)) + (kind,))
    for _ in range(300):                                                      # coincident points
        lon, lat = rng.uniform(-180, 180), rng.uniform(-60, 80)
        pairs.append((lon, lat, lon, lat, "same"))
    return pairs


def _exact_on_inputs(a, b):
    """The sp / gstat formula, 40 digits, on the fp64 half-angle values the device reads (what the function alone
    can be held to: the rounding of those values themselves is the arbiter's business)."""
    import mpmath as mp
    from oracle import arbiter
    with mp.workdps(40):
        sp1, cp1, sl1, cl1 = (mp.mpf(v) for v in a)
        sp2, cp2, sl2, cl2 = (mp.mpf(v) for v in b)
        sG, sL = sp1 * cp2 - cp1 * sp2, sl1 * cl2 - cl1 * sl2
        cc = (cp1 ** 2 - sp1 ** 2) * (cp2 ** 2 - sp2 ** 2)
        sG2 = sG ** 2
        S = sG2 + cc * sL ** 2
        cF2, C = cc + sG2, 1 - S
        w = mp.asin(mp.sqrt(S))
        R = mp.sqrt(S * C) / w
        H1, H2 = (3 * R - 1) / (2 * C), (3 * R + 1) / (2 * S)
        f = 1 / arbiter.F_INV
        return 2 * w * arbiter.A_KM * (1 + f * H1 * (1 - cF2) * (1 - sG2) - f * H2 * cF2 * sG2)


@pytest.fixture(scope="module")
def pair_refs():
    """The pairs of _pairs(), their half-angle values, S, and both 40-digit references -- once for the tests that share them."""
    from oracle import arbiter
    pairs = _pairs()
    n = len(pairs)
    tg = np.array([_trig(p[0], p[1]) + _trig(p[2], p[3]) for p in pairs])
    kind = np.array([p[4] for p in pairs])
    same = kind == "same"
    ref = np.array([float(arbiter.ellip_dist(p[0], p[1], p[2], p[3])) if p[4] != "same" else 0.0 for p in pairs])
    own = np.array([float(_exact_on_inputs(tg[i, :4], tg[i, 4:])) if not same[i] else 0.0 for i in range(n)])
    sd = np.array([_sd(tg[i, :4], tg[i, 4:]) for i in range(n)])
    for a in (tg, ref, own, sd):
        a.setflags(write=False)
    return dict(pairs=pairs, tg=tg, kind=kind, same=same, ref=ref, own=own, sd=sd)


@pytest.mark.gpu
def test_pair_distances_against_the_arbiter(probe, tmp_path, pair_refs):
    """ellip_pair_f64 and ellip_pair_fast on ~1.8e4 pairs: 10 m .. 3000 km apart, latitudes -60 .. 80, pairs on both
    sides of each near / far switch (S = 4e-3 for the fp64 function, 0.01 for the fast one) and coincident points
    (exactly 0 in both).

    Bars and what was measured on gfx950:
      * ellip_pair_fast: <= 6e-7 relative to the arbiter (twice the 3e-7 that TWX_F64_AMP is derived from);
        measured 2.56e-7;
      * ellip_pair_f64, its own arithmetic (against the same formula in 40 digits on the same fp64 half-angle values):
        <= 1e-11 relative at >= 100 m; measured 6.1e-12;
      * ellip_pair_f64 against the arbiter (from degrees): the half-angle values are each rounded to fp64 before the
        function sees them, which limits sin G and sin L to ~1e-16 absolute, i.e. the distance to ~2e-12 km
        ABSOLUTE at any separation -- ~3e-11 relative at 100 m (the ~5e-12 of the comment in twx_uk.h is the
        function's own arithmetic on those values, the figure above).  Bar: |d| <= 4e-12 km + 1e-13 h; measured 2.84e-12 km."""
    pairs, tg, kind, same = (pair_refs[k] for k in ("pairs", "tg", "kind", "same"))
    ref, own, sd = (pair_refs[k] for k in ("ref", "own", "sd"))
    n = len(pairs)
    h64, hf = _run(probe, tmp_path, "dist", tg, n)
    assert np.all(h64[same] == 0.0) and np.all(hf[same] == 0.0)
    for th, k in ((4e-3, "f64_switch"), (0.01, "fast_switch")):              # both sides of each switch reached
        s = sd[kind == k]
        assert (s < th).sum() > 500 and (s > th).sum() > 500, (k, (s < th).sum(), (s > th).sum())
    m = ~same
    assert ref[m].min() < 0.012 and ref[m].max() > 2900.0
    rel_fast = np.abs(hf[m] - ref[m]) / ref[m]
    far = m & (ref >= 0.1)
    rel_own = np.abs(h64[far] - own[far]) / own[far]
    abs64 = np.abs(h64[m] - ref[m])
    print("ellip_pair_fast: max rel %.3g; ellip_pair_f64: own max rel %.3g (>= 100 m), abs vs arbiter %.3g km"
          % (rel_fast.max(), rel_own.max(), abs64.max()))
    i = int(np.argmax(rel_fast))
    assert rel_fast.max() <= 6e-7, (rel_fast.max(), pairs[np.nonzero(m)[0][i]])
    i = int(np.argmax(rel_own))
    assert rel_own.max() <= 1e-11, (rel_own.max(), pairs[np.nonzero(far)[0][i]])
    bound = 4e-12 + 1e-13 * ref[m]
    i = int(np.argmax(abs64 / bound))
    assert np.all(abs64 <= bound), (abs64[i], pairs[np.nonzero(m)[0][i]])


@pytest.mark.gpu
def test_vario_pair_distance_against_the_arbiter(probe, tmp_path, pair_refs):
    """ellip_pair_vario (twx_vario.h: the semivariogram's pair distance, hardware reciprocal / reciprocal square root with
    Newton steps) on the pairs of the test above, next to ellip_pair_f64 on the same inputs:

      * coincident points: exactly 0;
      * S >= 4e-3 (both functions call ellip_far_f64): the same bits;
      * S < 4e-3: the bars ellip_pair_f64 is held to -- own arithmetic <= 1e-11 relative at >= 100 m, against the arbiter
        from degrees |d| <= 4e-12 km + 1e-13 h -- and <= 1e-14 relative to ellip_pair_f64 at >= 100 m (the larger of the two
        figures of the header's claim: "the main term to an ulp or two, the correction terms to ~1e-14").

    Measured on gfx950: own max rel 6.09e-12 (>= 100 m), abs vs arbiter 2.84e-12 km -- ellip_pair_f64's own figures --,
    max rel difference from ellip_pair_f64 3.67e-16 (>= 100 m): under two ulp, so the header's "a few ulp" holds and a
    pair changes its 5 km bin with probability ~1e-15."""
    pairs, tg, kind, same = (pair_refs[k] for k in ("pairs", "tg", "kind", "same"))
    ref, own, sd = (pair_refs[k] for k in ("ref", "own", "sd"))
    n = len(pairs)
    hv, h64 = _run(probe, tmp_path, "vdist", tg, n)
    assert np.all(hv[same] == 0.0) and not np.any(np.signbit(hv[same]))
    s = sd[kind == "f64_switch"]
    assert (s < 4e-3).sum() > 500 and (s >= 4e-3).sum() > 500, ((s < 4e-3).sum(), (s >= 4e-3).sum())
    far_side, near_side = ~same & (sd >= 4e-3), ~same & (sd < 4e-3)
    assert far_side.sum() > 500 and near_side.sum() > 500
    assert np.array_equal(hv[far_side].view(np.uint64), h64[far_side].view(np.uint64))
    m = ~same
    assert ref[near_side].min() < 0.012 and ref[near_side].max() > 800.0
    m100 = near_side & (ref >= 0.1)
    rel_own = np.abs(hv[m100] - own[m100]) / own[m100]
    rel_f64 = np.abs(hv[m100] - h64[m100]) / h64[m100]
    absv = np.abs(hv[m] - ref[m])
    print("ellip_pair_vario: own max rel %.3g (>= 100 m), abs vs arbiter %.3g km, vs ellip_pair_f64 max rel %.3g (>= 100 m)"
          % (rel_own.max(), absv.max(), rel_f64.max()))
    i = int(np.argmax(rel_own))
    assert rel_own.max() <= 1e-11, (rel_own.max(), pairs[np.nonzero(m100)[0][i]])
    bound = 4e-12 + 1e-13 * ref[m]
    i = int(np.argmax(absv / bound))
    assert np.all(absv <= bound), (absv[i], pairs[np.nonzero(m)[0][i]])
    i = int(np.argmax(rel_f64))
    assert rel_f64.max() <= 1e-14, (rel_f64.max(), pairs[np.nonzero(m100)[0][i]])


def _newton_arguments():
    rng = np.random.default_rng(13)
    sd = 10.0 ** rng.uniform(-13.0, math.log10(4e-3), 40000)                  # what ellip_pair_vario hands them
    P = np.full_like(sd, 0.01396484375)
    for c in (0.017352764423076924, 0.022372159090909092, 0.030381944444444444, 0.044642857142857144, 0.075,
              0.16666666666666666, 1.0):
        P = P * sd + c
    assert P.min() >= 1.0 and P.max() < 1.001
    e = np.arange(-66, 11)                                                    # 2^-66 < 1e-20, 2^10 > 1e3
    p2 = np.ldexp(1.0, e)
    parts = [sd, 2.0 * sd, 2.0 * (1.0 - sd), P,
             10.0 ** rng.uniform(-20.0, 3.0, 60000),
             p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf), np.nextafter(np.nextafter(p2, 0.0), 0.0),
             np.nextafter(np.nextafter(p2, np.inf), np.inf)]
    return np.concatenate(parts)


def _ulps(got, ref):
    _, e = np.frexp(ref)
    ulp = np.ldexp(np.longdouble(1), e - 53)                                  # ulp of the binade of the exact value
    return (np.abs(got.astype(np.longdouble) - ref) / ulp).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("helper", ("sqrt_nr", "rcp_nr1"))
def test_vario_newton_helpers(probe, tmp_path, helper):
    """rcp_nr1 and sqrt_nr (twx_vario.h) against long-double 1 / x and sqrt(x) on ~2.2e5 arguments: those
    ellip_pair_vario gives them (S in [1e-13, 4e-3], 2 S, 2 C near 2, P in [1, 1.001]), log-uniform x in [1e-20, 1e3],
    powers of two and their neighbours.  Bar: 2 ulp each ("an ulp or two").

    Measured on gfx950: sqrt_nr max 0.500 ulp (and still 0.500 without its second Newton step: the closing correction
    squares the error once more, so that step buys nothing the bar can see); rcp_nr1 max 0.500 ulp.

    This test found rcp_nr1 at 10.598 ulp (x = 8.3e-17) with the single Newton step it had: the hardware reciprocal is
    good to ~2^-25 here and one step leaves ~2^-50, 1.2e-15 relative -- inside the "~1e-14" twx_vario.h claims for the
    correction terms the reciprocal serves, but not "an ulp or two".  It has a second step since (two fma per use, three
    uses per pair of a point list)."""
    x = _newton_arguments()
    assert x.size > 200000 and x.min() > 0.0
    rcp, sq = _run(probe, tmp_path, "vmath", x, x.size)
    xl = x.astype(np.longdouble)
    u = _ulps(sq, np.sqrt(xl)) if helper == "sqrt_nr" else _ulps(rcp, 1 / xl)
    i = int(np.argmax(u))
    print("%s: max %.3f ulp at %r" % (helper, u[i], float(x[i])))
    assert u[i] <= 2.0, (helper, u[i], float(x[i]))
