"""Argument sets and float64 / long-double references for the tests of the kernels' sine and cosine (mw_math.h: sincos_fast_f32, the
reduction to a revolution fraction r followed by v_sin_f32 / v_cos_f32, and the polynomial sincos_f32), shared by the CPU tier
(tests/test_device_math_cpu.py: the reduction, on the host build of the same source) and the GPU tier (tests/test_device_math_gpu.py:
the instruction on top of it).

Every symmetric set is laid out [a, -a]: element i of the first half and element i of the second half are exact negatives, so the
symmetry tests compare the two halves of ONE launch.
"""
import numpy as np

import workloads

TWO_PI_LD = np.longdouble("6.283185307179586476925286766559")
MW_PI_F = np.float32(3.1415926536)          # mw_math.h

# The reduction's own error, as an error of sin / cos, for |x| <= 5e5 rad.  r = (p - rint(p)) + e is rounded once at the end: half an
# ulp of r, which is 2^-26 revolutions for |r| in [0.25, 0.5) and 2^-25 for |r| in [0.5, 1).  cos is flat where |r| >= 0.5 (|sin| there
# is < 0.05 for |r| <= 0.507) and steepest at |r| = 0.25: 2 pi 2^-26 = 9.4e-8.  sin is steepest at |r| = 0.5: 2 pi 2^-25 = 1.87e-7.  What
# the two FMAs of e add is below 2^-30 revolutions (3.7e-8 * |x| ulp-of-lo terms, x <= 5e5).
RED_BOUND_SIN = 1.9e-7
RED_BOUND_COS = 1.0e-7
RED_BOUND_REV = 2.0 ** -25 + 2.0 ** -30     # the same statement in revolutions, against a long-double fraction
POLY_BOUND = 1.5e-7                         # sincos_f32, |x| <= 1e5 (mw_math.h)
POLY_DOMAIN = 1.0e5
HARD_CAP = 1.0e-6                           # what the pond tolerances were written against


def _sym(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.concatenate([a, -a])


def _nearest_f32(v_ld):
    return np.asarray(v_ld, np.longdouble).astype(np.float64).astype(np.float32)


def uniform_sweep():
    """Set 1: 2^20 uniformly spaced values over [-2 pi, 2 pi] (2^19 over [0, 2 pi] and their negatives)."""
    return _sym(np.linspace(0.0, 2.0 * np.pi, 1 << 19))


def half_revolution_band():
    """Set 2: EVERY float32 with |x| / 2 pi in [0.4998, 0.5002] (about 2e4 values): the band around x = +-pi in which the host's r
    passes through +-0.5, rint's ties flip, and the instruction is used at and past the end of its nominal interval.  It contains every
    x near +-pi whose |r| lies in [0.4999, 0.5002]."""
    lo, hi = np.float32(2 * np.pi * 0.4998), np.float32(2 * np.pi * 0.5002)
    bits = np.arange(int(lo.view(np.int32)), int(hi.view(np.int32)) + 1, dtype=np.int32)
    return _sym(bits.view(np.float32))


def sincos_zeros():
    """Set 3: the nearest float32 to k pi/2 for every k in [0, 2^17) with its +-1 and +-2 ulp neighbours, both signs."""
    c = _nearest_f32(np.arange(1 << 17).astype(np.longdouble) * (TWO_PI_LD / 4))
    inf = np.float32(np.inf)
    u1, d1 = np.nextafter(c, inf), np.nextafter(c, -inf)
    return _sym(np.concatenate([c, u1, np.nextafter(u1, inf), d1, np.nextafter(d1, -inf)]))


def half_revolutions():
    """Set 4: the nearest float32 to (n + 1/2) 2 pi for n in [0, 16384), both signs."""
    return _sym(_nearest_f32((np.arange(16384).astype(np.longdouble) + np.longdouble(0.5)) * TWO_PI_LD))


def log_spaced(lo_log2, hi, seed):
    """Set 5: 2^18 magnitudes 2^e, e uniform in [lo_log2, log2 hi] (random mantissas, denormals included), both signs."""
    rng = np.random.default_rng(seed)
    a = np.exp2(rng.uniform(lo_log2, np.log2(hi), 1 << 18)).astype(np.float32)
    return _sym(np.minimum(a, np.float32(hi)))


def symmetric_sets():
    """Sets 1-5, name -> float32 [a, -a].  '5a' ends at 1e5 rad, '5b' covers 1e5 .. 5e5 (what omega*t reaches after a day)."""
    return {
        "1 uniform sweep [-2pi, 2pi]": uniform_sweep(),
        "2 band past +-0.5 revolutions": half_revolution_band(),
        "3 zeros of sin and cos": sincos_zeros(),
        "4 half revolutions": half_revolutions(),
        "5a log-spaced 2^-149 .. 1e5": log_spaced(-149.0, 1.0e5, 11),
        "5b log-spaced 1e5 .. 5e5": log_spaced(np.log2(1.0e5), 5.0e5, 12),
    }


def pond_phases(t):
    """Set 6b: frequency * (dx px + dy pz) + t speed in float32, pond_lattice(100) x pond_waves8()."""
    pos = workloads.pond_lattice(100)
    px, pz = pos[:, 0:1], pos[:, 2:3]
    w = np.asarray(workloads.pond_waves8(), np.float32)
    dx, dy, sp = w[None, :, 0], w[None, :, 1], w[None, :, 2]
    ph = np.float32(workloads.POND["frequency"]) * (dx * px + dy * pz) + np.float32(t) * sp
    assert ph.dtype == np.float32
    return np.ascontiguousarray(ph.ravel())


def box_muller_angles():
    """Set 6c: 2 pi u in float32 for 2^16 values of u in (0, 1] on the generator's 2^-24 lattice (uniform01), both ends included."""
    k = np.random.default_rng(13).integers(0, 1 << 24, 1 << 16).astype(np.uint32)
    k[0], k[1] = 0, (1 << 24) - 1
    u = (k + np.uint32(1)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (np.float32(2.0) * MW_PI_F) * u


def host_formed_sets():
    """The part of set 6 that needs no device: name -> float32."""
    return {
        "6b pond phases t=3.25": pond_phases(3.25),
        "6b pond phases t=3600": pond_phases(3600.0),
        "6c Box-Muller angles": box_muller_angles(),
    }


def ref64(x):
    """numpy float64 sin / cos of the float32 input widened to float64."""
    xd = np.asarray(x, np.float32).astype(np.float64)
    return np.sin(xd), np.cos(xd)


def of_fraction64(r):
    """float64 sin / cos of 2 pi r for a float32 revolution fraction r."""
    a = 2.0 * np.pi * np.asarray(r, np.float32).astype(np.float64)
    return np.sin(a), np.cos(a)


def fraction_error_rev(x, r, whole=False):
    """|r - (x / 2 pi - rint(x / 2 pi))| in revolutions, the fraction formed in long double.  Whole revolutions do not count (r may sit
    just past +0.5 where the exact fraction sits just above -0.5) unless whole=True."""
    q = np.asarray(x, np.float32).astype(np.longdouble) / TWO_PI_LD
    d = np.asarray(r, np.float32).astype(np.longdouble) - (q - np.rint(q))
    return np.abs(d if whole else d - np.rint(d)).astype(np.float64)


def three_numbers(x, s, c, r_host):
    """(total, hw, red), each a (sin, cos) pair of maxima: total = |result - f64(x)|, hw = |result - f64 sin/cos(2 pi r_host)|, red =
    |f64 sin/cos(2 pi r_host) - f64(x)| (the reduction alone)."""
    (sx, cx), (sr, cr) = ref64(x), of_fraction64(r_host)
    s, c = np.asarray(s, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    mx = lambda a, b: float(np.abs(a - b).max())
    return (mx(s, sx), mx(c, cx)), (mx(s, sr), mx(c, cr)), (mx(sr, sx), mx(cr, cx))
