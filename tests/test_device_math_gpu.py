"""GPU tier (-m gpu): the device sine / cosine itself, through the hooks mw_debug_sincos_fast (sincos_fast_f32: what every product
kernel runs -- the reduction to a revolution fraction r, then v_sin_f32 / v_cos_f32) and mw_debug_sincos (the polynomial sincos_f32),
against numpy float64 sin / cos of the float32 argument widened to float64.

Three numbers per argument set (tests/device_math_sets.py), for sin and cos separately:
    total = max |device - f64(x)|
    hw    = max |device - f64 sin/cos(2 pi r_host)|      r_host: the HOST build of the same reduction (emul.sincos)
    red   = max |f64 sin/cos(2 pi r_host) - f64(x)|       the reduction alone, asserted on the CPU (tests/test_device_math_cpu.py)

Bounds.  red_bound = 1.9e-7 (sin) / 1.0e-7 (cos) is derived (device_math_sets.py).  The instruction's share cannot be derived: it was
MEASURED once on an MI355X over sets 1 and 2, hw = HW_MEASURED below, and HW_BOUND = 1.5 x that is asserted (the sweep samples r, it is
not exhaustive).  The tight bound of every set is red_bound + HW_BOUND; the hard cap 1e-6 is a condition, not a measurement.

Measured on an MI355X, sin / cos (the module fixture prints this table on every run):
    set                                max |x|   max |r|   total                red                  hw
    1 uniform sweep [-2pi, 2pi]        6.28      0.499999  1.778e-7 / 1.773e-7  9.36e-8 / 9.36e-8    1.244e-7 / 1.191e-7
    2 band past +-0.5 revolutions      3.14      0.500000  9.38e-8 / 5.95e-8    9.36e-8 / 1.2e-10    5.0e-10 / 5.95e-8
    3 zeros of sin and cos             205886    0.502288  1.913e-7 / 1.151e-7  1.877e-7 / 9.43e-8   1.066e-7 / 1.050e-7
    4 half revolutions                 102941    0.500621  1.878e-7 / 6.12e-8   1.872e-7 / 7.1e-10   1.6e-9 / 6.08e-8
    5a log-spaced 2^-149 .. 1e5        99994     0.499982  1.560e-7 / 1.727e-7  9.34e-8 / 9.33e-8    1.132e-7 / 1.211e-7
    5b log-spaced 1e5 .. 5e5           499997    0.506994  1.991e-7 / 1.774e-7  1.870e-7 / 9.45e-8   1.243e-7 / 1.204e-7
    6a omega*t 64^2, 256^2 (6 grids)   568314    0.506575  1.834e-7 / 1.094e-7  1.855e-7 / 9.16e-8   8.74e-8 / 1.094e-7
    6b pond phases t = 3.25, 3600      4450      0.500049  1.700e-7 / 1.697e-7  1.042e-7 / 9.34e-8   1.211e-7 / 1.199e-7
    6c Box-Muller angles               6.28      0.499998  1.706e-7 / 1.740e-7  9.35e-8 / 9.35e-8    1.226e-7 / 1.200e-7
hw over sets 1 and 2: 1.244e-7 (sin) / 1.191e-7 (cos); asserted HW_BOUND = 1.866e-7 / 1.787e-7; tight bound 3.766e-7 / 2.787e-7.  The
sets that put r past +-0.5 (3, 4, 5b, 6a) show no larger hw than the sweep inside [-0.5, 0.5].  The polynomial sincos_f32 stays below
9.2e-8 on every set, the ones past its 1e5 rad domain included.
"""
import ctypes as C

import numpy as np
import pytest

import device_math_sets as D
import workloads

pytestmark = pytest.mark.gpu

# max |v_sin_f32(r) - sin(2 pi r)|, |v_cos_f32(r) - cos(2 pi r)| measured on an MI355X over sets 1 and 2, and what is asserted (1.5 x)
HW_MEASURED = {"sin": 1.244e-7, "cos": 1.191e-7}
HW_BOUND = {k: 1.5 * v for k, v in HW_MEASURED.items()}
TIGHT = {"sin": D.RED_BOUND_SIN + HW_BOUND["sin"], "cos": D.RED_BOUND_COS + HW_BOUND["cos"]}
MAX_LAUNCH = 1 << 22


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_sincos(mw, x, fast):
    """One launch of the hook over float32 x -> (sin, cos)."""
    x = np.ascontiguousarray(x, np.float32)
    assert 1 <= x.size <= MAX_LAUNCH
    s, c = np.empty_like(x), np.empty_like(x)
    fn = mw.lib().mw_debug_sincos_fast if fast else mw.lib().mw_debug_sincos
    mw.check(fn(_p(x), x.size, _p(s), _p(c)))
    return s, c


class Run:
    def __init__(self, mw, emul, x):
        self.x = np.ascontiguousarray(x, np.float32)
        self.s, self.c = device_sincos(mw, self.x, True)        # sincos_fast_f32
        self.ps, self.pc = device_sincos(mw, self.x, False)     # sincos_f32
        self.r = emul.sincos(self.x, fast=True)[2]
        self.total, self.hw, self.red = D.three_numbers(self.x, self.s, self.c, self.r)
        sx, cx = D.ref64(self.x)
        self.poly_total = (float(np.abs(self.ps - sx).max()), float(np.abs(self.pc - cx).max()))


@pytest.fixture(scope="module")
def runs(mw, emul):
    """name -> Run for sets 1-6: two launches per set (one per hook), computed once and left unchanged."""
    sets = dict(D.symmetric_sets())
    for N in (64, 256):                       # 6a: the arguments the FFTMesh kernels form (pinned bit for bit in test_gpu_parity.py)
        p = workloads.fftmesh_params(N)
        with mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                      choppiness=p.choppiness, gravity=p.gravity) as o:
            for t, tn in ((1.0 / 60.0, "1/60"), (3600.0, "3600"), (86400.0, "86400")):
                sets[f"6a omega*t N={N} t={tn}"] = o.debug_omega_t(t).ravel()
    sets.update(D.host_formed_sets())
    out = {name: Run(mw, emul, x) for name, x in sets.items()}
    print()
    for name, r in out.items():
        print(f"{name} (n={r.x.size}, max |x| {float(np.abs(r.x).max()):.6g}, max |r| {float(np.abs(r.r).max()):.6f}): "
              f"total {r.total[0]:.3e}/{r.total[1]:.3e}  red {r.red[0]:.3e}/{r.red[1]:.3e}  hw {r.hw[0]:.3e}/{r.hw[1]:.3e}  "
              f"sincos_f32 total {r.poly_total[0]:.3e}/{r.poly_total[1]:.3e}   (sin/cos)")
    return out


def symmetric(runs):
    return {k: v for k, v in runs.items() if k[0] in "12345"}


def test_sets_cover_what_the_kernels_reach(runs):
    assert len(runs) == 15 and all(np.isfinite(r.x).all() for r in runs.values())
    assert float(np.abs(runs["6a omega*t N=256 t=86400"].x).max()) > 4.0e5        # past the old "|x| <~ 1e5" comment
    assert max(float(np.abs(r.x).max()) for r in runs.values()) <= 6.0e5          # omega*t after a day: 5.7e5 rad
    assert max(float(np.abs(r.r).max()) for r in runs.values()) > 0.505           # and r past +-0.5


def test_hard_cap_both_hooks(runs):
    """total <= 1e-6 on sets 1-6 for both hooks: the looser figure the pond tolerances were written against."""
    for name, r in runs.items():
        assert max(r.total) <= D.HARD_CAP, f"set {name}: sincos_fast_f32 total sin {r.total[0]:.3e} / cos {r.total[1]:.3e} above 1e-6"
        assert max(r.poly_total) <= D.HARD_CAP, f"set {name}: sincos_f32 total sin {r.poly_total[0]:.3e} / cos {r.poly_total[1]:.3e} above 1e-6"


def test_instruction_error_where_it_was_measured(runs):
    """hw on sets 1 and 2 (where HW_MEASURED comes from) stays within 1.5 x the recorded measurement; 8e-7 would endanger the hard cap."""
    for name, r in runs.items():
        if name[0] in "12":
            assert r.hw[0] <= HW_BOUND["sin"] and r.hw[1] <= HW_BOUND["cos"], f"set {name}: hw sin {r.hw[0]:.3e} / cos {r.hw[1]:.3e}, bound {HW_BOUND}"
    assert max(HW_MEASURED.values()) < 8e-7


def test_tight_bound_per_set(runs):
    """total <= red_bound + HW_BOUND on every set, and the host's reduction alone within red_bound on the arguments of set 6 too.

    Measured on an MI355X (sin / cos): hw over sets 1 and 2 = 1.244e-7 / 1.191e-7 (HW_MEASURED); asserted HW_BOUND = 1.5 x that =
    1.866e-7 / 1.787e-7, so total <= 3.766e-7 / 2.787e-7.  The largest total measured is 1.991e-7 / 1.774e-7 (set 5b); the per-set
    table is in the module docstring."""
    for name, r in runs.items():
        assert r.red[0] <= D.RED_BOUND_SIN and r.red[1] <= D.RED_BOUND_COS, f"set {name}: reduction alone sin {r.red[0]:.3e} / cos {r.red[1]:.3e}"
        assert r.total[0] <= TIGHT["sin"] and r.total[1] <= TIGHT["cos"], (
            f"set {name}: total sin {r.total[0]:.3e} / cos {r.total[1]:.3e} above red_bound + hw_bound = {TIGHT['sin']:.3e} / {TIGHT['cos']:.3e} "
            f"(red {r.red[0]:.3e} / {r.red[1]:.3e}, hw {r.hw[0]:.3e} / {r.hw[1]:.3e})")


def test_pythagoras(runs):
    """|sin^2 + cos^2 - 1| in float64 from the device's float32 outputs <= 2 x the tight bound (the larger of the two: to first order
    the deviation is 2 (sin dsin + cos dcos) <= 2 hypot(dsin, dcos))."""
    bound = 2.0 * max(TIGHT.values())
    for name, r in runs.items():
        s, c = r.s.astype(np.float64), r.c.astype(np.float64)
        dev = float(np.abs(s * s + c * c - 1.0).max())
        assert dev <= bound, f"set {name}: |sin^2 + cos^2 - 1| = {dev:.3e} above {bound:.3e}"


def test_symmetry(runs):
    """sin(-x) == -sin(x) and cos(-x) == cos(x) over sets 1-5 (each laid out [a, -a]), both hooks: every step of either reduction is
    sign-symmetric in the source, and the time-reversal property of the FFTMesh path leans on it."""
    for name, r in symmetric(runs).items():
        m = r.x.size // 2
        assert (r.x[:m] == -r.x[m:]).all()
        for tag, s, c in (("sincos_fast_f32", r.s, r.c), ("sincos_f32", r.ps, r.pc)):
            bs, bc = int((s[:m] != -s[m:]).sum()), int((c[:m] != c[m:]).sum())
            assert bs == 0 and bc == 0, f"set {name}: {tag} breaks the symmetry at {bs} sines and {bc} cosines of {m}"


def test_polynomial_matches_host_bit_for_bit(runs, emul):
    """sincos_f32 is "identical code on host and device": over the sets with |x| <= 1e5 (Cody-Waite exact for |k| < 2^17) the device
    equals the host build bit for bit and stays within 1.5e-7 of float64."""
    seen = 0
    for name, r in runs.items():
        keep = np.abs(r.x) <= D.POLY_DOMAIN
        if not keep.any():
            continue
        seen += int(keep.sum())
        hs, hc, _ = emul.sincos(r.x[keep], fast=False)
        ds, dc = r.ps[keep], r.pc[keep]
        bs, bc = int((ds.view(np.int32) != hs.view(np.int32)).sum()), int((dc.view(np.int32) != hc.view(np.int32)).sum())
        assert bs == 0 and bc == 0, f"set {name}: device sincos_f32 differs from the host build at {bs} sines and {bc} cosines of {int(keep.sum())}"
        sx, cx = D.ref64(r.x[keep])
        es, ec = float(np.abs(ds - sx).max()), float(np.abs(dc - cx).max())
        assert es <= D.POLY_BOUND and ec <= D.POLY_BOUND, f"set {name}: sincos_f32 total sin {es:.3e} / cos {ec:.3e} above 1.5e-7"
    assert seen > 2_000_000


@pytest.mark.parametrize("fast", [True, False], ids=["sincos_fast_f32", "sincos_f32"])
def test_special_values(mw, fast):
    """Set 7: plain arithmetic, nothing here faults."""
    tiny, fmin = np.float32(1e-45), np.finfo(np.float32).tiny
    x = np.array([0.0, -0.0, tiny, -tiny, fmin, -fmin, np.inf, -np.inf, np.nan], np.float32)
    s, c = device_sincos(mw, x, fast)
    assert (s[:2] == 0).all() and (c[:2] == 1).all(), (s[:2], c[:2])
    assert (np.abs(s[2:6]) <= np.abs(x[2:6])).all() and (c[2:6] == 1).all(), (s[2:6], c[2:6])
    assert np.isnan(s[6:]).all() and np.isnan(c[6:]).all(), (s[6:], c[6:])


@pytest.mark.parametrize("fast", [True, False], ids=["sincos_fast_f32", "sincos_f32"])
def test_hook_edges(mw, runs, fast):
    """Set 8: ragged counts return the bits of one large call; n = 0 and NULL pointers are MW_EINVAL."""
    big = runs["1 uniform sweep [-2pi, 2pi]"]
    S, Cc = (big.s, big.c) if fast else (big.ps, big.pc)
    for n in (1, 255, 257, 1000003):
        s, c = device_sincos(mw, big.x[:n], fast)
        assert (s.view(np.int32) == S[:n].view(np.int32)).all() and (c.view(np.int32) == Cc[:n].view(np.int32)).all(), f"n = {n}"
    fn = mw.lib().mw_debug_sincos_fast if fast else mw.lib().mw_debug_sincos
    x, s, c = np.ones(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32)
    assert fn(_p(x), 0, _p(s), _p(c)) == mw.MW_EINVAL
    assert fn(_p(x), -1, _p(s), _p(c)) == mw.MW_EINVAL
    assert fn(None, 4, _p(s), _p(c)) == mw.MW_EINVAL
    assert fn(_p(x), 4, None, _p(c)) == mw.MW_EINVAL
    assert fn(_p(x), 4, _p(s), None) == mw.MW_EINVAL
    assert (s == 0).all() and (c == 0).all()
