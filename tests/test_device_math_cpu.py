"""CPU tier of the sine/cosine tests: the HOST build of mw_math.h (tests/emul, emul_sincos) against long-double and float64 references.

The host evaluates sin(2 pi r) in double where the device issues v_sin_f32 / v_cos_f32, so this tier pins everything up to the
instruction: the two-constant reduction to a revolution fraction r (revolution_fraction_f32) and the polynomial sincos_f32.  The
instruction itself is tests/test_device_math_gpu.py.  The argument sets and the derivation of the bounds are in
tests/device_math_sets.py.
"""
import numpy as np
import pytest

import device_math_sets as D


@pytest.fixture(scope="module")
def host(emul):
    """name -> (x, s, c, r) of the host sincos_fast_f32 over sets 1-5, computed once."""
    out = {}
    for name, x in D.symmetric_sets().items():
        out[name] = (x,) + emul.sincos(x, fast=True)
    return out


def test_sets_are_what_they_claim():
    sets = D.symmetric_sets()
    sizes = {k[:2].strip(): v.size for k, v in sets.items()}
    assert sizes == {"1": 1 << 20, "2": sizes["2"], "3": 10 << 17, "4": 2 << 14, "5a": 1 << 19, "5b": 1 << 19}
    assert 1.5e4 < sizes["2"] < 3e4
    for name, x in sets.items():
        m = x.size // 2
        assert x.dtype == np.float32 and np.isfinite(x).all() and (x[:m] == -x[m:]).all(), name
        assert np.abs(x).max() <= 5.0e5, name
    assert np.abs(sets["5a log-spaced 2^-149 .. 1e5"]).max() <= 1.0e5 and (np.abs(sets["5a log-spaced 2^-149 .. 1e5"]) < 1.2e-38).any()
    assert np.abs(sets["5b log-spaced 1e5 .. 5e5"]).min() >= 1.0e5


def test_reduction_against_long_double_fraction(host):
    """r against x / 2 pi - rint(x / 2 pi) in long double: within 2^-25 + 2^-30 revolutions and |r| <= 0.51 for |x| <= 5e5.  A wrong hi or
    lo constant, or a contracted x * hi - rint(p), fails here (with lo = 0 already set 1 is off by 4.5e-8 revolutions)."""
    for name, (x, s, c, r) in host.items():
        err = D.fraction_error_rev(x, r)
        i = int(err.argmax())
        print(f"{name}: max |r| = {float(np.abs(r).max()):.8f}, max fraction error = {err[i]:.4e} rev at x = {float(x[i])!r}")
        assert err[i] <= D.RED_BOUND_REV, f"set {name}: r off by {err[i]:.4e} revolutions at x = {float(x[i])!r} (bound {D.RED_BOUND_REV:.4e})"
        assert np.abs(r).max() <= 0.51, f"set {name}: max |r| = {float(np.abs(r).max())}"


def test_r_passes_half_a_revolution(host):
    """The sets do reach what they are for: r hits +-0.5 in the band around +-pi and goes past it at the half revolutions (the
    instruction is relied on slightly outside [-0.5, 0.5]: mw_math.h)."""
    assert (np.abs(host["2 band past +-0.5 revolutions"][3]) >= 0.5).any()
    r4 = np.abs(host["4 half revolutions"][3])
    assert (r4 > 0.5).sum() > 1000 and r4.min() > 0.49
    assert np.abs(host["5b log-spaced 1e5 .. 5e5"][3]).max() > 0.503


def test_reduction_error_as_error_of_sin_cos(host):
    """red: float64 sin / cos of 2 pi r against float64 sin / cos of x -- the quantity the GPU tier adds the instruction's error to."""
    for name, (x, s, c, r) in host.items():
        total, hw, red = D.three_numbers(x, s, c, r)
        print(f"{name}: red sin {red[0]:.3e} cos {red[1]:.3e}; host float32 result against f64(x): sin {total[0]:.3e} cos {total[1]:.3e}")
        assert red[0] <= D.RED_BOUND_SIN and red[1] <= D.RED_BOUND_COS, f"set {name}: reduction error sin {red[0]:.3e} / cos {red[1]:.3e}"
        # the host's float32 results are that double sine rounded once: r_out IS the r sincos_fast_f32 used
        assert hw[0] <= 2.0 ** -25 and hw[1] <= 2.0 ** -25, f"set {name}: host result is not the rounded sin/cos of 2 pi r ({hw})"


def test_reduction_is_odd(host):
    for name, (x, s, c, r) in host.items():
        m = x.size // 2
        assert (r[:m] == -r[m:]).all() and (s[:m] == -s[m:]).all() and (c[:m] == c[m:]).all(), name


def test_zero_and_denormal_arguments_reduce_to_plus_zero(emul):
    x = np.array([0.0, -0.0, 1e-45, -1e-45], np.float32)
    s, c, r = emul.sincos(x, fast=True)
    assert (r == 0).all() and not np.signbit(r).any()
    assert (s == 0).all() and (c == 1).all()


def test_polynomial_sincos_host(emul):
    """sincos_f32 (the reference form kept for mw_debug_sincos): <= 1.5e-7 absolute on |x| <= 1e5, where its Cody-Waite reduction is
    exact."""
    for name, x in D.symmetric_sets().items():
        x = x[np.abs(x) <= D.POLY_DOMAIN]
        if x.size == 0:
            continue
        s, c, _ = emul.sincos(x, fast=False)
        sx, cx = D.ref64(x)
        es, ec = float(np.abs(s - sx).max()), float(np.abs(c - cx).max())
        print(f"{name}: sincos_f32 host sin {es:.3e} cos {ec:.3e}")
        assert es <= D.POLY_BOUND and ec <= D.POLY_BOUND, f"set {name}: sincos_f32 sin {es:.3e} / cos {ec:.3e}"


def test_reduction_ends_where_the_comment_says(emul):
    """Negative control: the domain in mw_math.h is a checked fact.  p = x * hi is a float32; from 2^23 revolutions (5.3e7 rad) on it has
    no fraction bits left, rint(p) = p, and r is the error term alone: no longer a fraction of a revolution.  Sampled over |x| <= 1e9:
    some r is further than 2^-20 revolutions from the long-double fraction and max |r| exceeds 1 (no claim about every argument up
    there; what is left of r modulo one revolution is printed, not asserted)."""
    rng = np.random.default_rng(14)
    x = rng.uniform(-1.0e9, 1.0e9, 1 << 18).astype(np.float32)
    s, c, r = emul.sincos(x, fast=True)
    err = D.fraction_error_rev(x, r, whole=True)
    print(f"|x| <= 1e9: max |r| = {float(np.abs(r).max()):.3f}, max |r - fraction| = {err.max():.3f} rev, modulo one revolution "
          f"{D.fraction_error_rev(x, r).max():.3e} rev")
    assert err.max() > 2.0 ** -20 and np.abs(r).max() > 1.0, (err.max(), np.abs(r).max())
    inside = np.abs(x) <= 5.0e5
    assert inside.any() and D.fraction_error_rev(x[inside], r[inside]).max() <= D.RED_BOUND_REV
