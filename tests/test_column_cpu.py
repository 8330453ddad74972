"""CPU tier of the water column (mw_ocean_set_column / mw_ocean_query_column, include/mistral_water.h; csrc/water_column.h).

* the model on the float64 oracle: a layer is e^{-k d} times the surface for one spectrum bin, its velocity layer is the time derivative of
  its position layer, and linear interpolation between layers stays within the Lagrange bound of e^{-k d};
* the MW_HD query functions built with g++ (tests/column_shim.cpp) against the float64 restatement of tests/column_ref.py, which locates
  every layer and brackets afterwards: tolerances measured against that restatement, bit identities, edges, continuity, tiling;
* the five entry points are exported and declared, and refuse a NULL handle with a status, without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import column_ref as CR
import periodic_ref as PR
import surface_ref as S
import velocity_ref as V
import workloads
from conftest import REPO

f32 = np.float32
CSRC = os.path.join(REPO, "mistral-water_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return CR.build_shim(str(tmp_path_factory.mktemp("col") / "libcol_shim.so"))


# the oracle's layers at N = 64, choppiness 0.46, L = 4: computed once, shared, never written
N64, T64, DEPTHS64 = 64, 1.25, np.array([0.0, 2.0, 6.0, 18.0], f32)


@pytest.fixture(scope="module")
def layers(oracle):
    p = workloads.fftmesh_params(N64)
    h0, h0c = oracle.generate_spectrum(p, 7)
    pos, vel = CR.layers_f64(p, h0, h0c, T64, DEPTHS64)
    d = dict(p=p, pos64=pos, vel64=vel, pos=pos.astype(f32), vel=vel.astype(f32), umax=float(np.abs(vel[0]).max()), rc=S.rest_coords(N64, 1.0))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def world_points(n, seed, lo=-28.0, hi=28.0, ylo=-22.0, yhi=1.0):
    rng = np.random.default_rng(seed)
    xz = rng.uniform(lo, hi, (n, 2))
    return np.stack([xz[:, 0], rng.uniform(ylo, yhi, n), xz[:, 1]], -1).astype(f32)


# ---- the model, on the oracle ------------------------------------------------------------------------------------------------------
def single_bin(p, n, m, value=(0.03, -0.02)):
    h0 = np.zeros((p.N, p.N, 2), f32)
    h0[n, m] = value
    return h0, np.zeros_like(h0)


def test_a_layer_of_one_bin_is_the_surface_times_exp_minus_k_d(oracle):
    """One spectrum bin on N = 16: every output is that bin's value times a fixed pattern, so layer l's displacement and velocity are
    A_l = e^{-k d_l} times layer 0's, k the bin's wave number.  The oracle takes a float32 spectrum, so the depths are chosen as
    j ln 2 / k: A_l is 2^-j to float64 rounding, float32(A_l h0) = 2^-j h0 exactly, and the law holds to 1e-12 relative.  k is the
    float32-sequence value whose sqrt(g k) is the dispersion (column_ref.wave_number); it is held to the float64 formula
    pi |(2n - N, 2m - N)| / length to 4 float32 roundings.  A wrong k, sign or weighting order fails in the first digit."""
    p = workloads.fftmesh_params(16)
    n, m = 10, 9
    h0, h0c = single_bin(p, n, m)
    k = CR.wave_number(p)[n, m]
    k_formula = np.pi * np.hypot(2 * n - p.N, 2 * m - p.N) / p.length
    assert abs(k - k_formula) <= 4 * 2.0 ** -24 * k_formula
    # the dispersion the velocity weights with is sqrt(g k) of this k, floored to the base frequency (S/FFTMesh.cs:141-147)
    w0 = 2 * np.pi / p.length
    assert abs(V.fftmesh_omega(p)[n, m] - np.floor(np.sqrt(p.gravity * k) / w0) * w0) <= 1e-5
    depths = np.array([0.0, 1.0, 3.0]) * np.log(2.0) / k
    pos, vel = CR.layers_f64(p, h0, h0c, 0.75, depths)
    rest = oracle.rest_mesh(p)[0].astype(np.float64)
    d0 = pos[0] - rest
    assert np.abs(d0).max() > 1e-3 and np.abs(vel[0]).max() > 1e-3
    for l, d in enumerate(depths):
        A = np.exp(-k_formula * d) if l == 0 else np.exp(-k * d)
        assert abs(A - 2.0 ** -[0, 1, 3][l]) < 1e-15
        assert np.abs((pos[l] - rest) - A * d0).max() <= 1e-12 * np.abs(d0).max(), l
        assert np.abs(vel[l] - A * vel[0]).max() <= 1e-12 * np.abs(vel[0]).max(), l
    # the wrong wave number (half of it) is far outside
    assert np.abs((pos[1] - rest) - np.exp(-0.5 * k * depths[1]) * d0).max() > 0.2 * np.abs(d0).max()


def test_the_velocity_layer_is_the_time_derivative_of_the_position_layer(oracle):
    """Central difference in t of the oracle's position layer against its velocity layer, with the bound tests/test_velocity_cpu.py uses
    for the surface (phase rounding, truncation, the float32 cast of the weighted spectrum), every magnitude attenuated by A_l."""
    p = workloads.fftmesh_params(16)
    h0, h0c = oracle.generate_spectrum(p, 7)
    depths = [0.0, 0.7, 2.5]
    t, h = 1.25, 2.0 ** -7
    _, vel = CR.layers_f64(p, h0, h0c, t, depths)
    num = (CR.layers_f64(p, h0, h0c, t + h, depths)[0] - CR.layers_f64(p, h0, h0c, t - h, depths)[0]) / (2 * h)
    w, k = V.fftmesh_omega(p), CR.wave_number(p)
    ulp = float(np.spacing(f32(w.max() * (t + h))))
    for l, d in enumerate(depths):
        mag = (np.hypot(h0[..., 0], h0[..., 1]) + np.hypot(h0c[..., 0], h0c[..., 1])).astype(np.float64) * max(1.0, p.choppiness) * np.exp(-k * d)
        bound = (ulp / 2 * mag.sum() / h) + h * h / 6 * float((mag * w ** 3).sum()) + 2.0 ** -23 * float((mag * w).sum())
        # the position layer's spectrum is cast to float32 too: one more relative 2^-24 of every value, divided by 2h twice
        bound += 2.0 ** -24 * mag.sum() / h
        scale, err = np.abs(vel[l]).max(), np.abs(vel[l] - num[l]).max()
        assert scale > 0 and err <= bound and bound < 0.05 * scale, (l, err, bound, scale)
    assert np.abs(vel[2]).max() < np.abs(vel[1]).max() < np.abs(vel[0]).max()


def test_interpolation_between_layers_stays_within_the_lagrange_bound(oracle, shim):
    """Linear interpolation of f(d) = e^{-k d} on [d_l, d_{l+1}], width D: |f(d) - lin(d)| <= D^2 / 8 max |f''| = (k D)^2 / 8 e^{-k d_l}
    (the Lagrange remainder (d - d_l)(d_{l+1} - d) / 2 f''(xi), whose first factor is at most D^2 / 4).  So for one spectrum bin the
    rest-mode answer at a vertex label (weights 0 / 1: no interpolation inside the layer) differs from the exact float64 field at depth d
    by at most that fraction of the surface amplitude, plus float32 rounding: the layer arrays are cast to float32 (2^-24 of a
    coordinate) and the blend rounds three times (3 x 2^-24 of the larger operand).  The derivation gives the issue's constant, 1/8."""
    p = workloads.fftmesh_params(16)
    n, m = 10, 9
    h0, h0c = single_bin(p, n, m, value=(0.3, -0.2))
    k = CR.wave_number(p)[n, m]
    depths = np.array([0.0, 0.5, 1.5, 4.0], f32)
    t = 0.75
    pos, vel = CR.layers_f64(p, h0, h0c, t, depths)
    rest = oracle.rest_mesh(p)[0].astype(np.float64)
    amp, uamp = np.abs(pos[0] - rest).max(), np.abs(vel[0]).max()
    rc = S.rest_coords(p.N, p.unit_width)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    worst = 0.0
    for l in range(len(depths) - 1):
        D = float(depths[l + 1]) - float(depths[l])
        for frac in (0.25, 0.5, 0.8):
            d = f32(float(depths[l]) + frac * D)
            lab = np.stack([X.ravel(), np.full(X.size, d), Z.ravel()], -1)
            got = CR.query(shim, p.N, p.unit_width, 0.0, depths, pos.astype(f32), vel.astype(f32), CR.REST, lab).astype(np.float64)
            epos, evel = CR.layers_f64(p, h0, h0c, t, [float(d)])
            want_p = epos[0].copy()
            want_p[:, 1] -= float(d)
            lag = (k * D) ** 2 / 8 * np.exp(-k * float(depths[l]))
            rnd = 4 * 2.0 ** -24 * (np.abs(want_p).max() + float(depths[-1]))
            assert np.abs(got[:, CR.PX:CR.PZ + 1] - want_p).max() <= lag * amp + rnd, (l, frac)
            assert np.abs(got[:, CR.UX:CR.UZ + 1] - evel[0]).max() <= lag * uamp + 4 * 2.0 ** -24 * uamp, (l, frac)
            worst = max(worst, np.abs(got[:, CR.UX:CR.UZ + 1] - evel[0]).max() / (lag * uamp))
            assert np.array_equal(got[:, CR.DEPTH], np.full(X.size, d, np.float64)) and (got[:, CR.RESIDUAL] == 0).all()
    assert worst > 0.5   # the bound is attained to within a factor two at a midpoint: it is the right constant


# ---- the shim against the float64 restatement ------------------------------------------------------------------------------------------
# Measured on this tier against column_ref.query_f64 over the oracle's layers cast to float32 (N = 64, choppiness 0.46, L = 4, 20 000
# points per mode, both mesh types): the largest |shim - f64| was
#   velocity 7.8e-7 max|u_0| (world), 1.3e-7 (rest);  px py pz 5.8e-6 unit_width;  x0 z0 6.2e-6 unit_width;  rest_depth 1.7e-7 d_{L-1};
#   lambda 2.7e-7;  eta 4.2e-7;  residual 8.6e-6 unit_width.
# The assertions are 8 x those (the device's layers differ from the oracle's by up to REL_TOL, which moves the rounding, not its size).
TOL_U, TOL_P, TOL_X0, TOL_DEPTH, TOL_LAMBDA, TOL_ETA = 8 * 7.8e-7, 8 * 5.8e-6, 8 * 6.2e-6, 8 * 1.7e-7, 8 * 2.7e-7, 8 * 4.2e-7
RESIDUAL_CAP, LEFT_OUT_CAP = 1e-4, 0.01


def compare_with_f64(got, want, umax, uw, dmax, mode, tag=""):
    """got [n, 12] float32 against the restatement's rows; world points whose float64 residual exceeds 1e-4 unit widths are left out, at
    most 1 % of them.  Returns the measured figures."""
    want_nan = np.isnan(want).any(-1)
    assert np.array_equal(np.isnan(got).any(-1), want_nan), tag
    keep = ~want_nan
    if mode == CR.WORLD:
        keep &= ~(want[:, CR.RESIDUAL] > RESIDUAL_CAP * uw)
        assert (~keep & ~want_nan).mean() <= LEFT_OUT_CAP, tag
    d = np.abs(got.astype(np.float64) - want)[keep]
    fig = dict(u=d[:, CR.UX:CR.UZ + 1].max() / umax, p=d[:, CR.PX:CR.PZ + 1].max() / uw, x0=d[:, CR.X0:CR.Z0 + 1].max() / uw,
               depth=d[:, CR.DEPTH].max() / dmax, lam=d[:, CR.LAMBDA].max(), eta=d[:, CR.ETA].max())
    print(tag, {k: "%.3g" % v for k, v in fig.items()})
    assert fig["u"] <= TOL_U and fig["p"] <= TOL_P and fig["x0"] <= TOL_X0 and fig["depth"] <= TOL_DEPTH, (tag, fig)
    assert fig["lam"] <= TOL_LAMBDA and fig["eta"] <= TOL_ETA, (tag, fig)
    return keep, fig


@pytest.mark.parametrize("P", [0.0, 64.0])
def test_shim_equals_the_float64_restatement_on_oracle_layers(shim, layers, P):
    n = 20000
    uw, dmax = 1.0, float(DEPTHS64[-1])
    q = world_points(n, 1)
    want = CR.query_f64(N64, uw, P, DEPTHS64, layers["pos"], layers["vel"], CR.WORLD, q)
    # the condition on the input, checked on the restatement alone
    assert (want[:, CR.RESIDUAL] > RESIDUAL_CAP * uw).mean() <= LEFT_OUT_CAP
    got = CR.query(shim, N64, uw, P, DEPTHS64, layers["pos"], layers["vel"], CR.WORLD, q)
    keep, _ = compare_with_f64(got, want, layers["umax"], uw, dmax, CR.WORLD, "world P=%g" % P)
    # every regime is populated: air, each interval, below the deepest layer
    lam = want[keep, CR.LAMBDA]
    assert (want[keep, CR.DEPTH] < 0).sum() > 100 and (lam == 3).sum() > 1000
    assert all(((lam > l) & (lam < l + 1)).sum() > 1000 for l in range(3))
    # the early exit brackets as the all-layers restatement does (points within 1e-5 of an interface may round to either side)
    clear = np.abs(lam - np.round(lam)) > 1e-5
    assert np.array_equal(np.floor(got[keep, CR.LAMBDA][clear]), np.floor(lam[clear]))
    rng = np.random.default_rng(2)
    lab = np.stack([q[:, 0], rng.uniform(0, dmax, n), q[:, 2]], -1).astype(f32)
    want = CR.query_f64(N64, uw, P, DEPTHS64, layers["pos"], layers["vel"], CR.REST, lab)
    got = CR.query(shim, N64, uw, P, DEPTHS64, layers["pos"], layers["vel"], CR.REST, lab)
    compare_with_f64(got, want, layers["umax"], uw, dmax, CR.REST, "rest P=%g" % P)


# ---- bit identities of the shim ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0.0, 64.0])
def test_a_vertex_label_at_a_layer_depth_returns_the_layers_bits(shim, layers, P):
    """weights 0 / 1 inside the layer, s = 0 (or 1 at the deepest layer) between layers: every product is exact"""
    rc = layers["rc"]
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    for l, d in enumerate(DEPTHS64):
        lab = np.stack([X.ravel(), np.full(X.size, d, f32), Z.ravel()], -1)
        out = CR.query(shim, N64, 1.0, P, DEPTHS64, layers["pos"], layers["vel"], CR.REST, lab)
        want_p = layers["pos"][l].copy()
        want_p[:, 1] = want_p[:, 1] - d
        assert np.array_equal(bits(out[:, CR.PX:CR.PZ + 1]), bits(want_p)), l
        assert np.array_equal(bits(out[:, CR.UX:CR.UZ + 1]), bits(layers["vel"][l])), l
        assert np.array_equal(bits(out[:, CR.X0]), bits(X.ravel())) and np.array_equal(bits(out[:, CR.Z0]), bits(Z.ravel()))
        assert np.array_equal(out[:, CR.LAMBDA], np.full(X.size, l, f32)) and np.array_equal(bits(out[:, CR.ETA]), bits(layers["pos"][0][:, 1]))


def layer_as_surface(shim, layers, P, l, q):
    """y_l and u_l over world points, through the shim itself: layer l standing as the surface of a two-layer column, queried high in the
    air (eta is its height, p its point) and then exactly on it (s = 0: u is its velocity)"""
    sub = np.array([0.0, 1.0], f32)
    pos, vel = np.stack([layers["pos"][l], layers["pos"][l]]), np.stack([layers["vel"][l], layers["vel"][l]])
    high = q.copy()
    high[:, 1] = 1e6
    air = CR.query(shim, N64, 1.0, P, sub, pos, vel, CR.WORLD, high)
    on = q.copy()
    on[:, 1] = air[:, CR.ETA]
    at = CR.query(shim, N64, 1.0, P, sub, pos, vel, CR.WORLD, on)
    assert (at[:, CR.LAMBDA] == 0).all()
    return (air[:, CR.ETA] - DEPTHS64[l]).astype(f32), at[:, CR.UX:CR.UZ + 1]


@pytest.mark.parametrize("P", [0.0, 64.0])
def test_a_point_on_a_layer_has_s_zero_and_the_layers_velocity(shim, layers, P):
    q = world_points(500, 3)
    for l in range(len(DEPTHS64)):
        yl, ul = layer_as_surface(shim, layers, P, l, q)
        on = q.copy()
        on[:, 1] = yl
        out = CR.query(shim, N64, 1.0, P, DEPTHS64, layers["pos"], layers["vel"], CR.WORLD, on)
        assert np.array_equal(out[:, CR.LAMBDA], np.full(len(q), l, f32)), l
        assert np.array_equal(bits(out[:, CR.UX:CR.UZ + 1]), bits(ul)), l
        assert np.array_equal(bits(out[:, CR.DEPTH]), bits(np.full(len(q), DEPTHS64[l], f32))), l
        assert np.array_equal(bits(out[:, CR.PY]), bits(yl)), l


# ---- edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0.0, 64.0])
def test_air_surface_and_below_the_deepest_layer(shim, layers, P):
    q = world_points(300, 4)
    col = lambda pts: CR.query(shim, N64, 1.0, P, DEPTHS64, layers["pos"], layers["vel"], CR.WORLD, pts)
    y0, u0 = layer_as_surface(shim, layers, P, 0, q)
    # in the air
    air = q.copy()
    air[:, 1] = y0 + f32(2.5)
    a = col(air)
    assert (a[:, CR.UX:CR.UZ + 1] == 0).all() and (a[:, CR.LAMBDA] == 0).all()
    assert np.array_equal(bits(a[:, CR.DEPTH]), bits(y0 - air[:, 1])) and (a[:, CR.DEPTH] < 0).all()
    assert np.array_equal(bits(a[:, CR.ETA]), bits(y0)) and np.array_equal(bits(a[:, CR.PY]), bits(y0))
    # on the surface: in the water, s = 0
    on = q.copy()
    on[:, 1] = y0
    s = col(on)
    assert (s[:, CR.LAMBDA] == 0).all() and (s[:, CR.DEPTH] == 0).all() and np.array_equal(bits(s[:, CR.UX:CR.UZ + 1]), bits(u0))
    for c in (CR.PX, CR.PY, CR.PZ, CR.X0, CR.Z0, CR.ETA):
        assert np.array_equal(bits(s[:, c]), bits(a[:, c])), c
    assert (s[:, CR.RESIDUAL] >= a[:, CR.RESIDUAL]).all()   # the largest of the layers visited: layer 0 in the air, layers 0 and 1 here
    # below the deepest layer: its velocity, the hydrostatic continuation, continuous at y = y_{L-1}
    yb, ub = layer_as_surface(shim, layers, P, 3, q)
    deep = q.copy()
    deep[:, 1] = yb - f32(7.0)
    b = col(deep)
    assert (b[:, CR.LAMBDA] == 3).all() and np.array_equal(bits(b[:, CR.UX:CR.UZ + 1]), bits(ub))
    assert np.array_equal(bits(b[:, CR.DEPTH]), bits(DEPTHS64[3] + (yb - deep[:, 1])))
    just = q.copy()
    just[:, 1] = np.nextafter(yb, f32(np.inf))
    j = col(just)
    assert (j[:, CR.LAMBDA] < 3).all() and (j[:, CR.LAMBDA] > 3 - 1e-5).all()
    assert np.abs(j[:, CR.DEPTH] - DEPTHS64[3]).max() <= 4e-6 * DEPTHS64[3]
    assert np.abs(j[:, CR.UX:CR.UZ + 1] - ub).max() <= 1e-5 * layers["umax"]


@pytest.mark.parametrize("P", [0.0, 64.0])
def test_non_finite_inputs_and_depths_out_of_range_are_rows_of_nan(shim, layers, P):
    col = lambda mode, pts: CR.query(shim, N64, 1.0, P, DEPTHS64, layers["pos"], layers["vel"], mode, pts)
    bad = np.array([[np.nan, -1, 0], [0, np.nan, 0], [0, -1, np.nan], [np.inf, -1, 0], [0, np.inf, 0], [0, -np.inf, 0], [0, -1, -np.inf]], f32)
    assert np.isnan(col(CR.WORLD, bad)).all()
    assert np.isfinite(col(CR.WORLD, np.array([[0.25, -1, 0.5]], f32))).all()
    lab = np.array([[0, -1e-6, 0], [0, 18.001, 0], [0, np.nan, 0], [np.nan, 1, 0], [0, 1, np.inf], [0, np.inf, 0]], f32)
    assert np.isnan(col(CR.REST, lab)).all()
    ok = col(CR.REST, np.array([[0.5, 0.0, 0.5], [0.5, 18.0, 0.5]], f32))
    assert np.isfinite(ok).all() and (ok[:, CR.LAMBDA] == [0, 3]).all()
    off = col(CR.REST, np.array([[40.0, 1.0, 0.0], [0.0, 1.0, -32.0]], f32))   # off the footprint: NaN on the one mesh, a tile away on the tiling
    assert np.isnan(off).all() if P == 0.0 else np.isfinite(off).all()


@pytest.mark.parametrize("P", [0.0, 32.0])
def test_two_layers_a_millimetre_apart_under_a_steep_crest_never_divide_by_a_non_positive_number(shim, P):
    """Layers 1e-3 apart whose heights cross where the crest is steep (the deeper one is the steeper mesh here, on purpose): the first-l
    rule only ever divides by y_l - y_{l+1} with y_{l+1} < y <= y_l, so every row of a finite point is finite and 0 <= s <= 1."""
    R, uw = 32, 1.0
    rest = np.stack(np.meshgrid(S.rest_coords(R, uw), S.rest_coords(R, uw), indexing="ij"), -1).reshape(-1, 2)
    v0, _, _, vel0 = PR.periodic_synth(R, uw, 0.95, seed=3)
    disp = v0.astype(np.float64) - np.stack([rest[:, 0], np.zeros(len(rest)), rest[:, 1]], -1)
    mk = lambda a: (np.stack([rest[:, 0], np.zeros(len(rest)), rest[:, 1]], -1) + a * disp).astype(f32)
    depths = np.array([0.0, 1e-3, 2e-3, 6.0], f32)
    pos = np.stack([v0, mk(1.02), mk(0.97), mk(0.1)])
    vel = np.stack([vel0, vel0 * f32(1.02), vel0 * f32(0.97), vel0 * f32(0.1)])
    rng = np.random.default_rng(5)
    n = 20000
    xz = rng.uniform(-14, 14, (n, 2))
    eta = CR.layer_heights_f64(R, uw, P, depths, pos, xz)[0]
    y = np.where(rng.random(n) < 0.7, eta - rng.uniform(0, 4e-3, n), eta - rng.uniform(0, 8, n))
    q = np.stack([xz[:, 0], y, xz[:, 1]], -1).astype(f32)
    Y = CR.layer_heights_f64(R, uw, P, depths, pos, xz)
    assert ((Y[1] > Y[0]) | (Y[2] > Y[1])).sum() > 100   # the layers do cross
    out = CR.query(shim, R, uw, P, depths, pos, vel, CR.WORLD, q)
    assert np.isfinite(out).all()
    lam = out[:, CR.LAMBDA]
    assert (lam >= 0).all() and (lam <= 3).all()
    assert np.abs(out[:, CR.UX:CR.UZ + 1]).max() <= 1.05 * np.abs(vel).max()   # a blend with 0 <= s <= 1 never leaves its operands' range


# ---- continuity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0.0, 64.0])
def test_velocity_depth_and_lambda_are_continuous_across_every_interface(shim, layers, P):
    """Just above and just below y_l (one float32 step each way) the answers differ by the slope of the blend over two steps plus its
    rounding: |du| <= 2 ulp(y) / thickness * |u_l - u_{l+-1}| + 4 x 2^-23 max|u|, likewise the rest depth and lambda."""
    q = world_points(400, 6)
    col = lambda pts: CR.query(shim, N64, 1.0, P, DEPTHS64, layers["pos"], layers["vel"], CR.WORLD, pts)
    Yl = [layer_as_surface(shim, layers, P, l, q) for l in range(len(DEPTHS64))]
    eps = 2.0 ** -23
    for l in range(len(DEPTHS64)):
        yl = Yl[l][0]
        up, dn = q.copy(), q.copy()
        up[:, 1], dn[:, 1] = np.nextafter(yl, f32(np.inf)), np.nextafter(yl, f32(-np.inf))
        a, b = col(up), col(dn)
        step = (up[:, 1].astype(np.float64) - dn[:, 1])
        thick = np.full(len(q), np.inf)
        du = np.zeros(len(q))
        for m in (l - 1, l + 1):
            if 0 <= m < len(DEPTHS64):
                thick = np.minimum(thick, np.abs(Yl[m][0].astype(np.float64) - yl))
                du = np.maximum(du, np.abs(Yl[m][1].astype(np.float64) - Yl[l][1]).max(-1))
        ds = step / thick
        if l > 0:   # (above the surface is the air: u jumps to 0 there by the rule, the rest depth does not)
            assert (np.abs(a[:, CR.UX:CR.UZ + 1].astype(np.float64) - b[:, CR.UX:CR.UZ + 1]).max(-1) <= ds * du + 4 * eps * layers["umax"]).all(), l
            assert (np.abs(a[:, CR.LAMBDA].astype(np.float64) - b[:, CR.LAMBDA]) <= ds + 4 * eps * 4).all(), l
        gap = max(float(DEPTHS64[min(l + 1, 3)] - DEPTHS64[max(l - 1, 0)]), 1.0)
        assert (np.abs(a[:, CR.DEPTH].astype(np.float64) - b[:, CR.DEPTH]) <= ds * gap + step + 4 * eps * float(DEPTHS64[-1])).all(), l


# ---- tiling ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [CR.REST, CR.WORLD])
def test_translation_by_whole_tiles_is_exact(shim, layers, mode):
    """P = 64 is a power of two and the coordinates are multiples of 2^-8: q + k P is exact, so the row of the moved point is the row of
    the point with exactly kx P and kz P added to px, pz, x0, z0 (one float32 addition each) and every other field bit for bit -- seam
    strips and tile corners included (the check tests/test_periodic_cpu.py makes for the surface)."""
    P = PR.period(N64, 1.0)
    assert P == 64.0
    rng = np.random.default_rng(11)
    xz = PR.base_points(N64, 1.0, 400, rng, step=2.0 ** -8)
    assert (xz[:, 0] > layers["rc"][-1]).sum() > 50 and (xz[:, 1] > layers["rc"][-1]).sum() > 50
    y = np.round(rng.uniform(0 if mode == CR.REST else -20, 18 if mode == CR.REST else 1, len(xz)) * 256) / 256
    q = np.stack([xz[:, 0], y, xz[:, 1]], -1).astype(f32)
    col = lambda pts: CR.query(shim, N64, 1.0, P, DEPTHS64, layers["pos"], layers["vel"], mode, pts)
    base = col(q)
    assert np.isfinite(base).all()
    for kx in range(-3, 4):
        for kz in range(-3, 4):
            sh = np.array([kx * P, 0, kz * P], f32)
            moved = (q + sh).astype(f32)
            assert np.array_equal(moved.astype(np.float64), q.astype(np.float64) + sh.astype(np.float64))
            want = base.copy()
            for c, k in ((CR.PX, 0), (CR.X0, 0), (CR.PZ, 2), (CR.Z0, 2)):
                want[:, c] = base[:, c] + sh[k]
            assert np.array_equal(bits(col(moved)), bits(want)), (kx, kz)


# ---- exports and statuses without a GPU -----------------------------------------------------------------------------------------
COLUMN_SYMBOLS = ("mw_ocean_set_column", "mw_ocean_get_column", "mw_ocean_column_layers", "mw_ocean_query_column", "mw_ocean_query_column_device")


def test_column_symbols_are_exported_declared_and_refuse_a_null_handle(mw):
    from mistral_water import _native
    L = C.CDLL(_native.LIB_PATH)
    hdr = open(_native.HEADER_PATH).read()
    for s in COLUMN_SYMBOLS:
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr
    assert "#define MW_COLUMN_MAX_LAYERS 16" in hdr and mw.MW_COLUMN_MAX_LAYERS == 16 and mw.lib().mw_abi_version() == 4
    L = mw.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    depths = np.array([0.0, 1.0, 2.0], f32)
    # a NULL handle is refused before any other rule is looked at, whatever the other arguments are
    for d, n in ((depths, 3), (None, 0), (depths, 1), (depths, 17), (np.array([1.0, 2.0], f32), 2), (np.array([0.0, 0.0], f32), 2)):
        assert L.mw_ocean_set_column(None, None if d is None else p(d), n) == mw.MW_EINVAL and b"NULL handle" in L.mw_last_error()
    got, n = np.full(16, 7.0, f32), C.c_int32(7)
    assert L.mw_ocean_get_column(None, p(got), C.byref(n)) == mw.MW_EINVAL and n.value == 7 and (got == 7).all()
    a, b = C.c_void_p(7), C.c_void_p(7)
    assert L.mw_ocean_column_layers(None, -1, 0, C.byref(a), C.byref(b)) == mw.MW_EINVAL and a.value == 7 and b.value == 7
    xyz, out = np.zeros((4, 4), f32), np.full((4, 12), 7.0, f32)
    for fn in (L.mw_ocean_query_column, L.mw_ocean_query_column_device):
        assert fn(None, -1, 1, p(xyz), 4, 0, p(out)) == mw.MW_EINVAL and b"NULL handle" in L.mw_last_error()
    assert (out == 7).all()


def test_the_column_kernels_run_the_functions_the_shim_runs():
    """one source text: the kernel's body is col_query_point, both instantiations stand in a translation unit compiled with contraction
    off, as g++ compiles the shim, and the build recipes name that unit"""
    h = open(os.path.join(CSRC, "water_column.h")).read()
    k = h[h.index("void k_query_column("):]
    assert "col_query_point(m, tb, mode, q.x, q.y, q.z, iters, r)" in k and "__launch_bounds__(256) void k_query_column" in h
    assert h.count("sq_locate(") >= 2 and "velocity_weight(w, *pa, *pb, va, vb)" in h
    tu = open(os.path.join(CSRC, "water_column.hip")).read()
    assert tu.index('#include "mw_math.h"') < tu.index("#pragma clang fp contract(off)") < tu.index('#include "water_column.h"')
    assert "SqTiled{m}, tb" in tu and "(m, tb, mode" in tu and "k_column_weight<<<" in tu
    from mistral_water import _native
    assert "water_column.hip" in _native.TRANSLATION_UNITS
    assert "water_column.hip" in open(os.path.join(REPO, "tools", "build_variant.sh")).read()
    main = open(os.path.join(CSRC, "mistral_water.hip")).read()
    assert "k_query_column<<<" not in main and "k_query_column<<<" not in open(os.path.join(CSRC, "surface_services.inc")).read()


def test_the_layer_builders_weights(shim, oracle):
    """A is mirror-symmetric bit for bit (k_prep pairs (i, j) with its mirror under one weight), it is e^{-k d} of column_ref's k, the
    position pair is A times the spectrum and the velocity pair velocity_weight of THAT pair (attenuated first, then weighted)."""
    for N in (16, 64, 256):
        p = workloads.fftmesh_params(N)
        h0, h0c = oracle.generate_spectrum(p, 3)
        for d in (0.0, 0.37, 5.0):
            A, pa, pb, va, vb = CR.weights(shim, p, d, h0, h0c)
            m = (N - np.arange(N)) % N
            assert np.array_equal(bits(A), bits(A[m][:, m]))
            assert np.abs(A - np.exp(-CR.wave_number(p) * d)).max() <= 2.0 ** -22
            if d == 0.0:
                assert (A == 1).all() and np.array_equal(bits(pa), bits(h0))
            assert np.array_equal(bits(pa), bits(A[..., None] * h0)) and np.array_equal(bits(pb), bits(A[..., None] * h0c))
            w = V.fftmesh_omega(p).astype(f32)
            ra, rb = V.weight(pa, pb, w.astype(np.float64))
            assert np.array_equal(bits(va), bits(ra.astype(f32))) and np.array_equal(bits(vb), bits(rb.astype(f32)))
