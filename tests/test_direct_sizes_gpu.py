"""GPU tier: the separable direct sum (csrc/czt_kernels.h, csrc/direct_kernels.h) on the non-FFT grids users reach most easily --
every size above 2048 and every power of two whose length is not N * unit_width -- at the sizes where its two forms change shape.

direct_create picks the form.  Chirp-z runs where czt_size(N) != 0: the packed planes carry N + 1 inputs and N outputs per line, so the
cyclic convolution needs 2N lags and the transform size is M = the next power of two >= 2N (64 ... 4096, N <= 2048).  Two kinds of
grid sit at its edges:
  * N = 256, 512, 1024, 2048 with an incommensurate length: 2N = M, the convolution is exactly full (the largest negative lag -N wraps
    to slot M / 2, next to the largest positive lag N - 1);
  * N = 257, 513, 1025 (the first size of the next M) and 2047 (the largest odd size, M = 4096).
The MFMA GEMM form (k_gemm_f32_mfma, operands zero-padded to Np = ceil(N / 64) * 64, K = 2 Np) runs for every grid with 2048 < N <= 4096:
N = 2049 (Np = 2112 = 33 tiles, 63 padding lines), 3001 (Np = 3008), 4095 (Np = 4096, one padding line) and N = 4096 with a length
the FFT path refuses.

Every frame is checked against oracle.eval_matmul_f64 (complex128 matrix products) at the direct paths' stated 2e-5 of the field scale,
with the per-vertex whitecap bounds.  Besides the Phillips sea of test_direct_path_large_and_odd_grids each grid also runs a WHITE
spectrum (every index of h0 of the same size), so that every wave number and every lag carries as much weight as the spectral peak:
the highest wave numbers with their phases of thousands of radians, the last K tile of a GEMM, the chirp entry of the largest lag
(which only the pair output 0, input N uses)."""
import dataclasses

import numpy as np
import pytest

import surface_ref as S
import velocity_ref as V
import workloads

pytestmark = pytest.mark.gpu

CZT_FULL = [(256, 248.5), (512, 497.0), (1024, 993.0), (2048, 1987.0)]      # 2N = M: 512 ... 4096
CZT_NEXT = [(257, 257.0), (513, 513.0), (1025, 1025.0), (2047, 2047.0)]     # M = 1024, 2048, 4096, 4096
# (N, length, times): one time on the two largest grids (the f64 check is ~5e12 flop there)
GEMM = [(2049, 2049.0, (0.5, 16.0)), (3001, 2950.0, (0.5, 16.0)), (4095, 4095.0, (16.0,)), (4096, 3970.0, (0.5,))]
CZT_NAME, GEMM_NAME = "k_czt (2 launches", "k_gemm_f32_mfma"


def _params(oracle, N, L, choppiness=0.46):
    """the sea of test_direct_path_large_and_odd_grids: wave heights O(1) at every N and length"""
    return oracle.Params(N=N, unit_width=1.0, length=L, wind_x=14.45, wind_y=12.0, amplitude=1.5e-8 * (1024.0 / N) ** 2 * (L / N) ** 2,
                         choppiness=choppiness)


def _ocean(mw, p, seed=4):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, seed=seed, device=0)


def _plan(o):
    """the kernel names of the plan the handle runs (mw_ocean_profile_kernels: one step per enqueue on the direct path)"""
    assert o.max_batch == 1, "the direct path (one step per enqueue) was expected"
    prof = o.profile_kernels(nsteps=1, iters=2)
    print(f"MEASURE plan N={o.N}: " + "; ".join(f"{k} {ms:.3f} ms" for k, ms in prof))
    return [k for k, _ in prof]


def _white_spectrum(N, seed):
    """h0, h0conj with every entry of the same distribution: the displacement stays below half a unit width, no fold"""
    rng = np.random.default_rng(seed)
    s = 0.05 / N
    return tuple((rng.standard_normal((N, N, 2)) * s).astype(np.float32) for _ in range(2))


def _check_frame(oracle, p, frame, h0, h0c, t, tag, rel=2e-5):
    v, n, c = frame
    vd, nd, cd, hds = oracle.eval_matmul_f64(p, h0, h0c, t, return_hds=True)
    rest = oracle.rest_mesh(p)[0]
    scale = max(float(np.abs(vd - rest).max()), 1e-3)
    # what assert_parity holds to `rel`: the error beyond one ulp of the stored coordinate, over the field scale
    excess = float((np.abs(v - vd) - np.abs(vd) * 2.0 ** -23).max()) / scale
    print(f"MEASURE {tag}: vertices {excess:.2e} of the field scale (height alone {float(np.abs(v[:, 1] - vd[:, 1]).max()) / scale:.2e})")
    workloads.assert_parity(v, n, c, vd, nd, cd, rest, rel=rel, tag=tag, hds=hds)


@pytest.mark.parametrize("N,L", CZT_FULL + CZT_NEXT, ids=[str(g[0]) for g in CZT_FULL + CZT_NEXT])
def test_chirp_z_at_the_transform_size_edges(mw, oracle, N, L):
    """The three-launch chirp-z plan (k_czt twice + k_czt_assemble_white) where the convolution is exactly full and one size past it,
    at two times with the Phillips sea and once with a white spectrum."""
    p = _params(oracle, N, L)
    with _ocean(mw, p) as o:
        kinds = _plan(o)
        assert kinds[0].startswith(CZT_NAME) and kinds[1] == "k_czt_assemble_white", kinds
        h0, h0c = o.get_spectrum()
        for t in (0.5, 16.0):
            _check_frame(oracle, p, o.evaluate(t), h0, h0c, t, f"chirp-z N={N} t={t}")
        w0, w0c = _white_spectrum(N, N)
        o.set_spectrum(w0, w0c)
        _check_frame(oracle, p, o.evaluate(0.5), w0, w0c, 0.5, f"chirp-z N={N} white t=0.5")


@pytest.mark.parametrize("N,L,times", GEMM, ids=[str(g[0]) for g in GEMM])
def test_gemm_form_at_its_product_sizes(mw, oracle, N, L, times):
    """The GEMM form in the product default (no switch set) on grids above 2048, N = 4096 included when its length is not 4096 (the FFT
    path must refuse it).  A float32 sum of K = 2 Np products per output on the matrix cores (an fmaf chain in k order): its rounding
    error is a random walk of K steps of ~2^-24 of the partial sum, ~sqrt(K) * 2^-24 = 5.4e-6 of an output at K = 8192 per stage,
    inside 2e-5 of the field scale for both stages together.  The phases k_j pos_b of the E tables are exact in f64 (k_direct_tables):
    with the float32 wave number of the reference they alone were 7.7e-6 (vertices) and 1.5x the normal bound off at N = 4095, and
    1e-4 of the scale with the white spectrum.  A frame evaluated again after another one is the same bit pattern."""
    p = _params(oracle, N, L)
    with _ocean(mw, p) as o:
        kinds = _plan(o)
        assert kinds[0].startswith(GEMM_NAME), kinds
        h0, h0c = o.get_spectrum()
        for t in times:
            _check_frame(oracle, p, o.evaluate(t), h0, h0c, t, f"GEMM N={N} t={t}")
        a = o.evaluate(times[0])
        o.evaluate(times[0] + 3.0)
        b = o.evaluate(times[0])
        assert all((x == y).all() for x, y in zip(a, b)), "two evaluations at the same t differ"
        w0, w0c = _white_spectrum(N, N)
        o.set_spectrum(w0, w0c)
        _check_frame(oracle, p, o.evaluate(0.5), w0, w0c, 0.5, f"GEMM N={N} white t=0.5")


@pytest.mark.parametrize("N,L,plan", [(2048, 1987.0, CZT_NAME), (2049, 2049.0, GEMM_NAME)], ids=["chirp-z-2048", "gemm-2049"])
def test_velocity_on_the_largest_chirp_z_and_the_smallest_gemm_grid(mw, oracle, N, L, plan):
    """mw_ocean_velocity (the frame pipeline on the weighted spectrum) against the f64 oracle fed that spectrum (tests/velocity_ref.py)"""
    p = _params(oracle, N, L)
    with _ocean(mw, p) as o:
        assert _plan(o)[0].startswith(plan)
        o.evaluate(0.75)
        vel = o.velocity()
        h0, h0c = o.get_spectrum()
    ref = V.fftmesh_velocity_f64(p, h0, h0c, 0.75)
    scale = float(np.abs(ref).max())
    err = np.abs(vel - ref)
    print(f"MEASURE velocity N={N}: max |err| / field scale {float(err.max()) / scale:.2e}")
    assert (err <= 2e-5 * scale + np.abs(ref) * 2.0 ** -23).all(), (N, float(err.max()) / scale)


def test_surface_query_on_a_gemm_grid(mw, oracle):
    """mw_ocean_query_surface on the GEMM form's frame (N = 2049).  Rest mode at every vertex's rest position: the barycentric weights
    are exactly 0 and 1 there (surface_query.h), so position and whitecap are the vertex's own values exactly; the normal is normalised
    once more (within 2 ulp).  World mode against the float64 brute force in local windows (test_fftmesh_1024_world_mode_in_local_windows),
    at points near the centre of the mesh."""
    N = 2049
    p = _params(oracle, N, 2049.0, choppiness=1.2)
    with _ocean(mw, p) as o:
        assert _plan(o)[0].startswith(GEMM_NAME)
        v, n, c = o.evaluate(3.25)
        white = c[:, 0].copy()
        out = o.query_surface(S.rest_plane(N, p.unit_width), mode="rest")
        assert np.array_equal(out[:, :3], v) and np.array_equal(out[:, 6], white) and (out[:, 7] == 0).all()
        assert np.abs(out[:, 3:6] - n).max() <= 2.0 ** -22
        # points in the middle 500 x 500 of the 2049 x 2049 mesh: check_world holds a resolved point to a residual of 1e-4 unit widths,
        # which float32 resolves only where |x|, |z| < 512 (farther out 1e-4 is under 2 ulp of the coordinate)
        dmax = float(np.abs(v[:, [0, 2]] - S.rest_plane(N, p.unit_width)).max())
        xz = np.random.default_rng(11).uniform(-250.0, 250.0, (200, 2)).astype(np.float32)
        w = o.query_surface(xz)
        nuniq, nfold, nmissed = S.check_world(w, xz, v, n, white, p.unit_width, S.window_triangles(N, p.unit_width, dmax + 2.0),
                                              unique_exact=False)
        assert nuniq >= 0.5 * len(xz) and nmissed <= 0.02 * nuniq, (nuniq, nfold, nmissed)


def test_reinit_spectrum_with_a_new_length_on_a_gemm_handle(mw, oracle):
    """The GEMM form's E tables depend on (unit_width, length) and are rebuilt by reinit_spectrum when the length changes (direct_tables,
    on the handle's stream; no enqueue builds tables).  After evaluate, reinit_spectrum(length = ...), evaluate the handle must be the
    handle a fresh create with the new parameters gives, bit for bit, and match the oracle at the new length and spectrum."""
    old = _params(oracle, 2049, 2049.0)
    L = 2300.0
    new = dataclasses.replace(old, length=L, wind_x=-3.0, wind_y=6.0, amplitude=1.5e-8 * (1024.0 / 2049) ** 2 * (L / 2049) ** 2)
    with _ocean(mw, old, seed=3) as o:
        assert _plan(o)[0].startswith(GEMM_NAME)
        o.evaluate(0.5)                                            # tables of the old length in use
        o.reinit_spectrum(length=new.length, wind=(new.wind_x, new.wind_y), amplitude=new.amplitude, seed=9)
        a = o.evaluate(1.25)
        h0, h0c = o.get_spectrum()
    with _ocean(mw, new, seed=9) as f:
        b = f.evaluate(1.25)
        g0, g0c = f.get_spectrum()
    assert (h0 == g0).all() and (h0c == g0c).all()
    assert all((x == y).all() for x, y in zip(a, b)), "reinit + evaluate must equal create + evaluate"
    _check_frame(oracle, new, a, h0, h0c, 1.25, "GEMM reinit N=2049")


# (N, unit_width, length, amplitude, MW_DIRECT_CZT, kernel of the plan): the grids, winds and amplitudes of test_both_forms_of_the_direct_sum
REINIT = [(12, 1.0, 12.39, 0.01, 1, "k_czt_one"),                # chirp-z, one launch
          (65, 0.5, 40.0, 1e-5, 1, "k_czt_rows_assemble"),       # chirp-z, M = 256, two launches
          (65, 0.5, 40.0, 1e-5, 0, GEMM_NAME)]                   # GEMM at Np = 128: two tiles per axis, 63 padding lines


@pytest.mark.parametrize("N,u,L,amp,czt,kernel", REINIT, ids=["chirp-z-one-12", "chirp-z-two-65", "gemm-65"])
def test_reinit_before_the_first_frame_on_both_forms(mw, oracle, N, u, L, amp, czt, kernel):
    """The tables of both forms are built when the handle is created and replaced by reinit_spectrum, never by an enqueue (direct_tables).
    A handle whose length changes before its first frame -- the tables of creation never used -- must then be the handle a fresh create
    with the new length gives: spectrum, frame and velocity bit for bit, on the plan expected.  A handle at the original length is held
    to the f64 oracle at the direct paths' 2e-5 first, so that what is compared bit for bit is a frame of the right sea."""
    p = oracle.Params(N=N, unit_width=u, length=L, wind_x=5.0, wind_y=3.0, amplitude=amp, choppiness=0.8)
    new = dataclasses.replace(p, length=1.3 * L)
    try:
        mw.set_switch("MW_DIRECT_CZT", czt)      # read when a handle is created
        with _ocean(mw, p) as o:
            h0, h0c = o.get_spectrum()
            _check_frame(oracle, p, o.evaluate(1.25), h0, h0c, 1.25, f"reinit N={N} czt={czt} original length")
        with _ocean(mw, p) as o:
            o.reinit_spectrum(length=new.length, seed=9)      # no frame since creation
            a = o.get_spectrum() + o.evaluate(1.25) + (o.velocity(),)
            assert any(kernel in k for k in _plan(o)), kernel
        with _ocean(mw, new, seed=9) as f:
            b = f.get_spectrum() + f.evaluate(1.25) + (f.velocity(),)
            assert any(kernel in k for k in _plan(f)), kernel
    finally:
        mw.set_switch("MW_DIRECT_CZT", 1)
    assert len(a) == 6 and all(np.isfinite(x).all() for x in a) and np.abs(a[5]).max() > 0
    for name, x, y in zip(("h0", "h0conj", "vertices", "normals", "colours", "velocity"), a, b):
        assert (x == y).all(), f"reinit + evaluate differs from create + evaluate in {name}"
