"""Batched OceanRenderer handles (mw_ocean_create_batch) at every texture size and tile count, through the C ABI.

A handle of T > 1 tiles does not run the launches a single handle runs (csrc/ocean_renderer_device.h, or_launch_passes): all fields of a
column job in one pass-1 workgroup (gridDim.y == 1) with grouped spectrum loads, the unsplit packed pass 2, streaming exchange stores,
k_or_normal_white<true>, and a tile offset in every kernel.  Below 2048^2 those forms run only for a batched handle.  The header's promise
(include/mistral_water.h: "Per-tile results are identical to single handles of seed + k") is held here bit for bit at every instantiated
size and under both plans of a planar frame; the shape bench.py times with --tiles is held to the float64 oracle on its own, since single
handles share the code under test.

Device destinations are one tile longer than the call needs and pre-filled with a sentinel: a tile offset with a wrong multiplier lands
there or leaves a tile unwritten (an unwritten tile keeps the sentinel and fails the comparison with its single handle)."""
import ctypes as C

import numpy as np
import pytest

import or_bounds
from test_ocean_renderer import _frame_dts, shipped, tol_check

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e5                                  # no texel of any texture comes near it (heights and displacements are metres)
NAMES = ("height", "disp", "normal", "white")


@pytest.fixture(params=["packed", "three"])
def plan(request, mw):
    """MW_OR_PACKED = 1: two transforms per planar frame wherever the phase texture is mirror-symmetric; 0: the shaders' three."""
    try:
        mw.set_switch("MW_OR_PACKED", 1 if request.param == "packed" else 0)
        yield request.param
    finally:
        mw.set_switch("MW_OR_PACKED", 1)


def _kw(mw, rp, **over):
    kw = dict(resolution=rp.resolution, unit_width=0.75, length=rp.length, wind=(rp.wind_x, rp.wind_y), amplitude=rp.amplitude,
              choppiness=rp.choppiness, gravity=rp.gravity, mult=rp.mult, semantics=mw.MW_SEM_OCEANRENDERER)
    kw.update(over)
    return kw


def _guarded(shape_per_tile, tiles):
    import torch
    return torch.full((tiles + 1,) + tuple(shape_per_tile), SENTINEL, dtype=torch.float32, device="cuda")


def _deliver(o, bufs, what):
    """After the call that wrote `bufs`: the extra tile still holds the sentinel; -> the tiles the call owns."""
    o.synchronize()
    for name, b in zip(NAMES, bufs):
        assert bool((b[o.ntiles] == SENTINEL).all()), f"{what}: {name} written past tile {o.ntiles - 1}"
    return [b[:o.ntiles] for b in bufs]


def _frame(mw, o, dt, rgba=False):
    """One GenerateTexture() of every tile of `o` through the device form -> [tiles, M, M(, c)] tensors (height, disp, normal, white)."""
    import torch
    M = o.N
    tails = ((4,),) * 4 if rgba else ((), (2,), (3,), ())
    bufs = [_guarded((M, M) + t, o.ntiles) for t in tails]
    torch.cuda.synchronize()                        # the fill ran on torch's stream, the call runs on the handle's
    fn = mw.lib().mw_ocean_generate_texture_rgba_device if rgba else mw.lib().mw_ocean_generate_texture_device
    mw.check(fn(o.handle, C.c_float(dt), *[C.c_void_p(b.data_ptr()) for b in bufs]))
    return _deliver(o, bufs, f"M={M} tiles={o.ntiles} {'rgba' if rgba else 'planar'} dt={dt}")


def _mesh(mw, o):
    """mw_ocean_displace_mesh_device of every tile -> [tiles, res^2(, 3)] tensors (vertices, normals, colours)."""
    import torch
    nv = o.mesh_resolution ** 2
    bufs = [_guarded((nv, 3), o.ntiles), _guarded((nv, 3), o.ntiles), _guarded((nv,), o.ntiles)]
    torch.cuda.synchronize()
    mw.check(mw.lib().mw_ocean_displace_mesh_device(o.handle, *[C.c_void_p(b.data_ptr()) for b in bufs]))
    return _deliver(o, bufs, f"M={o.N} tiles={o.ntiles} mesh")


def _assert_tile(batch, single, k, tag, names=NAMES):
    """Tile k of the batched handle's arrays has the bits of the single handle's."""
    import torch
    for name, x, y in zip(names, batch, single):
        x, y = x[k], y[0]
        if not torch.equal(x, y):
            diff = (x != y)
            raise AssertionError(f"{tag}, tile {k}, {name}: {int(diff.sum())} of {diff.numel()} values differ, "
                                 f"largest difference {float((x - y).abs().max()):.3e}")


def _assert_distinct(tex, tag):
    import torch
    T = tex.shape[0]
    for i in range(T):
        for j in range(i + 1, T):
            assert not torch.equal(tex[i], tex[j]), f"{tag}: tiles {i} and {j} are the same ocean"


def _compare(mw, b, singles, dt, tag, rgba=False):
    """One frame of the batched handle and of every single handle; every tile bit for bit.  -> the batched handle's tensors."""
    B = _frame(mw, b, dt, rgba)
    for k, o in enumerate(singles):
        _assert_tile(B, _frame(mw, o, dt, rgba), k, f"{tag} dt={dt}{' rgba' if rgba else ''}")
    return B


def _compare_mesh(mw, b, singles, tag):
    V = _mesh(mw, b)
    for k, o in enumerate(singles):
        _assert_tile(V, _mesh(mw, o), k, f"{tag} mesh", names=("vertices", "normals", "colours"))


def _compare_phase(b, singles, tag):
    ph = b.get_phase().reshape(len(singles), b.N, b.N)
    for k, o in enumerate(singles):
        assert (ph[k] == o.get_phase()).all(), f"{tag}: phase of tile {k}"
    return ph


def _close(handles):
    for o in handles:
        o.close()


# ---- 1. every texture size: each tile equals its single handle, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("resolution", [8, 16, 32, 64, 128, 256])
def test_batched_tiles_equal_single_handles_at_every_size(mw, resolution, plan):
    """T = 3 (odd, > 2) at M = 64 ... 2048: four planar frames over a paused frame, the ten-minute jump (fmod path) and a negative step,
    then an RGBA frame (three transforms and the imag planes of a batch, k_or_pack_rgba over tiles), the vertex stage, and one more planar
    frame (the packed plan again after an RGBA call) -- every texture of every tile, and the phase, against single handles of seed + k."""
    rp = shipped(resolution)
    T, seed = 3, 5
    tag = f"M={rp.M} {plan}"
    singles = []
    try:
        with mw.Ocean(seed=seed, ntiles=T, **_kw(mw, rp)) as b:
            assert mw.lib().mw_ocean_batch_size(b.handle) == T and b.N == rp.M
            singles = [mw.Ocean(seed=seed + k, **_kw(mw, rp)) for k in range(T)]
            dts = [float(x) for x in _frame_dts(8)[[0, 3, 5, 6]]]        # 0.016, 0.0 (paused), 600.0 (fmod path), -0.02
            assert dts[1] == 0.0 and dts[2] == 600.0 and dts[3] < 0.0
            for f, dt in enumerate(dts):
                B = _compare(mw, b, singles, dt, f"{tag} frame {f}")
                _assert_distinct(B[0], f"{tag} frame {f}")
                if f == 0:      # the switch is live: the same frame of the same oceans under the other plan differs in the last bits
                    try:
                        mw.set_switch("MW_OR_PACKED", 0 if plan == "packed" else 1)
                        with mw.Ocean(seed=seed, ntiles=T, **_kw(mw, rp)) as other:
                            H_other = _frame(mw, other, dt)[0]
                    finally:
                        mw.set_switch("MW_OR_PACKED", 1 if plan == "packed" else 0)
                    assert not bool((B[0] == H_other).all()), f"{tag}: both settings of MW_OR_PACKED gave the same heights"
                    del H_other
                del B
            _compare_phase(b, singles, f"{tag} after frame {len(dts) - 1}")
            _compare(mw, b, singles, 0.05, tag, rgba=True)
            _compare_mesh(mw, b, singles, tag)
            _compare(mw, b, singles, 0.02, f"{tag} after rgba")
            _compare_phase(b, singles, f"{tag} at the end")
    finally:
        _close(singles)


def test_batched_tiles_equal_single_handles_at_4096(mw):
    """M = 4096 has the three-transform plan only (MW_OR_PACKED_MAX_M); its P = 16, 1024-thread workgroups gain a blockIdx.z.  T = 2, two
    frames, compared on the device (about 1 GB of textures per frame stays there)."""
    rp = shipped(512)
    T, seed = 2, 5
    tag = f"M={rp.M}"
    singles = []
    try:
        with mw.Ocean(seed=seed, ntiles=T, **_kw(mw, rp)) as b:
            assert b.N == 4096
            singles = [mw.Ocean(seed=seed + k, **_kw(mw, rp)) for k in range(T)]
            for f, dt in enumerate((0.016, 600.0)):
                B = _compare(mw, b, singles, dt, f"{tag} frame {f}")
                _assert_distinct(B[0], f"{tag} frame {f}")
                del B
            _compare_mesh(mw, b, singles, tag)
            _compare_phase(b, singles, tag)
    finally:
        _close(singles)


# ---- 2. the timed shape against the oracle ---------------------------------------------------------------------------------------------
def test_timed_batched_shape_against_the_oracle(mw, oracle, plan):
    """What bench.py times with --tiles 4 (resolution 128, 1024^2 textures, one call per frame of 4 oceans) has no parity gate there (the
    gate runs for one tile only).  The last tile of such a handle against the float64 oracle: frames 0 and 2 at the usual bounds, the
    phase after frame 2 against the strict-float32 recurrence bit for bit.  Not through single handles: they share the code under test."""
    rp = shipped(128)
    M, T, k = rp.M, 4, 3
    with mw.Ocean(seed=1, ntiles=T, **_kw(mw, rp)) as b:
        g0, g0c = b.get_spectrum()
        init4 = np.concatenate([g0[k], g0c[k]], -1)
        del g0, g0c
        ph = np.zeros((M, M), np.float32)
        for f, dt in enumerate(float(x) for x in _frame_dts(3)):
            B = _frame(mw, b, dt)
            if f == 0:
                _assert_distinct(B[0], f"M={M} T={T} {plan}")
            if f in (0, 2):
                h, d, n, w = (x[k].cpu().numpy() for x in B)
                H, D, Nn, W, G = oracle.renderer_step_f64(rp, init4, ph, dt, literal_passes=False)
                tol_check(h, H, 3e-6, f"height, tile {k} frame {f}"); tol_check(d, D, 3e-6, f"disp, tile {k} frame {f}")
                or_bounds.assert_normal_white(n, w, Nn, W, rp.length, D[..., 0], G, D[..., 1], H, tag=f"M={M} T={T} {plan} tile {k} frame {f}")
            else:
                oracle.renderer_advance_phase(rp, init4, ph, dt)
            del B
        assert (b.get_phase()[k] == ph).all()


# ---- 3. the two single-handle sizes nobody compares with the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [16, 64])
def test_single_handle_vs_oracle_at_128_and_512(mw, oracle, resolution, plan):
    """M = 128 and M = 512, single handle: what test_gpu_generate_texture_vs_oracle does for its sizes, then one generate_texture_steps
    call of 5 frames -- frames 0 and 4 against the oracle, the phase after the call bit for bit."""
    rp = shipped(resolution)
    M = rp.M
    with mw.Ocean(seed=5, **_kw(mw, rp)) as o:
        assert o.N == M
        init4 = oracle.renderer_initial_spectrum(rp, 5)
        g0, g0c = o.get_spectrum()                                # device-generated spectrum: the oracle's up to device libm
        sc = np.abs(init4).max()
        assert np.abs(g0 - init4[..., :2]).max() < 5e-6 * sc and np.abs(g0c - init4[..., 2:]).max() < 5e-6 * sc
        o.set_spectrum(init4[..., :2], init4[..., 2:])            # the SAME spectrum from here on
        ph = np.zeros((M, M), np.float32)

        def against_oracle(tex, dt, tag):
            h, d, n, w = tex
            H, D, Nn, W, G = oracle.renderer_step_f64(rp, init4, ph, dt, literal_passes=False)      # advances ph
            tol_check(h, H, 3e-6, f"height {tag}"); tol_check(d, D, 3e-6, f"disp {tag}")
            or_bounds.assert_normal_white(n, w, Nn, W, rp.length, D[..., 0], G, D[..., 1], H, tag=f"M={M} {plan} {tag}")
        for dt in (0.016, 0.033, 0.3, 25.0):
            against_oracle(o.generate_texture(dt), dt, f"dt={dt}")
        tex = o.generate_texture_rgba(0.016)                       # the normal / whitecap passes alone, on the device's own textures
        oracle.renderer_advance_phase(rp, init4, ph, 0.016)
        rn, rw, mn, mw_ = or_bounds.assert_normal_white_stage(oracle, rp, *tex, tag=f"M={M}")
        assert mn < 2e-3 * max(1.0, M / 1024.0) ** 2, mn
        dts = _frame_dts(5)
        F = o.generate_texture_steps(dts)
        for f, dt in enumerate(float(x) for x in dts):
            if f in (0, 4):
                against_oracle([x[f] for x in F], dt, f"steps frame {f}")
            else:
                oracle.renderer_advance_phase(rp, init4, ph, dt)
        assert (o.get_phase() == ph).all()


# ---- 4. tile-count edges, at M = 64 --------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_batch_of_one_is_a_single_handle(mw, plan):
    """mw_ocean_create_batch(..., 1): the textures of mw_ocean_create with the same seed, and everything a single handle accepts
    (the refusals of a batched handle test tiles != 1)."""
    rp = shipped(8)
    with mw.Ocean(seed=6, **_kw(mw, rp)) as single, mw.Ocean(seed=6, **_kw(mw, rp)) as one:
        one.close()                                                   # the wrapper's ntiles = 1 goes through mw_ocean_create:
        mw.check(mw.lib().mw_ocean_create_batch(C.byref(one.params), 1, C.byref(one._h)))    # the same wrapper around a batch of one
        assert mw.lib().mw_ocean_batch_size(one.handle) == 1 and mw.lib().mw_ocean_batch_size(single.handle) == 1
        assert one.max_frames() == single.max_frames() == 32
        for x, y in zip(one.get_spectrum(), single.get_spectrum()):
            assert (x == y).all()
        tag = f"batch of one {plan}"
        for dt in (0.016, 0.3):
            _compare(mw, one, [single], dt, tag)
        _compare(mw, one, [single], 0.05, tag, rgba=True)
        _compare_mesh(mw, one, [single], tag)
        dts = _frame_dts(3)
        for x, y in zip(one.generate_texture_steps(dts), single.generate_texture_steps(dts)):
            assert (x == y).all()
        xz = np.random.default_rng(2).uniform(-4.0, 4.0, (500, 2)).astype(np.float32)
        for mode in ("world", "rest"):
            for frame in (-1, 1):
                qa, qb = one.query_surface(xz, mode=mode, frame=frame), single.query_surface(xz, mode=mode, frame=frame)
                assert np.array_equal(_bits(qa), _bits(qb)), (mode, frame)
        _compare_phase(one, [single], tag)


@pytest.mark.parametrize("T", [2, 64])
def test_tile_count_edges_equal_single_handles(mw, T, plan):
    """T = 2: where or_all_fields / or_call_is_big switch to the batched launch forms; T = 64: the maximum (gridDim.z == 64).  Every tile
    after each of two frames, and its phase."""
    rp = shipped(8)
    seed, dts = 11, (0.016, 0.3)
    tag = f"M={rp.M} T={T} {plan}"
    with mw.Ocean(seed=seed, ntiles=T, **_kw(mw, rp)) as b:
        assert mw.lib().mw_ocean_batch_size(b.handle) == T and b.max_frames() == 0
        frames = [_frame(mw, b, dt) for dt in dts]
        _assert_distinct(frames[-1][0], tag)
        ph = b.get_phase()
        for k in range(T):
            with mw.Ocean(seed=seed + k, **_kw(mw, rp)) as o:
                for f, dt in enumerate(dts):
                    _assert_tile(frames[f], _frame(mw, o, dt), k, f"{tag} frame {f}")
                assert (ph[k] == o.get_phase()).all(), f"{tag}: phase of tile {k}"


@pytest.mark.parametrize("T", [0, 65])
def test_tile_count_out_of_range_is_refused(mw, T):
    with pytest.raises(mw.MistralWaterError) as e:
        mw.Ocean(seed=1, ntiles=T, **_kw(mw, shipped(8)))
    assert e.value.status == mw.MW_EINVAL


# ---- 5. state of a batch routes tile k to tile k, at M = 256 ------------------------------------------------------------------------------
def test_batch_set_spectrum_routes_each_tile(mw, oracle, plan):
    """Tile-major mw_ocean_set_spectrum: three different spectra (the oracle's, seeds out of order); each tile is then the single handle
    given that tile's spectrum."""
    rp = shipped(32)
    T = 3
    init = np.stack([oracle.renderer_initial_spectrum(rp, s) for s in (9, 4, 6)])          # [T, M, M, 4]
    assert not (init[0] == init[1]).all() and not (init[1] == init[2]).all()
    singles = []
    try:
        with mw.Ocean(seed=2, ntiles=T, **_kw(mw, rp)) as b:
            singles = [mw.Ocean(seed=40, **_kw(mw, rp)) for _ in range(T)]
            b.generate_texture(0.1)                                # not from a fresh handle: set_spectrum restarts the phase
            b.set_spectrum(init[..., :2], init[..., 2:])
            for k, o in enumerate(singles):
                o.set_spectrum(init[k, ..., :2], init[k, ..., 2:])
            g0, g0c = b.get_spectrum()
            for k, o in enumerate(singles):
                s0, s0c = o.get_spectrum()
                assert (g0[k] == s0).all() and (g0c[k] == s0c).all(), k
            tag = f"M={rp.M} set_spectrum {plan}"
            for dt in (0.016, 0.3):
                B = _compare(mw, b, singles, dt, tag)
                _assert_distinct(B[0], tag)
            _compare_phase(b, singles, tag)
    finally:
        _close(singles)


def test_batch_reinit_spectrum_reseeds_each_tile(mw, plan):
    """mw_ocean_reinit_spectrum(seed) on a batch: tile k is the single handle re-initialised with seed + k; the phase is untouched."""
    rp = shipped(32)
    T = 3
    singles = []
    try:
        with mw.Ocean(seed=3, ntiles=T, **_kw(mw, rp)) as b:
            singles = [mw.Ocean(seed=3 + k, **_kw(mw, rp)) for k in range(T)]
            tag = f"M={rp.M} reinit {plan}"
            _compare(mw, b, singles, 0.4, tag)
            before = b.get_phase()
            assert before.any()
            b.reinit_spectrum(seed=20, wind=(9.0, -4.0))
            for k, o in enumerate(singles):
                o.reinit_spectrum(seed=20 + k, wind=(9.0, -4.0))
            assert (b.get_phase() == before).all()
            g0, g0c = b.get_spectrum()
            for k, o in enumerate(singles):
                s0, s0c = o.get_spectrum()
                assert (g0[k] == s0).all() and (g0c[k] == s0c).all(), k
            assert not (g0[0] == g0[1]).all() and not (g0[1] == g0[2]).all() and not (g0[0] == g0[2]).all()
            B = _compare(mw, b, singles, 0.033, tag)
            _assert_distinct(B[0], tag)
            _compare_phase(b, singles, tag)
    finally:
        _close(singles)


def test_one_asymmetric_tile_moves_the_whole_batch_to_three_transforms(mw, oracle):
    """phase_sym is one flag per handle: a phase texture that is not mirror-symmetric on tile 1 alone selects the three-transform plan for
    the whole call whatever the switch says -- tiles 0 and 2 included -- and the library's own phases, set back, return it to the packed
    plan (its bits, not the other plan's)."""
    rp = shipped(32)
    M, T = rp.M, 3
    singles = []
    try:
        with mw.Ocean(seed=8, ntiles=T, **_kw(mw, rp)) as b:
            singles = [mw.Ocean(seed=8 + k, **_kw(mw, rp)) for k in range(T)]
            g0, g0c = b.get_spectrum()
            init4 = np.concatenate([g0[1], g0c[1]], -1)
            mw.set_switch("MW_OR_PACKED", 1)
            _compare(mw, b, singles, 0.4, f"M={M} before set_phase")
            own = b.get_phase()                                     # every tile's own, library-made phase: mirror-symmetric
            mirror = (-np.arange(M)) % M
            assert all((own[k] == own[k][mirror][:, mirror]).all() for k in range(T))
            bad = own.copy()
            bad[1] = np.random.default_rng(3).uniform(0, 6.2, (M, M)).astype(np.float32)
            assert not (bad[1] == bad[1][mirror][:, mirror]).all()
            b.set_phase(bad)
            B = _frame(mw, b, 0.05)                                 # the switch says packed
            mw.set_switch("MW_OR_PACKED", 0)
            for k, o in enumerate(singles):
                o.set_phase(bad[k])
                _assert_tile(B, _frame(mw, o, 0.05), k, f"M={M} asymmetric tile 1, singles on three transforms")
            ph = bad[1].copy()
            H, D, Nn, W, G = oracle.renderer_step_f64(rp, init4, ph, 0.05, literal_passes=False)
            h, d, n, w = (x[1].cpu().numpy() for x in B)
            tol_check(h, H, 3e-6, "height, injected phase"); tol_check(d, D, 3e-6, "disp, injected phase")
            or_bounds.assert_normal_white(n, w, Nn, W, rp.length, D[..., 0], G, D[..., 1], H, tag=f"M={M} tile 1, injected phase")
            assert (_compare_phase(b, singles, f"M={M} injected phase")[1] == ph).all()
            # back to the packed plan: every tile takes a phase the library made
            mw.set_switch("MW_OR_PACKED", 1)
            b.set_phase(own)
            for k, o in enumerate(singles):
                o.set_phase(own[k])
            b.set_phase(b.get_phase())
            B = _compare(mw, b, singles, 0.02, f"M={M} own phases back, packed")
            mw.set_switch("MW_OR_PACKED", 0)
            with mw.Ocean(seed=8, **_kw(mw, rp)) as three:          # ... and those are not the three-transform plan's bits
                three.set_phase(own[0])
                assert not bool((_frame(mw, three, 0.02)[0][0] == B[0][0]).all())
    finally:
        mw.set_switch("MW_OR_PACKED", 1)
        _close(singles)


def test_batch_choppiness_and_normal_length_reach_every_tile(mw, plan):
    """mw_ocean_set_choppiness and mw_ocean_set_normal_length between frames: each tile is the single handle that received the same change."""
    rp = shipped(32)
    T = 3
    singles = []
    try:
        with mw.Ocean(seed=13, ntiles=T, **_kw(mw, rp)) as b:
            singles = [mw.Ocean(seed=13 + k, **_kw(mw, rp)) for k in range(T)]
            tag = f"M={rp.M} {plan}"
            first = _compare(mw, b, singles, 0.016, tag)
            for o in [b] + singles:
                o.set_choppiness(1.3)
            chop = _compare(mw, b, singles, 0.0, f"{tag} choppiness 1.3")      # a paused frame: only the choppiness moved
            import torch
            assert not torch.equal(first[1], chop[1])               # (the packed plan's heights share a transform with Dz: not compared)
            for o in [b] + singles:
                o.normal_length = 0.5 * rp.length
            nl = _compare(mw, b, singles, 0.0, f"{tag} normal length halved")   # ... and now only the normal pass's length
            assert torch.equal(chop[0], nl[0]) and torch.equal(chop[1], nl[1]) and not torch.equal(chop[2], nl[2])
            _compare(mw, b, singles, 0.033, f"{tag} after both")
    finally:
        _close(singles)
