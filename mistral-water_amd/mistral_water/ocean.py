"""Ocean handle + FFTMesh / OceanRenderer mirrors (reference: Assets/Mistral Water/Scripts/*.cs)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as nat


_hip = None


def _d2h(ptr, shape, dtype=np.float32):
    """Copy a raw device pointer handed out by the C ABI into a new host array (hipMemcpy, synchronous)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(shape, dtype)
    rc = _hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2)
    if rc != 0:
        raise RuntimeError(f"hipMemcpy D2H failed ({rc})")
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class Vector2:
    x: float = 0.0
    y: float = 0.0


class Ocean:
    """Thin RAII wrapper of an ``mw_ocean*``."""

    def __init__(self, *, resolution, unit_width=1.0, length=1.0, wind=(1.0, 1.0), amplitude=1.0, choppiness=1.0,
                 gravity=9.81, t_division=1.0, mult=1.0, seed=1, semantics=nat.MW_SEM_FFTMESH, device=0, ntiles=1):
        """ntiles > 1 (OceanRenderer semantics): a batched handle, tile k = seed + k; every OceanRenderer array then carries a
        leading tile axis (mw_ocean_create_batch)."""
        self._h = C.c_void_p()
        self.params = nat.MwParams(int(resolution), float(unit_width), float(length), float(wind[0]), float(wind[1]),
                                   float(amplitude), float(choppiness), float(gravity), float(t_division), float(mult),
                                   int(seed), int(semantics), int(device))
        self.ntiles = int(ntiles)
        if self.ntiles == 1:
            nat.check(nat.lib().mw_ocean_create(C.byref(self.params), C.byref(self._h)))
        else:
            nat.check(nat.lib().mw_ocean_create_batch(C.byref(self.params), self.ntiles, C.byref(self._h)))
        self.N = nat.lib().mw_ocean_grid_size(self._h)
        self.mesh_resolution = int(resolution)
        self.semantics = int(semantics)

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            nat.lib().mw_ocean_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def set_stream(self, hip_stream: int | None):
        """Run the handle's work on `hip_stream` (a hipStream_t as int).  0 is HIP's legacy default stream -- what
        ``torch.cuda.current_stream().cuda_stream`` is unless a side stream is current; ``None`` returns to the handle's
        own private non-blocking stream (mw_ocean_use_own_stream)."""
        if hip_stream is None:
            nat.check(nat.lib().mw_ocean_use_own_stream(self._h))
        else:
            nat.check(nat.lib().mw_ocean_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        nat.check(nat.lib().mw_ocean_synchronize(self._h))

    def set_choppiness(self, c: float):
        nat.check(nat.lib().mw_ocean_set_choppiness(self._h, C.c_float(c)))

    def set_periodic(self, on: bool = True):
        """The surface services (query_surface, query_velocity, hull_forces, step_bodies) read the infinite tiling of the FFTMesh
        frame instead of the one footprint (mw_ocean_set_periodic).  MW_ENOTCOMMENSURATE unless unit_width * N == length with N even;
        MW_ESTATE on an OceanRenderer handle.  raycast() reads the one footprint and refuses a periodic handle; raycast_tiled() casts
        on the tiling whatever the switch says."""
        nat.check(nat.lib().mw_ocean_set_periodic(self._h, 1 if on else 0))

    def _get_periodic(self):
        on, period = C.c_int32(0), C.c_float(0.0)
        nat.check(nat.lib().mw_ocean_get_periodic(self._h, C.byref(on), C.byref(period)))
        return bool(on.value), float(period.value)

    @property
    def periodic(self) -> bool:
        return self._get_periodic()[0]

    @property
    def period(self) -> float:
        """P = float32(N) * unit_width where the grid repeats (whether or not the switch is on), else 0."""
        return self._get_periodic()[1]

    # -- spectrum ----------------------------------------------------------------------------
    def set_spectrum(self, h0, h0conj):
        h0 = np.ascontiguousarray(h0, np.float32)
        h0conj = np.ascontiguousarray(h0conj, np.float32)
        assert h0.size == 2 * self.N * self.N * self.ntiles and h0conj.size == h0.size
        nat.check(nat.lib().mw_ocean_set_spectrum(self._h, _p(h0), _p(h0conj)))

    def _t(self, *shape):
        """Array shape with the leading tile axis of a batched handle."""
        return ((self.ntiles,) if self.ntiles > 1 else ()) + tuple(shape)

    def get_spectrum(self):
        h0 = np.empty(self._t(self.N, self.N, 2), np.float32)
        h0c = np.empty(self._t(self.N, self.N, 2), np.float32)
        nat.check(nat.lib().mw_ocean_get_spectrum(self._h, _p(h0), _p(h0c)))
        return h0, h0c

    def reinit_spectrum(self, length=None, wind=None, amplitude=None, seed=None):
        """Regenerate the initial spectrum in place (mw_ocean_reinit_spectrum); None keeps the handle's current value.
        OceanRenderer: RenderInitial() again, phase untouched (S/OceanRenderer.cs:98-109)."""
        p = self.params
        length = p.length if length is None else float(length)
        wx, wy = (p.wind_x, p.wind_y) if wind is None else (float(wind[0]), float(wind[1]))
        amplitude = p.amplitude if amplitude is None else float(amplitude)
        seed = p.seed if seed is None else int(seed)
        nat.check(nat.lib().mw_ocean_reinit_spectrum(self._h, C.c_float(length), C.c_float(wx), C.c_float(wy), C.c_float(amplitude),
                                                     C.c_uint64(seed)))
        p.length, p.wind_x, p.wind_y, p.amplitude, p.seed = length, wx, wy, amplitude, seed

    def get_phase(self):
        """OceanRenderer: the stateful phase texture [M, M] (texel (px,py) at [py, px])."""
        ph = np.empty(self._t(self.N, self.N), np.float32)
        nat.check(nat.lib().mw_ocean_get_phase(self._h, _p(ph)))
        return ph

    def set_phase(self, phase):
        ph = np.ascontiguousarray(phase, np.float32)
        assert ph.size == self.N * self.N * self.ntiles
        nat.check(nat.lib().mw_ocean_set_phase(self._h, _p(ph)))

    @property
    def normal_length(self) -> float:
        """OceanRenderer: normalMat._Length (S/OceanRenderer.cs:163) -- set at creation, not by reinit_spectrum; part of a checkpoint."""
        return float(nat.lib().mw_ocean_normal_length(self._h))

    @normal_length.setter
    def normal_length(self, v: float):
        nat.check(nat.lib().mw_ocean_set_normal_length(self._h, C.c_float(v)))

    def set_timer(self, t: float):
        nat.check(nat.lib().mw_ocean_set_timer(self._h, C.c_float(t)))

    def rest_mesh(self):
        n = self.mesh_resolution
        v = np.empty((n * n, 3), np.float32)
        nr = np.empty((n * n, 3), np.float32)
        uv = np.empty((n * n, 2), np.float32)
        idx = np.empty((nat.lib().mw_ocean_index_count(self._h),), np.int32)
        nat.check(nat.lib().mw_ocean_rest_mesh(self._h, _p(v), _p(nr), _p(uv), _p(idx)))
        return v, nr, uv, idx

    # -- FFTMesh semantics -------------------------------------------------------------------
    def evaluate(self, t: float):
        """EvaluateWaves(t): (vertices [N*N,3], normals [N*N,3], colors [N*N,4]) on the host."""
        NN = self.N * self.N
        v = np.empty((NN, 3), np.float32)
        n = np.empty((NN, 3), np.float32)
        c = np.empty((NN, 4), np.float32)
        nat.check(nat.lib().mw_ocean_evaluate(self._h, C.c_float(t), _p(v), _p(n), _p(c)))
        return v, n, c

    def evaluate_into(self, t: float, vertices, normals, colors):
        """EvaluateWaves(t) into caller arrays kept across frames (the reference's vertMeow/normals, S/FFTMesh.cs:90-99);
        register them once with ``host_register`` and the copy runs at PCIe rate instead of the pageable ~9 GB/s."""
        nat.check(nat.lib().mw_ocean_evaluate(self._h, C.c_float(t), _p(vertices), _p(normals), _p(colors)))

    def update(self, delta_time: float):
        NN = self.N * self.N
        v = np.empty((NN, 3), np.float32)
        n = np.empty((NN, 3), np.float32)
        c = np.empty((NN, 4), np.float32)
        nat.check(nat.lib().mw_ocean_update(self._h, C.c_float(delta_time), _p(v), _p(n), _p(c)))
        return v, n, c

    @property
    def timer(self) -> float:
        return nat.lib().mw_ocean_timer(self._h)

    def reset_timer(self):
        nat.check(nat.lib().mw_ocean_reset_timer(self._h))

    @property
    def max_batch(self) -> int:
        return nat.lib().mw_ocean_max_batch(self._h)

    def evaluate_device(self, times, d_vertices: int, d_normals: int, d_white: int, rgba: bool = False):
        """Enqueue len(times) independent time-steps; outputs are raw device pointers (ints)."""
        tt = np.ascontiguousarray(times, np.float32)
        nat.check(nat.lib().mw_ocean_evaluate_device(self._h, _p(tt), tt.size, C.c_void_p(d_vertices),
                                                     C.c_void_p(d_normals), C.c_void_p(d_white),
                                                     nat.MW_OUT_COLOR_RGBA if rgba else nat.MW_OUT_WHITE_SCALAR))

    def profile_kernels(self, nsteps: int = 1, iters: int = 20):
        ms = (C.c_float * 8)()
        names = (C.c_char_p * 8)()
        nk = C.c_int32(0)
        nat.check(nat.lib().mw_ocean_profile_kernels(self._h, nsteps, iters, ms, names, C.byref(nk)))
        return [(names[k].decode(), float(ms[k])) for k in range(nk.value)]

    def profile_kernels_stats(self, nsteps: int = 1, iters: int = 20):
        """[(kernel name, {mean, median, p10, p90, min, max} in ms)] over `iters` launches (mw_ocean_profile_kernels_stats)."""
        st = (C.c_float * 48)()
        names = (C.c_char_p * 8)()
        nk = C.c_int32(0)
        nat.check(nat.lib().mw_ocean_profile_kernels_stats(self._h, nsteps, iters, st, names, C.byref(nk)))
        keys = ("mean", "median", "p10", "p90", "min", "max")
        return [(names[k].decode(), {kk: float(st[6 * k + i]) for i, kk in enumerate(keys)}) for k in range(nk.value)]

    def debug_evaluate_hds(self, t: float):
        """EvaluateWaves(t) plus hds [N*N, 2] exactly as the kernels hold it (test hook of the whitecap stage)."""
        NN = self.N * self.N
        v, n = np.empty((NN, 3), np.float32), np.empty((NN, 3), np.float32)
        c, h = np.empty((NN, 4), np.float32), np.empty((NN, 2), np.float32)
        nat.check(nat.lib().mw_debug_evaluate_hds(self._h, C.c_float(t), _p(v), _p(n), _p(c), _p(h)))
        return v, n, c, h

    def debug_omega_t(self, t: float):
        out = np.empty((self.N, self.N), np.float32)
        nat.check(nat.lib().mw_debug_omega_t(self._h, C.c_float(t), _p(out)))
        return out

    # -- OceanRenderer semantics -------------------------------------------------------------
    def generate_texture(self, delta_time: float):
        M = self.N
        h = np.empty(self._t(M, M), np.float32)
        d = np.empty(self._t(M, M, 2), np.float32)
        n = np.empty(self._t(M, M, 3), np.float32)
        w = np.empty(self._t(M, M), np.float32)
        nat.check(nat.lib().mw_ocean_generate_texture(self._h, C.c_float(delta_time), _p(h), _p(d), _p(n), _p(w)))
        return h, d, n, w

    def generate_texture_rgba(self, delta_time: float):
        """One GenerateTexture() as the reference's four ARGBFloat render targets, [M,M,4] each
        (S/OceanRenderer.cs:143-146): height (Re h, Im h, Re h, Im h), displacement (Re Dx, Im Dx, Re Dz, Im Dz),
        normal (n, 1), white (w, w, w, 1)."""
        M = self.N
        t = [np.empty(self._t(M, M, 4), np.float32) for _ in range(4)]
        nat.check(nat.lib().mw_ocean_generate_texture_rgba(self._h, C.c_float(delta_time), *[_p(a) for a in t]))
        return tuple(t)

    def advance_phase(self, delta_times):
        """The phase texture after len(delta_times) more frames, no textures produced (mw_ocean_advance_phase): seek / skip."""
        dts = np.ascontiguousarray(delta_times, np.float32)
        nat.check(nat.lib().mw_ocean_advance_phase(self._h, _p(dts), int(dts.size)))

    def max_frames(self) -> int:
        return nat.lib().mw_ocean_max_frames(self._h)

    def generate_texture_steps_device(self, delta_times, d_height=None, d_disp=None, d_normal=None, d_white=None, rgba: bool = False):
        """len(delta_times) consecutive GenerateTexture() calls in one enqueue (asynchronous).  Device destinations are raw
        pointers of [n][M*M*...] arrays; None keeps the frames of that texture in the handle (frame_textures)."""
        dts = np.ascontiguousarray(delta_times, np.float32)
        fn = nat.lib().mw_ocean_generate_texture_steps_rgba_device if rgba else nat.lib().mw_ocean_generate_texture_steps_device
        nat.check(fn(self._h, _p(dts), int(dts.size), d_height, d_disp, d_normal, d_white))

    def frame_textures(self, frame: int):
        """Device pointers (ints, None when that texture went to a caller buffer) of frame `frame` of the latest steps call."""
        ptrs = [C.c_void_p() for _ in range(4)]
        nat.check(nat.lib().mw_ocean_frame_textures(self._h, int(frame), *[C.byref(q) for q in ptrs]))
        return tuple(q.value for q in ptrs)

    def generate_texture_steps(self, delta_times, rgba: bool = False):
        """Host form (mw_ocean_generate_texture_steps[_rgba]): -> (height [n,M,M], disp [n,M,M,2], normal [n,M,M,3], white [n,M,M]), or the
        four ARGBFloat targets [n,M,M,4] each with rgba=True."""
        dts = np.ascontiguousarray(delta_times, np.float32)
        n, M = int(dts.size), self.N
        tails = ((4,),) * 4 if rgba else ((), (2,), (3,), ())
        out = tuple(np.empty((n, M, M) + t, np.float32) for t in tails)
        fn = nat.lib().mw_ocean_generate_texture_steps_rgba if rgba else nat.lib().mw_ocean_generate_texture_steps
        nat.check(fn(self._h, _p(dts), n, *[_p(a) for a in out]))
        return out

    def displace_mesh(self):
        """The ocean material's vertex stage (W/TestOcean.shader:61-79) on the resolution^2 mesh, from the textures
        of the latest generate_texture*(): -> (vertices [n,3], normals [n,3], colors [n])."""
        n = self.mesh_resolution * self.mesh_resolution
        v, nr, c = np.empty(self._t(n, 3), np.float32), np.empty(self._t(n, 3), np.float32), np.empty(self._t(n), np.float32)
        nat.check(nat.lib().mw_ocean_displace_mesh(self._h, _p(v), _p(nr), _p(c)))
        return v, nr, c

    # -- surface queries (mw_ocean_query_surface) ----------------------------------------------
    _QUERY_MODES = {"rest": nat.MW_QUERY_REST, "world": nat.MW_QUERY_WORLD}

    def query_surface(self, xz, mode: str = "world", frame: int = -1, iterations: int = 0):
        """Height, normal and whitecap of the displaced mesh at horizontal points xz [n, 2] -> [n, 8] float32 rows
        (px, py, pz, nx, ny, nz, white, residual).  mode "world": xz is a point on the displaced surface (buoyancy);
        "rest": a rest-plane position (NaN off the mesh).  frame -1 = the latest frame; k = frame k of the latest
        OceanRenderer steps call.  iterations 0 = the library default (8), at most 64."""
        xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
        out = np.empty((xz.shape[0], 8), np.float32)
        nat.check(nat.lib().mw_ocean_query_surface(self._h, int(frame), self._QUERY_MODES[mode], _p(xz), xz.shape[0],
                                                    int(iterations), _p(out)))
        return out

    def query_surface_device(self, d_xz: int, n: int, d_out: int, mode: str = "world", frame: int = -1, iterations: int = 0):
        """Device-pointer form: d_xz [n][2] (8-byte aligned), d_out [n][8] (16-byte aligned) float32; asynchronous on the
        handle's stream (synchronize() or the stream before reading d_out)."""
        nat.check(nat.lib().mw_ocean_query_surface_device(self._h, int(frame), self._QUERY_MODES[mode], C.c_void_p(d_xz), int(n),
                                                           int(iterations), C.c_void_p(d_out)))

    # -- surface velocity (mw_ocean_velocity) --------------------------------------------------
    def _velocity_vertices(self):
        return self.N * self.N if self.semantics == nat.MW_SEM_FFTMESH else self.mesh_resolution * self.mesh_resolution

    def velocity(self, frame: int = -1):
        """Time derivative of the vertices of the frame query_surface reads -> [n, 3] float32, computed from the spectrum.
        FFTMesh: per unit of the time argument t (divide by t_division for per second of Update's deltaTime);
        OceanRenderer: per second of delta_time, at the handle's current phase (frame -1, or the last frame of the latest steps call)."""
        out = np.empty((self._velocity_vertices(), 3), np.float32)
        nat.check(nat.lib().mw_ocean_velocity(self._h, int(frame), _p(out)))
        return out

    def velocity_device(self, d_velocity: int, frame: int = -1):
        """Device-pointer form: d_velocity [n][3] float32; asynchronous on the handle's stream."""
        nat.check(nat.lib().mw_ocean_velocity_device(self._h, int(frame), C.c_void_p(d_velocity)))

    def query_velocity(self, xz, mode: str = "world", frame: int = -1, iterations: int = 0):
        """Velocity of the water at horizontal points xz [n, 2], located exactly as query_surface locates them -> [n, 4] float32
        rows (vx, vy, vz, residual); units as velocity()."""
        xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
        out = np.empty((xz.shape[0], 4), np.float32)
        nat.check(nat.lib().mw_ocean_query_velocity(self._h, int(frame), self._QUERY_MODES[mode], _p(xz), xz.shape[0],
                                                     int(iterations), _p(out)))
        return out

    def query_velocity_device(self, d_xz: int, n: int, d_out: int, mode: str = "world", frame: int = -1, iterations: int = 0):
        """Device-pointer form: d_xz [n][2] (8-byte aligned), d_out [n][4] (16-byte aligned) float32; asynchronous."""
        nat.check(nat.lib().mw_ocean_query_velocity_device(self._h, int(frame), self._QUERY_MODES[mode], C.c_void_p(d_xz), int(n),
                                                            int(iterations), C.c_void_p(d_out)))

    # -- the water column (mw_ocean_set_column) --------------------------------------------------
    def set_column(self, depths):
        """The rest depths of the column's layers, depths[0] == 0 < depths[1] < ... (2 to MW_COLUMN_MAX_LAYERS of them); None or an
        empty sequence releases the column.  FFTMesh handles only."""
        d = np.ascontiguousarray([] if depths is None else depths, np.float32).reshape(-1)
        nat.check(nat.lib().mw_ocean_set_column(self._h, _p(d) if d.size else None, int(d.size)))

    @property
    def column(self):
        """The depths of the column's layers, [L] float32 (empty: no column)."""
        n, d = C.c_int32(0), np.zeros(nat.MW_COLUMN_MAX_LAYERS, np.float32)
        nat.check(nat.lib().mw_ocean_get_column(self._h, _p(d), C.byref(n)))
        return d[:n.value].copy()

    def column_layers(self, layer: int, frame: int = -1):
        """Device pointers (ints) of one layer of the latest frame: (positions [N*N][3], velocities [N*N][3]); layer 0 is the surface mesh
        and the surface velocity.  Valid until the next frame, column or spectrum change."""
        pos, vel = C.c_void_p(), C.c_void_p()
        nat.check(nat.lib().mw_ocean_column_layers(self._h, int(frame), int(layer), C.byref(pos), C.byref(vel)))
        return pos.value, vel.value

    def column_layer_arrays(self, layer: int):
        """column_layers(layer) copied to the host: (positions [N*N, 3], velocities [N*N, 3]) float32."""
        pos, vel = self.column_layers(layer)
        self.synchronize()
        n = self.N * self.N
        return _d2h(pos, (n, 3)), _d2h(vel, (n, 3))

    def query_column(self, xyz, mode: str = "world", frame: int = -1, iterations: int = 0):
        """The water at points xyz [n, 3] (or [n, 4], the fourth float ignored) -> [n, 12] float32 rows
        (ux, uy, uz, rest_depth, px, py, pz, lambda, x0, z0, eta, residual).  mode "world": (x, y, z) is a position in the water;
        "rest": (x0, d, z0) a particle's rest-plane position and rest depth.  rho * g * rest_depth is the pressure there."""
        a = np.asarray(xyz, np.float32)
        a = a.reshape(-1, a.shape[-1] if a.ndim > 1 and a.shape[-1] in (3, 4) else 3)
        q = np.zeros((a.shape[0], 4), np.float32)
        q[:, :a.shape[1]] = a
        out = np.empty((q.shape[0], 12), np.float32)
        nat.check(nat.lib().mw_ocean_query_column(self._h, int(frame), self._QUERY_MODES[mode], _p(q), q.shape[0], int(iterations), _p(out)))
        return out

    def query_column_device(self, d_xyz: int, n: int, d_out: int, mode: str = "world", frame: int = -1, iterations: int = 0):
        """Device-pointer form: d_xyz [n][4], d_out [n][12] float32, both 16-byte aligned; asynchronous on the handle's stream."""
        nat.check(nat.lib().mw_ocean_query_column_device(self._h, int(frame), self._QUERY_MODES[mode], C.c_void_p(d_xyz), int(n),
                                                          int(iterations), C.c_void_p(d_out)))

    # -- draught (mw_ocean_set_draught) -----------------------------------------------------------
    def set_draught(self, on: bool = True):
        """Switch the hull family to the water column: hull_forces, step_bodies and their device forms give every instance vertex the
        column's rest depth (pressure over rho g) and, with drag on, the column's water velocity instead of the surface's
        (mw_ocean_set_draught).  Read per call; needs a column (set_column) by the time of the call, MW_ESTATE otherwise.  FFTMesh handles
        only; the fleet calls refuse a handle with draught on."""
        nat.check(nat.lib().mw_ocean_set_draught(self._h, 1 if on else 0))

    @property
    def draught(self) -> bool:
        on = C.c_int32(0)
        nat.check(nat.lib().mw_ocean_get_draught(self._h, C.byref(on)))
        return bool(on.value)

    # -- hull forces (mw_ocean_hull_forces) ----------------------------------------------------
    def _hull_coeffs(self, density, gravity, linear_drag, quadratic_drag, velocity_scale):
        if velocity_scale is None:  # per second of delta_time: FFTMesh velocities are per unit of t = delta_time / t_division
            velocity_scale = 1.0 / self.params.t_division if self.semantics == nat.MW_SEM_FFTMESH else 1.0
        return np.asarray([density, gravity, linear_drag, quadratic_drag, velocity_scale], np.float32)

    def hull_forces(self, hull_xyz, triangles, bodies, density=1000.0, gravity=9.81, linear_drag=0.0, quadratic_drag=0.0,
                    velocity_scale=None, frame: int = -1, iterations: int = 0):
        """Buoyancy and drag on nbodies instances of one hull -> [nbodies, 8] float32 rows (Fx, Fy, Fz, wetted_area, tx, ty, tz,
        residual), torque about each body's reference point.  hull_xyz [nverts, 3] and triangles [ntris, 3] in body space,
        (b - a) x (c - a) pointing out; bodies [nbodies, 16] (pack_bodies).  velocity_scale None: 1 / t_division (FFTMesh, per
        second of delta_time) or 1 (OceanRenderer).  With both drag coefficients 0 no velocity is computed.  With draught on
        (set_draught) every vertex reads the water column: its rest depth for the pressure, its velocity for the drag."""
        hull = np.ascontiguousarray(hull_xyz, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        bodies = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
        cf = self._hull_coeffs(density, gravity, linear_drag, quadratic_drag, velocity_scale)
        out = np.empty((bodies.shape[0], 8), np.float32)
        nat.check(nat.lib().mw_ocean_hull_forces(self._h, int(frame), _p(hull), hull.shape[0], _p(tris), tris.shape[0], _p(bodies),
                                                  bodies.shape[0], _p(cf), int(iterations), _p(out)))
        return out

    def hull_forces_device(self, d_hull_xyz: int, nverts: int, d_triangles: int, ntris: int, d_bodies: int, nbodies: int, d_out: int,
                           density=1000.0, gravity=9.81, linear_drag=0.0, quadratic_drag=0.0, velocity_scale=None, frame: int = -1,
                           iterations: int = 0):
        """Device-pointer form: d_hull_xyz [nverts][3] float32, d_triangles [ntris][3] int32, d_bodies [nbodies][16] and d_out
        [nbodies][8] float32 (16-byte aligned); asynchronous on the handle's stream.  Indices are not checked on the host: one
        outside [0, nverts) makes every row NaN."""
        cf = self._hull_coeffs(density, gravity, linear_drag, quadratic_drag, velocity_scale)
        nat.check(nat.lib().mw_ocean_hull_forces_device(self._h, int(frame), C.c_void_p(d_hull_xyz), int(nverts), C.c_void_p(d_triangles),
                                                         int(ntris), C.c_void_p(d_bodies), int(nbodies), _p(cf), int(iterations),
                                                         C.c_void_p(d_out)))


    # -- raycasts (mw_ocean_raycast) -----------------------------------------------------------
    @staticmethod
    def pack_rays(origins, directions, tmin=0.0, tmax=np.inf):
        """[n, 8] float32 rays (ox, oy, oz, tmin, dx, dy, dz, tmax) of mw_ocean_raycast; the four arguments broadcast against each
        other (one origin for many directions, one tmax for all, ...)."""
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        d = np.asarray(directions, np.float32).reshape(-1, 3)
        t0 = np.asarray(tmin, np.float32).reshape(-1)
        t1 = np.asarray(tmax, np.float32).reshape(-1)
        (n,) = np.broadcast_shapes(o.shape[:1], d.shape[:1], t0.shape, t1.shape)   # empty origins with scalar tmin / tmax: n = 0
        rays = np.empty((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, t0, d, t1
        return rays

    def raycast(self, origins, directions, tmin=0.0, tmax=np.inf, frame: int = -1):
        """First hit of the rays o + t d, tmin <= t <= tmax (t in units of d), on the surface query_surface reads ->
        (out [n, 8] float32 rows (t, px, py, pz, nx, ny, nz, white), hit [n, 2] int32 rows (triangle id, facing)).  A miss: t = +inf,
        NaN, (-1, 0); an invalid ray: NaN, (-1, 0).  facing +1: the ray met the water from above, -1: from below.  A segment p0 -> p1 is
        raycast(p0, p1 - p0, 0, 1).  frame -1 = the latest frame; k = frame k of the latest OceanRenderer steps call."""
        rays = self.pack_rays(origins, directions, tmin, tmax)
        out = np.empty((rays.shape[0], 8), np.float32)
        hit = np.empty((rays.shape[0], 2), np.int32)
        nat.check(nat.lib().mw_ocean_raycast(self._h, int(frame), _p(rays), rays.shape[0], _p(out), _p(hit)))
        return out, hit

    def raycast_device(self, d_rays: int, n: int, d_out: int, d_hit: int = 0, frame: int = -1):
        """Device-pointer form: d_rays [n][8] and d_out [n][8] float32 (16-byte aligned), d_hit [n][2] int32 (8-byte aligned; 0 = none);
        asynchronous on the handle's stream (synchronize() or the stream before reading d_out)."""
        nat.check(nat.lib().mw_ocean_raycast_device(self._h, int(frame), C.c_void_p(d_rays), int(n), C.c_void_p(d_out),
                                                     C.c_void_p(d_hit) if d_hit else None))

    # -- tiled raycasts (mw_ocean_raycast_tiled) -------------------------------------------------
    def raycast_tiled(self, origins, directions, tmin=0.0, tmax=np.inf, reach: int = nat.MW_RC_DEFAULT_REACH, frame: int = -1):
        """First hit of the rays on the infinite tiling of the FFTMesh frame (the surface of set_periodic, whatever the switch says),
        among the (2 reach + 1)^2 tiles around the tile of each ray's origin -> (out [n, 8] float32 rows (t, px, py, pz, nx, ny, nz,
        white), hit [n, 4] int32 rows (tiled triangle id = 2 (ai N + aj) + upper, facing, tile x, tile z)).  A miss: t = +inf, NaN,
        (-1, 0, 0, 0); out of reach (nothing hit and the ray left the window's reach inside [tmin, tmax] and the surface's height range):
        the same with id -2; an invalid ray: NaN, (-1, 0, 0, 0).  MW_ENOTCOMMENSURATE unless the grid repeats (period > 0)."""
        rays = self.pack_rays(origins, directions, tmin, tmax)
        out = np.empty((rays.shape[0], 8), np.float32)
        hit = np.empty((rays.shape[0], 4), np.int32)
        nat.check(nat.lib().mw_ocean_raycast_tiled(self._h, int(frame), _p(rays), rays.shape[0], int(reach), _p(out), _p(hit)))
        return out, hit

    def raycast_tiled_device(self, d_rays: int, n: int, d_out: int, d_hit: int = 0, reach: int = nat.MW_RC_DEFAULT_REACH, frame: int = -1):
        """Device-pointer form: d_rays [n][8] and d_out [n][8] float32, d_hit [n][4] int32 (0 = none), all 16-byte aligned; asynchronous
        on the handle's stream (synchronize() or the stream before reading d_out)."""
        nat.check(nat.lib().mw_ocean_raycast_tiled_device(self._h, int(frame), C.c_void_p(d_rays), int(n), int(reach), C.c_void_p(d_out),
                                                           C.c_void_p(d_hit) if d_hit else None))

    def raycast_tree(self, frame: int = -1, tiled: bool = False):
        """Test hook (mw_debug_raycast_tree): the hierarchy raycast() (tiled: raycast_tiled()) of this frame would traverse, built by
        the cast's own launches -> (box [nodes, 8] float32 rows (lo.x, lo.y, lo.z, 0, hi.x, hi.y, hi.z, 0), B, nb, D): leaf blocks of
        B cells, nb a side, at level D; level L is a 2^L x 2^L grid from node (4^L - 1) / 3, row-major.  A node no kernel wrote is
        NaN."""
        geom = np.zeros(3, np.int32)
        cap = (4 ** 10 - 1) // 3   # the deepest tree: leaf level MW_RC_MAX_LEVEL = 9 (csrc/raycast.h)
        box = np.empty((cap, 8), np.float32)
        nat.check(nat.lib().mw_debug_raycast_tree(self._h, int(frame), int(bool(tiled)), _p(box), cap, _p(geom)))
        nodes = (4 ** (int(geom[2]) + 1) - 1) // 3
        return box[:nodes].copy(), int(geom[0]), int(geom[1]), int(geom[2])

    @staticmethod
    def query_mesh(R: int, unit_width: float, vert, norm, white, xz, mode: str = "world", iterations: int = 0, vel=None, wstride: int = 1):
        """Test hook (mw_debug_query_mesh), no handle: query_surface's kernel on a caller's mesh -- vert and norm [R*R, 3], white [R*R]
        (stored with `wstride` floats per vertex, the whitecap in channel 0) -> out [n, 8]; with vel [R*R, 3] also query_velocity's
        kernel -> (out, vout [n, 4])."""
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))
        vert, norm, xz = f(vert, (-1, 3)), f(norm, (-1, 3)), f(xz, (-1, 2))
        wh = np.ascontiguousarray(np.repeat(f(white, (-1, 1)), int(wstride), 1))
        vel = None if vel is None else f(vel, (-1, 3))
        out = np.empty((xz.shape[0], 8), np.float32)
        vout = None if vel is None else np.empty((xz.shape[0], 4), np.float32)
        nat.check(nat.lib().mw_debug_query_mesh(int(R), float(unit_width), _p(vert), _p(norm), _p(wh), int(wstride), _p(vel),
                                                 Ocean._QUERY_MODES[mode], int(iterations), _p(xz), xz.shape[0], _p(out), _p(vout)))
        return out if vel is None else (out, vout)

    # -- floating bodies (mw_ocean_step_bodies) --------------------------------------------------
    def step_bodies(self, hull_xyz, triangles, bodies, mass, dt, substeps: int = 1, density=1000.0, gravity=9.81, linear_drag=0.0,
                    quadratic_drag=0.0, velocity_scale=None, frame: int = -1, iterations: int = 0, return_forces: bool = False):
        """Advance nbodies instances of one hull by dt in `substeps` semi-implicit Euler substeps under buoyancy, drag and gravity, on
        the frozen surface of `frame` -> bodies [nbodies, 16] float32 (p _ q v _ w _), and with return_forces the hull-forces rows
        [nbodies, 8] of the last substep (at the state at its start).  bodies is updated in place when it is a C-contiguous float32
        array (the same array is returned); mass [nbodies, 8] (pack_mass) about each body's centre of mass p, the hull about p too.
        The other arguments mean what they mean in hull_forces; gravity also pulls the bodies along -y.  With draught on (set_draught)
        every substep reads the water column, whose layers are built once per call."""
        hull = np.ascontiguousarray(hull_xyz, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
        m = np.ascontiguousarray(mass, np.float32).reshape(-1, nat.MW_BODY_NMASS)
        if m.shape[0] != b.shape[0]:
            raise ValueError(f"step_bodies: {b.shape[0]} bodies but {m.shape[0]} mass rows")
        cf = self._hull_coeffs(density, gravity, linear_drag, quadratic_drag, velocity_scale)
        out = np.empty((b.shape[0], 8), np.float32) if return_forces else None
        nat.check(nat.lib().mw_ocean_step_bodies(self._h, int(frame), _p(hull), hull.shape[0], _p(tris), tris.shape[0], _p(b), _p(m),
                                                  b.shape[0], _p(cf), float(dt), int(substeps), int(iterations),
                                                  _p(out)))
        return (b, out) if return_forces else b

    def step_bodies_device(self, d_hull_xyz: int, nverts: int, d_triangles: int, ntris: int, d_bodies: int, d_mass: int, nbodies: int,
                           dt, substeps: int = 1, d_out: int = 0, density=1000.0, gravity=9.81, linear_drag=0.0, quadratic_drag=0.0,
                           velocity_scale=None, frame: int = -1, iterations: int = 0):
        """Device-pointer form: d_bodies [nbodies][16] float32 updated in place, d_mass [nbodies][8], d_out [nbodies][8] or 0 (16-byte
        aligned); asynchronous on the handle's stream.  An invalid mass row gives that body a NaN row and leaves it unchanged."""
        cf = self._hull_coeffs(density, gravity, linear_drag, quadratic_drag, velocity_scale)
        nat.check(nat.lib().mw_ocean_step_bodies_device(self._h, int(frame), C.c_void_p(d_hull_xyz), int(nverts), C.c_void_p(d_triangles),
                                                         int(ntris), C.c_void_p(d_bodies), C.c_void_p(d_mass), int(nbodies), _p(cf),
                                                         float(dt), int(substeps), int(iterations), C.c_void_p(d_out or None)))

    # -- moorings (mw_ocean_step_moored) -----------------------------------------------------------
    def step_moored(self, hull_xyz, triangles, bodies, mass, lines, dt, substeps: int = 1, density=1000.0, gravity=9.81, linear_drag=0.0,
                    quadratic_drag=0.0, velocity_scale=None, frame: int = -1, iterations: int = 0, return_forces: bool = False,
                    return_tension: bool = False):
        """step_bodies with mooring lines -> bodies [nbodies, 16] (updated in place when it is a C-contiguous float32 array), then with
        return_forces the water rows [nbodies, 8] of the last substep and with return_tension the tensions [nbodies, K] at its start.
        lines [nbodies, K, 12] (pack_lines), K in [1, 8]: per slot the attachment point h (body space, about p), the unstretched length
        L0, the anchor a (world), the stiffness k and the damping c along the line; a slot with k == 0 and c == 0 is empty.  Every
        substep adds the taut lines' pull and torque to the water row before integrating (the returned rows stay the water's alone).
        Everything else as step_bodies; the integrator needs (dt / substeps) sqrt(k_total / m) < 2."""
        hull = np.ascontiguousarray(hull_xyz, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
        m = np.ascontiguousarray(mass, np.float32).reshape(-1, nat.MW_BODY_NMASS)
        ln = np.ascontiguousarray(lines, np.float32)
        if ln.ndim != 3 or ln.shape[2] != nat.MW_MOORING_NLINE:
            raise ValueError(f"step_moored: lines must be [nbodies, K, {nat.MW_MOORING_NLINE}], got {ln.shape}")
        if m.shape[0] != b.shape[0] or ln.shape[0] != b.shape[0]:
            raise ValueError(f"step_moored: {b.shape[0]} bodies but {m.shape[0]} mass rows and {ln.shape[0]} rows of lines")
        cf = self._hull_coeffs(density, gravity, linear_drag, quadratic_drag, velocity_scale)
        out = np.empty((b.shape[0], 8), np.float32) if return_forces else None
        ten = np.empty((b.shape[0], ln.shape[1]), np.float32) if return_tension else None
        nat.check(nat.lib().mw_ocean_step_moored(self._h, int(frame), _p(hull), hull.shape[0], _p(tris), tris.shape[0], _p(b), _p(m),
                                                  _p(ln), ln.shape[1], b.shape[0], _p(cf), float(dt), int(substeps), int(iterations),
                                                  _p(out), _p(ten)))
        res = (b,) + ((out,) if return_forces else ()) + ((ten,) if return_tension else ())
        return res if len(res) > 1 else b

    def step_moored_device(self, d_hull_xyz: int, nverts: int, d_triangles: int, ntris: int, d_bodies: int, d_mass: int, d_lines: int,
                           lines_per_body: int, nbodies: int, dt, substeps: int = 1, d_out: int = 0, d_tension: int = 0, density=1000.0,
                           gravity=9.81, linear_drag=0.0, quadratic_drag=0.0, velocity_scale=None, frame: int = -1, iterations: int = 0):
        """Device-pointer form: d_bodies [nbodies][16] updated in place, d_mass [nbodies][8], d_lines [nbodies][lines_per_body][12],
        d_out [nbodies][8] or 0 (16-byte aligned), d_tension [nbodies][lines_per_body] or 0; asynchronous on the handle's stream.  An
        invalid mass row or slot gives that body a NaN row and NaN tensions and leaves it unchanged; so does a NaN water row."""
        cf = self._hull_coeffs(density, gravity, linear_drag, quadratic_drag, velocity_scale)
        nat.check(nat.lib().mw_ocean_step_moored_device(self._h, int(frame), C.c_void_p(d_hull_xyz), int(nverts), C.c_void_p(d_triangles),
                                                         int(ntris), C.c_void_p(d_bodies), C.c_void_p(d_mass), C.c_void_p(d_lines),
                                                         int(lines_per_body), int(nbodies), _p(cf), float(dt), int(substeps),
                                                         int(iterations), C.c_void_p(d_out or None), C.c_void_p(d_tension or None)))

    # -- mixed fleets (mw_ocean_fleet_forces, mw_ocean_step_fleet) --------------------------------
    def _fleet_coeffs(self, nhulls, coeffs):
        """[nhulls, 5] float32 rows (density, gravity, linear_drag, quadratic_drag, velocity_scale): None = water at rest drag (1000,
        9.81, 0, 0, the default velocity scale) for every hull; one row is broadcast; a NaN velocity_scale means the default."""
        default = self._hull_coeffs(1000.0, 9.81, 0.0, 0.0, None)
        if coeffs is None:
            return np.ascontiguousarray(np.broadcast_to(default, (nhulls, nat.MW_HULL_NCOEFFS)))
        cf = np.asarray(coeffs, np.float32)
        cf = np.array(np.broadcast_to(cf.reshape(-1, nat.MW_HULL_NCOEFFS), (nhulls, nat.MW_HULL_NCOEFFS)), np.float32, order="C")  # rows, hull by hull
        cf[:, 4] = np.where(np.isnan(cf[:, 4]), default[4], cf[:, 4])
        return cf

    @staticmethod
    def _fleet_arrays(hull_xyz, triangles, hulls):
        hull = np.ascontiguousarray(hull_xyz, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        table = np.ascontiguousarray(hulls, np.int32).reshape(-1, nat.MW_FLEET_NHULL)
        return hull, tris, table

    def fleet_forces(self, hull_xyz, triangles, hulls, bodies, coeffs=None, frame: int = -1, iterations: int = 0):
        """hull_forces for a mixed fleet in one call -> [total_bodies, 8] float32 rows.  hull_xyz, triangles and hulls as pack_fleet
        makes them (every hull's geometry concatenated, indices local to their hull, hulls [nhulls, 5] = vert_first, nverts, tri_first,
        ntris, nbodies); bodies [total_bodies, 16] hull after hull in table order; coeffs [nhulls, 5] rows of (density, gravity,
        linear_drag, quadratic_drag, velocity_scale), one row for all, or None.  A body's row has the bits hull_forces gives on its hull
        alone; the velocity field is computed once, and only when some hull has drag."""
        hull, tris, table = self._fleet_arrays(hull_xyz, triangles, hulls)
        b = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
        cf = self._fleet_coeffs(table.shape[0], coeffs)
        out = np.empty((b.shape[0], 8), np.float32)
        nat.check(nat.lib().mw_ocean_fleet_forces(self._h, int(frame), _p(hull), hull.shape[0], _p(tris), tris.shape[0], _p(table),
                                                   table.shape[0], _p(b), b.shape[0], _p(cf), int(iterations), _p(out)))
        return out

    def fleet_forces_device(self, d_hull_xyz: int, total_verts: int, d_triangles: int, total_tris: int, hulls, d_bodies: int,
                            total_bodies: int, d_out: int, coeffs=None, frame: int = -1, iterations: int = 0):
        """Device-pointer form: the geometry, d_bodies [total_bodies][16] and d_out [total_bodies][8] on the device (16-byte aligned), hulls
        and coeffs host arrays; asynchronous on the handle's stream.  A triangle index outside its hull's [0, nverts) makes the rows of
        that hull's bodies NaN."""
        table = np.ascontiguousarray(hulls, np.int32).reshape(-1, nat.MW_FLEET_NHULL)
        cf = self._fleet_coeffs(table.shape[0], coeffs)
        nat.check(nat.lib().mw_ocean_fleet_forces_device(self._h, int(frame), C.c_void_p(d_hull_xyz), int(total_verts),
                                                          C.c_void_p(d_triangles), int(total_tris), _p(table), table.shape[0],
                                                          C.c_void_p(d_bodies), int(total_bodies), _p(cf), int(iterations),
                                                          C.c_void_p(d_out)))

    def step_fleet(self, hull_xyz, triangles, hulls, bodies, mass, dt, substeps: int = 1, wrench=None, coeffs=None, frame: int = -1,
                   iterations: int = 0, return_forces: bool = False):
        """step_bodies for a mixed fleet in one call -> bodies [total_bodies, 16] (updated in place when it is a C-contiguous float32
        array), and with return_forces the water rows [total_bodies, 8] of the last substep.  wrench [total_bodies, 8] = (Fx, Fy, Fz, _,
        tx, ty, tz, _) or None: an external force and torque about p in world axes, constant over the call, added to the water row of
        every substep (the returned rows stay the water's alone).  Everything else as fleet_forces and step_bodies; a body's state has
        the bits step_bodies gives on its hull alone."""
        hull, tris, table = self._fleet_arrays(hull_xyz, triangles, hulls)
        b = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
        m = np.ascontiguousarray(mass, np.float32).reshape(-1, nat.MW_BODY_NMASS)
        w = None if wrench is None else np.ascontiguousarray(wrench, np.float32).reshape(-1, 8)
        if m.shape[0] != b.shape[0] or (w is not None and w.shape[0] != b.shape[0]):
            raise ValueError(f"step_fleet: {b.shape[0]} bodies but {m.shape[0]} mass rows"
                             + ("" if w is None else f" and {w.shape[0]} wrench rows"))
        cf = self._fleet_coeffs(table.shape[0], coeffs)
        out = np.empty((b.shape[0], 8), np.float32) if return_forces else None
        nat.check(nat.lib().mw_ocean_step_fleet(self._h, int(frame), _p(hull), hull.shape[0], _p(tris), tris.shape[0], _p(table),
                                                 table.shape[0], _p(b), _p(m), _p(w), b.shape[0], _p(cf), float(dt), int(substeps),
                                                 int(iterations), _p(out)))
        return (b, out) if return_forces else b

    def step_fleet_device(self, d_hull_xyz: int, total_verts: int, d_triangles: int, total_tris: int, hulls, d_bodies: int, d_mass: int,
                          total_bodies: int, dt, substeps: int = 1, d_wrench: int = 0, d_out: int = 0, coeffs=None, frame: int = -1,
                          iterations: int = 0):
        """Device-pointer form: d_bodies [total_bodies][16] updated in place, d_mass, d_wrench (0 = none) and d_out (0 = none)
        [total_bodies][8], 16-byte aligned; hulls and coeffs host arrays; asynchronous on the handle's stream.  An invalid mass row or a
        non-finite wrench row gives that body a NaN row and leaves it unchanged."""
        table = np.ascontiguousarray(hulls, np.int32).reshape(-1, nat.MW_FLEET_NHULL)
        cf = self._fleet_coeffs(table.shape[0], coeffs)
        nat.check(nat.lib().mw_ocean_step_fleet_device(self._h, int(frame), C.c_void_p(d_hull_xyz), int(total_verts),
                                                        C.c_void_p(d_triangles), int(total_tris), _p(table), table.shape[0],
                                                        C.c_void_p(d_bodies), C.c_void_p(d_mass), C.c_void_p(d_wrench or None),
                                                        int(total_bodies), _p(cf), float(dt), int(substeps), int(iterations),
                                                        C.c_void_p(d_out or None)))

    # -- rigged fleets (mw_ocean_step_rigged) ------------------------------------------------------
    def step_rigged(self, hull_xyz, triangles, hulls, bodies, mass, lines, dt, substeps: int = 1, targets=None, wrench=None, coeffs=None,
                    frame: int = -1, iterations: int = 0, return_forces: bool = False, return_tension: bool = False):
        """step_fleet with lines on every body -> bodies [total_bodies, 16] (updated in place when it is a C-contiguous float32 array),
        then with return_forces the water rows [total_bodies, 8] of the last substep and with return_tension the tensions
        [total_bodies, K] at its start.  lines [total_bodies, K, 12] as step_moored's (pack_lines); targets [total_bodies, K] int32 or
        None (every slot anchored): MW_RIG_ANCHOR (-1) makes a slot's a a fixed world point, j >= 0 an attachment point in the body space
        of body j (a tow line).  Every slot is evaluated at the state all bodies had at the start of the substep.  A line between two
        bodies is written in both tables (h and a exchanged, the same L0, k, c): its two ends then pull with opposite bits; a one-sided
        slot pulls its owner alone.  Everything else as step_fleet and step_moored."""
        hull, tris, table = self._fleet_arrays(hull_xyz, triangles, hulls)
        b = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
        m = np.ascontiguousarray(mass, np.float32).reshape(-1, nat.MW_BODY_NMASS)
        w = None if wrench is None else np.ascontiguousarray(wrench, np.float32).reshape(-1, 8)
        ln = np.ascontiguousarray(lines, np.float32)
        if ln.ndim != 3 or ln.shape[2] != nat.MW_MOORING_NLINE:
            raise ValueError(f"step_rigged: lines must be [total_bodies, K, {nat.MW_MOORING_NLINE}], got {ln.shape}")
        tg = None if targets is None else np.ascontiguousarray(targets, np.int32)
        if m.shape[0] != b.shape[0] or ln.shape[0] != b.shape[0] or (w is not None and w.shape[0] != b.shape[0]):
            raise ValueError(f"step_rigged: {b.shape[0]} bodies but {m.shape[0]} mass rows and {ln.shape[0]} rows of lines"
                             + ("" if w is None else f" and {w.shape[0]} wrench rows"))
        if tg is not None and tg.shape != ln.shape[:2]:
            raise ValueError(f"step_rigged: targets must be {ln.shape[:2]}, got {tg.shape}")
        cf = self._fleet_coeffs(table.shape[0], coeffs)
        out = np.empty((b.shape[0], 8), np.float32) if return_forces else None
        ten = np.empty((b.shape[0], ln.shape[1]), np.float32) if return_tension else None
        nat.check(nat.lib().mw_ocean_step_rigged(self._h, int(frame), _p(hull), hull.shape[0], _p(tris), tris.shape[0], _p(table),
                                                  table.shape[0], _p(b), _p(m), _p(w), _p(ln), _p(tg), ln.shape[1], b.shape[0], _p(cf),
                                                  float(dt), int(substeps), int(iterations), _p(out), _p(ten)))
        res = (b,) + ((out,) if return_forces else ()) + ((ten,) if return_tension else ())
        return res if len(res) > 1 else b

    def step_rigged_device(self, d_hull_xyz: int, total_verts: int, d_triangles: int, total_tris: int, hulls, d_bodies: int, d_mass: int,
                           d_lines: int, lines_per_body: int, total_bodies: int, dt, substeps: int = 1, d_targets: int = 0,
                           d_wrench: int = 0, d_out: int = 0, d_tension: int = 0, coeffs=None, frame: int = -1, iterations: int = 0):
        """Device-pointer form: d_bodies [total_bodies][16] updated in place, d_mass, d_wrench (0 = none) and d_out (0 = none)
        [total_bodies][8], d_lines [total_bodies][lines_per_body][12], all 16-byte aligned; d_targets (0 = all anchored, int32) and
        d_tension (0 = none) [total_bodies][lines_per_body]; hulls and coeffs host arrays; asynchronous on the handle's stream.  An
        invalid mass, wrench or slot, a target out of range or the body itself gives that body a NaN row and NaN tensions and leaves it
        unchanged; so does a tow line to a body whose state is not finite."""
        table = np.ascontiguousarray(hulls, np.int32).reshape(-1, nat.MW_FLEET_NHULL)
        cf = self._fleet_coeffs(table.shape[0], coeffs)
        nat.check(nat.lib().mw_ocean_step_rigged_device(self._h, int(frame), C.c_void_p(d_hull_xyz), int(total_verts),
                                                         C.c_void_p(d_triangles), int(total_tris), _p(table), table.shape[0],
                                                         C.c_void_p(d_bodies), C.c_void_p(d_mass), C.c_void_p(d_wrench or None),
                                                         C.c_void_p(d_lines or None), C.c_void_p(d_targets or None), int(lines_per_body),
                                                         int(total_bodies), _p(cf), float(dt), int(substeps), int(iterations),
                                                         C.c_void_p(d_out or None), C.c_void_p(d_tension or None)))


def pack_fleet(hulls):
    """(hull_xyz [total_verts, 3] float32, triangles [total_tris, 3] int32, table [nhulls, 5] int32) of Ocean.fleet_forces / step_fleet
    from (hull_xyz, triangles, nbodies) triples: the geometry concatenated in order, triangle indices left local to their hull, table
    rows (vert_first, nverts, tri_first, ntris, nbodies)."""
    xs, ts, rows = [], [], []
    v0 = t0 = 0
    for hull_xyz, triangles, nbodies in hulls:
        x = np.asarray(hull_xyz, np.float32).reshape(-1, 3)
        t = np.asarray(triangles, np.int32).reshape(-1, 3)
        xs.append(x); ts.append(t)
        rows.append((v0, x.shape[0], t0, t.shape[0], int(nbodies)))
        v0 += x.shape[0]; t0 += t.shape[0]
    if not rows:
        raise ValueError("pack_fleet: no hulls")
    return (np.ascontiguousarray(np.concatenate(xs)), np.ascontiguousarray(np.concatenate(ts)),
            np.asarray(rows, np.int32).reshape(-1, nat.MW_FLEET_NHULL))


def hull_mass_properties(hull_xyz, triangles, density=1000.0):
    """(mass, centroid [3], inertia [3, 3]) of the closed hull (outward winding) of uniform density: the inertia tensor about the
    centroid in hull axes (off-diagonal entries -int x y dm), from mw_hull_mass_properties (f64 sums; no device needed)."""
    hull = np.ascontiguousarray(hull_xyz, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    out = np.empty(10, np.float32)
    nat.check(nat.lib().mw_hull_mass_properties(_p(hull), hull.shape[0], _p(tris), tris.shape[0], float(density), _p(out)))
    xx, yy, zz, xy, xz, yz = (float(v) for v in out[4:10])
    return float(out[0]), out[1:4].copy(), np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], np.float32)


def pack_mass(mass, inertia):
    """mass rows [n, 8] float32 (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz, 0) for Ocean.step_bodies from mass [n] (or a scalar) and inertia
    tensors [n, 3, 3] (or one [3, 3]) about the centre of mass in body axes; n is broadcast."""
    m = np.atleast_1d(np.asarray(mass, np.float32))
    I = np.asarray(inertia, np.float32).reshape(-1, 3, 3)
    n = max(len(m), len(I))
    m, I = np.broadcast_to(m, (n,)), np.broadcast_to(I, (n, 3, 3))
    out = np.zeros((n, 8), np.float32)
    out[:, 0] = m
    out[:, 1], out[:, 2], out[:, 3] = I[:, 0, 0], I[:, 1, 1], I[:, 2, 2]
    out[:, 4], out[:, 5], out[:, 6] = I[:, 0, 1], I[:, 0, 2], I[:, 1, 2]
    return out


def pack_lines(nbodies, lines_per_body, attach=None, anchor=None, rest_length=0.0, stiffness=0.0, damping=0.0):
    """lines [nbodies, lines_per_body, 12] float32 for Ocean.step_moored: per slot (hx, hy, hz, L0, ax, ay, az, k, c, 0, 0, 0).  Called
    with the two counts alone it gives empty slots to fill in (out[b, s, 0:3] = h, [3] = L0, [4:7] = a, [7] = k, [8] = c); attach and
    anchor [nbodies, lines_per_body, 3] and rest_length, stiffness, damping [nbodies, lines_per_body] (or scalars) are broadcast."""
    n, K = int(nbodies), int(lines_per_body)
    if not 1 <= K <= nat.MW_MOORING_MAX_LINES:
        raise ValueError(f"pack_lines: lines_per_body must be in [1, {nat.MW_MOORING_MAX_LINES}]")
    out = np.zeros((n, K, nat.MW_MOORING_NLINE), np.float32)
    if attach is not None:
        out[:, :, 0:3] = np.broadcast_to(np.asarray(attach, np.float32), (n, K, 3))
    if anchor is not None:
        out[:, :, 4:7] = np.broadcast_to(np.asarray(anchor, np.float32), (n, K, 3))
    out[:, :, 3] = np.broadcast_to(np.asarray(rest_length, np.float32), (n, K))
    out[:, :, 7] = np.broadcast_to(np.asarray(stiffness, np.float32), (n, K))
    out[:, :, 8] = np.broadcast_to(np.asarray(damping, np.float32), (n, K))
    return out


def pack_bodies(position, rotation=None, velocity=None, angular_velocity=None):
    """bodies [n, 16] float32 for Ocean.hull_forces from position [n, 3], rotation quaternions [n, 4] (x, y, z, w; default identity),
    velocity [n, 3] and angular_velocity [n, 3] (default 0), all in the ocean's object space."""
    pos = np.asarray(position, np.float32).reshape(-1, 3)
    n = pos.shape[0]
    out = np.zeros((n, 16), np.float32)
    out[:, 0:3] = pos
    out[:, 7] = 1.0
    if rotation is not None:
        out[:, 4:8] = np.asarray(rotation, np.float32).reshape(n, 4)
    if velocity is not None:
        out[:, 8:11] = np.asarray(velocity, np.float32).reshape(n, 3)
    if angular_velocity is not None:
        out[:, 12:15] = np.asarray(angular_velocity, np.float32).reshape(n, 3)
    return out


class _Mesh:
    """The handful of UnityEngine.Mesh members the reference assigns (S/FFTMesh.cs:134-138,277-279)."""
    vertices = normals = colors = uv = indices = None


class FFTMesh:
    """Mirror of ``public class FFTMesh : MonoBehaviour`` (S/FFTMesh.cs): same public fields
    (:9-23), same Awake()/Update() lifecycle (:60-84); the private numerical methods are the GPU."""

    def __init__(self, device: int = 0, seed: int = 1):
        self.choppiness = 1.0          # :9
        self.tDivision = 1.0           # :11
        self.resolution = 50           # :13
        self.unitWidth = 1.0           # :15
        self.generate = False          # :17
        self.length = 1.0              # :19
        self.wind = Vector2(1.0, 1.0)  # :21
        self.amplitude = 1.0           # :23
        self.gravity = 9.81            # G, :52
        self.mesh = _Mesh()
        self._device, self._seed = device, seed
        self.fixedSeed = False         # True: every regeneration reproduces the same sea (tests); the reference draws anew
        self._generation = 0
        self._ocean = None
        self._timer = 0.0

    # SetParams + GenerateMesh (:90-139).  GenerateMesh draws fresh UnityEngine.Random values every time it runs
    # (:114-116), so each regeneration is a NEW sea state: the seed advances with a generation counter.
    def _regenerate(self):
        if self._ocean is not None:
            self._ocean.close()
        seed = self._seed if self.fixedSeed else self._seed + self._generation
        self._generation += 1
        self._ocean = Ocean(resolution=self.resolution, unit_width=self.unitWidth, length=self.length,
                            wind=(self.wind.x, self.wind.y), amplitude=self.amplitude, choppiness=self.choppiness,
                            gravity=self.gravity, t_division=self.tDivision, seed=seed, device=self._device)
        v, n, uv, idx = self._ocean.rest_mesh()
        self.mesh.vertices, self.mesh.normals, self.mesh.uv, self.mesh.indices = v, n, uv, idx

    def Awake(self):  # :75-84
        self._regenerate()

    def Update(self, deltaTime: float):  # :60-73
        if self.generate:
            self._timer = 0.0
            self._regenerate()
            self.generate = False
        self._timer = float(np.float32(self._timer) + np.float32(deltaTime) / np.float32(self.tDivision))  # :70
        self.EvaluateWaves(self._timer)

    def EvaluateWaves(self, t: float):  # :224-280
        self._ocean.set_choppiness(self.choppiness)  # :244-245 read the live field
        v, n, c = self._ocean.evaluate(t)
        self.mesh.vertices, self.mesh.normals, self.mesh.colors = v, n, c  # :277-279

    def SampleSurface(self, xz, world: bool = True, iterations: int = 0):
        """Not in the reference: the mesh's surface at horizontal points xz [n, 2] of the latest EvaluateWaves (Ocean.query_surface)."""
        return self._ocean.query_surface(xz, mode="world" if world else "rest", iterations=iterations)

    def SampleColumn(self, xyz, world: bool = True):
        """Not in the reference: the water below the surface at points xyz [n, 3] of the latest EvaluateWaves (Ocean.query_column; set
        the layers with ocean.set_column first)."""
        return self._ocean.query_column(xyz, mode="world" if world else "rest")

    @property
    def timer(self):
        return self._timer

    @property
    def ocean(self) -> Ocean:
        return self._ocean


class OceanRenderer:
    """Mirror of ``public class OceanRenderer : MonoBehaviour`` (S/OceanRenderer.cs:10-19, :76-110)."""

    def __init__(self, device: int = 0, seed: int = 1):
        self.mult = 2.0            # :11
        self.unitWidth = 1.0       # :12
        self.resolution = 256      # :13
        self.length = 256.0        # :14
        self.choppiness = 1.5      # :16
        self.amplitude = 1.0       # :18
        self.wind = Vector2()      # :19
        self.gravity = 9.81
        self.mesh = _Mesh()
        self.heightTexture = self.displacementTexture = self.normalTexture = self.whiteTexture = None
        self._device, self._seed = device, seed
        self._ocean = None
        self._old = None

    def _key(self):
        return (self.length, self.wind.x, self.wind.y, self.amplitude)

    def _create(self):
        if self._ocean is not None:
            self._ocean.close()
        self._ocean = Ocean(resolution=self.resolution, unit_width=self.unitWidth, length=self.length,
                            wind=(self.wind.x, self.wind.y), amplitude=self.amplitude, choppiness=self.choppiness,
                            gravity=self.gravity, mult=self.mult, seed=self._seed,
                            semantics=nat.MW_SEM_OCEANRENDERER, device=self._device)
        self._old = self._key()

    def Awake(self):  # :76-89  SetParams, GenerateMesh, RenderInitial
        self._create()
        v, n, uv, idx = self._ocean.rest_mesh()
        self.mesh.vertices, self.mesh.normals, self.mesh.uv, self.mesh.indices = v, n, uv, idx

    def Update(self, deltaTime: float):  # :91-110
        self.GenerateTexture(deltaTime)                   # with the values the materials carried into this frame (:93)
        self._ocean.set_choppiness(self.choppiness)       # spectrumMat._Choppiness for the NEXT frame (:96)
        if self._old != self._key():  # :98-109 RenderInitial again with the same seeds; the phase textures keep running
            self._ocean.reinit_spectrum(length=self.length, wind=(self.wind.x, self.wind.y), amplitude=self.amplitude)
            self._old = self._key()

    def GenerateTexture(self, deltaTime: float):  # :216-316
        h, d, n, w = self._ocean.generate_texture(deltaTime)
        self.heightTexture, self.displacementTexture, self.normalTexture, self.whiteTexture = h, d, n, w

    def GenerateTextures(self, deltaTimes):
        """Not in the reference: len(deltaTimes) consecutive GenerateTexture() calls in one enqueue (bit-identical to the per-frame calls);
        returns the frames [n, M, M(, c)] and leaves the LAST one in the component's textures, as n calls of Update would."""
        H, D, Nn, W = self._ocean.generate_texture_steps(deltaTimes)
        self.heightTexture, self.displacementTexture, self.normalTexture, self.whiteTexture = H[-1], D[-1], Nn[-1], W[-1]
        return H, D, Nn, W

    def SampleSurface(self, xz, world: bool = True, frame: int = -1, iterations: int = 0):
        """Not in the reference: the displaced mesh's surface at horizontal points xz [n, 2] (Ocean.query_surface); frame -1 = what
        the latest GenerateTexture() shows, k = frame k of the latest GenerateTextures()."""
        return self._ocean.query_surface(xz, mode="world" if world else "rest", frame=frame, iterations=iterations)

    @property
    def ocean(self) -> Ocean:
        return self._ocean


class Tiles:
    """Independent tiles (seed = seed0 + k) on several devices with an RCCL gather of finished outputs
    (include/mistral_water.h, mw_tiles_*).  ``devices`` lists one device ordinal per tile (single-process form); pass
    ``comm_id``/``rank``/``nranks`` instead for the one-process-per-GPU form.  FFTMesh semantics (default): ``evaluate`` /
    ``outputs``; OceanRenderer semantics (``max_steps`` 1, the tile axis is the only one that shards there):
    ``generate_texture`` / ``textures``."""

    def __init__(self, *, resolution, ntiles=1, devices=None, max_steps=1, unit_width=1.0, length=1.0, wind=(1.0, 1.0), amplitude=1.0,
                 choppiness=1.0, gravity=9.81, seed=1, comm_id=None, rank=0, nranks=1, device=0, semantics=nat.MW_SEM_FFTMESH,
                 mult=1.0):
        self._h = C.c_void_p()
        self.params = nat.MwParams(int(resolution), float(unit_width), float(length), float(wind[0]), float(wind[1]),
                                   float(amplitude), float(choppiness), float(gravity), 1.0, float(mult), int(seed), int(semantics), 0)
        if comm_id is None:
            dv = None if devices is None else (C.c_int32 * ntiles)(*[int(d) for d in devices])
            nat.check(nat.lib().mw_tiles_create(C.byref(self.params), int(ntiles), dv, int(max_steps), C.byref(self._h)))
        else:
            buf = (C.c_ubyte * nat.MW_COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
            nat.check(nat.lib().mw_tiles_create_rank(C.byref(self.params), int(device), int(max_steps), buf, int(rank), int(nranks),
                                                     C.byref(self._h)))
        self.N = int(resolution) * (8 if semantics == nat.MW_SEM_OCEANRENDERER else 1)   # synthesis grid (S/OceanRenderer.cs:136)
        self.max_steps = int(max_steps)

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * nat.MW_COMM_ID_BYTES)()
        nat.check(nat.lib().mw_comm_unique_id(buf))
        return bytes(buf)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            nat.lib().mw_tiles_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def count(self):
        return nat.lib().mw_tiles_count(self._h)

    @property
    def local_count(self):
        return nat.lib().mw_tiles_local_count(self._h)

    def set_spectrum(self, k, h0, h0conj):
        o = nat.lib().mw_tiles_ocean(self._h, int(k))
        h0 = np.ascontiguousarray(h0, np.float32)
        h0conj = np.ascontiguousarray(h0conj, np.float32)
        nat.check(nat.lib().mw_ocean_set_spectrum(C.c_void_p(o), _p(h0), _p(h0conj)))

    def get_spectrum(self, k):
        o = nat.lib().mw_tiles_ocean(self._h, int(k))
        h0 = np.empty((self.N, self.N, 2), np.float32)
        h0c = np.empty((self.N, self.N, 2), np.float32)
        nat.check(nat.lib().mw_ocean_get_spectrum(C.c_void_p(o), _p(h0), _p(h0c)))
        return h0, h0c

    def evaluate(self, times, rgba: bool = False):
        tt = np.ascontiguousarray(times, np.float32)
        nat.check(nat.lib().mw_tiles_evaluate(self._h, _p(tt), tt.size, nat.MW_OUT_COLOR_RGBA if rgba else nat.MW_OUT_WHITE_SCALAR))

    def outputs(self, k):
        """Device pointers (ints) of local tile k: vertices, normals, white."""
        v, n, w = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nat.check(nat.lib().mw_tiles_outputs(self._h, int(k), C.byref(v), C.byref(n), C.byref(w)))
        return v.value, n.value, w.value

    def generate_texture(self, delta_time: float):
        """OceanRenderer tiles: one GenerateTexture() on every local tile (asynchronous)."""
        nat.check(nat.lib().mw_tiles_generate_texture(self._h, C.c_float(delta_time)))

    def textures(self, k):
        """OceanRenderer tiles: device pointers (ints) of local tile k's height, disp_xz, normal_xyz, white textures."""
        h, d, n, w = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nat.check(nat.lib().mw_tiles_textures(self._h, int(k), C.byref(h), C.byref(d), C.byref(n), C.byref(w)))
        return h.value, d.value, n.value, w.value

    def generate_texture_steps(self, delta_times):
        """OceanRenderer tiles (max_steps > 1): len(delta_times) consecutive GenerateTexture() calls on every local tile, one enqueue each."""
        dts = np.ascontiguousarray(delta_times, np.float32)
        nat.check(nat.lib().mw_tiles_generate_texture_steps(self._h, _p(dts), int(dts.size)))

    def frames(self, k):
        """OceanRenderer tiles (max_steps > 1): device pointers of local tile k's [max_steps] frames: height, disp_xz, normal_xyz, white."""
        h, d, n, w = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nat.check(nat.lib().mw_tiles_frames(self._h, int(k), C.byref(h), C.byref(d), C.byref(n), C.byref(w)))
        return h.value, d.value, n.value, w.value

    def gather(self, step: int = 0, root: int = 0):
        nat.check(nat.lib().mw_tiles_gather(self._h, int(step), int(root)))

    def gathered(self):
        """(device pointer of the root buffer or None, floats per tile)."""
        ptr, fpt = C.c_void_p(), C.c_int64()
        nat.check(nat.lib().mw_tiles_gathered(self._h, C.byref(ptr), C.byref(fpt)))
        return ptr.value, fpt.value

    def synchronize(self):
        nat.check(nat.lib().mw_tiles_synchronize(self._h))


def host_register(array):
    """Page-lock a numpy array for the lifetime of its use as an output buffer (mw_host_register)."""
    nat.check(nat.lib().mw_host_register(_p(array), array.nbytes))


def host_unregister(array):
    nat.check(nat.lib().mw_host_unregister(_p(array)))


def gerstner_displace(pos_xyz, waves, amplitude: float, frequency: float, steepness: float, t: float, device: int = 0):
    """W/MistralWaterLib.cginc:154-180 Displacement() in Gerstner mode on host arrays.
    ``waves`` = [(dir.x, dir.y, speed), ...]; ``amplitude`` is the already x0.01-scaled value (:172)."""
    pos = np.ascontiguousarray(pos_xyz, np.float32)
    wv = np.ascontiguousarray(waves, np.float32).reshape(-1, 3)
    out = np.empty_like(pos)
    nat.check(nat.lib().mw_gerstner_displace(_p(pos), pos.size // 3, _p(wv), wv.shape[0], C.c_float(amplitude),
                                             C.c_float(frequency), C.c_float(steepness), C.c_float(t), _p(out), device))
    return out


def gerstner_displace_steps_device(d_pos: int, nverts: int, waves, amplitude: float, frequency: float, steepness: float,
                                   times, d_out: int, stream: int = 0):
    """len(times) displaced copies of one device-resident lattice in one launch: d_out is [len(times)][nverts*3]."""
    wv = np.ascontiguousarray(waves, np.float32).reshape(-1, 3)
    tt = np.ascontiguousarray(times, np.float32)
    nat.check(nat.lib().mw_gerstner_displace_steps_device(C.c_void_p(d_pos), nverts, _p(wv), wv.shape[0], C.c_float(amplitude),
                                                          C.c_float(frequency), C.c_float(steepness), _p(tt), tt.size,
                                                          C.c_void_p(d_out), C.c_void_p(stream) if stream else None))


class PondMaterial:
    """Displacement properties of the pond material (W/MistralWaterProperty.cginc, W/MistralWaterLib.cginc:53-66), under
    the material's own property names, and its vertex-stage ``Displacement()`` (:154-180) on host or device arrays.

    ``mode``: ``MW_POND_WAVE`` (Wave, :127-152), ``MW_POND_GERSTNER`` (Gerstner, :71-99) or
    ``MW_POND_GERSTNER_LEVEL_ONE`` (GerstnerLevelOne, :101-125)."""

    def __init__(self, mode=nat.MW_POND_GERSTNER, _Amplitude=10.0, _Frequency=2.58, _Speed=1.0, _Steepness=0.99,
                 _Smoothing=1.0, _WSpeed=(0, 0, 0, 0), _WDirectionAB=(0, 0, 0, 0), _WDirectionCD=(0, 0, 0, 0)):
        self.mode = mode
        self._Amplitude, self._Frequency, self._Speed = _Amplitude, _Frequency, _Speed
        self._Steepness, self._Smoothing = _Steepness, _Smoothing
        self._WSpeed, self._WDirectionAB, self._WDirectionCD = tuple(_WSpeed), tuple(_WDirectionAB), tuple(_WDirectionCD)

    def _c(self):
        p = nat.MwPondParams()
        p.mode, p.amplitude, p.frequency, p.speed = self.mode, self._Amplitude, self._Frequency, self._Speed
        p.steepness, p.smoothing = self._Steepness, self._Smoothing
        p.wspeed[:], p.dir_ab[:], p.dir_cd[:] = list(self._WSpeed), list(self._WDirectionAB), list(self._WDirectionCD)
        return p

    def displace(self, pos_xyz, t: float, normals: bool = True, device: int = 0):
        """-> (displaced vertices, normals or None) for host vertices [n,3] at _Time.y = t."""
        pos = np.ascontiguousarray(pos_xyz, np.float32)
        out = np.empty_like(pos)
        nrm = np.empty_like(pos) if normals else None
        p = self._c()
        nat.check(nat.lib().mw_pond_displace(C.byref(p), _p(pos), pos.size // 3, C.c_float(t), _p(out),
                                             _p(nrm) if normals else None, device))
        return out, nrm

    def displace_device(self, d_pos: int, nverts: int, t: float, d_out: int, d_normals: int = 0, stream: int = 0):
        """Device pointers (ints), asynchronous on ``stream`` (a hipStream_t as int, 0 = default stream)."""
        p = self._c()
        nat.check(nat.lib().mw_pond_displace_device(C.byref(p), C.c_void_p(d_pos), nverts, C.c_float(t), C.c_void_p(d_out),
                                                    C.c_void_p(d_normals) if d_normals else None,
                                                    C.c_void_p(stream) if stream else None))
