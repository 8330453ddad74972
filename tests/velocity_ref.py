"""References of the surface velocity (mw_ocean_velocity, include/mistral_water.h) built from the oracle: the time derivative of every
frame output is the frame pipeline run on the weighted spectrum (i w h0, -i w h0c) (csrc/velocity_kernels.h), so the f64 oracle fed
that spectrum, minus the rest mesh, is the velocity -- checked against central differences of the oracle itself in
tests/test_velocity_cpu.py."""
import numpy as np

from oracle import oracle as O


def weight(h0, h0c, w):
    """(h0, h0c) [..., 2] float32 -> (i w h0, -i w h0c) in float64 (w broadcast over the leading axes)."""
    h0 = np.asarray(h0, np.float64)
    h0c = np.asarray(h0c, np.float64)
    w = np.asarray(w, np.float64)
    a = np.stack([-w * h0[..., 1], w * h0[..., 0]], -1)
    b = np.stack([w * h0c[..., 1], -w * h0c[..., 0]], -1)
    return a, b


def fftmesh_omega(p):
    """omega(i, j) [N, N] in the library's strict float32 sequence (S/FFTMesh.cs:141-147): the oracle's dispersion at t = 1."""
    return O.dispersion_grid(p, 1.0).astype(np.float64)


def fftmesh_velocity_f64(p, h0, h0c, t, power=1):
    """Velocity of the FFTMesh vertices [N*N, 3] at t (power = 3: the third time derivative); f64 oracle, FFT or matmul form."""
    w = fftmesh_omega(p)
    a, b = np.asarray(h0, np.float64), np.asarray(h0c, np.float64)
    for _ in range(power):
        a, b = weight(a, b, w)
    a, b = a.astype(np.float32), b.astype(np.float32)
    ev = O.eval_fft_f64 if (p.commensurate and p.N % 2 == 0 and p.N >= 8 and (p.N & (p.N - 1)) == 0) else O.eval_matmul_f64
    v = ev(p, a, b, t)[0]
    return v - O.rest_mesh(p)[0].astype(np.float64)


def renderer_omega(rp):
    """or_omega [py, px] (F/FFTCommon.cginc:58-67, 101-114) in strict float32, texel (px, py) at [py, px]."""
    M = rp.M
    f = np.float32
    n = np.arange(M)
    n = np.where(n < M // 2, n, n - M).astype(np.float32)
    k = (f(2.0) * f(np.pi) * n).astype(np.float32) / f(rp.length)
    k = k.astype(np.float32)
    kx, kz = k[None, :], k[:, None]  # [py, px]: x along px
    wl = np.sqrt((kx * kx + kz * kz).astype(np.float32)).astype(np.float32)
    q = ((wl * wl).astype(np.float32) / f(370.0)).astype(np.float32) / f(370.0)
    inner = (f(rp.gravity) * wl).astype(np.float32) * (f(1.0) + q.astype(np.float32)).astype(np.float32)
    return np.sqrt(inner.astype(np.float32)).astype(np.float32)


def renderer_velocity_f64(rp, init4, phase):
    """OceanRenderer velocity [res*res, 3] at the phase texture `phase` ([py, px] float32), per second of delta_time: the vertex stage
    (W/TestOcean.shader:65-66) with a zero rest coordinate over the rate textures of the weighted initial spectrum.  The phase advances
    by omega * delta_time * mult (S/OceanRenderer.cs:223): the weight is omega * mult, formed in float32 as the kernel forms it."""
    w = (renderer_omega(rp) * np.float32(rp.mult)).astype(np.float32)
    a, b = weight(init4[..., :2], init4[..., 2:], w)
    iv = np.concatenate([a, b], -1).astype(np.float32)
    ph = np.ascontiguousarray(phase, np.float32).copy()
    htex, dtex, _, _ = O.renderer_textures_f64(rp, iv, ph, 0.0)
    M = rp.M
    v, _, _ = O.renderer_mesh_vertex_stage_f64(rp, 0.0, htex[..., 0], dtex[..., [0, 2]], np.tile([0.0, 1.0, 0.0], (M, M, 1)), np.zeros((M, M)))
    return v
