// FFTMesh.cs -- drop-in for Assets/Mistral Water/Scripts/FFTMesh.cs: the same component name, Inspector fields
// (reference :9-23) and Unity messages (Awake / Update, :60-84); the private numerical methods -- the Phillips /
// htilde0 spectrum fill, htilde, the O(N^4) Displacement loop and the Jacobian of EvaluateWaves (:141-280) -- are
// libmistral_water.so on an MI355X.  Written against include/mistral_water.h; nothing of the reference's method
// bodies is kept.  Not compilable in the build image (no C# toolchain, UnityEngine.dll is proprietary):
// tests/test_csharp_binding.py checks every native call of this file against MistralWaterNative.cs.
using System;
using System.Runtime.InteropServices;
using UnityEngine;
using Native = MistralWaterNative;

public class FFTMesh : MonoBehaviour
{
    // ---- Inspector fields: names, types and defaults of the reference ------------------------------------------
    public float choppiness = 1f;
    public float tDivision = 1f;
    public int resolution = 50;
    public float unitWidth = 1f;
    public bool generate = false;
    public float length = 1f;
    public Vector2 wind = new Vector2(1f, 1f);
    public float amplitude = 1f;

    // ---- additions (the reference never seeds UnityEngine.Random; the library's generator is a documented counter RNG)
    public ulong seed = 1;
    public bool fixedSeed = false;   // true: every regeneration reproduces the same sea; false: a new one, like GenerateMesh
    public int device = 0;

    IntPtr ocean = IntPtr.Zero;
    ulong generation = 0;
    MeshFilter filter;
    Mesh mesh;
    Vector3[] vertices, displaced, normals;
    Vector2[] uvs;
    Color[] colors;
    int[] indices;
    GCHandle pinDisplaced, pinNormals, pinColors;
    float timer = 0f;

    void Awake()
    {
        filter = GetComponent<MeshFilter>();
        if (filter == null) filter = gameObject.AddComponent<MeshFilter>();
        mesh = new Mesh();
        mesh.indexFormat = UnityEngine.Rendering.IndexFormat.UInt32;   // 1024^2 vertices do not fit 16-bit indices
        filter.mesh = mesh;
        Regenerate();
    }

    void Update()
    {
        if (generate)
        {
            timer = 0f;
            Regenerate();
            generate = false;
        }
        timer += Time.deltaTime / tDivision;
        EvaluateWaves(timer);
    }

    void OnDestroy() { Release(); }

    // SetParams + GenerateMesh: handle, rest mesh, spectrum (a fresh draw on every regeneration unless fixedSeed)
    void Regenerate()
    {
        Release();
        Native.Params p = new Native.Params();
        Native.mw_params_default(ref p, (int)Native.Semantics.FFTMesh);
        p.resolution = resolution;
        p.unit_width = unitWidth;
        p.length = length;
        p.wind_x = wind.x;
        p.wind_y = wind.y;
        p.amplitude = amplitude;
        p.choppiness = choppiness;
        p.t_division = tDivision;
        p.seed = fixedSeed ? seed : seed + generation;
        p.device = device;
        generation++;
        Native.Check(Native.mw_ocean_create(ref p, out ocean));

        int n = resolution * resolution;
        vertices = new Vector3[n];
        displaced = new Vector3[n];
        normals = new Vector3[n];
        uvs = new Vector2[n];
        colors = new Color[n];
        indices = new int[(int)Native.mw_ocean_index_count(ocean)];
        Native.Check(Native.mw_ocean_rest_mesh(ocean, vertices, normals, uvs, indices));
        mesh.Clear();
        mesh.vertices = vertices;
        mesh.SetIndices(indices, MeshTopology.Triangles, 0);
        mesh.normals = normals;
        mesh.uv = uvs;

        // the three arrays EvaluateWaves fills every frame stay page-locked for the life of the handle
        pinDisplaced = Native.Pin(displaced, n * 12);
        pinNormals = Native.Pin(normals, n * 12);
        pinColors = Native.Pin(colors, n * 16);
    }

    void EvaluateWaves(float t)
    {
        Native.Check(Native.mw_ocean_set_choppiness(ocean, choppiness));   // the reference reads the live field every frame
        Native.Check(Native.mw_ocean_evaluate(ocean, t, displaced, normals, colors));
        mesh.vertices = displaced;
        mesh.normals = normals;
        mesh.colors = colors;
    }

    /// Not in the reference: SampleSurface, hull forces and bodies read the infinite tiling of the mesh (period = resolution * unitWidth)
    /// instead of the one footprint, so nothing that drifts off the patch is lost.  Throws unless unitWidth * resolution == length and the
    /// resolution is even; raycasts refuse a periodic handle.
    public void SetPeriodic(bool on = true)
    {
        Native.Check(Native.mw_ocean_set_periodic(ocean, on ? 1 : 0));
    }

    /// Not in the reference: the displaced mesh's surface at horizontal points, xz = {x0, z0, x1, z1, ...} in the mesh's object space;
    /// result (8 floats per point) = position xyz, normal xyz, whitecap, residual.  world = true: xz lies on the displaced surface (the
    /// buoyancy question "how high is the water here?"); false: xz is a rest-plane position (NaN off the mesh).  Surface of the latest Update().
    public void SampleSurface(float[] xz, float[] result, bool world = true)
    {
        if (result.Length < xz.Length * 4) throw new ArgumentException("result needs 8 floats per point");
        Native.Check(Native.mw_ocean_query_surface(ocean, -1, world ? Native.QueryWorld : Native.QueryRest, xz, xz.Length / 2, 0, result));
    }

    /// Not in the reference: the water's velocity at horizontal points xz (x0, z0, x1, z1, ...), located exactly as SampleSurface locates
    /// them; result = (vx, vy, vz, residual) per point, the velocity PER SECOND of Update's deltaTime (the library's value is per unit of
    /// the time argument, which Update advances by deltaTime / tDivision).  Drag needs the water's velocity relative to the hull.
    public void SampleVelocity(float[] xz, float[] result, bool world = true)
    {
        if (result.Length < xz.Length * 2) throw new ArgumentException("result needs 4 floats per point");
        Native.Check(Native.mw_ocean_query_velocity(ocean, -1, world ? Native.QueryWorld : Native.QueryRest, xz, xz.Length / 2, 0, result));
        for (int k = 0; k < xz.Length / 2; k++)
            for (int c = 0; c < 3; c++) result[4 * k + c] /= tDivision;
    }

    /// Not in the reference: the water below the surface.  SetColumn names the rest depths of the layers (depths[0] == 0, strictly increasing,
    /// 2 to 16 of them; null releases them); SampleColumn then answers at points xyz_ = {x, y, z, unused, ...} (4 floats per point) of the
    /// latest Update(): result (12 floats per point) = velocity xyz PER SECOND of Update's deltaTime, rest depth (density * gravity * rest
    /// depth is the pressure), position xyz, layer coordinate, rest point x0 z0, surface height over the point, residual.  world = false:
    /// the point is a particle's label (x0, rest depth, z0).
    public void SetColumn(float[] depths)
    {
        Native.Check(Native.mw_ocean_set_column(ocean, depths, depths == null ? 0 : depths.Length));
    }

    public void SampleColumn(float[] xyz_, float[] result, bool world = true)
    {
        if (result.Length < xyz_.Length * 3) throw new ArgumentException("result needs 12 floats per point");
        Native.Check(Native.mw_ocean_query_column(ocean, -1, world ? Native.QueryWorld : Native.QueryRest, xyz_, xyz_.Length / 4, 0, result));
        for (int k = 0; k < xyz_.Length / 4; k++)
            for (int c = 0; c < 3; c++) result[12 * k + c] /= tDivision;
    }

    /// Not in the reference: HullForces and StepBodies read the water column (SetColumn) under every hull vertex instead of the surface
    /// above it: the pressure at the vertex's rest depth and the water's velocity down there.  For keels, spar buoys and deep hulls.
    public void SetDraught(bool on = true)
    {
        Native.Check(Native.mw_ocean_set_draught(ocean, on ? 1 : 0));
    }

    /// Not in the reference: the first hit of rays on the displaced surface of the latest Update() (mw_ocean_raycast), in the mesh's
    /// object space.  rays (8 floats per ray) = origin xyz, tmin, direction xyz, tmax: t is in units of the direction, a segment
    /// p0 -> p1 is (p0, 0, p1 - p0, 1).  result (8 floats per ray) = t, point xyz, normal xyz, whitecap; t = +infinity on a miss, NaN
    /// for an invalid ray.  hit (2 ints per ray, may be null) = triangle id, facing: +1 the ray met the water from above, -1 from below.
    public void Raycast(float[] rays, float[] result, int[] hit = null)
    {
        if (rays.Length % 8 != 0) throw new ArgumentException("rays needs 8 floats per ray");
        if (result.Length < rays.Length) throw new ArgumentException("result needs 8 floats per ray");
        if (hit != null && hit.Length < rays.Length / 4) throw new ArgumentException("hit needs 2 ints per ray");
        Native.Check(Native.mw_ocean_raycast(ocean, -1, rays, rays.Length / 8, result, hit));
    }

    /// Not in the reference: buoyancy and drag on bodies sharing one hull mesh, from the surface of the latest Update()
    /// (mw_ocean_hull_forces).  result (8 floats per body) = force xyz, wetted area, torque xyz about the centre of mass, residual, in
    /// the ocean's object space (unscaled ocean transform assumed: ocean.TransformDirection maps them to world space).  The water
    /// velocity the drag uses is per second of Update's deltaTime (the library's value per unit of t, over tDivision).  Drag 0 computes no velocity.
    public void HullForces(Mesh hull, Rigidbody[] bodies, float[] result, float density = 1000f, float linearDrag = 0f, float quadraticDrag = 0f)
    {
        if (result.Length < bodies.Length * 8) throw new ArgumentException("result needs 8 floats per body");
        float[] hullXyz, packed;
        int[] triangles;
        Native.PackHull(transform, hull, bodies, out hullXyz, out triangles, out packed);
        float[] coeffs = { density, -Physics.gravity.y, linearDrag, quadraticDrag, 1f / tDivision };
        Native.Check(Native.mw_ocean_hull_forces(ocean, -1, hullXyz, hullXyz.Length / 3, triangles, triangles.Length / 3, packed, bodies.Length, coeffs, 0, result));
    }

    /// Evaluate the ocean Unity itself generated: pass the reference's own htilde0 draws (verttilde / vertConj).
    public void SetSpectrum(Vector2[] h0, Vector2[] h0conj)
    {
        Native.Check(Native.mw_ocean_set_spectrum(ocean, h0, h0conj));
    }

    void Release()
    {
        Native.Unpin(pinDisplaced);
        Native.Unpin(pinNormals);
        Native.Unpin(pinColors);
        if (ocean != IntPtr.Zero)
        {
            Native.mw_ocean_destroy(ocean);
            ocean = IntPtr.Zero;
        }
    }
}
