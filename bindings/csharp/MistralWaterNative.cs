// MistralWaterNative.cs -- the P/Invoke layer over libmistral_water.so (include/mistral_water.h, MW_ABI_VERSION 4).
//
// Drop into Assets/Mistral Water/Scripts/ next to the two MonoBehaviours of this folder; the shared object goes to
// Assets/Plugins/x86_64/libmistral_water.so.  Every extern below mirrors one prototype of the header, argument for
// argument; tests/test_csharp_binding.py parses this file and checks names, argument counts and kinds, struct field
// order and sizes against the header, because no C# toolchain exists in the build image to compile it.
//
// Marshalling: Vector2 / Vector3 / Vector4 / Color are blittable sequential float structs, so a managed array of them is
// pinned by the marshaller and arrives as float*; IntPtr carries device pointers, streams and opaque handles.
using System;
using System.Runtime.InteropServices;
using UnityEngine;

public static class MistralWaterNative
{
    const string Lib = "mistral_water";

    public const int AbiVersion = 4;
    public const int CommIdBytes = 128;

    public enum Status { OK = 0, EINVAL = 1, ENOTPOW2 = 2, ENOTCOMMENSURATE = 3, ENOMEM = 4, EDEVICE = 5, ESTATE = 6 }
    public enum Semantics { FFTMesh = 0, OceanRenderer = 1 }
    public enum PondMode { Wave = 0, Gerstner = 1, GerstnerLevelOne = 2 }
    public const uint OutWhiteScalar = 0u, OutColorRgba = 1u;
    public const int QueryRest = 0, QueryWorld = 1;
    public const int HullNCoeffs = 5;
    public const int BodyNMass = 8;
    public const int RcDefaultReach = 16, RcMaxReach = 1024;
    public const int FleetMaxHulls = 32, FleetNHull = 5;
    public const int MooringMaxLines = 8, MooringNLine = 12;
    public const int RigAnchor = -1;
    public const int ColumnMaxLayers = 16;

    [StructLayout(LayoutKind.Sequential)]   // mw_params: 56 bytes
    public struct Params
    {
        public int resolution;
        public float unit_width;
        public float length;
        public float wind_x;
        public float wind_y;
        public float amplitude;
        public float choppiness;
        public float gravity;
        public float t_division;
        public float mult;
        public ulong seed;
        public int semantics;
        public int device;
    }

    [StructLayout(LayoutKind.Sequential)]   // mw_pond_params: 72 bytes
    public struct PondParams
    {
        public int mode;
        public float amplitude;
        public float frequency;
        public float speed;
        public float steepness;
        public float smoothing;
        public Vector4 wspeed;
        public Vector4 dir_ab;
        public Vector4 dir_cd;
    }

    // ---- library ------------------------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern int mw_abi_version();
    [DllImport(Lib)] public static extern IntPtr mw_build_id();
    [DllImport(Lib)] public static extern IntPtr mw_last_error();
    [DllImport(Lib)] public static extern int mw_device_count();
    [DllImport(Lib)] public static extern void mw_params_default(ref Params p, int semantics);

    // ---- lifecycle ----------------------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_ocean_create(ref Params p, out IntPtr ocean);
    [DllImport(Lib)] public static extern void mw_ocean_destroy(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_create_batch(ref Params p, int ntiles, out IntPtr ocean);
    [DllImport(Lib)] public static extern int mw_ocean_batch_size(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_set_stream(IntPtr ocean, IntPtr hipStream);
    [DllImport(Lib)] public static extern Status mw_ocean_use_own_stream(IntPtr ocean);
    [DllImport(Lib)] public static extern IntPtr mw_ocean_get_stream(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_synchronize(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_set_choppiness(IntPtr ocean, float choppiness);
    [DllImport(Lib)] public static extern Status mw_ocean_set_periodic(IntPtr ocean, int on);
    [DllImport(Lib)] public static extern Status mw_ocean_get_periodic(IntPtr ocean, out int on, out float period);

    // ---- spectrum and state -------------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_ocean_set_spectrum(IntPtr ocean, Vector2[] h0, Vector2[] h0conj);
    [DllImport(Lib)] public static extern Status mw_ocean_get_spectrum(IntPtr ocean, [Out] Vector2[] h0, [Out] Vector2[] h0conj);
    [DllImport(Lib)] public static extern Status mw_ocean_reinit_spectrum(IntPtr ocean, float length, float windX, float windY, float amplitude, ulong seed);
    [DllImport(Lib)] public static extern Status mw_ocean_get_phase(IntPtr ocean, [Out] float[] phase);
    [DllImport(Lib)] public static extern Status mw_ocean_set_phase(IntPtr ocean, float[] phase);
    [DllImport(Lib)] public static extern Status mw_ocean_set_timer(IntPtr ocean, float timer);
    [DllImport(Lib)] public static extern float mw_ocean_normal_length(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_set_normal_length(IntPtr ocean, float normalLength);
    [DllImport(Lib)] public static extern float mw_ocean_timer(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_reset_timer(IntPtr ocean);

    // ---- mesh ---------------------------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_ocean_rest_mesh(IntPtr ocean, [Out] Vector3[] vertices, [Out] Vector3[] normals, [Out] Vector2[] uvs, [Out] int[] indices);
    [DllImport(Lib)] public static extern long mw_ocean_index_count(IntPtr ocean);
    [DllImport(Lib)] public static extern int mw_ocean_grid_size(IntPtr ocean);

    // ---- FFTMesh.EvaluateWaves ----------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_ocean_evaluate(IntPtr ocean, float t, [Out] Vector3[] vertices, [Out] Vector3[] normals, [Out] Color[] colors);
    [DllImport(Lib)] public static extern Status mw_ocean_update(IntPtr ocean, float deltaTime, [Out] Vector3[] vertices, [Out] Vector3[] normals, [Out] Color[] colors);
    [DllImport(Lib)] public static extern Status mw_ocean_evaluate_device(IntPtr ocean, float[] t, int nsteps, IntPtr dVertices, IntPtr dNormals, IntPtr dWhite, uint flags);
    [DllImport(Lib)] public static extern int mw_ocean_max_batch(IntPtr ocean);

    // ---- OceanRenderer.GenerateTexture --------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture(IntPtr ocean, float deltaTime, [Out] float[] height, [Out] Vector2[] dispXZ, [Out] Vector3[] normal, [Out] float[] white);
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_device(IntPtr ocean, float deltaTime, IntPtr dHeight, IntPtr dDispXZ, IntPtr dNormal, IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_rgba(IntPtr ocean, float deltaTime, [Out] Color[] height, [Out] Color[] displacement, [Out] Color[] normal, [Out] Color[] white);
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_rgba_device(IntPtr ocean, float deltaTime, IntPtr dHeight, IntPtr dDisplacement, IntPtr dNormal, IntPtr dWhite);
    // nframes consecutive GenerateTexture() calls in one enqueue (bit-identical to nframes single calls, the phase included); device destinations [nframes][...]
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_steps_device(IntPtr ocean, float[] deltaTime, int nframes, IntPtr dHeight, IntPtr dDispXZ, IntPtr dNormal, IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_steps_rgba_device(IntPtr ocean, float[] deltaTime, int nframes, IntPtr dHeight, IntPtr dDisplacement, IntPtr dNormal, IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_steps(IntPtr ocean, float[] deltaTime, int nframes, [Out] float[] height, [Out] Vector2[] dispXZ, [Out] Vector3[] normal, [Out] float[] white);
    [DllImport(Lib)] public static extern Status mw_ocean_generate_texture_steps_rgba(IntPtr ocean, float[] deltaTime, int nframes, [Out] Color[] height, [Out] Color[] displacement, [Out] Color[] normal, [Out] Color[] white);
    [DllImport(Lib)] public static extern int mw_ocean_max_frames(IntPtr ocean);
    [DllImport(Lib)] public static extern Status mw_ocean_advance_phase(IntPtr ocean, float[] deltaTime, int nframes);
    [DllImport(Lib)] public static extern Status mw_ocean_frame_textures(IntPtr ocean, int frame, out IntPtr dHeight, out IntPtr dDispXZ, out IntPtr dNormal, out IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_ocean_displace_mesh(IntPtr ocean, [Out] Vector3[] vertices, [Out] Vector3[] normals, [Out] float[] colors);
    [DllImport(Lib)] public static extern Status mw_ocean_displace_mesh_device(IntPtr ocean, IntPtr dVertices, IntPtr dNormals, IntPtr dColors);
    // surface queries: xz [n][2] -> result [n][8] = (px, py, pz, nx, ny, nz, white, residual); frame -1 = latest
    [DllImport(Lib)] public static extern Status mw_ocean_query_surface(IntPtr ocean, int frame, int mode, float[] xz, long n, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_query_surface_device(IntPtr ocean, int frame, int mode, IntPtr dXz, long n, int iterations, IntPtr dResult);
    // surface velocity: per vertex [R*R][3], or at xz [n][2] -> result [n][4] = (vx, vy, vz, residual); FFTMesh per unit of t, OceanRenderer per second
    [DllImport(Lib)] public static extern Status mw_ocean_velocity(IntPtr ocean, int frame, [Out] Vector3[] velocity);
    [DllImport(Lib)] public static extern Status mw_ocean_velocity_device(IntPtr ocean, int frame, IntPtr dVelocity);
    [DllImport(Lib)] public static extern Status mw_ocean_query_velocity(IntPtr ocean, int frame, int mode, float[] xz, long n, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_query_velocity_device(IntPtr ocean, int frame, int mode, IntPtr dXz, long n, int iterations, IntPtr dResult);
    // hull forces: hullXyz [nverts][3], triangles [ntris][3], bodies [nbodies][16] (p _ q v _ w _), coeffs [HullNCoeffs] (density, gravity,
    // linearDrag, quadraticDrag, velocityScale) -> result [nbodies][8] = (Fx, Fy, Fz, wettedArea, tx, ty, tz, residual)
    [DllImport(Lib)] public static extern Status mw_ocean_hull_forces(IntPtr ocean, int frame, float[] hullXyz, int nverts, int[] triangles, int ntris, float[] bodies, int nbodies, float[] coeffs, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_hull_forces_device(IntPtr ocean, int frame, IntPtr dHullXyz, int nverts, IntPtr dTriangles, int ntris, IntPtr dBodies, int nbodies, float[] coeffs, int iterations, IntPtr dResult);
    // floating bodies: massProperties [10] = (mass, centroid xyz, Ixx Iyy Izz Ixy Ixz Iyz); bodies [nbodies][16] updated in place, mass
    // [nbodies][BodyNMass] = (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz, 0) about the centre of mass, result [nbodies][8] or null (the last substep's row)
    [DllImport(Lib)] public static extern Status mw_hull_mass_properties(float[] hullXyz, int nverts, int[] triangles, int ntris, float density, [Out] float[] massProperties);
    [DllImport(Lib)] public static extern Status mw_ocean_step_bodies(IntPtr ocean, int frame, float[] hullXyz, int nverts, int[] triangles, int ntris, [In] [Out] float[] bodies, float[] mass, int nbodies, float[] coeffs, float dt, int substeps, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_step_bodies_device(IntPtr ocean, int frame, IntPtr dHullXyz, int nverts, IntPtr dTriangles, int ntris, IntPtr dBodies, IntPtr dMass, int nbodies, float[] coeffs, float dt, int substeps, int iterations, IntPtr dResult);
    // moorings: step_bodies with lines [nbodies][linesPerBody][MooringNLine] = (hx, hy, hz, L0 | ax, ay, az, k | c, _, _, _) from a point of the body
    // (body space, about p) to a fixed anchor (world); linesPerBody in [1, MooringMaxLines]; tension [nbodies][linesPerBody] or null
    [DllImport(Lib)] public static extern Status mw_ocean_step_moored(IntPtr ocean, int frame, float[] hullXyz, int nverts, int[] triangles, int ntris, [In] [Out] float[] bodies, float[] mass, float[] lines, int linesPerBody, int nbodies, float[] coeffs, float dt, int substeps, int iterations, [Out] float[] result, [Out] float[] tension);
    [DllImport(Lib)] public static extern Status mw_ocean_step_moored_device(IntPtr ocean, int frame, IntPtr dHullXyz, int nverts, IntPtr dTriangles, int ntris, IntPtr dBodies, IntPtr dMass, IntPtr dLines, int linesPerBody, int nbodies, float[] coeffs, float dt, int substeps, int iterations, IntPtr dResult, IntPtr dTension);
    // mixed fleets: every hull's geometry concatenated (triangle indices local to their hull), hulls [nhulls][FleetNHull] = (vertFirst, nverts,
    // triFirst, ntris, nbodies), coeffs [nhulls][HullNCoeffs]; bodies, mass, wrench [totalBodies][8] = (Fx, Fy, Fz, _, tx, ty, tz, _) or null
    // and result hull after hull in table order; a body's row and state have the bits of the single-hull call on its hull alone
    [DllImport(Lib)] public static extern Status mw_ocean_fleet_forces(IntPtr ocean, int frame, float[] hullXyz, int totalVerts, int[] triangles, int totalTris, int[] hulls, int nhulls, float[] bodies, int totalBodies, float[] coeffs, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_fleet_forces_device(IntPtr ocean, int frame, IntPtr dHullXyz, int totalVerts, IntPtr dTriangles, int totalTris, int[] hulls, int nhulls, IntPtr dBodies, int totalBodies, float[] coeffs, int iterations, IntPtr dResult);
    [DllImport(Lib)] public static extern Status mw_ocean_step_fleet(IntPtr ocean, int frame, float[] hullXyz, int totalVerts, int[] triangles, int totalTris, int[] hulls, int nhulls, [In] [Out] float[] bodies, float[] mass, float[] wrench, int totalBodies, float[] coeffs, float dt, int substeps, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_step_fleet_device(IntPtr ocean, int frame, IntPtr dHullXyz, int totalVerts, IntPtr dTriangles, int totalTris, int[] hulls, int nhulls, IntPtr dBodies, IntPtr dMass, IntPtr dWrench, int totalBodies, float[] coeffs, float dt, int substeps, int iterations, IntPtr dResult);
    // rigged fleets: step_fleet with step_moored's lines [totalBodies][linesPerBody][MooringNLine] and targets [totalBodies][linesPerBody] or null
    // (RigAnchor: a is a fixed world point; j >= 0: a is a point in the body space of body j, a tow line); tension [totalBodies][linesPerBody] or null
    [DllImport(Lib)] public static extern Status mw_ocean_step_rigged(IntPtr ocean, int frame, float[] hullXyz, int totalVerts, int[] triangles, int totalTris, int[] hulls, int nhulls, [In] [Out] float[] bodies, float[] mass, float[] wrench, float[] lines, int[] targets, int linesPerBody, int totalBodies, float[] coeffs, float dt, int substeps, int iterations, [Out] float[] result, [Out] float[] tension);
    [DllImport(Lib)] public static extern Status mw_ocean_step_rigged_device(IntPtr ocean, int frame, IntPtr dHullXyz, int totalVerts, IntPtr dTriangles, int totalTris, int[] hulls, int nhulls, IntPtr dBodies, IntPtr dMass, IntPtr dWrench, IntPtr dLines, IntPtr dTargets, int linesPerBody, int totalBodies, float[] coeffs, float dt, int substeps, int iterations, IntPtr dResult, IntPtr dTension);
    // raycasts: rays [n][8] = (ox, oy, oz, tmin, dx, dy, dz, tmax) -> result [n][8] = (t, px, py, pz, nx, ny, nz, white), hit [n][2] =
    // (triangle, facing) or null; a miss: t = +infinity, an invalid ray: NaN
    [DllImport(Lib)] public static extern Status mw_ocean_raycast(IntPtr ocean, int frame, float[] rays, long n, [Out] float[] result, [Out] int[] hit);
    [DllImport(Lib)] public static extern Status mw_ocean_raycast_device(IntPtr ocean, int frame, IntPtr dRays, long n, IntPtr dResult, IntPtr dHit);
    // tiled raycasts (the periodic surface, whatever the switch says): the (2 reach + 1)^2 tiles around the origin's; hit [n][4] =
    // (tiled triangle id, facing, tile x, tile z) or null; id -1: a miss, -2: the ray left the window's reach unhit
    [DllImport(Lib)] public static extern Status mw_ocean_raycast_tiled(IntPtr ocean, int frame, float[] rays, long n, int reach, [Out] float[] result, [Out] int[] hit);
    [DllImport(Lib)] public static extern Status mw_ocean_raycast_tiled_device(IntPtr ocean, int frame, IntPtr dRays, long n, int reach, IntPtr dResult, IntPtr dHit);

    // the water column (FFTMesh handles): layers at rest depths 0 = d_0 < d_1 < ...; xyz [n][4] (fourth float ignored), result [n][12] =
    // ux uy uz rest_depth | px py pz lambda | x0 z0 eta residual; rho g rest_depth is the pressure at the point
    [DllImport(Lib)] public static extern Status mw_ocean_set_column(IntPtr ocean, float[] depths, int nlayers);
    [DllImport(Lib)] public static extern Status mw_ocean_get_column(IntPtr ocean, [Out] float[] depths, out int nlayers);
    [DllImport(Lib)] public static extern Status mw_ocean_column_layers(IntPtr ocean, int frame, int layer, out IntPtr dPositions, out IntPtr dVelocities);
    [DllImport(Lib)] public static extern Status mw_ocean_query_column(IntPtr ocean, int frame, int mode, float[] xyz, long n, int iterations, [Out] float[] result);
    [DllImport(Lib)] public static extern Status mw_ocean_query_column_device(IntPtr ocean, int frame, int mode, IntPtr dXyz, long n, int iterations, IntPtr dResult);

    // draught (FFTMesh handles): with it on, mw_ocean_hull_forces and mw_ocean_step_bodies read the water column under every hull vertex
    // (rest depth for the pressure, the column's velocity for the drag); needs a column by the time of the call; the fleet calls refuse it
    [DllImport(Lib)] public static extern Status mw_ocean_set_draught(IntPtr ocean, int on);
    [DllImport(Lib)] public static extern Status mw_ocean_get_draught(IntPtr ocean, out int on);

    // ---- page-locked output arrays ------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_host_register(IntPtr ptr, UIntPtr bytes);
    [DllImport(Lib)] public static extern Status mw_host_unregister(IntPtr ptr);

    // ---- independent tiles on several devices, RCCL gather ------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_comm_unique_id([Out] byte[] id);
    [DllImport(Lib)] public static extern Status mw_tiles_create(ref Params p, int ntiles, int[] devices, int maxSteps, out IntPtr tiles);
    [DllImport(Lib)] public static extern Status mw_tiles_create_rank(ref Params p, int device, int maxSteps, byte[] commId, int rank, int nranks, out IntPtr tiles);
    [DllImport(Lib)] public static extern void mw_tiles_destroy(IntPtr tiles);
    [DllImport(Lib)] public static extern int mw_tiles_count(IntPtr tiles);
    [DllImport(Lib)] public static extern int mw_tiles_local_count(IntPtr tiles);
    [DllImport(Lib)] public static extern IntPtr mw_tiles_ocean(IntPtr tiles, int localK);
    [DllImport(Lib)] public static extern Status mw_tiles_evaluate(IntPtr tiles, float[] times, int nsteps, uint flags);
    // the outputs of the LATEST mw_tiles_evaluate: a tile that is gathered owns two output sets used alternately -- ask again after every evaluate once mw_tiles_gather is in use
    [DllImport(Lib)] public static extern Status mw_tiles_outputs(IntPtr tiles, int localK, out IntPtr dVertices, out IntPtr dNormals, out IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_tiles_generate_texture(IntPtr tiles, float deltaTime);
    [DllImport(Lib)] public static extern Status mw_tiles_textures(IntPtr tiles, int localK, out IntPtr dHeight, out IntPtr dDispXZ, out IntPtr dNormal, out IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_tiles_generate_texture_steps(IntPtr tiles, float[] deltaTime, int nframes);
    [DllImport(Lib)] public static extern Status mw_tiles_frames(IntPtr tiles, int localK, out IntPtr dHeight, out IntPtr dDispXZ, out IntPtr dNormal, out IntPtr dWhite);
    [DllImport(Lib)] public static extern Status mw_tiles_gather(IntPtr tiles, int step, int root);
    [DllImport(Lib)] public static extern Status mw_tiles_gathered(IntPtr tiles, out IntPtr dGathered, out long floatsPerTile);
    [DllImport(Lib)] public static extern Status mw_tiles_synchronize(IntPtr tiles);

    // ---- pond ---------------------------------------------------------------------------------------------------
    [DllImport(Lib)] public static extern Status mw_gerstner_displace(Vector3[] pos, long nverts, Vector3[] waves, int nwaves, float amplitude, float frequency, float steepness, float t, [Out] Vector3[] outPos, int device);
    [DllImport(Lib)] public static extern Status mw_gerstner_displace_device(IntPtr dPos, long nverts, Vector3[] waves, int nwaves, float amplitude, float frequency, float steepness, float t, IntPtr dOut, IntPtr hipStream);
    [DllImport(Lib)] public static extern Status mw_gerstner_displace_steps_device(IntPtr dPos, long nverts, Vector3[] waves, int nwaves, float amplitude, float frequency, float steepness, float[] t, int nsteps, IntPtr dOut, IntPtr hipStream);
    [DllImport(Lib)] public static extern int mw_gerstner_max_steps(int nwaves);
    [DllImport(Lib)] public static extern Status mw_pond_displace(ref PondParams p, Vector3[] pos, long nverts, float t, [Out] Vector3[] outPos, [Out] Vector3[] outNormal, int device);
    [DllImport(Lib)] public static extern Status mw_pond_displace_device(ref PondParams p, IntPtr dPos, long nverts, float t, IntPtr dOut, IntPtr dOutNormal, IntPtr hipStream);

    // ---- helpers ------------------------------------------------------------------------------------------------
    public static string LastError() { return Marshal.PtrToStringAnsi(mw_last_error()); }

    public static void Check(Status s)
    {
        if (s != Status.OK) throw new InvalidOperationException("libmistral_water: " + s + ": " + LastError());
    }

    /// Packs the arrays of mw_ocean_hull_forces for bodies that share one hull mesh (one prefab): the mesh's vertices about the
    /// first body's centre of mass, scaled by its lossyScale (worldCenterOfMass = TransformPoint(centerOfMass)), its triangles, and
    /// per body (p _ q v _ w _) in the OCEAN'S OBJECT SPACE -- the space of the ocean's vertex outputs -- with p the body's centre of
    /// mass, so the torque the call returns is about it.  The ocean's transform is assumed unscaled (rotation and translation only);
    /// forces and torques map back to world space with ocean.TransformDirection.
    public static void PackHull(Transform ocean, Mesh hull, Rigidbody[] bodies, out float[] hullXyz, out int[] triangles, out float[] packed)
    {
        Vector3[] v = hull.vertices;
        Vector3 s = bodies.Length > 0 ? bodies[0].transform.lossyScale : Vector3.one;
        Vector3 c = bodies.Length > 0 ? bodies[0].centerOfMass : Vector3.zero;
        hullXyz = new float[v.Length * 3];
        for (int k = 0; k < v.Length; k++)
        {
            hullXyz[3 * k] = (v[k].x - c.x) * s.x; hullXyz[3 * k + 1] = (v[k].y - c.y) * s.y; hullXyz[3 * k + 2] = (v[k].z - c.z) * s.z;
        }
        triangles = hull.triangles;
        packed = new float[bodies.Length * 16];
        Quaternion inv = Quaternion.Inverse(ocean.rotation);
        for (int b = 0; b < bodies.Length; b++)
        {
            Rigidbody r = bodies[b];
            Vector3 p = ocean.InverseTransformPoint(r.worldCenterOfMass);
            Quaternion q = inv * r.rotation;
            Vector3 vel = ocean.InverseTransformDirection(r.velocity), w = ocean.InverseTransformDirection(r.angularVelocity);
            int o = 16 * b;
            packed[o] = p.x; packed[o + 1] = p.y; packed[o + 2] = p.z;
            packed[o + 4] = q.x; packed[o + 5] = q.y; packed[o + 6] = q.z; packed[o + 7] = q.w;
            packed[o + 8] = vel.x; packed[o + 9] = vel.y; packed[o + 10] = vel.z;
            packed[o + 12] = w.x; packed[o + 13] = w.y; packed[o + 14] = w.z;
        }
    }

    /// Page-locks a managed array for as long as the returned handle lives (mw_host_register): the per-frame copy of the
    /// results into it then runs at PCIe rate instead of the pageable ~9 GB/s.  Release with Unpin.
    public static GCHandle Pin(Array a, int bytes)
    {
        GCHandle h = GCHandle.Alloc(a, GCHandleType.Pinned);
        Check(mw_host_register(h.AddrOfPinnedObject(), (UIntPtr)(ulong)bytes));
        return h;
    }

    public static void Unpin(GCHandle h)
    {
        if (!h.IsAllocated) return;
        mw_host_unregister(h.AddrOfPinnedObject());
        h.Free();
    }
}
