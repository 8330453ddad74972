// FFTMesh.hpp / OceanRenderer -- C++ mirror of the reference's two MonoBehaviours over the C ABI.
//
// The reference's host language is C# (Unity); the build image has no C# toolchain, so the compiled host side
// above include/mistral_water.h is C++ (and Python for the tests).  Public field names and the Awake()/Update()
// lifecycle follow S/FFTMesh.cs:9-23,60-84 and S/OceanRenderer.cs:10-19,76-110; everything the reference
// computes in private methods is delegated to libmistral_water.so (HIP, MI355X).  Header-only.
#pragma once
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mistral_water.h"

namespace mistral_water {

struct Vector2 { float x = 0.f, y = 0.f; };
struct Vector3 { float x = 0.f, y = 0.f, z = 0.f; };
struct Color { float r = 0.f, g = 0.f, b = 0.f, a = 0.f; };
static_assert(sizeof(Vector3) == 12 && sizeof(Color) == 16 && sizeof(Vector2) == 8, "blittable Unity structs");

// the UnityEngine.Mesh members the reference assigns (S/FFTMesh.cs:134-138,277-279)
struct Mesh {
    std::vector<Vector3> vertices, normals;
    std::vector<Vector2> uv;
    std::vector<Color> colors;
    std::vector<int32_t> indices;
};

inline void check(mw_status s) {
    if (s != MW_OK) throw std::runtime_error(std::string("mistral_water: ") + mw_last_error());
}

// one answer of mw_ocean_query_surface: the displaced mesh's surface point, its normal, whitecap and the horizontal residual
struct SurfaceSample { Vector3 position, normal; float white = 0.f, residual = 0.f; };
static_assert(sizeof(SurfaceSample) == 32, "[n][8] floats of mw_ocean_query_surface");
// xz: horizontal points {x, z} (Vector2 x = x, y = z); world = true: points on the displaced surface (buoyancy), false: rest positions
inline void query_surface(mw_ocean* o, int32_t frame, const std::vector<Vector2>& xz, std::vector<SurfaceSample>& out, bool world,
                          int32_t iterations) {
    out.resize(xz.size());
    check(mw_ocean_query_surface(o, frame, world ? MW_QUERY_WORLD : MW_QUERY_REST, xz.empty() ? nullptr : &xz[0].x, (int64_t)xz.size(),
                                 iterations, out.empty() ? nullptr : &out[0].position.x));
}

// one answer of mw_ocean_query_velocity: the water's velocity at the point mw_ocean_query_surface locates, and the same residual
struct VelocitySample { Vector3 velocity; float residual = 0.f; };
static_assert(sizeof(VelocitySample) == 16, "[n][4] floats of mw_ocean_query_velocity");
inline void query_velocity(mw_ocean* o, int32_t frame, const std::vector<Vector2>& xz, std::vector<VelocitySample>& out, bool world,
                           int32_t iterations) {
    out.resize(xz.size());
    check(mw_ocean_query_velocity(o, frame, world ? MW_QUERY_WORLD : MW_QUERY_REST, xz.empty() ? nullptr : &xz[0].x, (int64_t)xz.size(),
                                  iterations, out.empty() ? nullptr : &out[0].velocity.x));
}

// mw_ocean_query_column: a point in the water (or a particle's label (x0, rest depth, z0)) and its answer
struct ColumnPoint { Vector3 point; float unused = 0.f; };
static_assert(sizeof(ColumnPoint) == 16, "[n][4] floats of mw_ocean_query_column");
struct ColumnSample { Vector3 velocity; float restDepth = 0.f; Vector3 position; float lambda = 0.f; float x0 = 0.f, z0 = 0.f, eta = 0.f, residual = 0.f; };
static_assert(sizeof(ColumnSample) == 48, "[n][12] floats of mw_ocean_query_column");

// mw_ocean_raycast: one ray (t in units of direction; a segment p0 -> p1 is {p0, 0, p1 - p0, 1}) and its first hit on the surface
// (t = +inf on a miss, NaN for an invalid ray); facing +1: the ray met the water from above, -1: from below; triangle -1: no hit
struct Ray { Vector3 origin; float tmin = 0.f; Vector3 direction; float tmax = std::numeric_limits<float>::infinity(); };
static_assert(sizeof(Ray) == 32, "[n][8] floats of mw_ocean_raycast");
struct RayHit { float t = 0.f; Vector3 point, normal; float white = 0.f; };
static_assert(sizeof(RayHit) == 32, "[n][8] floats of mw_ocean_raycast");
struct RayHitId { int32_t triangle = -1, facing = 0; };
inline void raycast(mw_ocean* o, int32_t frame, const std::vector<Ray>& rays, std::vector<RayHit>& out, std::vector<RayHitId>* ids) {
    out.resize(rays.size());
    if (ids) ids->resize(rays.size());
    check(mw_ocean_raycast(o, frame, rays.empty() ? nullptr : &rays[0].origin.x, (int64_t)rays.size(), out.empty() ? nullptr : &out[0].t,
                           ids && !ids->empty() ? &(*ids)[0].triangle : nullptr));
}

// mw_ocean_hull_forces: one body (64 B: reference point, rotation quaternion, velocity, angular velocity, in the ocean's object space)
// and one answer (force, wetted area, torque about the reference point, residual)
struct HullBody { Vector3 position; float pad0 = 0.f; float qx = 0.f, qy = 0.f, qz = 0.f, qw = 1.f; Vector3 velocity; float pad1 = 0.f;
                  Vector3 angularVelocity; float pad2 = 0.f; };
static_assert(sizeof(HullBody) == 64, "[nbodies][16] floats of mw_ocean_hull_forces");
struct HullForce { Vector3 force; float wettedArea = 0.f; Vector3 torque; float residual = 0.f; };
static_assert(sizeof(HullForce) == 32, "[nbodies][8] floats of mw_ocean_hull_forces");
// hull: body-space vertices and triangles ((b - a) x (c - a) pointing out), shared by all bodies
inline void hull_forces(mw_ocean* o, int32_t frame, const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles,
                        const std::vector<HullBody>& bodies, std::vector<HullForce>& out, float density, float gravity, float linearDrag,
                        float quadraticDrag, float velocityScale) {
    out.resize(bodies.size());
    const float coeffs[MW_HULL_NCOEFFS] = {density, gravity, linearDrag, quadraticDrag, velocityScale};
    check(mw_ocean_hull_forces(o, frame, hull.empty() ? nullptr : &hull[0].x, (int32_t)hull.size(), triangles.empty() ? nullptr : &triangles[0],
                               (int32_t)(triangles.size() / 3), bodies.empty() ? nullptr : &bodies[0].position.x, (int32_t)bodies.size(),
                               coeffs, 0, out.empty() ? nullptr : &out[0].force.x));
}

// mw_hull_mass_properties: mass, centroid and inertia tensor entries (Ixx Iyy Izz Ixy Ixz Iyz, about the centroid) of a closed hull
struct MassProperties { float mass = 0.f; Vector3 centroid; float inertia[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; };
inline MassProperties hull_mass_properties(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, float density) {
    float o[10];
    check(mw_hull_mass_properties(hull.empty() ? nullptr : &hull[0].x, (int32_t)hull.size(), triangles.empty() ? nullptr : &triangles[0],
                                  (int32_t)(triangles.size() / 3), density, o));
    MassProperties r;
    r.mass = o[0];
    r.centroid = {o[1], o[2], o[3]};
    for (int k = 0; k < 6; k++) r.inertia[k] = o[4 + k];
    return r;
}
// mw_ocean_step_bodies: one mass row (m, Ixx Iyy Izz Ixy Ixz Iyz about the centre of mass, body axes)
struct BodyMass { float mass = 1.f; float inertia[6] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f}; float pad = 0.f; };
static_assert(sizeof(BodyMass) == MW_BODY_NMASS * sizeof(float), "[nbodies][MW_BODY_NMASS] floats of mw_ocean_step_bodies");
inline BodyMass body_mass(const MassProperties& p) {
    BodyMass m;
    m.mass = p.mass;
    for (int k = 0; k < 6; k++) m.inertia[k] = p.inertia[k];
    return m;
}
// bodies advanced in place by dt in `substeps` substeps on the frozen surface of `frame`; forces (optional) gets the last substep's rows
inline void step_bodies(mw_ocean* o, int32_t frame, const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles,
                        std::vector<HullBody>& bodies, const std::vector<BodyMass>& mass, float dt, int32_t substeps, float density,
                        float gravity, float linearDrag, float quadraticDrag, float velocityScale, std::vector<HullForce>* forces) {
    if (forces) forces->resize(bodies.size());
    const float coeffs[MW_HULL_NCOEFFS] = {density, gravity, linearDrag, quadraticDrag, velocityScale};
    check(mw_ocean_step_bodies(o, frame, hull.empty() ? nullptr : &hull[0].x, (int32_t)hull.size(), triangles.empty() ? nullptr : &triangles[0],
                               (int32_t)(triangles.size() / 3), bodies.empty() ? nullptr : &bodies[0].position.x,
                               mass.empty() ? nullptr : &mass[0].mass, (int32_t)bodies.size(), coeffs, dt, substeps, 0,
                               forces && !forces->empty() ? &(*forces)[0].force.x : nullptr));
}

// mw_ocean_step_moored: one slot of a body's lines -- from `attach` (body space, about the centre of mass) to the fixed `anchor` (world)
struct MooringLine {
    Vector3 attach; float restLength = 0.f;
    Vector3 anchor; float stiffness = 0.f;  // stiffness == 0 and damping == 0: an empty slot
    float damping = 0.f; float pad[3] = {0.f, 0.f, 0.f};
};
static_assert(sizeof(MooringLine) == MW_MOORING_NLINE * sizeof(float), "[nbodies][K][MW_MOORING_NLINE] floats of mw_ocean_step_moored");
// step_bodies with lines [nbodies * linesPerBody], body after body; tension (optional) gets each slot's pull at the start of the last substep
inline void step_moored(mw_ocean* o, int32_t frame, const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles,
                        std::vector<HullBody>& bodies, const std::vector<BodyMass>& mass, const std::vector<MooringLine>& lines,
                        int32_t linesPerBody, float dt, int32_t substeps, float density, float gravity, float linearDrag, float quadraticDrag,
                        float velocityScale, std::vector<HullForce>* forces, std::vector<float>* tension) {
    if (forces) forces->resize(bodies.size());
    if (tension) tension->resize(lines.size());
    const float coeffs[MW_HULL_NCOEFFS] = {density, gravity, linearDrag, quadraticDrag, velocityScale};
    check(mw_ocean_step_moored(o, frame, hull.empty() ? nullptr : &hull[0].x, (int32_t)hull.size(), triangles.empty() ? nullptr : &triangles[0],
                               (int32_t)(triangles.size() / 3), bodies.empty() ? nullptr : &bodies[0].position.x,
                               mass.empty() ? nullptr : &mass[0].mass, lines.empty() ? nullptr : &lines[0].attach.x, linesPerBody,
                               (int32_t)bodies.size(), coeffs, dt, substeps, 0, forces && !forces->empty() ? &(*forces)[0].force.x : nullptr,
                               tension && !tension->empty() ? tension->data() : nullptr));
}

class FFTMesh {
public:
    // ---- public Inspector fields, S/FFTMesh.cs:9-23 -------------------------------------------------
    float choppiness = 1.f;
    float tDivision = 1.f;
    int resolution = 50;
    float unitWidth = 1.f;
    bool generate = false;
    float length = 1.f;
    Vector2 wind{1.f, 1.f};
    float amplitude = 1.f;
    // ---- additions: the constants the reference hard-codes, and what Unity supplies implicitly --------
    float gravity = 9.81f;  // G, S/FFTMesh.cs:52
    uint64_t seed = 1;      // the reference never seeds UnityEngine.Random
    bool fixedSeed = false; // true: every regeneration reproduces the same sea (tests); false: a new one, like GenerateMesh
    int device = 0;
    Mesh mesh;

    ~FFTMesh() { mw_ocean_destroy(ocean_); }

    void Awake() {  // S/FFTMesh.cs:75-84
        SetParamsAndGenerateMesh();
    }
    void Update(float deltaTime) {  // S/FFTMesh.cs:60-73
        if (generate) {
            timer_ = 0.f;
            SetParamsAndGenerateMesh();
            generate = false;
        }
        timer_ += deltaTime / tDivision;
        EvaluateWaves(timer_);
    }
    void EvaluateWaves(float t) {  // S/FFTMesh.cs:224-280
        check(mw_ocean_set_choppiness(ocean_, choppiness));
        check(mw_ocean_evaluate(ocean_, t, &mesh.vertices[0].x, &mesh.normals[0].x, &mesh.colors[0].r));
    }
    // Not in the reference: the surface services read the infinite tiling of the frame (include/mistral_water.h, the periodic surface);
    // throws unless unitWidth * resolution == length with an even resolution
    void SetPeriodic(bool on = true) { check(mw_ocean_set_periodic(ocean_, on ? 1 : 0)); }
    // Not in the reference: the surface of the latest EvaluateWaves() at horizontal points (include/mistral_water.h, surface queries)
    void QuerySurface(const std::vector<Vector2>& xz, std::vector<SurfaceSample>& out, bool world = true, int32_t iterations = 0) {
        query_surface(ocean_, -1, xz, out, world, iterations);
    }
    // Not in the reference: the velocity of every vertex of the latest frame, per second of Update's deltaTime (the library's value is
    // per unit of t, and Update advances t by deltaTime / tDivision)
    void Velocity(std::vector<Vector3>& out) {
        out.resize((size_t)resolution * resolution);
        check(mw_ocean_velocity(ocean_, -1, &out[0].x));
        for (auto& v : out) { v.x /= tDivision; v.y /= tDivision; v.z /= tDivision; }
    }
    // ... and at horizontal points, located as QuerySurface locates them (per second, as Velocity)
    void QueryVelocity(const std::vector<Vector2>& xz, std::vector<VelocitySample>& out, bool world = true, int32_t iterations = 0) {
        query_velocity(ocean_, -1, xz, out, world, iterations);
        for (auto& s : out) { s.velocity.x /= tDivision; s.velocity.y /= tDivision; s.velocity.z /= tDivision; }
    }
    // Not in the reference: the water below the surface of the latest EvaluateWaves() at points in the water (world) or particle labels
    // (x0, rest depth, z0); SetColumn names the layers' rest depths (depths[0] == 0, strictly increasing, 2 to 16; empty releases them).
    // Velocity per second, as Velocity
    void SetColumn(const std::vector<float>& depths) { check(mw_ocean_set_column(ocean_, depths.empty() ? nullptr : depths.data(), (int32_t)depths.size())); }
    void SampleColumn(const std::vector<ColumnPoint>& xyz, std::vector<ColumnSample>& out, bool world = true, int32_t iterations = 0) {
        out.resize(xyz.size());
        check(mw_ocean_query_column(ocean_, -1, world ? MW_QUERY_WORLD : MW_QUERY_REST, xyz.empty() ? nullptr : &xyz[0].point.x, (int64_t)xyz.size(),
                                    iterations, out.empty() ? nullptr : &out[0].velocity.x));
        for (auto& s : out) { s.velocity.x /= tDivision; s.velocity.y /= tDivision; s.velocity.z /= tDivision; }
    }
    // Not in the reference: HullForces and StepBodies read the column (SetColumn) under every hull vertex instead of the surface above it:
    // the pressure at the vertex's rest depth, the water's velocity down there (include/mistral_water.h, draught)
    void SetDraught(bool on = true) { check(mw_ocean_set_draught(ocean_, on ? 1 : 0)); }
    // Not in the reference: the first hit of rays on the surface of the latest EvaluateWaves() (mouse picking, projectile segments, ...)
    void Raycast(const std::vector<Ray>& rays, std::vector<RayHit>& out, std::vector<RayHitId>* ids = nullptr) {
        raycast(ocean_, -1, rays, out, ids);
    }
    // Not in the reference: buoyancy and drag on bodies sharing one hull, from the latest EvaluateWaves() (drag uses the water's
    // velocity per second of Update's deltaTime: the library's value over tDivision)
    void HullForces(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, const std::vector<HullBody>& bodies,
                    std::vector<HullForce>& out, float density = 1000.f, float gravity = 9.81f, float linearDrag = 0.f,
                    float quadraticDrag = 0.f) {
        hull_forces(ocean_, -1, hull, triangles, bodies, out, density, gravity, linearDrag, quadraticDrag, 1.f / tDivision);
    }
    // Not in the reference: advance bodies sharing one hull (about their centres of mass) by deltaTime seconds on the surface of the
    // latest EvaluateWaves(), in `substeps` substeps on the device
    void StepBodies(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, std::vector<HullBody>& bodies,
                    const std::vector<BodyMass>& mass, float deltaTime, int32_t substeps = 1, float density = 1000.f, float gravity = 9.81f,
                    float linearDrag = 0.f, float quadraticDrag = 0.f, std::vector<HullForce>* forces = nullptr) {
        step_bodies(ocean_, -1, hull, triangles, bodies, mass, deltaTime, substeps, density, gravity, linearDrag, quadraticDrag,
                    1.f / tDivision, forces);
    }
    // Not in the reference: StepBodies with mooring lines, linesPerBody slots per body (lines [bodies.size() * linesPerBody])
    void StepMoored(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, std::vector<HullBody>& bodies,
                    const std::vector<BodyMass>& mass, const std::vector<MooringLine>& lines, int32_t linesPerBody, float deltaTime,
                    int32_t substeps = 1, float density = 1000.f, float gravity = 9.81f, float linearDrag = 0.f, float quadraticDrag = 0.f,
                    std::vector<HullForce>* forces = nullptr, std::vector<float>* tension = nullptr) {
        step_moored(ocean_, -1, hull, triangles, bodies, mass, lines, linesPerBody, deltaTime, substeps, density, gravity, linearDrag,
                    quadraticDrag, 1.f / tDivision, forces, tension);
    }
    float timer() const { return timer_; }
    mw_ocean* handle() { return ocean_; }

private:
    void SetParamsAndGenerateMesh() {  // S/FFTMesh.cs:90-139
        mw_ocean_destroy(ocean_);
        ocean_ = nullptr;
        mw_params p;
        mw_params_default(&p, MW_SEM_FFTMESH);
        p.resolution = resolution; p.unit_width = unitWidth; p.length = length; p.wind_x = wind.x; p.wind_y = wind.y;
        p.amplitude = amplitude; p.choppiness = choppiness; p.gravity = gravity; p.t_division = tDivision;
        // GenerateMesh draws fresh UnityEngine.Random values every time it runs (S/FFTMesh.cs:114-116): each regeneration
        // is a NEW sea state unless fixedSeed asks for reproducibility
        p.seed = fixedSeed ? seed : seed + generation_;
        generation_++;
        p.device = device;
        check(mw_ocean_create(&p, &ocean_));
        const size_t nn = (size_t)resolution * resolution;
        mesh.vertices.resize(nn); mesh.normals.resize(nn); mesh.uv.resize(nn); mesh.colors.resize(nn);
        mesh.indices.resize((size_t)mw_ocean_index_count(ocean_));
        check(mw_ocean_rest_mesh(ocean_, &mesh.vertices[0].x, &mesh.normals[0].x, &mesh.uv[0].x, mesh.indices.data()));
    }
    mw_ocean* ocean_ = nullptr;
    float timer_ = 0.f;
    uint64_t generation_ = 0;
};

class OceanRenderer {
public:
    // ---- public Inspector fields, S/OceanRenderer.cs:10-19 -------------------------------------------
    float mult = 2.f;
    float unitWidth = 1.f;
    int resolution = 256;
    float length = 256.f;
    float choppiness = 1.5f;
    float amplitude = 1.f;
    Vector2 wind;
    float gravity = 9.81f;
    uint64_t seed = 1;
    int device = 0;
    Mesh mesh;
    // the four result textures bound to the ocean material (S/OceanRenderer.cs:310-313), M = 8*resolution
    std::vector<float> heightTexture, displacementTexture, normalTexture, whiteTexture;

    ~OceanRenderer() { mw_ocean_destroy(ocean_); }

    void Awake() {  // S/OceanRenderer.cs:76-89: SetParams, GenerateMesh, RenderInitial
        Create();
        const size_t nn = (size_t)resolution * resolution;
        mesh.vertices.resize(nn); mesh.normals.resize(nn); mesh.uv.resize(nn);
        mesh.indices.resize((size_t)mw_ocean_index_count(ocean_));
        check(mw_ocean_rest_mesh(ocean_, &mesh.vertices[0].x, &mesh.normals[0].x, &mesh.uv[0].x, mesh.indices.data()));
    }
    void Update(float deltaTime) {  // S/OceanRenderer.cs:91-110
        GenerateTexture(deltaTime);                            // with the values the materials carried into this frame (:93)
        check(mw_ocean_set_choppiness(ocean_, choppiness));    // spectrumMat._Choppiness for the NEXT frame (:96)
        if (oldLength_ != length || oldWind_.x != wind.x || oldWind_.y != wind.y || oldAmplitude_ != amplitude) {
            // RenderInitial again with the same seeds (:98-109): the phase textures keep running
            check(mw_ocean_reinit_spectrum(ocean_, length, wind.x, wind.y, amplitude, seed));
            oldLength_ = length; oldWind_ = wind; oldAmplitude_ = amplitude;
        }
    }
    void GenerateTexture(float deltaTime) {  // S/OceanRenderer.cs:216-316
        const size_t mm = (size_t)M_ * M_;
        heightTexture.resize(mm); displacementTexture.resize(2 * mm); normalTexture.resize(3 * mm); whiteTexture.resize(mm);
        check(mw_ocean_generate_texture(ocean_, deltaTime, heightTexture.data(), displacementTexture.data(),
                                        normalTexture.data(), whiteTexture.data()));
    }
    // The same frame as the four ARGBFloat render targets in the shaders' channel layout (S/OceanRenderer.cs:143-146):
    // what oceanMat.SetTexture("_Height"/"_Anim"/"_Bump"/"_White") binds (:310-313).  4 floats per texel each.
    void GenerateTextureRGBA(float deltaTime, std::vector<float>& height, std::vector<float>& anim, std::vector<float>& bump,
                             std::vector<float>& white) {
        const size_t mm = (size_t)M_ * M_ * 4;
        height.resize(mm); anim.resize(mm); bump.resize(mm); white.resize(mm);
        check(mw_ocean_generate_texture_rgba(ocean_, deltaTime, height.data(), anim.data(), bump.data(), white.data()));
    }
    // The ocean material's vertex stage (W/TestOcean.shader:61-79) applied to `mesh` from the latest frame's textures:
    // displaced vertices, per-vertex normals and foam factor, for a consumer that does not bind textures.
    void DisplaceMesh(std::vector<Vector3>& vertices, std::vector<Vector3>& normals, std::vector<float>& foam) {
        const size_t nn = (size_t)resolution * resolution;
        vertices.resize(nn); normals.resize(nn); foam.resize(nn);
        check(mw_ocean_displace_mesh(ocean_, &vertices[0].x, &normals[0].x, foam.data()));
    }
    // Not in the reference: the surface DisplaceMesh() describes (frame -1) or frame k of the latest steps call, at horizontal points
    void QuerySurface(const std::vector<Vector2>& xz, std::vector<SurfaceSample>& out, bool world = true, int32_t frame = -1,
                      int32_t iterations = 0) {
        query_surface(ocean_, frame, xz, out, world, iterations);
    }
    // Not in the reference: the water's velocity per second of delta_time at the handle's current phase (frame -1)
    void Velocity(std::vector<Vector3>& out) {
        out.resize((size_t)resolution * resolution);
        check(mw_ocean_velocity(ocean_, -1, &out[0].x));
    }
    void QueryVelocity(const std::vector<Vector2>& xz, std::vector<VelocitySample>& out, bool world = true, int32_t iterations = 0) {
        query_velocity(ocean_, -1, xz, out, world, iterations);
    }
    // Not in the reference: the first hit of rays on the surface DisplaceMesh() describes (frame -1) or frame k of the latest steps call
    void Raycast(const std::vector<Ray>& rays, std::vector<RayHit>& out, std::vector<RayHitId>* ids = nullptr, int32_t frame = -1) {
        raycast(ocean_, frame, rays, out, ids);
    }
    // Not in the reference: buoyancy and drag on bodies sharing one hull, from the surface DisplaceMesh() describes (frame -1) or
    // frame k of the latest steps call (drag on: frame -1 or the last one)
    void HullForces(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, const std::vector<HullBody>& bodies,
                    std::vector<HullForce>& out, float density = 1000.f, float gravity = 9.81f, float linearDrag = 0.f,
                    float quadraticDrag = 0.f, int32_t frame = -1) {
        hull_forces(ocean_, frame, hull, triangles, bodies, out, density, gravity, linearDrag, quadraticDrag, 1.f);
    }
    // Not in the reference: advance bodies sharing one hull (about their centres of mass) by deltaTime seconds on the surface
    // DisplaceMesh() describes (frame -1) or frame k of the latest steps call, in `substeps` substeps on the device
    void StepBodies(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, std::vector<HullBody>& bodies,
                    const std::vector<BodyMass>& mass, float deltaTime, int32_t substeps = 1, float density = 1000.f, float gravity = 9.81f,
                    float linearDrag = 0.f, float quadraticDrag = 0.f, std::vector<HullForce>* forces = nullptr, int32_t frame = -1) {
        step_bodies(ocean_, frame, hull, triangles, bodies, mass, deltaTime, substeps, density, gravity, linearDrag, quadraticDrag, 1.f,
                    forces);
    }
    // Not in the reference: StepBodies with mooring lines, linesPerBody slots per body (lines [bodies.size() * linesPerBody])
    void StepMoored(const std::vector<Vector3>& hull, const std::vector<int32_t>& triangles, std::vector<HullBody>& bodies,
                    const std::vector<BodyMass>& mass, const std::vector<MooringLine>& lines, int32_t linesPerBody, float deltaTime,
                    int32_t substeps = 1, float density = 1000.f, float gravity = 9.81f, float linearDrag = 0.f, float quadraticDrag = 0.f,
                    std::vector<HullForce>* forces = nullptr, std::vector<float>* tension = nullptr, int32_t frame = -1) {
        step_moored(ocean_, frame, hull, triangles, bodies, mass, lines, linesPerBody, deltaTime, substeps, density, gravity, linearDrag,
                    quadraticDrag, 1.f, forces, tension);
    }

private:
    void Create() {
        mw_ocean_destroy(ocean_);
        ocean_ = nullptr;
        mw_params p;
        mw_params_default(&p, MW_SEM_OCEANRENDERER);
        p.resolution = resolution; p.unit_width = unitWidth; p.length = length; p.wind_x = wind.x; p.wind_y = wind.y;
        p.amplitude = amplitude; p.choppiness = choppiness; p.gravity = gravity; p.mult = mult; p.seed = seed;
        p.device = device;
        check(mw_ocean_create(&p, &ocean_));
        M_ = mw_ocean_grid_size(ocean_);
        oldLength_ = length; oldWind_ = wind; oldAmplitude_ = amplitude;
    }
    mw_ocean* ocean_ = nullptr;
    int M_ = 0;
    float oldLength_ = 0.f, oldAmplitude_ = 0.f;
    Vector2 oldWind_;
};

// The pond material's displacement properties (W/MistralWaterLib.cginc:53-66) and its vertex-stage Displacement()
// (:154-180) in the three modes of the shader library.
class PondMaterial {
public:
    int mode = MW_POND_GERSTNER;   // _DISPLACEMENTMODE_*: MW_POND_WAVE / MW_POND_GERSTNER / MW_POND_GERSTNER_LEVEL_ONE
    float _Amplitude = 10.f, _Frequency = 2.58f, _Speed = 0.f, _Steepness = 0.99f, _Smoothing = 1.f;  // M/Pond Water Mat.mat
    float _WSpeed[4] = {1.2f, 0.71f, 1.1f, 0.73f};
    float _WDirectionAB[4] = {0.3f, 0.73f, 0.85f, 0.25f};
    float _WDirectionCD[4] = {-0.25f, 1.11f, 0.5f, 0.5f};
    int device = 0;

    // time = _Time.y; normals may be null
    void Displacement(const std::vector<Vector3>& in, float time, std::vector<Vector3>& out, std::vector<Vector3>* normals) const {
        mw_pond_params p;
        p.mode = mode; p.amplitude = _Amplitude; p.frequency = _Frequency; p.speed = _Speed; p.steepness = _Steepness;
        p.smoothing = _Smoothing;
        for (int i = 0; i < 4; i++) { p.wspeed[i] = _WSpeed[i]; p.dir_ab[i] = _WDirectionAB[i]; p.dir_cd[i] = _WDirectionCD[i]; }
        out.resize(in.size());
        if (normals) normals->resize(in.size());
        if (in.empty()) return;
        check(mw_pond_displace(&p, &in[0].x, (int64_t)in.size(), time, &out[0].x, normals ? &(*normals)[0].x : nullptr, device));
    }
};

}  // namespace mistral_water
