// host_demo.cpp -- drives the C++ FFTMesh mirror for a few frames (needs an MI355X at run time).
#include <cstdio>
#include "FFTMesh.hpp"

int main() {
    using namespace mistral_water;
    try {
        FFTMesh m;
        m.resolution = 256; m.unitWidth = 1.f; m.length = 256.f; m.wind = {14.45f, 12.f}; m.amplitude = 2.4e-7f;
        m.choppiness = 0.46f;
        m.Awake();
        for (int f = 0; f < 3; f++) m.Update(1.f / 60.f);
        double hmax = 0;
        for (auto& v : m.mesh.vertices) hmax = hmax > (v.y < 0 ? -v.y : v.y) ? hmax : (v.y < 0 ? -v.y : v.y);
        std::printf("FFTMesh 256^2: timer = %.9g, max|height| = %.9g, colour[0] = %.9g\n", m.timer(), hmax, m.mesh.colors[0].r);
        std::vector<SurfaceSample> here;
        m.QuerySurface({{0.f, 0.f}, {10.5f, -3.25f}}, here);  // how high is the water at these two points of the displaced surface?
        std::printf("FFTMesh 256^2: water height at (0, 0) = %.6g (residual %.2g)\n", here[0].position.y, here[0].residual);
        std::vector<VelocitySample> flow;
        m.QueryVelocity({{0.f, 0.f}}, flow);  // and how fast does it move there (per second)?
        std::printf("FFTMesh 256^2: water velocity at (0, 0) = (%.6g, %.6g, %.6g)\n", flow[0].velocity.x, flow[0].velocity.y, flow[0].velocity.z);
        // and what does it do to a 2 x 1 x 4 crate floating at (0, 0, 0), moving at 1 m/s along x?
        std::vector<Vector3> crate;
        for (int k = 0; k < 8; k++) crate.push_back({k & 4 ? 1.f : -1.f, k & 2 ? 0.5f : -0.5f, k & 1 ? 2.f : -2.f});
        const std::vector<int32_t> faces = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
        std::vector<HullBody> crates(1);
        crates[0].velocity = {1.f, 0.f, 0.f};
        std::vector<HullForce> push;
        m.HullForces(crate, faces, crates, push, 1000.f, 9.81f, 10.f, 50.f);
        std::printf("FFTMesh 256^2: force on the crate = (%.6g, %.6g, %.6g), wetted area %.4g\n", push[0].force.x, push[0].force.y,
                    push[0].force.z, push[0].wettedArea);
        OceanRenderer r;
        r.resolution = 16; r.length = 60.f; r.amplitude = 0.41f; r.choppiness = 0.46f; r.mult = 1.5f; r.wind = {14.45f, 12.f};
        r.Awake();
        r.Update(1.f / 60.f);
        std::vector<float> H, A, B, W;
        r.GenerateTextureRGBA(1.f / 60.f, H, A, B, W);
        std::vector<Vector3> dv, dn;
        std::vector<float> foam;
        r.DisplaceMesh(dv, dn, foam);
        r.QuerySurface({{1.f, 2.f}}, here);
        std::printf("OceanRenderer: water height at (1, 2) = %.6g\n", here[0].position.y);
        std::printf("OceanRenderer 128^2: height.r[0] = %.5f, bump.a[0] = %.1f, vertex[0].y = %.5f\n", H[0], B[3], dv[0].y);
        PondMaterial pond;
        std::vector<Vector3> grid(1000), moved, nrm;
        for (int k = 0; k < 1000; k++) grid[k] = {0.1f * (k % 40), 0.f, 0.1f * (k / 40)};
        pond.Displacement(grid, 2.f, moved, &nrm);
        std::printf("pond Gerstner: vertex[7] = (%.4f, %.4f, %.4f)\n", moved[7].x, moved[7].y, moved[7].z);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
