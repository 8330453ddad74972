/*
 * mistral_water_hooks.h -- measurement and test hooks of libmistral_water.so.
 *
 * NOT part of the drop-in boundary (include/mistral_water.h): a host integration never calls these and the C# import table
 * (bindings/csharp/MistralWaterNative.cs) does not carry them.  bench.py uses the measurement hook, tests/ use the rest
 * to compare intermediate quantities of the kernels (omega*t, hds, the device sincos) with the oracle bit for bit.
 * mw_debug_raycast_tree returns the raycasts' device-built hierarchy, which tests/ compare box for box with the serial build.
 * mw_debug_query_mesh runs the footprint surface and velocity query kernels on a caller's mesh.
 */
#ifndef MISTRAL_WATER_HOOKS_H
#define MISTRAL_WATER_HOOKS_H

#include "mistral_water.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement hook (bench.py): times each kernel of one FFTMesh step with hipEvents on the
 * handle's stream.  ms_out[k] = mean duration of kernel k over iters launches of `nsteps` batched
 * time-steps; names_out[k] = static kernel name.  Returns the kernel count through *nkernels.      */
mw_status mw_ocean_profile_kernels(mw_ocean* o, int32_t nsteps, int32_t iters, float* ms_out, const char** names_out,
                                   int32_t* nkernels);

/* the same measurement as a distribution: stats_out[6 k + 0..5] = mean, median, p10, p90, min, max of kernel k's `iters` launch
 * durations in milliseconds (bench.py prints the median beside the mean so that roofline.frac can be recomputed from a
 * rocprofv3 kernel trace of the same command, profiles/<round>_*_kernel_pcts.json)                                          */
mw_status mw_ocean_profile_kernels_stats(mw_ocean* o, int32_t nsteps, int32_t iters, float* stats_out, const char** names_out,
                                         int32_t* nkernels);

/* time-steps of one pass-1 column job kept on one XCD when an enqueue carries nsteps time-steps (0 = plain grid) */
int32_t mw_debug_pass1_time_group(mw_ocean* o, int32_t nsteps);

/* ---- test hooks (used by tests/ only; not needed by a host integration) ---------------------------------
 * mw_debug_omega_t: omega(i,j)*t [N*N, idx = i*N + j] exactly as the kernels form it -- the quantised dispersion
 * (S/FFTMesh.cs:146,183) is compared bit for bit with the oracle.  mw_debug_get_omega: the stored table in its
 * transposed [j][i] layout.  mw_debug_sincos: the library's range-reduced sin/cos on n host floats.            */
mw_status mw_debug_omega_t(mw_ocean* o, float t, float* out_host);
/* one EvaluateWaves(t) that also returns hds [N*N*2] = (d.x, d.z) of S/FFTMesh.cs:247 as the kernels hold it: the whitecap
 * stage (forward differences, edge rules :258-274, halo rows between workgroups) is then checked bit for bit           */
mw_status mw_debug_evaluate_hds(mw_ocean* o, float t, float* vertices_xyz, float* normals_xyz, float* colors_rgba, float* hds_xy);
mw_status mw_debug_get_omega(mw_ocean* o, float* out_host);
mw_status mw_debug_sincos(const float* x_host, int32_t n, float* s_host, float* c_host);
/* the pond kernels' hardware-sine variant (v_sin_f32 / v_cos_f32 after an exact revolution count) */
mw_status mw_debug_sincos_fast(const float* x_host, int32_t n, float* s_host, float* c_host);
/* one wave applies the in-wave exchange of the 1024-point transform (v_permlane16_swap / v_permlane32_swap: the wave's four 16-lane rows
 * <-> the low two bits of the slot index) to inout_host [64 lanes][16 slots][2]: the instructions are checked against the index map the
 * host emulation uses (index work: bit for bit)                                                                                      */
mw_status mw_debug_wave_transpose4(float* inout_host);
/* The library's run-time plan switches (csrc/mw_switches.h: MW_P1_TGROUP, MW_CZT_ONE, MW_CZT_FUSED, MW_DIRECT_CZT, MW_TILES_FORCE_RCCL,
 * MW_OR_PACKED).  Every alternative plan gives the same bits as
 * the default (MW_OR_PACKED = 0, the OceanRenderer's three-transform plan: the same textures to float32 rounding); the tests select them here.  Process-wide; MW_DIRECT_CZT and MW_P1_TGROUP are read when a handle is created, the rest per
 * call.  A product build never reads the environment; MW_EINVAL for an unknown name (get: INT32_MIN).                                 */
mw_status mw_debug_set_switch(const char* name, int32_t value);
int32_t mw_debug_get_switch(const char* name);
/* streams `bytes` of device memory through `width`-byte per-lane loads (4, 8 or 16): FETCH_SIZE calibration */
mw_status mw_debug_stream_read(int64_t bytes, int32_t width, int32_t iters);
/* The hierarchy a raycast of `frame` would traverse, built by the cast's own launches after the cast's own checks (tiled = 0:
 * mw_ocean_raycast, the footprint; tiled = 1: mw_ocean_raycast_tiled, one tile) with the same statuses.  geom = (B leaf block side in
 * cells, nb leaf blocks per side, D leaf level), filled even when box_host is NULL; the tree has (4^(D+1) - 1) / 3 nodes, level L a
 * 2^L x 2^L grid from node (4^L - 1) / 3, row-major.  box_host [nodes][8] = lo.x lo.y lo.z 0 hi.x hi.y hi.z 0; MW_EINVAL (and nothing
 * written to box_host) when capacity_nodes is below the node count.  The tree buffer is set to 0xFF bytes before the build: a node no
 * kernel wrote comes back NaN.  Waits for the handle's stream.                                                                      */
mw_status mw_debug_raycast_tree(mw_ocean* o, int32_t frame, int32_t tiled, float* box_host, int64_t capacity_nodes, int32_t geom[3]);
/* The footprint queries (mw_ocean_query_surface, mw_ocean_query_velocity) on a caller's mesh, without a handle: host arrays vert and norm
 * [R*R][3], white [R*R][wstride] (wstride 1 or 4, the whitecap in channel 0), vel [R*R][3] or NULL; xz [n][2] -> out [n][8] as
 * mw_ocean_query_surface writes it and, when vel is given, vout [n][4] as mw_ocean_query_velocity writes it.  The arrays are copied to
 * the device, the services' own launches run on them (the same kernels, grid rule and iterations mapping), the rows are copied back.
 * The queries' argument rules with their statuses, and R >= 2, unit_width > 0: MW_EINVAL, before the device is touched.  n == 0
 * returns MW_OK and reads no array.                                                                                              */
mw_status mw_debug_query_mesh(int32_t R, float unit_width, const float* vert, const float* norm, const float* white, int32_t wstride,
                              const float* vel, int32_t mode, int32_t iterations, const float* xz, int64_t n, float* out, float* vout);

#ifdef __cplusplus
}
#endif
#endif /* MISTRAL_WATER_HOOKS_H */
