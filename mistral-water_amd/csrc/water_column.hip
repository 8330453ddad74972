// water_column.hip -- the kernels of the water column (water_column.h): the layer builder's weight kernel and both instantiations of
// the column query, compiled without floating-point contraction.  As in surface_tiled.hip the pragma stands after mw_math.h, which sets
// its own inside its strict helpers, and before the headers whose MW_HD functions the kernels run: the column is the strict float32 the
// g++ build of the same functions computes (tests/column_shim.cpp), on a periodic handle and on the one footprint alike.
#include <hip/hip_runtime.h>

#include "mw_math.h"
#pragma clang fp contract(off)
#define MW_VEL_NO_KERNELS  // velocity_weight alone: the velocity kernels are mistral_water.hip's
#define MW_COL_KERNELS
#include "water_column.h"

namespace mw {

hipError_t column_weight_launch(hipStream_t s, int N, float length, float gravity, float depth, const cf* h0, const cf* h0c, cf* ph0, cf* ph0c,
                                cf* vh0, cf* vh0c) {
    const unsigned nb = (unsigned)(((size_t)N * N + 255) / 256);
    k_column_weight<<<dim3(nb), dim3(256), 0, s>>>(N, length, gravity, depth, h0, h0c, ph0, ph0c, vh0, vh0c);
    return hipGetLastError();
}

hipError_t column_query_launch(hipStream_t s, const SqMesh& m, const ColTable& tb, int mode, int iters, const float4* xyz, int64_t n, float4* out) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (m.period != 0.f) k_query_column<<<grid, block, 0, s>>>(SqTiled{m}, tb, mode, iters, xyz, n, out);
    else k_query_column<<<grid, block, 0, s>>>(m, tb, mode, iters, xyz, n, out);
    return hipGetLastError();
}

}  // namespace mw
