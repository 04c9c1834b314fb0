// ft_table.hpp -- the per-feature table of the kernels that take tails, bounds and circular coordinates feature by feature
// (maf_inverse.hip's FT variant: nf_arnsf_inverse_ft; nsf_circ.hip: nf_nsf_wide_ft).  Written by flows/maf_pack.py (feature_rows /
// table_from_rows): 8 rows of n 32-bit words, column = the kernel's own feature order (degree order there, tile position order here).
#pragma once

namespace nf {

enum { FT_COL = 0, FT_TAILS, FT_BOUND, FT_SCALE, FT_WSIN, FT_WCOS, FT_BIAS, FT_PERIODIC };

// What the conditioner reads of a feature (nets/made.py:250-252, nets/resnet.py:92-104: every pass starts with the preprocessing): the
// periodic features of utils/nn.py:64-129 for a circular coordinate, the value itself otherwise.  ft: the table with row stride D
// (global memory with wave-uniform addresses in maf_inverse.hip, a copy in LDS in nsf_circ.hip).
// sinf / cosf, not the fast intrinsics: the reference evaluates torch.sin / torch.cos.
__device__ __forceinline__ float ft_feed(const float *__restrict__ ft, int D, int f, float x) {
    if (__float_as_int(ft[FT_PERIODIC * D + f]) == 0) return x;
    const float a = ft[FT_SCALE * D + f] * x;
    return ft[FT_WSIN * D + f] * sinf(a) + ft[FT_WCOS * D + f] * cosf(a) + ft[FT_BIAS * D + f];
}

}  // namespace nf
