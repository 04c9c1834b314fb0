// affine_wide.hip -- nf_affine_wide: a RealNVP coupling layer beyond the chain kernels' shapes (realnvp_chain.hip: d <= 16, widths <= 64)
// as ONE launch at inference -- MaskedAffineFlow(MLP s, MLP t) (affine/coupling.py:209-229) and AffineCouplingBlock(MLP)
// (:117-171, :232-267) over nets/mlp.py:5-58, d <= 128, up to 512 hidden slots.  made_fwd.hip's tile engine (the body text of
// made_fwd_body.hpp under its own kernel name) in plain-MLP mode with the coupling epilogue, EPI 4: the conditioner reads only the
// identity features, which the layer leaves as they are, so BOTH directions are one conditioner pass followed by the element-wise
// map.  The pack (flows/affine_wide_pack.py) stacks the s-net and the t-net into one MLP with a block-diagonal hidden-to-hidden weight
// -- the engine's prefix skipping stops the s row-blocks at the s columns -- and folds the mask into the initial layer's columns.
// Exact-fp32 MFMA, deterministic (fixed-order log-det reduction), no scratch memory (tests/test_host_affine_wide.py).
#include "mlp_tile.hpp"

namespace nf {

template <int NSB>
__global__ void __launch_bounds__(64 * MF_NW, 1)
affine_wide_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                   const int *__restrict__ table, int64_t B, int acc_mode, int direction) {
    constexpr int EPI = 4, TR = MF_ROWS;
    constexpr bool FT = false;
    const RqsParams<float> p{};
    float *const save = nullptr, *const x_pad = nullptr;
    unsigned *const bits = nullptr;
    const int64_t Bp = 0;
#include "made_fwd_body.hpp"
}

template <int NSB>
static int affine_wide_launch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, int64_t B, int direction,
                              int acc, hipStream_t st) {
    const int64_t ntiles = (B + MF_ROWS - 1) / MF_ROWS;
    const int grid = persistent_grid(ntiles);        // persistent: one workgroup per CU
    const size_t lds = sizeof(float) * ((size_t)8 * NSB * 4 * 8 * MF_ROWS + MF_XFLOATS);
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&affine_wide_kernel<NSB>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((affine_wide_kernel<NSB>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x, (float *)y,
                       (float *)logdet, (const float *)blob, (const int *)table, B, acc, direction);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

// include/nf_mi355x.h
extern "C" int nf_affine_wide(const void *z, void *y, void *logdet, const void *blob, const int32_t *table, int64_t B, int D,
                              int hidden_padded, int direction, int acc, nf_stream_t stream) {
    if (B < 0 || D < 2 || D > 128 || (direction != 0 && direction != 1) || acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (hidden_padded != 256 && hidden_padded != 512) return NF_ENOTSUP;
    if (B == 0) return NF_OK;
    if (!z || !y || !logdet || !blob || !table) return NF_EFAULT;
    if ((D & 3) == 0 && nf_misaligned16(z, y)) return NF_EINVAL;        // rows a multiple of 4 floats long move as 16-byte vectors
    hipStream_t st = (hipStream_t)stream;
    if (hidden_padded == 256) return nf::affine_wide_launch<1>(z, y, logdet, blob, table, B, direction, acc, st);
    return nf::affine_wide_launch<2>(z, y, logdet, blob, table, B, direction, acc, st);
}
