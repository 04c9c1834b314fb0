// made_fwd_train_ft.hip -- nf_made_forward_train_ft: MADE.forward under autograd for the autoregressive spline layers whose mask is
// permuted and / or whose circular coordinates pass the periodic preprocessing first (nets/made.py:250-252, 296-304 over
// utils/nn.py:64-129 inside core.py:87-102): made_fwd.hip's EPI-3 training forward behind the x-tile load of made_fwd_ft.hip
// (the body text of made_fwd_body.hpp with FT set).  64-ROW TILES ONLY, whatever mf_tr128() says: the 128-row instantiation of EPI 3 has no register left for
// the feed (it spills 8 values without it), so this path's chain runs on 64-row tiles too (nf_made_backward_t64, made_bwd.hip) -- the
// `bits` layout depends on the tile height.  No scratch memory in either instantiation (tests/test_host_arnsf_train_ft.py).
#include "mlp_tile.hpp"

namespace nf {

template <int NSB>
__global__ void __launch_bounds__(64 * MF_NW, 1)
made_fwd_train_ft_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                         const int *__restrict__ table, int64_t B, float *__restrict__ save, unsigned *__restrict__ bits, int64_t Bp,
                         float *__restrict__ x_pad) {
    // y = params (B, mult D) in position order; logdet = x_pos (B, D): EPI 3 has no log-det, the body's FT tile load writes there
    constexpr int EPI = 3, TR = MF_ROWS;
    constexpr bool FT = true;
    constexpr int direction = 0;             // (EPI 4 only: affine_wide.hip)
    const int acc_mode = NF_LD_WRITE;
    const RqsParams<float> p{};
#include "made_fwd_body.hpp"
}

template <int NSB>
static int made_fwd_train_ft_launch(const void *x, void *params, void *x_pos, const void *blob, const int32_t *table, int64_t B, void *save,
                                    void *bits, void *x_pad, hipStream_t st) {
    const int64_t ntiles = (B + MF_ROWS - 1) / MF_ROWS;
    const int grid = persistent_grid(ntiles);        // persistent: one workgroup per CU
    const size_t lds = sizeof(float) * ((size_t)8 * NSB * 4 * 8 * MF_ROWS + MF_XFLOATS);
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&made_fwd_train_ft_kernel<NSB>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((made_fwd_train_ft_kernel<NSB>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x, (float *)params,
                       (float *)x_pos, (const float *)blob, (const int *)table, B, (float *)save, (unsigned *)bits, ntiles * MF_ROWS,
                       (float *)x_pad);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

// include/nf_mi355x.h.  x_pad: Bp rows of 128 floats (D <= 128), Bp = B rounded up to 64.
extern "C" int nf_made_forward_train_ft(const void *x, void *params, void *save, void *bits, void *x_pad, void *x_pos, const void *blob,
                                        const int32_t *table, int64_t B, int D, int hidden_padded, int mult, nf_stream_t stream) {
    if (B < 0 || D < 2 || D > 128 || mult < 1) return NF_EINVAL;
    if (hidden_padded != 256 && hidden_padded != 512) return NF_ENOTSUP;
    if (B == 0) return NF_OK;
    if (!x || !params || !save || !bits || !x_pad || !x_pos || !blob || !table) return NF_EFAULT;
    if (nf_misaligned16(params, save, x_pad)) return NF_EINVAL;       // written with 16-byte stores (x and x_pos: element by element)
    hipStream_t st = (hipStream_t)stream;
    if (hidden_padded == 256) return nf::made_fwd_train_ft_launch<1>(x, params, x_pos, blob, table, B, save, bits, x_pad, st);
    return nf::made_fwd_train_ft_launch<2>(x, params, x_pos, blob, table, B, save, bits, x_pad, st);
}
