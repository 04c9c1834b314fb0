// made_fwd.hip -- ONE pass of MADE (nets/made.py:296-304: initial MaskedLinear, residual blocks :196-214, final MaskedLinear; every
// linear is F.linear(x, weight * mask, bias), :80-81) as ONE launch, with the element-wise affine transform of
// MaskedAffineAutoregressive.forward (flows/affine/autoregressive.py:24-27 -> :101-110) as its epilogue: the single-pass direction
// of MAF (BASELINE configs[4]: 10 layers, d = 128, hidden 512), which round 3 still ran as six library GEMMs + element-wise passes
// per layer.  Exact-fp32 MFMA; bound: the fp32 MFMA rate on the MASKED work (53 % of the dense blocks at config 5).
//
// Geometry (host packer: flows/made_pack.py)
//   * a workgroup of 8 waves owns 64 rows for the WHOLE network; hidden slots = units sorted by degree, Hp = 256 NSB (NSB = 1, 2);
//     every GEMM is transposed, Out^T[units x 64 rows] = W . Act^T, on v_mfma_f32_32x32x2_f32: lane (hh = lane >> 5, n = lane & 31)
//     holds sample n of a 32-sample block; its 16 accumulator registers are output rows 8 q + 4 hh + i of a 32-row block.
//   * the pre-activations live in ACCUMULATOR registers for the whole network (h: the residual stream, t: a block's inner layer:
//     2 x 32 registers per wave and tensor); what the NEXT layer contracts over -- relu(h), relu(t), raw h for the final layer -- is
//     published to LDS in B-operand order act[k / 8][hh][64 samples][4] (one ds_write_b128 per register quad: the natural order of
//     the accumulators IS that order; one ds_read_b128 = the B values of four k-steps), 128 KB at Hp = 512.
//   * work items: NSB = 2: wave w owns hidden row-blocks {w, 15 - w} for both sample blocks; NSB = 1 and the final layer: row-blocks
//     {w, 7 - w}, the first for sample block 0, the second for sample block 1.  With the units sorted by degree row-block rb needs
//     the k-groups [0, nkg(rb)), nkg ~ 4 (rb + 1): the pairing gives every wave the same number of MFMAs (68 k-groups per hidden
//     layer at config 5), so the waves meet at the layer boundaries without waiting.
//   * weights: every WAVE walks one contiguous stream for the whole network (its items in consumption order; per item a bias group
//     of 4 KB, then 1 KB per k-group, lane = its own 16 bytes) through an 8-entry register ring of plain global loads that is
//     requested 8 entries (8 KB) ahead of the MFMAs -- across item, layer and TILE boundaries
//     (the stream ends with a copy of its first 8 entries; the workgroups are persistent over the 64-row tiles): no LDS, no barrier
//     and no start-up bubble for the weights anywhere.  No LDS-DMA in this kernel, so the compiler's own counted vmcnt waits are
//     exact.
//   * two LDS-only barriers per layer boundary (all reads of the old activations done | new ones published).
//   * x tile: 64 rows x Dp features in the same B-operand order (32 KB): B operand of the initial layer and the x of the affine
//     epilogue, which overwrites it in place with z = scale x + shift; the tile leaves with 16-byte stores.
// Algorithmic work per row: 2 (D H + 2 NB H^2 + H mult D) FLOP dense (2.49 MFLOP at config 5), 1.33 MFLOP masked; HBM: 4 D in,
// 4 D + 4 out (affine) resp. 4 mult D out (raw parameters).
#include "mlp_tile.hpp"

namespace nf {

// (the body is the text of made_fwd_body.hpp: made_fwd_train_ft.hip compiles it once more behind a gathered, fed x tile)
template <int NSB, int EPI, int TR = MF_ROWS>
__global__ void __launch_bounds__(64 * MF_NW, 1)
made_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                const int *__restrict__ table, int64_t B, int acc_mode, RqsParams<float> p, float *__restrict__ save,
                unsigned *__restrict__ bits, int64_t Bp) {
    constexpr bool FT = false;
    constexpr int direction = 0;             // (EPI 4 only: affine_wide.hip)
    float *const x_pad = nullptr;
#include "made_fwd_body.hpp"
}

template <int NSB, int EPI, int TR = MF_ROWS>
static int made_fwd_launch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, int64_t B, int acc, hipStream_t st,
                           const RqsParams<float> &p = RqsParams<float>(), void *save = nullptr, void *bits = nullptr, int table_dp = 128) {
    const int64_t ntiles = (B + TR - 1) / TR;
    const int grid = persistent_grid(ntiles);        // persistent: one workgroup per CU (160 KB of LDS at Hp = 512)
    const int xfloats = table_dp > 128 ? 2 * MF_XFLOATS : MF_XFLOATS;       // x tile: 64 rows x Dp (<= 256 next to 256 hidden slots)
    const size_t lds = sizeof(float) * ((size_t)8 * NSB * 4 * 8 * TR + xfloats);       // (TR = 128: 128 rows x Dp <= 64 = the same 32 KB)
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&made_fwd_kernel<NSB, EPI, TR>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((made_fwd_kernel<NSB, EPI, TR>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x, (float *)y,
                       (float *)logdet, (const float *)blob, (const int *)table, B, acc, p, (float *)save, (unsigned *)bits,
                       (B + MF_ROWS - 1) / MF_ROWS * MF_ROWS);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

static int made_fwd_check(int64_t B, int D, int hidden_padded, int mult, int dmax = 128) {
    if (B < 0 || D < 2 || D > dmax || mult < 1) return NF_EINVAL;
    if (hidden_padded != 256 && hidden_padded != 512) return NF_ENOTSUP;
    return NF_OK;
}

// MaskedAffineAutoregressive.forward in one launch (affine/autoregressive.py:24-27, :101-110 over nets/made.py:296-304).
extern "C" int nf_made_forward_affine(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, int64_t B, int D,
                                      int hidden_padded, int acc, nf_stream_t stream) {
    const int rc = made_fwd_check(B, D, hidden_padded, 2);
    if (rc != NF_OK) return rc;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !y || !logdet || !blob || !table) return NF_EFAULT;
    if ((D & 3) == 0 && nf_misaligned16(x, y)) return NF_EINVAL;        // rows a multiple of 4 floats long move as 16-byte vectors
    hipStream_t st = (hipStream_t)stream;
    if (hidden_padded == 256) return nf::made_fwd_launch<1, 0>(x, y, logdet, blob, table, B, acc, st);
    return nf::made_fwd_launch<2, 0>(x, y, logdet, blob, table, B, acc, st);
}

// MADE.forward (nets/made.py:296-304) in one launch: params (B, mult D), rows mult f + p as the reference's final layer orders them.
extern "C" int nf_made_forward(const void *x, void *params, const void *blob, const int32_t *table, int64_t B, int D,
                               int hidden_padded, int mult, nf_stream_t stream) {
    const int rc = made_fwd_check(B, D, hidden_padded, mult);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!x || !params || !blob || !table) return NF_EFAULT;
    // x rows a multiple of 4 floats long are read, parameter rows of such a length written, as 16-byte vectors (the row lengths
    // are the device table's: params is held to the alignment whatever they are)
    if (((D & 3) == 0 && nf_misaligned16(x)) || nf_misaligned16(params)) return NF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hidden_padded == 256) return nf::made_fwd_launch<1, 1>(x, params, nullptr, blob, table, B, NF_LD_WRITE, st);
    return nf::made_fwd_launch<2, 1>(x, params, nullptr, blob, table, B, NF_LD_WRITE, st);
}

// MaskedPiecewiseRationalQuadraticAutoregressive.forward (neural_spline/autoregressive.py:94-134, density direction of the
// autoregressive spline layer; wrapper.py:241-245) in one launch: MADE + the element-wise spline with 8 bins and linear tails.
// blob / table: flows/made_pack.pack_made_forward(made, 23, spline=True).
extern "C" int nf_made_forward_spline(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, int64_t B, int D,
                                      int hidden_padded, int acc, double tail_bound, double min_bin_width, double min_bin_height,
                                      double min_derivative, nf_stream_t stream) {
    const int rc = made_fwd_check(B, D, hidden_padded, 23);
    if (rc != NF_OK) return rc;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (min_bin_width * nf::F_K > 1.0 || min_bin_height * nf::F_K > 1.0) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !y || !logdet || !blob || !table) return NF_EFAULT;
    if ((D & 3) == 0 && nf_misaligned16(x, y)) return NF_EINVAL;        // rows a multiple of 4 floats long move as 16-byte vectors
    auto p = nf::make_rqs_params<float>(nf::F_K, NF_TAILS_LINEAR, tail_bound, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipStream_t st = (hipStream_t)stream;
    if (hidden_padded == 256) return nf::made_fwd_launch<1, 2>(x, y, logdet, blob, table, B, acc, st, p);
    return nf::made_fwd_launch<2, 2>(x, y, logdet, blob, table, B, acc, st, p);
}

// 128-row tiles of the 256-slot training kernels on (1, default) / off (0); returns the previous setting.  A forward and its backward
// must run under the same setting (the ReLU-sign words are indexed by tile).
extern "C" int nf_config_made_tr128(int on) {
    const int prev = nf::mf_tr128_switch();
    nf::mf_tr128_switch() = on ? 1 : 0;
    return prev;
}

// Rows per tile of nf_made_forward_train / nf_made_backward at this batch under the current setting (mf_tr128 decides for both); every
// other MADE entry point runs MF_ROWS-row tiles, which is also the answer for B <= 0.
extern "C" int nf_made_tile_rows(int64_t B, int D, int hidden_padded) {
    return nf::mf_tr128(B, hidden_padded, (D + 31) / 32 * 32) ? 128 : nf::MF_ROWS;
}

// MADE.forward under autograd: nf_made_forward + the operands of nf_made_backward / nf_made_wgrad (csrc/made_bwd.hip).  Bp = B rounded
// up to 64; save: (2 num_blocks + 1) x Bp x hidden_padded floats; bits: (Bp / 64) x 2 num_blocks x 2 x 512 dwords.
extern "C" int nf_made_forward_train(const void *x, void *params, void *save, void *bits, const void *blob, const int32_t *table,
                                     int64_t B, int D, int hidden_padded, int mult, nf_stream_t stream) {
    const int rc = made_fwd_check(B, D, hidden_padded, mult, hidden_padded == 256 ? 256 : 128);   // (a 64 KB x tile fits next to 256 slots)
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!x || !params || !save || !bits || !blob || !table) return NF_EFAULT;
    if (((D & 3) == 0 && nf_misaligned16(x)) || nf_misaligned16(params, save)) return NF_EINVAL;   // as nf_made_forward; save: 16-byte stores
    hipStream_t st = (hipStream_t)stream;
    const int dp = (D + 31) / 32 * 32;
    if (nf::mf_tr128(B, hidden_padded, dp))      // (256 slots, <= 64 features, whole 128-row tiles: nf_made_backward decides the same way)
        return nf::made_fwd_launch<1, 3, 128>(x, params, nullptr, blob, table, B, NF_LD_WRITE, st, nf::RqsParams<float>(), save, bits, dp);
    if (hidden_padded == 256) return nf::made_fwd_launch<1, 3>(x, params, nullptr, blob, table, B, NF_LD_WRITE, st, nf::RqsParams<float>(), save, bits, dp);
    return nf::made_fwd_launch<2, 3>(x, params, nullptr, blob, table, B, NF_LD_WRITE, st, nf::RqsParams<float>(), save, bits, dp);
}
