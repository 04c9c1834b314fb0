// nsf_tile.hpp -- what the two one-launch NSF coupling kernels share (nsf_wide.hip: the context-free layer with the optional fused LU;
// nsf_ctx.hip: the context-conditioned layer): the x tile in LDS with its columns sorted into positions, the final layer in groups with
// the spline in registers, the batch-shared spline on the identity half, the per-row log-det through LDS in a fixed order and the store
// of the tile.  nsf_wide.hip's header describes the layer; the engine (rings, items, publish) is mlp_tile.hpp's.
//
// Two forms.  This header: constants, the position index and the identity half's spline, as __forceinline__ templates.  The three stages
// of the tile loop -- nsf_tile_load.hpp (x columns -> sorted positions, padding zeroed, the context tail), nsf_tile_final.hpp (publish,
// rolled loop over the final items, register spline, log-det partials, identity spline in the density direction) and nsf_tile_store.hpp
// (fixed-order row sum, tile -> y) -- are TEXT FRAGMENTS that each kernel #includes inside its tile loop; they use the kernel's own
// locals, listed at the top of each fragment.  Why not functions: written as __forceinline__ templates (AMD clang 22.0.0git, ROCm 7.2)
// the same statements came out scheduled and register-allocated differently in all 48 instantiations -- four LU instantiations of
// nsf_wide_kernel above the registers they had (205 -> 216 in one), and with the weight ring taken by reference its eight entries went
// to scratch memory (160 bytes per lane); these kernels sit at 205-229 VGPRs with a spill history.  As included text both kernels compile
// to the instruction streams they had when each carried its own copy (profiles/nsf_tile_refactor_kernels.txt).
#pragma once
#include "mlp_tile.hpp"

namespace nf {

constexpr int nsf_tabw(int KB) { return 3 * (KB + 1); }          // floats per identity feature: cumw[K + 1] | cumh[K + 1] | deriv[K + 1]
constexpr int nsf_tab_floats(int KB) { return KB == 16 ? 3328 : 2048; }   // table region at the start of the activation region (64 features)
constexpr int nsf_nfi(int KB) { return KB == 16 ? 8 : 4; }       // final items a wave may own (flows/nsf_wide_pack.bins_geometry)

// float index of POSITION `pos` of row `row` (0 .. TR - 1) of the tile in B-operand order [pos / 4][row][4]
template <int TR>
__device__ __forceinline__ int nsf_xidx(int pos, int row) { return ((pos >> 2) * TR + row) * 4 + (pos & 3); }

// batch-shared spline on the identity columns of the tile, in place; thread = (row n = tid % TR, feature residue tid / TR)
template <bool INV, int TR, int KB>
__device__ __forceinline__ float nsf_identity(float *xreg, const float *tabs, const RqsParams<float> &p, int nI, int tid) {
    const int n = tid % TR;
    float ld = 0.0f;
#pragma unroll 1
    for (int i = tid / TR; i < nI; i += 64 * MF_NW / TR) {
        float *xp = xreg + nsf_xidx<TR>(i, n);                // identity feature i sits at position i
        float y, lad;
        rqs_table_fast<INV, KB>(p, *xp, tabs + i * nsf_tabw(KB), y, lad);
        *xp = y;
        ld += lad;
    }
    return ld;
}

}  // namespace nf
