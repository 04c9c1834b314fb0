// realnvp_block.hpp -- what realnvp_chain.hip and realnvp_train.hip share for the "coupling block" record of the RealNVP chain blob:
// one AffineCouplingBlock (Split -> AffineCoupling -> Merge, channel / channel_inv) whose param_map is a plain MLP, with the Permute
// that stands directly behind it.
//
// Reference semantics: normflows/flows/affine/coupling.py:117-171 (AffineCoupling: param = param_map(z1); scale=True: shift =
// param[:, 0::2], scale_ = param[:, 1::2]; the three scale maps), :232-267 (the block), flows/reshape.py:30-34, 59-64 (channel:
// z1 = the first ceil(d/2) columns; channel_inv: z2 = the first ceil(d/2) columns), flows/mixing.py:32-54 (Permute).  No non-finite
// -> NaN substitution here: that rule is MaskedAffineFlow's.
//
//   record CouplingBlock : [3, c1, flip + 2 scale_map, has_perm, pf[d], pi[d], mlp]
//     c1 = columns of z1 (the MLP's input width), flip = 1 for channel_inv (z1 = the LAST c1 columns), scale_map = NF_SCALE_*
//     (NF_SCALE_NONE: scale=False, the MLP's c2 = d - c1 outputs are the shift; otherwise 2 c2 outputs, shift at 2 c, scale_ at 2 c + 1),
//     pf / pi = the Permute's index maps, y[i] = x[pf[i]] in the forward direction (behind the block), y[i] = x[pi[i]] in the inverse
//     direction (in front of it); the identity, unread, when has_perm = 0.  The host checks that both are permutations of 0 .. d - 1.
//
// lane = sample and the coordinates sit in registers, while c1, flip and the index maps are run-time values of the blob: every move
// between columns goes through the lane's own LDS columns (static register index, computed LDS address), so no register array is
// indexed dynamically (that would send it to scratch).
#pragma once
#include "common.hpp"

namespace nf {

constexpr int RB_DMAX = 16;            // coordinates (RN_DMAX / RT_DMAX) = the most MLP outputs (2 c2 at d = 16)
constexpr int RB_CMAX = RB_DMAX / 2;   // transformed columns: c2 = d - c1 is floor(d/2) or ceil(d/2)

struct RbRecord {
    int c1, c2, o1, o2, smap;
    bool has_perm;
    const float *pf, *pi, *mlp;
};

__device__ __forceinline__ RbRecord rb_decode(const float *__restrict__ rec, int d) {
    RbRecord b;
    const int code = (int)rec[2];
    b.c1 = (int)rec[1];
    b.c2 = d - b.c1;
    b.o1 = (code & 1) ? b.c2 : 0;      // first column of z1 / z2 (affine_coupling_kernel's z1_off / z2_off)
    b.o2 = (code & 1) ? 0 : b.c1;
    b.smap = code >> 1;
    b.has_perm = rec[3] != 0.0f;
    b.pf = rec + 4;
    b.pi = b.pf + d;
    b.mlp = b.pi + d;
    return b;
}

// x[i] <- x[idx[i]] through the lane's columns `col` (stride cs; at least d of them)
__device__ __forceinline__ void rb_gather(float (&x)[RB_DMAX], float *col, int cs, int d, const float *__restrict__ idx) {
#pragma unroll
    for (int i = 0; i < RB_DMAX; ++i)
        if (i < d) col[(size_t)i * cs] = x[i];
#pragma unroll
    for (int i = 0; i < RB_DMAX; ++i)
        if (i < d) x[i] = col[(size_t)(int)idx[i] * cs];
}

// the transpose of rb_gather for a cotangent: g[idx[i]] <- g[i]
__device__ __forceinline__ void rb_scatter(float (&g)[RB_DMAX], float *col, int cs, int d, const float *__restrict__ idx) {
#pragma unroll
    for (int i = 0; i < RB_DMAX; ++i)
        if (i < d) col[(size_t)(int)idx[i] * cs] = g[i];
#pragma unroll
    for (int i = 0; i < RB_DMAX; ++i)
        if (i < d) g[i] = col[(size_t)i * cs];
}

// JB outputs of one linear for one lane, a[c] = bias[c] + sum_i W[c][i] cur[i] with the inputs ascending per output, the weights in
// tiles of JB rows x 8 columns (wide wave-uniform loads issued together) -- realnvp_train.hip's rt_rows_fwd for the inference kernel:
// one scalar load per FMA leaves the 32 MLPs of the reference README's model waiting a memory round trip each (measured: 5.5 ms per
// launch at any batch size).
template <int JB>
__device__ __forceinline__ void rb_rows_fwd(const float *__restrict__ W, const float *__restrict__ bvec, const float *cur, float *nxt,
                                            int nin, int cs, bool leaky, float slope) {
    float a[JB];
#pragma unroll
    for (int c = 0; c < JB; ++c) a[c] = bvec[c];
    int i = 0;
    for (; i + 8 <= nin; i += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = cur[(size_t)(i + u) * cs];
#pragma unroll
        for (int c = 0; c < JB; ++c)
#pragma unroll
            for (int u = 0; u < 8; ++u) a[c] = fmaf(W[(size_t)c * nin + i + u], x[u], a[c]);
    }
    for (; i < nin; ++i) {
        const float x = cur[(size_t)i * cs];
#pragma unroll
        for (int c = 0; c < JB; ++c) a[c] = fmaf(W[(size_t)c * nin + i], x, a[c]);
    }
#pragma unroll
    for (int c = 0; c < JB; ++c) {
        if (leaky) a[c] = a[c] > 0.0f ? a[c] : a[c] * slope;     // LeakyReLU(slope) behind every linear but the last (mlp.py:31-38)
        nxt[(size_t)c * cs] = a[c];
    }
}

// y = MLP(columns [0, n_0) of `buf`) for one lane; buf = the lane's 2 x hmax LDS columns (stride cs), used in turn by the layers.
__device__ __forceinline__ void rb_mlp_lds(const float *__restrict__ rec, float (&y)[RB_DMAX], float *buf, int cs, int hmax) {
    const int nlin = (int)rec[0];
    const float slope = rec[1];
    const float *sizes = rec + 2;
    const float *w = sizes + nlin + 1;
    float *cur = buf, *nxt = buf + (size_t)hmax * cs;
    for (int k = 0; k < nlin; ++k) {
        const int nin = (int)sizes[k], nout = (int)sizes[k + 1];
        const float *W = w, *bvec = w + (size_t)nout * nin;
        const bool last = k == nlin - 1;
        int j = 0;
        for (; j + 4 <= nout; j += 4) rb_rows_fwd<4>(W + (size_t)j * nin, bvec + j, cur, nxt + (size_t)j * cs, nin, cs, !last, slope);
        if (nout - j >= 2) {
            rb_rows_fwd<2>(W + (size_t)j * nin, bvec + j, cur, nxt + (size_t)j * cs, nin, cs, !last, slope);
            j += 2;
        }
        if (j < nout) rb_rows_fwd<1>(W + (size_t)j * nin, bvec + j, cur, nxt + (size_t)j * cs, nin, cs, !last, slope);
        float *tmp = cur; cur = nxt; nxt = tmp;
        w = bvec + nout;
    }
    const int dout = (int)sizes[nlin];
#pragma unroll
    for (int i = 0; i < RB_DMAX; ++i) y[i] = i < dout ? cur[(size_t)i * cs] : 0.0f;
}

// One transformed coordinate and its log-det term (affine_coupling_kernel's formulas, affine.hip)
__device__ __forceinline__ float rb_apply(float v, float sh, float sc, int smap, int direction, float &ld) {
    if (smap == NF_SCALE_NONE) return direction == 0 ? v + sh : v - sh;
    if (smap == NF_SCALE_EXP) {
        ld += direction == 0 ? sc : -sc;
        return direction == 0 ? v * M<float>::exp(sc) + sh : (v - sh) * M<float>::exp(-sc);
    }
    const float sg = sigmoid(sc + 2.0f), lg = M<float>::log(sg);
    if (smap == NF_SCALE_SIGMOID) {
        ld += direction == 0 ? -lg : lg;
        return direction == 0 ? v / sg + sh : (v - sh) * sg;
    }
    ld += direction == 0 ? lg : -lg;
    return direction == 0 ? v * sg + sh : (v - sh) / sg;
}

// Its backward (affine_coupling_bwd_kernel's formulas, affine_bwd.hip): g = cotangent of the output, gl = of the row's log-det
__device__ __forceinline__ void rb_apply_bwd(float v, float sh, float sc, float g, float gl, int smap, int direction, float &gv,
                                             float &gsh, float &gsc) {
    if (smap == NF_SCALE_NONE) {
        gv = g; gsh = direction == 0 ? g : -g; gsc = 0.0f;
    } else if (smap == NF_SCALE_EXP) {
        if (direction == 0) {          // y = v e^sc + sh, ld = +sum sc
            const float e = M<float>::exp(sc);
            gv = g * e; gsh = g; gsc = g * v * e + gl;
        } else {                       // y = (v - sh) e^-sc, ld = -sum sc
            const float e = M<float>::exp(-sc);
            gv = g * e; gsh = -g * e; gsc = -(g * (v - sh) * e + gl);
        }
    } else {
        const float sg = sigmoid(sc + 2.0f), om = 1.0f - sg;   // d sg / d sc = sg (1 - sg), d log sg / d sc = 1 - sg
        const bool mult = (smap == NF_SCALE_SIGMOID_INV) == (direction == 0);   // y uses * sg (else / sg)
        if (direction == 0) {
            if (mult) { gv = g * sg; gsh = g; gsc = g * v * sg * om + gl * om; }            // ld = +sum log sg
            else { gv = g / sg; gsh = g; gsc = -(g * v * om / sg + gl * om); }              // ld = -sum log sg
        } else {
            if (mult) { gv = g * sg; gsh = -g * sg; gsc = g * (v - sh) * sg * om + gl * om; }   // ld = +sum log sg
            else { gv = g / sg; gsh = -g / sg; gsc = -(g * (v - sh) * om / sg + gl * om); }     // ld = -sum log sg
        }
    }
}

}  // namespace nf
