// realnvp_train.hip -- the training twin of realnvp_chain.hip for gfx950: a run of MaskedAffineFlow(MLP s, MLP t) / ActNorm /
// AffineConstFlow / AffineCouplingBlock(MLP) + Permute records under autograd as THREE launches per step (forward with saves, backward, slab reduction) where the
// layer-by-layer route runs one library GEMM + one LeakyReLU launch per Linear, MaskedAffineFn and a log-det fold per layer, and
// autograd replays all of it (BASELINE configs[0]: several dozen launches per layer and direction on an 8 KB problem).
//
// Reference semantics: normflows/flows/affine/coupling.py:38-54 (AffineConstFlow / ActNorm), :209-229 (MaskedAffineFlow),
// nets/mlp.py:5-58 (Linear + LeakyReLU stack); the gradients are what PyTorch autograd derives from those lines.
//
// Blob: exactly realnvp_chain.hip's (core.py::_pack_realnvp documents it); here it is gathered on the device from the live
// parameters in every forward (flows/realnvp_pack.py).  The gradient slabs and the reduced gradient blob have the SAME layout: a
// parameter's gradient is the slice of the gradient blob at the parameter's offset in the weight blob.
//
// Mapping: lane = sample, `rows` lanes per workgroup (nf_realnvp_train_rows: 256, 128 or 64, the largest whose LDS fits), a
// persistent grid of <= NF_PERSISTENT_WORKGROUPS workgroups walking row tiles.  The d <= 16 coordinates and their cotangents live
// in registers.  LDS holds, per lane, one column per value, columns `rows + 1` floats apart (odd: the lane-indexed accesses of the
// MLP passes and the unit-indexed accesses of the weight-gradient contraction are both free of bank conflicts):
//   [0, act)                     the inputs of every Linear of ONE MLP (act = max over the run's MLPs of sum(sizes[:-1]), >= d)
//   [act, act + hmax)            gradient column A (also the forward's output column)
//   [act + hmax, act + 2 hmax)   gradient column B
// LDS bytes = (act + 2 hmax) (rows + 1) 4 <= 160 KB; above 64 KB through opt_in_lds.
//
// Saves: save[q, r, 0..d) = the input of the q-th EXECUTED record for row r; nothing else.  The backward recomputes both MLPs of
// a record from that input (one MLP's activations at a time: the t-net runs twice in the inverse direction, where the s-net's
// cotangent needs t) -- saving activations would cost act x B floats per MLP and a second pass over HBM for a 2-wide problem.
//
// Parameter gradients: contracted over the workgroup's lanes in a fixed order (dW[j,i] = sum_lane g[j][lane] a[i][lane]) and added
// into the slab that ONLY this workgroup writes; one reduction launch sums the slabs in a fixed order (train_reduce.hpp).  No float
// atomics: gradients are bit-identical from run to run.  Scratch bound: grid x blob floats <= 2^24 floats (64 MiB); the grid is
// lowered below NF_PERSISTENT_WORKGROUPS where the blob is larger than 64 K floats.
#include "common.hpp"
#include "realnvp_block.hpp"
#include "train_reduce.hpp"

namespace nf {

constexpr int RT_DMAX = 16;
constexpr size_t RT_LDS_MAX = 160 * 1024;
constexpr int64_t RT_SCRATCH_MAX_FLOATS = (int64_t)1 << 24;      // 64 MiB of slabs

__device__ __forceinline__ int rt_mlp_size(const float *__restrict__ rec) {
    const int nlin = (int)rec[0];
    int n = 2 + nlin + 1;
    for (int k = 0; k < nlin; ++k) n += ((int)rec[2 + k] + 1) * (int)rec[3 + k];
    return n;
}

// JB outputs of one linear for one lane: a[c] = bias[c] + sum_i W[c][i] cur[i], inputs ascending per output (realnvp_chain.hip's
// order: the same values bit for bit).  The weights come in tiles of JB rows x 8 columns -- wide wave-uniform loads issued together:
// one load at a time the kernel waits a memory round trip per four FMAs (measured: 3.4 ms per step of BASELINE configs[0]).
template <int JB>
__device__ __forceinline__ void rt_rows_fwd(const float *__restrict__ W, const float *__restrict__ bvec, const float *cur, float *nxt,
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

// y[0..d) = MLP(columns [0, n_0) of A) for one lane.  A = this lane's first activation column, cs = column stride; the input of
// linear k is left in columns [sum_{k' < k} n_k', + n_k).  `out` = this lane's scratch column for the last linear's outputs.
__device__ __forceinline__ void rt_mlp_fwd(const float *__restrict__ rec, float (&y)[RT_DMAX], float *A, float *out, int cs) {
    const int nlin = (int)rec[0];
    const float slope = rec[1];
    const float *sizes = rec + 2;
    const float *w = sizes + nlin + 1;
    int aoff = 0;
    for (int k = 0; k < nlin; ++k) {
        const int nin = (int)sizes[k], nout = (int)sizes[k + 1];
        const float *W = w, *bvec = w + (size_t)nout * nin;
        const bool last = k == nlin - 1;
        const float *cur = A + (size_t)aoff * cs;
        float *nxt = last ? out : A + (size_t)(aoff + nin) * cs;
        int j = 0;
        for (; j + 4 <= nout; j += 4) rt_rows_fwd<4>(W + (size_t)j * nin, bvec + j, cur, nxt + (size_t)j * cs, nin, cs, !last, slope);
        if (nout - j >= 2) {
            rt_rows_fwd<2>(W + (size_t)j * nin, bvec + j, cur, nxt + (size_t)j * cs, nin, cs, !last, slope);
            j += 2;
        }
        if (j < nout) rt_rows_fwd<1>(W + (size_t)j * nin, bvec + j, cur, nxt + (size_t)j * cs, nin, cs, !last, slope);
        aoff += nin;
        w = bvec + nout;
    }
    const int dout = (int)sizes[nlin];
#pragma unroll
    for (int i = 0; i < RT_DMAX; ++i) y[i] = i < dout ? out[(size_t)i * cs] : 0.0f;
}

// IB input cotangents of one linear for one lane: gnxt[u] = (sum_j W[j][i0 + u] gcur[j]) x the LeakyReLU derivative of the input
// (1 where the activation is > 0, else slope: with slope >= 0 the activation's sign is the pre-activation's, and at 0 torch takes
// slope as well); weights in tiles of 4 rows x IB columns.
template <int IB>
__device__ __forceinline__ void rt_cols_bwd(const float *__restrict__ W, const float *gcur, const float *a, float *gnxt, int nin,
                                            int nout, int cs, bool leaky, float slope) {
    float s[IB];
#pragma unroll
    for (int u = 0; u < IB; ++u) s[u] = 0.0f;
    int j = 0;
    for (; j + 4 <= nout; j += 4) {
        float g[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = gcur[(size_t)(j + c) * cs];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int u = 0; u < IB; ++u) s[u] = fmaf(W[(size_t)(j + c) * nin + u], g[c], s[u]);
    }
    for (; j < nout; ++j) {
        const float g = gcur[(size_t)j * cs];
#pragma unroll
        for (int u = 0; u < IB; ++u) s[u] = fmaf(W[(size_t)j * nin + u], g, s[u]);
    }
#pragma unroll
    for (int u = 0; u < IB; ++u) {
        if (leaky) s[u] *= a[(size_t)u * cs] > 0.0f ? 1.0f : slope;
        gnxt[(size_t)u * cs] = s[u];
    }
}

__device__ __forceinline__ void rt_store_cols(const float (&x)[RT_DMAX], float *col, int cs, int d) {
#pragma unroll
    for (int i = 0; i < RT_DMAX; ++i)
        if (i < d) col[(size_t)i * cs] = x[i];
}

__global__ void __launch_bounds__(256)
realnvp_train_fwd_kernel(const float *__restrict__ z, float *__restrict__ y, float *__restrict__ logdet, float *__restrict__ save,
                         const float *__restrict__ blob, int64_t B, int direction, int act) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int bs = blockDim.x, cs = bs + 1;
    float *A = reinterpret_cast<float *>(smem_raw) + threadIdx.x;
    float *G = A + (size_t)act * cs;
    const int nrec = (int)blob[0], d = (int)blob[1];
    const float *offs = blob + 4;
    const int64_t ntiles = (B + bs - 1) / bs;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * bs + threadIdx.x;
        const bool valid = r < B;
        float v[RT_DMAX];
#pragma unroll
        for (int i = 0; i < RT_DMAX; ++i) v[i] = (valid && i < d) ? z[r * d + i] : 0.0f;
        float ld = 0.0f;
        for (int q = 0; q < nrec; ++q) {
            const int ri = direction == 0 ? q : nrec - 1 - q;
            const float *rec = blob + (int)offs[ri];
            if (valid) {
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i)
                    if (i < d) save[((int64_t)q * B + r) * d + i] = v[i];
            }
            if ((int)rec[0] == 1) {
                const float *s = rec + 4, *t = s + d;
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) {
                    if (i < d) {
                        if (direction == 0) { v[i] = v[i] * M<float>::exp(s[i]) + t[i]; ld += s[i]; }
                        else { v[i] = (v[i] - t[i]) * M<float>::exp(-s[i]); ld -= s[i]; }
                    }
                }
            } else if ((int)rec[0] == 3) {
                // the coupling block record (realnvp_block.hpp): columns move through the lane's G columns (>= d of them, free
                // between MLP passes), the MLP reads z1 from the first c1 columns of A
                const RbRecord k = rb_decode(rec, d);
                if (direction == 1 && k.has_perm) rb_gather(v, G, cs, d, k.pi);
                float z2[RB_CMAX], par[RT_DMAX];
                rt_store_cols(v, G, cs, d);
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i)
                    if (i < k.c1) A[(size_t)i * cs] = G[(size_t)(k.o1 + i) * cs];
#pragma unroll
                for (int i = 0; i < RB_CMAX; ++i) z2[i] = i < k.c2 ? G[(size_t)(k.o2 + i) * cs] : 0.0f;
                rt_mlp_fwd(k.mlp, par, A, G, cs);
                rt_store_cols(v, G, cs, d);
#pragma unroll
                for (int i = 0; i < RB_CMAX; ++i) {
                    if (i < k.c2) {
                        const float sh = k.smap == NF_SCALE_NONE ? par[i] : par[2 * i];
                        const float sc = k.smap == NF_SCALE_NONE ? 0.0f : par[2 * i + 1];
                        G[(size_t)(k.o2 + i) * cs] = rb_apply(z2[i], sh, sc, k.smap, direction, ld);
                    }
                }
                const bool move = direction == 0 && k.has_perm;
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i)
                    if (i < d) v[i] = G[(size_t)(move ? (int)k.pf[i] : i) * cs];
            } else {
                const bool has_s = rec[1] != 0.0f, has_t = rec[2] != 0.0f;
                const float *b = rec + 4;
                const float *p = b + d;
                float zm[RT_DMAX], sc[RT_DMAX], tr[RT_DMAX];
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) { zm[i] = i < d ? b[i] * v[i] : 0.0f; sc[i] = 0.0f; tr[i] = 0.0f; }
                if (has_s) {
                    rt_store_cols(zm, A, cs, d);
                    rt_mlp_fwd(p, sc, A, G, cs);
                    p += rt_mlp_size(p);
                }
                if (has_t) {
                    rt_store_cols(zm, A, cs, d);
                    rt_mlp_fwd(p, tr, A, G, cs);
                }
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) {
                    if (i < d) {
                        const float s_ = M<float>::finite(sc[i]) ? sc[i] : M<float>::nan();   // coupling.py:213-214
                        const float t_ = M<float>::finite(tr[i]) ? tr[i] : M<float>::nan();
                        const float m = 1.0f - b[i];
                        if (direction == 0) { v[i] = zm[i] + m * (v[i] * M<float>::exp(s_) + t_); ld += m * s_; }
                        else { v[i] = zm[i] + m * (v[i] - t_) * M<float>::exp(-s_); ld -= m * s_; }
                    }
                }
            }
        }
        if (valid) {
#pragma unroll
            for (int i = 0; i < RT_DMAX; ++i)
                if (i < d) y[r * d + i] = v[i];
            logdet[r] = ld;
        }
    }
}

// Backward of one MLP whose linears' inputs sit in A's columns (rt_mlp_fwd): gout = the cotangent of its d outputs; adds the
// cotangent of its d inputs to gin.  With wflag the weight / bias gradients are contracted over the workgroup's lanes and added
// into slabrec (this record's place in the workgroup's slab).  Called by every thread of the workgroup (barriers inside when wflag).
__device__ __forceinline__ void rt_mlp_bwd(const float *__restrict__ rec, const float (&gout)[RT_DMAX], float (&gin)[RT_DMAX], float *A,
                                           float *G, int cs, int hmax, float *__restrict__ slabrec, bool wflag) {
    const int nlin = (int)rec[0];
    const float slope = rec[1];
    const float *sizes = rec + 2;
    const int bs = blockDim.x, tid = threadIdx.x;
    int aoff = 0, woff = 2 + nlin + 1;
    for (int k = 0; k < nlin; ++k) {
        aoff += (int)sizes[k];
        woff += ((int)sizes[k] + 1) * (int)sizes[k + 1];
    }
    float *gcur = G, *gnxt = G + (size_t)hmax * cs;
    rt_store_cols(gout, gcur, cs, (int)sizes[nlin]);
    for (int k = nlin - 1; k >= 0; --k) {
        const int nin = (int)sizes[k], nout = (int)sizes[k + 1];
        woff -= (nin + 1) * nout;
        aoff -= nin;
        const float *W = rec + woff;
        const float *a = A + (size_t)aoff * cs;
        if (wflag) {
            __syncthreads();                     // every lane's gcur and activation columns are written
            const float *gb = gcur - tid, *ab = a - tid;
            const int nW = nout * nin, n = nW + nout;
            for (int o = tid; o < n; o += bs) {
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                if (o < nW) {
                    const int j = o / nin, i = o - j * nin;
                    const float *gj = gb + (size_t)j * cs, *ai = ab + (size_t)i * cs;
                    for (int l = 0; l < bs; l += 16) {       // (bs is a multiple of 64; 32 LDS reads in flight per step)
#pragma unroll
                        for (int u = 0; u < 16; u += 4) {
                            s0 = fmaf(gj[l + u], ai[l + u], s0);
                            s1 = fmaf(gj[l + u + 1], ai[l + u + 1], s1);
                            s2 = fmaf(gj[l + u + 2], ai[l + u + 2], s2);
                            s3 = fmaf(gj[l + u + 3], ai[l + u + 3], s3);
                        }
                    }
                } else {
                    const float *gj = gb + (size_t)(o - nW) * cs;
                    for (int l = 0; l < bs; l += 4) {
                        s0 += gj[l];
                        s1 += gj[l + 1];
                        s2 += gj[l + 2];
                        s3 += gj[l + 3];
                    }
                }
                slabrec[woff + o] += (s0 + s1) + (s2 + s3);
            }
        }
        // cotangent of this linear's input, through the LeakyReLU in front of it (rt_cols_bwd)
        int i = 0;
        for (; i + 8 <= nin; i += 8) rt_cols_bwd<8>(W + i, gcur, a + (size_t)i * cs, gnxt + (size_t)i * cs, nin, nout, cs, k > 0, slope);
        if (nin - i >= 4) {
            rt_cols_bwd<4>(W + i, gcur, a + (size_t)i * cs, gnxt + (size_t)i * cs, nin, nout, cs, k > 0, slope);
            i += 4;
        }
        if (nin - i >= 2) {
            rt_cols_bwd<2>(W + i, gcur, a + (size_t)i * cs, gnxt + (size_t)i * cs, nin, nout, cs, k > 0, slope);
            i += 2;
        }
        if (i < nin) rt_cols_bwd<1>(W + i, gcur, a + (size_t)i * cs, gnxt + (size_t)i * cs, nin, nout, cs, k > 0, slope);
        float *tmp = gcur; gcur = gnxt; gnxt = tmp;
    }
    if (wflag) __syncthreads();                  // the last contraction has read its columns: the caller may overwrite them
    const int din = (int)sizes[0];
#pragma unroll
    for (int i = 0; i < RT_DMAX; ++i)
        if (i < din) gin[i] += gcur[(size_t)i * cs];
}

// wmask: bit 2 ri = the s-net (ActNorm: s; coupling block: its one MLP) of record ri needs its gradient, bit 2 ri + 1 = the t-net
// (ActNorm: t; unused for a coupling block).
__global__ void __launch_bounds__(256)
realnvp_train_bwd_kernel(const float *__restrict__ save, const float *__restrict__ gy, const float *__restrict__ gld,
                         float *__restrict__ gz, const float *__restrict__ blob, float *__restrict__ slabs, int64_t B, int direction,
                         int act, int64_t nblob, unsigned long long wmask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int bs = blockDim.x, cs = bs + 1, tid = threadIdx.x;
    float *A = reinterpret_cast<float *>(smem_raw) + tid;
    float *G = A + (size_t)act * cs;
    const int nrec = (int)blob[0], d = (int)blob[1], hmax = (int)blob[2];
    const float *offs = blob + 4;
    float *slab = slabs + (size_t)blockIdx.x * nblob;
    if (wmask) {
        for (int64_t i = tid; i < nblob; i += bs) slab[i] = 0.0f;
        __syncthreads();
    }
    const int64_t ntiles = (B + bs - 1) / bs;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * bs + tid;
        const bool valid = r < B;          // a lane past the batch runs on zeros: every cotangent it produces is 0
        float g[RT_DMAX];
#pragma unroll
        for (int i = 0; i < RT_DMAX; ++i) g[i] = (valid && gy && i < d) ? gy[r * d + i] : 0.0f;
        const float gl = (valid && gld) ? gld[r] : 0.0f;
        for (int q = nrec - 1; q >= 0; --q) {
            const int ri = direction == 0 ? q : nrec - 1 - q;
            const int roff = (int)offs[ri];
            const float *rec = blob + roff;
            const int wbits = (int)((wmask >> (2 * ri)) & 3ull);
            float v[RT_DMAX];
#pragma unroll
            for (int i = 0; i < RT_DMAX; ++i) v[i] = (valid && i < d) ? save[((int64_t)q * B + r) * d + i] : 0.0f;
            if ((int)rec[0] == 1) {            // actnorm_bwd's formulas (coupling.py:38-54); the log-det is per sample: gs gets +- gld per row
                const float *s = rec + 4, *t = s + d;
                float gs[RT_DMAX], gt[RT_DMAX];
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) {
                    gs[i] = 0.0f; gt[i] = 0.0f;
                    if (i < d) {
                        if (direction == 0) {
                            const float e = M<float>::exp(s[i]);
                            gs[i] = g[i] * v[i] * e + gl; gt[i] = g[i]; g[i] = g[i] * e;
                        } else {
                            const float e = M<float>::exp(-s[i]);
                            gs[i] = -(g[i] * (v[i] - t[i]) * e + gl); gt[i] = -(g[i] * e); g[i] = g[i] * e;
                        }
                    }
                }
                if (wbits) {
                    rt_store_cols(gs, G, cs, d);
                    rt_store_cols(gt, G + (size_t)d * cs, cs, d);          // (2 d <= 2 hmax columns)
                    __syncthreads();
                    if (tid < 2 * d && ((wbits >> (tid < d ? 0 : 1)) & 1)) {
                        const float *col = G - tid + (size_t)tid * cs;
                        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                        for (int l = 0; l < bs; l += 4) { s0 += col[l]; s1 += col[l + 1]; s2 += col[l + 2]; s3 += col[l + 3]; }
                        slab[roff + 4 + tid] += (s0 + s1) + (s2 + s3);
                    }
                    __syncthreads();
                }
            } else if ((int)rec[0] == 3) {
                // the coupling block record (realnvp_block.hpp); its one MLP is side 0 (bit 2 ri).  Forward direction: the Permute
                // ran behind the block, so its transpose meets the cotangent first; inverse direction: it ran in front of the
                // block, so the block's input is recomputed from the saved one and the transpose comes last.
                const RbRecord k = rb_decode(rec, d);
                if (k.has_perm) {
                    if (direction == 0) rb_scatter(g, G, cs, d, k.pf);
                    else rb_gather(v, G, cs, d, k.pi);
                }
                float z2[RB_CMAX], g2[RB_CMAX], gz2[RB_CMAX], par[RT_DMAX], gp[RT_DMAX], gin[RT_DMAX];
                rt_store_cols(v, G, cs, d);
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i)
                    if (i < k.c1) A[(size_t)i * cs] = G[(size_t)(k.o1 + i) * cs];
#pragma unroll
                for (int i = 0; i < RB_CMAX; ++i) z2[i] = i < k.c2 ? G[(size_t)(k.o2 + i) * cs] : 0.0f;
                rt_store_cols(g, G, cs, d);
#pragma unroll
                for (int i = 0; i < RB_CMAX; ++i) g2[i] = i < k.c2 ? G[(size_t)(k.o2 + i) * cs] : 0.0f;
                rt_mlp_fwd(k.mlp, par, A, G, cs);
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) { gp[i] = 0.0f; gin[i] = 0.0f; }
#pragma unroll
                for (int i = 0; i < RB_CMAX; ++i) {
                    gz2[i] = 0.0f;
                    if (i < k.c2) {
                        const float sh = k.smap == NF_SCALE_NONE ? par[i] : par[2 * i];
                        const float sc = k.smap == NF_SCALE_NONE ? 0.0f : par[2 * i + 1];
                        float gsh, gsc;
                        rb_apply_bwd(z2[i], sh, sc, g2[i], gl, k.smap, direction, gz2[i], gsh, gsc);
                        if (!valid) { gsh = 0.0f; gsc = 0.0f; }      // (0 * e^s is NaN for an overflowing s of the zero row)
                        if (k.smap == NF_SCALE_NONE) gp[i] = gsh;
                        else { gp[2 * i] = gsh; gp[2 * i + 1] = gsc; }
                    }
                }
                if (q > 0 || gz != nullptr || (wbits & 1))      // somebody reads the cotangent of this record's input, or the MLP's
                    rt_mlp_bwd(k.mlp, gp, gin, A, G, cs, hmax, slab + roff + (int)(k.mlp - rec), (wbits & 1) != 0);
                // merge: the identity half keeps its cotangent and gains the MLP's, the transformed half takes the coupling's
                rt_store_cols(g, G, cs, d);
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i)
                    if (i < k.c1) G[(size_t)(k.o1 + i) * cs] += gin[i];
#pragma unroll
                for (int i = 0; i < RB_CMAX; ++i)
                    if (i < k.c2) G[(size_t)(k.o2 + i) * cs] = gz2[i];
                if (direction == 1 && k.has_perm) {            // u[i] = x[pi[i]]: gx[pi[i]] = gu[i]
#pragma unroll
                    for (int i = 0; i < RT_DMAX; ++i)
                        if (i < d) g[i] = G[(size_t)i * cs];
                    rb_scatter(g, G, cs, d, k.pi);
                } else {
#pragma unroll
                    for (int i = 0; i < RT_DMAX; ++i)
                        if (i < d) g[i] = G[(size_t)i * cs];
                }
            } else {
                const bool has_s = rec[1] != 0.0f, has_t = rec[2] != 0.0f;
                const float *b = rec + 4;
                const float *ps = b + d;
                const float *pt = has_s ? ps + rt_mlp_size(ps) : ps;
                if (!has_s && !has_t) continue;           // y = z, log-det 0: the cotangent passes through
                float zm[RT_DMAX], sc[RT_DMAX], tr[RT_DMAX], gs[RT_DMAX], gt[RT_DMAX], gzm[RT_DMAX];
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) { zm[i] = i < d ? b[i] * v[i] : 0.0f; sc[i] = 0.0f; tr[i] = 0.0f; gzm[i] = 0.0f; }
                bool t_live = false;                       // the t-net's activations are the ones in LDS
                if (has_t && direction == 1) {             // the inverse direction's s cotangent needs t
                    rt_store_cols(zm, A, cs, d);
                    rt_mlp_fwd(pt, tr, A, G, cs);
                    t_live = !has_s;
                }
                if (has_s) {
                    rt_store_cols(zm, A, cs, d);
                    rt_mlp_fwd(ps, sc, A, G, cs);
                }
                // masked_affine_bwd_kernel's formulas (affine_bwd.hip), non-finite s / t -> NaN first
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i) {
                    gs[i] = 0.0f; gt[i] = 0.0f;
                    if (i < d) {
                        const float s_ = M<float>::finite(sc[i]) ? sc[i] : M<float>::nan();
                        const float t_ = M<float>::finite(tr[i]) ? tr[i] : M<float>::nan();
                        const float bi = b[i], nb = 1.0f - bi, gi = g[i];
                        if (direction == 0) {
                            const float e = M<float>::exp(s_);
                            g[i] = gi * (bi + nb * e);
                            gs[i] = nb * (gi * v[i] * e + gl);
                            gt[i] = nb * gi;
                        } else {
                            const float e = M<float>::exp(-s_);
                            g[i] = gi * (bi + nb * e);
                            gs[i] = -nb * (gi * (v[i] - t_) * e + gl);
                            gt[i] = -nb * gi * e;
                        }
                        if (!valid) { gs[i] = 0.0f; gt[i] = 0.0f; }      // (0 * e^s is NaN for an overflowing s of the zero row)
                    }
                }
                const bool chain = q > 0 || gz != nullptr;     // somebody reads the cotangent of this record's input
                if (has_s && (chain || (wbits & 1)))
                    rt_mlp_bwd(ps, gs, gzm, A, G, cs, hmax, slab + roff + (int)(ps - rec), (wbits & 1) != 0);
                if (has_t && (chain || (wbits & 2))) {
                    if (!t_live) {
                        float tmp[RT_DMAX];
                        rt_store_cols(zm, A, cs, d);
                        rt_mlp_fwd(pt, tmp, A, G, cs);
                    }
                    rt_mlp_bwd(pt, gt, gzm, A, G, cs, hmax, slab + roff + (int)(pt - rec), (wbits & 2) != 0);
                }
                // the nets see b z (coupling.py:210): their input cotangents reach z through the mask
#pragma unroll
                for (int i = 0; i < RT_DMAX; ++i)
                    if (i < d) g[i] += b[i] * gzm[i];
            }
        }
        if (gz && valid) {
#pragma unroll
            for (int i = 0; i < RT_DMAX; ++i)
                if (i < d) gz[r * d + i] = g[i];
        }
    }
}

// grads[e] = sum over the workgroups' slabs in a fixed order (train_reduce.hpp: chunk lanes, then lane order).
__global__ void __launch_bounds__(64 * RL)
realnvp_train_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ grads, int64_t n, int chunks) {
    __shared__ float sm[RL][64];
    for (int64_t e0 = (int64_t)blockIdx.x * 64; e0 < n; e0 += (int64_t)gridDim.x * 64)
        wgrad_reduce_group(slabs, grads, nullptr, n, n, n, chunks, 0, 1, 0, nullptr, 0, e0, sm);
}

static inline size_t rt_lds(int hmax, int act, int rows) { return (size_t)(act + 2 * hmax) * (rows + 1) * sizeof(float); }

static inline int rt_rows(int hmax, int act) {
    for (int rows = 256; rows >= 64; rows >>= 1)
        if (rt_lds(hmax, act, rows) <= RT_LDS_MAX) return rows;
    return 0;
}

static inline int rt_grid(int64_t B, int rows, int64_t nblob) {
    int grid = persistent_grid((B + rows - 1) / rows);
    if (nblob > 0 && (int64_t)grid * nblob > RT_SCRATCH_MAX_FLOATS) grid = (int)(RT_SCRATCH_MAX_FLOATS / nblob);
    return grid < 1 ? 1 : grid;
}

static inline int rt_check(int64_t B, int d, int hmax, int act, int direction) {
    if (B < 0 || d < 1 || hmax < 1 || act < 1 || (direction != 0 && direction != 1)) return NF_EINVAL;
    if (d > RT_DMAX || hmax > 64) return NF_ENOTSUP;
    if (hmax < d || act < d) return NF_EINVAL;
    if (rt_rows(hmax, act) == 0) return NF_ENOTSUP;
    return NF_OK;
}

}  // namespace nf

extern "C" int nf_realnvp_train_rows(int hmax, int act_floats) {
    if (hmax < 1 || act_floats < 1) return NF_EINVAL;
    if (hmax > 64) return NF_ENOTSUP;
    const int rows = nf::rt_rows(hmax, act_floats);
    return rows ? rows : NF_ENOTSUP;
}

extern "C" int64_t nf_realnvp_train_scratch_floats(int64_t B, int hmax, int act_floats, int64_t blob_floats) {
    if (B < 0 || blob_floats < 1 || blob_floats > nf::RT_SCRATCH_MAX_FLOATS) return NF_EINVAL;
    const int rows = nf_realnvp_train_rows(hmax, act_floats);
    if (rows < 0) return rows;
    return (int64_t)nf::rt_grid(B, rows, blob_floats) * blob_floats;
}

extern "C" int nf_realnvp_chain_train_fwd(const void *z, void *y, void *logdet, void *save, const void *blob, int64_t B, int d,
                                          int hmax, int act_floats, int direction, nf_stream_t stream) {
    const int rc = nf::rt_check(B, d, hmax, act_floats, direction);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!z || !y || !logdet || !save || !blob) return NF_EFAULT;
    const int rows = nf::rt_rows(hmax, act_floats);
    const size_t lds = nf::rt_lds(hmax, act_floats, rows);
    static nf::LdsOptIn opted;
    if (nf::opt_in_lds(reinterpret_cast<const void *>(&nf::realnvp_train_fwd_kernel), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL(nf::realnvp_train_fwd_kernel, dim3(nf::rt_grid(B, rows, 0)), dim3(rows), lds, (hipStream_t)stream,
                       (const float *)z, (float *)y, (float *)logdet, (float *)save, (const float *)blob, B, direction, act_floats);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_realnvp_chain_bwd(const void *save, const void *gy, const void *gld, void *gz, const void *blob, void *slabs,
                                    void *grads, int64_t B, int d, int hmax, int act_floats, int64_t blob_floats, int direction,
                                    int64_t wmask, nf_stream_t stream) {
    const int rc = nf::rt_check(B, d, hmax, act_floats, direction);
    if (rc != NF_OK) return rc;
    if (blob_floats < 1 || blob_floats > nf::RT_SCRATCH_MAX_FLOATS) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!save || !blob || (wmask && (!slabs || !grads))) return NF_EFAULT;
    if (!gz && !wmask) return NF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rows = nf::rt_rows(hmax, act_floats);
    const size_t lds = nf::rt_lds(hmax, act_floats, rows);
    const int grid = nf::rt_grid(B, rows, blob_floats);
    static nf::LdsOptIn opted;
    if (nf::opt_in_lds(reinterpret_cast<const void *>(&nf::realnvp_train_bwd_kernel), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL(nf::realnvp_train_bwd_kernel, dim3(grid), dim3(rows), lds, st, (const float *)save, (const float *)gy,
                       (const float *)gld, (float *)gz, (const float *)blob, (float *)slabs, B, direction, act_floats, blob_floats,
                       (unsigned long long)wmask);
    NF_CHECK_LAUNCH();
    if (wmask) {
        hipLaunchKernelGGL(nf::realnvp_train_reduce_kernel, dim3(nf::grid_for(blob_floats, 64)), dim3(64 * nf::RL), 0, st,
                           (const float *)slabs, (float *)grads, blob_floats, grid);
        NF_CHECK_LAUNCH();
    }
    return NF_OK;
}
