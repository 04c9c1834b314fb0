// resnet_ctx_train.hip -- the GLU-gated ResidualNet conditioner (nets/resnet.py:7-104 with context_features) under autograd:
// a training forward that saves what the backward reads, the input-gradient backward (g_x, g_context and every layer's output
// gradient) and the weight gradients as one launch over 64 x 64 tiles plus a fixed-order reduction.  No float atomics anywhere.
//
// Network (reference order: relu, linear0, relu, linear1, GLU, residual add):
//   h0 = W0 [x; c] + b0;  per block  t = W1 relu(h) + b1,  u = W2 relu(t) + b2,  a = Wc c + bc,  h' = h + u * s(a);  out = Wf h_NB + bf
//
// Geometry (packer: flows/ctx_train_pack.py)
//   * a workgroup of 4 waves owns a tile of 64 rows; the grid is persistent over the tiles.
//   * every product is transposed, Out^T[32 units x 32 rows] = W . Act^T, on v_mfma_f32_32x32x2_f32: lane (hh = lane >> 5,
//     n = lane & 31) holds row n of a 32-row sample block, its 16 accumulators units 8 q + 4 hh + i of a 32-unit block.  A wave
//     owns the unit blocks w, w + 4 (hidden <= 256: at most two) for both sample blocks, for every hidden layer, so the residual
//     stream h (forward) and its gradient (backward) stay in the registers of the lanes that produced them.
//   * per 8-step of the contraction a lane reads one 16-byte piece of its weight row (global, L2-resident) and one of each of its
//     two activation rows (LDS) and issues 8 MFMAs: k = k0 + 4 hh + j for MFMA j on both operands.
//   * the x tile holds [x | 0 | c | 0] at positions [0, nI), [PI, PI + C) (PI = nI rounded up to 32), as csrc/nsf_ctx.hip does;
//     the context row stride may be 0 (context.expand(B, C)).
//   * save (row-major, Bp = B rounded up to 64): slots [Bp][Hp]: 0 = h0, per block b: 1 + 4 b = t, 2 + 4 b = u, 3 + 4 b = s(a),
//     4 + 4 b = h_{b+1}; then the x tile [Bp][Kin].  G (backward): 0 = g_h0, per block 1 + 3 b = g_t, 2 + 3 b = g_u, 3 + 3 b = g_a.
//     Rows beyond the batch hold the network of a zero input in save and zeros in G; the weight gradients read rows < B only.
#include "common.hpp"

namespace nf {

typedef float rc_f32x16 __attribute__((ext_vector_type(16)));
typedef float rc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RC_ROWS = 64;
constexpr int RC_THREADS = 256;
constexpr int RC_MAXU = 2;             // hidden unit blocks per wave (Hp <= 256)

// table (int32, flows/ctx_train_pack.py): the shape, then float offsets of the padded matrices inside the blob
enum {
    RT_NI = 0, RT_C, RT_PI, RT_KIN, RT_H, RT_HP, RT_NB, RT_O, RT_OP,
    RT_W0 = 10, RT_B0, RT_WF, RT_BF, RT_WFT, RT_W0T,
    RT_BLK = 16,                       // per block (8 each): W1, b1, W2, b2, Wc, bc, W2T, W1T
    RT_WCT = 16 + 8 * 4,               // per block: WcT
    RT_LEN = RT_WCT + 4
};

__device__ __forceinline__ int rc_unit(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// acc[s] += W[32 units][K] . act[32 s + n][K]^T  (W: row stride ldw floats; act: LDS, row stride lda floats; K a multiple of 8)
__device__ __forceinline__ void rc_mm(const float *__restrict__ W, int ldw, int K, const float *act, int lda, int lane,
                                      rc_f32x16 (&acc)[2]) {
    const int n = lane & 31, hh = lane >> 5;
    const float *wp = W + (size_t)n * ldw + 4 * hh;
    const float *a0 = act + n * lda + 4 * hh;
    const float *a1 = act + (32 + n) * lda + 4 * hh;
#pragma unroll 4
    for (int k = 0; k < K; k += 8) {
        const rc_f32x4 wv = *reinterpret_cast<const rc_f32x4 *>(wp + k);
        const rc_f32x4 x0 = *reinterpret_cast<const rc_f32x4 *>(a0 + k);
        const rc_f32x4 x1 = *reinterpret_cast<const rc_f32x4 *>(a1 + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j], x0[j], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j], x1[j], acc[1], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ void rc_bias(const float *__restrict__ bias, int u0, int hh, rc_f32x16 (&acc)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float b = bias ? bias[u0 + rc_unit(r, hh)] : 0.0f;
        acc[0][r] = b;
        acc[1][r] = b;
    }
}

// a unit block's values -> LDS act[row][unit] (optionally through relu)
template <bool RELU>
__device__ __forceinline__ void rc_publish(float *act, int lda, int u0, int lane, const rc_f32x16 (&acc)[2]) {
    const int n = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rc_f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = RELU ? fmaxf(acc[s][4 * q + i], 0.0f) : acc[s][4 * q + i];
            *reinterpret_cast<rc_f32x4 *>(act + (32 * s + n) * lda + u0 + 8 * q + 4 * hh) = v;
        }
}

// a unit block's values <-> a row-major [rows][ld] global image of the tile (all 64 rows exist: the buffers hold Bp rows)
__device__ __forceinline__ void rc_store(float *dst, int ld, int u0, int lane, const rc_f32x16 (&acc)[2]) {
    const int n = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<rc_f32x4 *>(dst + (size_t)(32 * s + n) * ld + u0 + 8 * q + 4 * hh) =
                rc_f32x4{acc[s][4 * q], acc[s][4 * q + 1], acc[s][4 * q + 2], acc[s][4 * q + 3]};
}

__device__ __forceinline__ void rc_load(const float *src, int ld, int u0, int lane, rc_f32x16 (&acc)[2]) {
    const int n = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const rc_f32x4 v = *reinterpret_cast<const rc_f32x4 *>(src + (size_t)(32 * s + n) * ld + u0 + 8 * q + 4 * hh);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[s][4 * q + i] = v[i];
        }
}

__global__ void __launch_bounds__(RC_THREADS, 1)
rc_forward_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ c, int64_t ldc, float *__restrict__ out,
                  float *__restrict__ save, const float *__restrict__ blob, const int *__restrict__ tab, int64_t B, int64_t Bp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nI = tab[RT_NI], C = tab[RT_C], PI = tab[RT_PI], Kin = tab[RT_KIN], Hp = tab[RT_HP], NB = tab[RT_NB];
    const int O = tab[RT_O], Op = tab[RT_OP];
    const int ldi = Kin + 4, lda = Hp + 4;
    float *xin = lds;                          // [64][Kin + 4]
    float *act = lds + RC_ROWS * ldi;          // [64][Hp + 4]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, hh = lane >> 5;
    const int nub = Hp / 32;
    const int64_t ntiles = Bp / RC_ROWS;
    const size_t slot = (size_t)Bp * Hp;
    float *insave = save + (size_t)(4 * NB + 1) * slot;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * RC_ROWS;
        // ---- x tile [x | 0 | c | 0] -> LDS and save --------------------------------------------------------------------------------
        for (int e = tid; e < RC_ROWS * Kin; e += RC_THREADS) {
            const int r = e / Kin, p = e - r * Kin;
            const int64_t row = row0 + r;
            float v = 0.0f;
            if (row < B) {
                if (p < PI) {
                    if (p < nI) v = x[row * ldx + p];
                } else if (p - PI < C) {
                    v = c[row * ldc + (p - PI)];
                }
            }
            xin[r * ldi + p] = v;
            insave[(size_t)row * Kin + p] = v;
        }
        __syncthreads();
        rc_f32x16 h[RC_MAXU][2];
        // ---- initial layer --------------------------------------------------------------------------------------------------------
#pragma unroll
        for (int i = 0; i < RC_MAXU; ++i) {
            const int ub = w + 4 * i;
            if (ub < nub) {
                rc_bias(blob + tab[RT_B0], 32 * ub, hh, h[i]);
                rc_mm(blob + tab[RT_W0] + (size_t)32 * ub * Kin, Kin, Kin, xin, ldi, lane, h[i]);
                rc_store(save + row0 * Hp, Hp, 32 * ub, lane, h[i]);
            }
        }
        // ---- gated residual blocks ----------------------------------------------------------------------------------------------------
        for (int b = 0; b < NB; ++b) {
            const int *bt = tab + RT_BLK + 8 * b;
            float *st = save + (size_t)(1 + 4 * b) * slot + row0 * Hp;
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i)
                if (w + 4 * i < nub) rc_publish<true>(act, lda, 32 * (w + 4 * i), lane, h[i]);
            __syncthreads();
            rc_f32x16 t[RC_MAXU][2];
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i) {
                const int ub = w + 4 * i;
                if (ub < nub) {
                    rc_bias(blob + bt[1], 32 * ub, hh, t[i]);
                    rc_mm(blob + bt[0] + (size_t)32 * ub * Hp, Hp, Hp, act, lda, lane, t[i]);
                    rc_store(st, Hp, 32 * ub, lane, t[i]);
                }
            }
            __syncthreads();                   // every wave has read relu(h)
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i)
                if (w + 4 * i < nub) rc_publish<true>(act, lda, 32 * (w + 4 * i), lane, t[i]);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i) {
                const int ub = w + 4 * i;
                if (ub < nub) {
                    rc_f32x16 u[2], a[2];
                    rc_bias(blob + bt[3], 32 * ub, hh, u);
                    rc_mm(blob + bt[2] + (size_t)32 * ub * Hp, Hp, Hp, act, lda, lane, u);
                    rc_bias(blob + bt[5], 32 * ub, hh, a);
                    rc_mm(blob + bt[4] + (size_t)32 * ub * (Kin - PI), Kin - PI, Kin - PI, xin + PI, ldi, lane, a);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float g = 1.0f / (1.0f + expf(-a[s][r]));      // F.glu: first half * sigmoid(second half)
                            a[s][r] = g;
                            h[i][s][r] += u[s][r] * g;
                        }
                    rc_store(st + slot, Hp, 32 * ub, lane, u);
                    rc_store(st + 2 * slot, Hp, 32 * ub, lane, a);
                    rc_store(st + 3 * slot, Hp, 32 * ub, lane, h[i]);
                }
            }
            __syncthreads();                   // every wave has read relu(t)
        }
        // ---- final layer on the raw block output ------------------------------------------------------------------------------------
#pragma unroll
        for (int i = 0; i < RC_MAXU; ++i)
            if (w + 4 * i < nub) rc_publish<false>(act, lda, 32 * (w + 4 * i), lane, h[i]);
        __syncthreads();
        for (int ob = w; ob < Op / 32; ob += 4) {
            rc_f32x16 o[2];
            rc_bias(blob + tab[RT_BF], 32 * ob, hh, o);
            rc_mm(blob + tab[RT_WF] + (size_t)32 * ob * Hp, Hp, Hp, act, lda, lane, o);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int64_t row = row0 + 32 * s + n;
                if (row < B)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int col = 32 * ob + rc_unit(r, hh);
                        if (col < O) out[row * O + col] = o[s][r];
                    }
            }
        }
        __syncthreads();                       // the next tile overwrites the x tile and the activations
    }
}

__global__ void __launch_bounds__(RC_THREADS, 1)
rc_backward_kernel(const float *__restrict__ gout, const float *__restrict__ save, float *__restrict__ G, float *__restrict__ gx,
                   float *__restrict__ gc, const float *__restrict__ blob, const int *__restrict__ tab, int64_t B, int64_t Bp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nI = tab[RT_NI], C = tab[RT_C], PI = tab[RT_PI], Kin = tab[RT_KIN], Hp = tab[RT_HP], NB = tab[RT_NB];
    const int O = tab[RT_O], Op = tab[RT_OP];
    const int lda = (Hp > 128 ? Hp : 128) + 4;
    float *actA = lds;                         // [64][max(Hp, 128) + 4]: g_out pieces, g_u, g_t, g_h0
    float *actB = lds + RC_ROWS * lda;         // [64][Hp + 4]: g_a
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, hh = lane >> 5;
    const int nub = Hp / 32;
    const int64_t ntiles = Bp / RC_ROWS;
    const size_t slot = (size_t)Bp * Hp;
    const bool has_in = 32 * w < Kin;          // the wave's unit block of the input gradient [g_x | 0 | g_c | 0]
    const bool ctx_blk = has_in && 32 * w >= PI;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * RC_ROWS;
        rc_f32x16 g[RC_MAXU][2], gin[2];
#pragma unroll
        for (int i = 0; i < RC_MAXU; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) g[i][s] = rc_f32x16{};
        gin[0] = rc_f32x16{};
        gin[1] = rc_f32x16{};
        // ---- g_h = Wf^T g_out, over 128-column pieces of g_out ---------------------------------------------------------------------
        for (int k0 = 0; k0 < Op; k0 += 128) {
            const int kw = Op - k0 < 128 ? Op - k0 : 128;
            for (int e = tid; e < RC_ROWS * kw; e += RC_THREADS) {
                const int r = e / kw, k = e - r * kw;
                const int64_t row = row0 + r;
                actA[r * lda + k] = (row < B && k0 + k < O) ? gout[row * O + k0 + k] : 0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i) {
                const int ub = w + 4 * i;
                if (ub < nub) rc_mm(blob + tab[RT_WFT] + (size_t)32 * ub * Op + k0, Op, kw, actA, lda, lane, g[i]);
            }
            __syncthreads();
        }
        // ---- blocks in reverse order ------------------------------------------------------------------------------------------------
        for (int b = NB - 1; b >= 0; --b) {
            const int *bt = tab + RT_BLK + 8 * b;
            const float *st = save + (size_t)(1 + 4 * b) * slot + row0 * Hp;       // t, u, s(a)
            const float *sh = save + (size_t)(4 * b) * slot + row0 * Hp;           // the block's input h
            float *gt_dst = G + (size_t)(1 + 3 * b) * slot + row0 * Hp;            // g_t, g_u, g_a
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i) {
                const int ub = w + 4 * i;
                if (ub < nub) {
                    rc_f32x16 u[2], sa[2];
                    rc_load(st + slot, Hp, 32 * ub, lane, u);
                    rc_load(st + 2 * slot, Hp, 32 * ub, lane, sa);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float gg = g[i][s][r], sg = sa[s][r];
                            u[s][r] = gg * u[s][r] * sg * (1.0f - sg);     // g_a
                            sa[s][r] = gg * sg;                            // g_u
                        }
                    rc_store(gt_dst + slot, Hp, 32 * ub, lane, sa);
                    rc_store(gt_dst + 2 * slot, Hp, 32 * ub, lane, u);
                    rc_publish<false>(actA, lda, 32 * ub, lane, sa);
                    rc_publish<false>(actB, lda, 32 * ub, lane, u);
                }
            }
            __syncthreads();
            rc_f32x16 gt[RC_MAXU][2];
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i) {
                const int ub = w + 4 * i;
                if (ub < nub) {
                    gt[i][0] = rc_f32x16{};
                    gt[i][1] = rc_f32x16{};
                    rc_mm(blob + bt[6] + (size_t)32 * ub * Hp, Hp, Hp, actA, lda, lane, gt[i]);      // W2^T g_u
                    rc_f32x16 t[2];
                    rc_load(st, Hp, 32 * ub, lane, t);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) gt[i][s][r] = t[s][r] > 0.0f ? gt[i][s][r] : 0.0f;
                    rc_store(gt_dst, Hp, 32 * ub, lane, gt[i]);
                }
            }
            if (ctx_blk)                                                                      // g_c += Wc^T g_a
                rc_mm(blob + tab[RT_WCT + b] + (size_t)(32 * w - PI) * Hp, Hp, Hp, actB, lda, lane, gin);
            __syncthreads();                   // every wave has read g_u and g_a
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i)
                if (w + 4 * i < nub) rc_publish<false>(actA, lda, 32 * (w + 4 * i), lane, gt[i]);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < RC_MAXU; ++i) {
                const int ub = w + 4 * i;
                if (ub < nub) {
                    rc_f32x16 d[2] = {rc_f32x16{}, rc_f32x16{}}, hv[2];
                    rc_mm(blob + bt[7] + (size_t)32 * ub * Hp, Hp, Hp, actA, lda, lane, d);        // W1^T g_t
                    rc_load(sh, Hp, 32 * ub, lane, hv);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) g[i][s][r] += hv[s][r] > 0.0f ? d[s][r] : 0.0f;
                }
            }
            __syncthreads();                   // every wave has read g_t
        }
        // ---- initial layer: g_h0 -> G, [g_x | g_c] += W0^T g_h0 ----------------------------------------------------------------------
#pragma unroll
        for (int i = 0; i < RC_MAXU; ++i) {
            const int ub = w + 4 * i;
            if (ub < nub) {
                rc_store(G + row0 * Hp, Hp, 32 * ub, lane, g[i]);
                rc_publish<false>(actA, lda, 32 * ub, lane, g[i]);
            }
        }
        __syncthreads();
        if (has_in) {
            rc_mm(blob + tab[RT_W0T] + (size_t)32 * w * Hp, Hp, Hp, actA, lda, lane, gin);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int64_t row = row0 + 32 * s + n;
                if (row < B)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int p = 32 * w + rc_unit(r, hh);
                        if (p < PI) {
                            if (p < nI) gx[row * nI + p] = gin[s][r];
                        } else if (p - PI < C) {
                            gc[row * C + (p - PI)] = gin[s][r];
                        }
                    }
            }
        }
        __syncthreads();                       // the next tile overwrites the activations
    }
}

// ---- weight gradients ------------------------------------------------------------------------------------------------------------
// job (16 int32, flows/ctx_train_pack.py): dW[n0 .. n0 + 64)[positions k0 .. k0 + 64) of one layer over one chunk of rows
//   0 gsel (-1: g_out, else a G slot)  1 N (valid units)  2 asel (-1: the saved x tile, else a save slot)  3 akoff (position offset)
//   4 KP (positions)  5 relu (of the A operand)  6 K1  7 P1  8 K2 (position p -> column p < P1 ? (p < K1 ? p : -) : K1 + p - P1 if < K2)
//   9 wout (flat offset of dW)  10 ldW (its columns)  11 bout (flat offset of db, -1: none)  12 n0  13 k0
constexpr int RC_JOB = 16;
constexpr int RC_PART = 64 * 64 + 64;

__global__ void __launch_bounds__(RC_THREADS, 2)
rc_wgrad_kernel(const float *__restrict__ gout, const float *__restrict__ save, const float *__restrict__ G, const int *__restrict__ jobs,
                const int *__restrict__ tab, float *__restrict__ part, int njobs, int64_t B, int64_t Bp, int64_t chunk) {
    __shared__ __attribute__((aligned(16))) float red[2][RC_PART];
    const int Hp = tab[RT_HP], NB = tab[RT_NB], Kin = tab[RT_KIN], O = tab[RT_O];
    const int *jb = jobs + (size_t)blockIdx.x * RC_JOB;
    const int gsel = jb[0], N = jb[1], asel = jb[2], akoff = jb[3], KP = jb[4], relu = jb[5], n0 = jb[12], k0 = jb[13];
    const int K1 = jb[6], P1 = jb[7], K2 = jb[8];
    const bool bias = jb[11] >= 0 && k0 == 0;
    const size_t slot = (size_t)Bp * Hp;
    const float *gbase = gsel < 0 ? gout : G + (size_t)gsel * slot;
    const int ldg = gsel < 0 ? O : Hp;
    const float *abase = (asel < 0 ? save + (size_t)(4 * NB + 1) * slot : save + (size_t)asel * slot) + akoff;
    const int lda = asel < 0 ? Kin : Hp;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = lane & 31, hh = lane >> 5;
    bool gok[2], aok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        gok[j] = n0 + 32 * j + n < N;
        const int p = k0 + 32 * j + n;
        aok[j] = p < KP && (p < P1 ? p < K1 : p - P1 < K2);
    }
    const int64_t r_begin = (int64_t)blockIdx.y * chunk;
    int64_t r_end = r_begin + chunk;
    if (r_end > B) r_end = B;
    rc_f32x16 acc[2][2] = {{rc_f32x16{}, rc_f32x16{}}, {rc_f32x16{}, rc_f32x16{}}};
    float bsum[2] = {0.0f, 0.0f};
#pragma unroll 2
    for (int64_t r = r_begin + 2 * w + hh; r - hh < r_end; r += 8) {
        float gv[2] = {0.0f, 0.0f}, av[2] = {0.0f, 0.0f};
        if (r < r_end) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (gok[j]) gv[j] = gbase[r * ldg + n0 + 32 * j + n];
                if (aok[j]) {
                    const float v = abase[r * lda + k0 + 32 * j + n];
                    av[j] = relu ? fmaxf(v, 0.0f) : v;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            bsum[i] += gv[i];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[i], av[j], acc[i][j], 0, 0, 0);
        }
    }
    // the four waves' partial tiles -> one, in a fixed order: ((w0 + w1) + w2) + w3 (each bias sum: lane half 0 + lane half 1)
    bsum[0] += __shfl_xor(bsum[0], 32);
    bsum[1] += __shfl_xor(bsum[1], 32);
    auto put = [&](float *dst) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(32 * i + rc_unit(r, hh)) * 64 + 32 * j + n] = acc[i][j][r];
        if (hh == 0) {
            dst[4096 + n] = bsum[0];
            dst[4096 + 32 + n] = bsum[1];
        }
    };
    if (w < 2) put(red[w]);
    __syncthreads();
    for (int e = tid; e < RC_PART; e += RC_THREADS) red[0][e] += red[1][e];
    __syncthreads();
    for (int v = 2; v < 4; ++v) {
        if (w == v) put(red[1]);
        __syncthreads();
        for (int e = tid; e < RC_PART; e += RC_THREADS) red[0][e] += red[1][e];
        __syncthreads();
    }
    float *dst = part + ((size_t)blockIdx.y * njobs + blockIdx.x) * RC_PART;
    for (int e = tid; e < (bias ? RC_PART : 4096); e += RC_THREADS) dst[e] = red[0][e];
}

__global__ void rc_wgrad_reduce_kernel(const float *__restrict__ part, const int *__restrict__ jobs, float *__restrict__ grads, int njobs,
                                       int nchunks) {
    const int job = blockIdx.x;
    const int *jb = jobs + (size_t)job * RC_JOB;
    const int N = jb[1], KP = jb[4], K1 = jb[6], P1 = jb[7], K2 = jb[8], wout = jb[9], ldW = jb[10], bout = jb[11], n0 = jb[12], k0 = jb[13];
    for (int e = threadIdx.x; e < RC_PART; e += blockDim.x) {
        int dstoff = -1;
        if (e < 4096) {
            const int nl = e >> 6, p = k0 + (e & 63);
            const int col = p >= KP ? -1 : p < P1 ? (p < K1 ? p : -1) : (p - P1 < K2 ? K1 + p - P1 : -1);
            if (n0 + nl < N && col >= 0) dstoff = wout + (n0 + nl) * ldW + col;
        } else if (bout >= 0 && k0 == 0 && n0 + e - 4096 < N) {
            dstoff = bout + n0 + e - 4096;
        }
        if (dstoff < 0) continue;
        float v = 0.0f;
        for (int ch = 0; ch < nchunks; ++ch) v += part[((size_t)ch * njobs + job) * RC_PART + e];     // fixed order: deterministic
        grads[dstoff] = v;
    }
}

static size_t rc_fwd_lds(int Kin, int Hp) { return sizeof(float) * (size_t)RC_ROWS * ((Kin + 4) + (Hp + 4)); }
static size_t rc_bwd_lds(int Hp) { return sizeof(float) * (size_t)RC_ROWS * 2 * ((Hp > 128 ? Hp : 128) + 4); }
static int rc_grid(int64_t Bp) {
    const int64_t nt = Bp / RC_ROWS;
    return persistent_grid(nt);        // persistent: one workgroup per CU
}

}  // namespace nf

// shape checks shared by the three entry points: NF_EINVAL for a malformed call, NF_ENOTSUP outside the built coverage
static int rc_check(int64_t B, int nI, int C, int hidden, int out_features, int num_blocks) {
    if (B < 0 || nI < 1 || C < 1 || hidden < 1 || out_features < 1 || num_blocks < 1) return NF_EINVAL;
    // hidden > 256 (two more unit blocks per wave next to h, t, u and the gate) is not built: it would spill
    if (hidden > 256 || num_blocks > 4) return NF_ENOTSUP;
    const int Kin = (nI + 31) / 32 * 32 + (C + 31) / 32 * 32;
    if (Kin > 128 || out_features > 65536) return NF_ENOTSUP;
    return NF_OK;
}

extern "C" int64_t nf_resnet_ctx_save_floats(int64_t B, int nI, int C, int hidden, int num_blocks) {
    if (B < 0 || nI < 1 || C < 1 || hidden < 1 || num_blocks < 1 || num_blocks > 4) return NF_EINVAL;
    const int64_t Bp = (B + 63) / 64 * 64, Hp = (hidden + 31) / 32 * 32;
    const int64_t Kin = (nI + 31) / 32 * 32 + (C + 31) / 32 * 32;
    return (4 * num_blocks + 1) * Bp * Hp + Bp * Kin;
}

extern "C" int64_t nf_resnet_ctx_grad_floats(int64_t B, int hidden, int num_blocks) {
    if (B < 0 || hidden < 1 || num_blocks < 1 || num_blocks > 4) return NF_EINVAL;
    const int64_t Bp = (B + 63) / 64 * 64, Hp = (hidden + 31) / 32 * 32;
    return (3 * num_blocks + 1) * Bp * Hp;
}

// row chunks of the weight-gradient launch: one per 1024 rows, at most 64, and at most as many as keep the partial tiles within
// RC_PART_CAP floats (a wide final layer has many jobs); a function of (B, njobs) only, so the reduction order is fixed
constexpr int64_t RC_PART_CAP = (int64_t)1 << 25;

extern "C" int nf_resnet_ctx_wgrad_chunks(int64_t B, int njobs) {
    if (B < 0 || njobs < 1) return NF_EINVAL;
    int64_t c = (B + 1023) / 1024;
    c = c < 1 ? 1 : c > 64 ? 64 : c;
    const int64_t fit = RC_PART_CAP / ((int64_t)njobs * nf::RC_PART);
    if (c > fit) c = fit < 1 ? 1 : fit;
    return (int)c;
}

extern "C" int64_t nf_resnet_ctx_scratch_floats(int64_t B, int njobs) {
    if (B < 0 || njobs < 1) return NF_EINVAL;
    return (int64_t)nf_resnet_ctx_wgrad_chunks(B, njobs) * njobs * nf::RC_PART;
}

extern "C" int nf_resnet_ctx_forward_train(const void *x, int64_t ldx, const void *context, int64_t ldc, void *out, void *save,
                                           const void *blob, const int32_t *table, int64_t B, int nI, int C, int hidden,
                                           int out_features, int num_blocks, nf_stream_t stream) {
    const int rc = rc_check(B, nI, C, hidden, out_features, num_blocks);
    if (rc != NF_OK) return rc;
    if (ldx < nI || ldc < 0) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !context || !out || !save || !blob || !table) return NF_EFAULT;
    if (nf_misaligned16(save, blob)) return NF_EINVAL;       // 16-byte stores / loads (x, context, out: element by element)
    const int Hp = (hidden + 31) / 32 * 32, Kin = (nI + 31) / 32 * 32 + (C + 31) / 32 * 32;
    const int64_t Bp = (B + 63) / 64 * 64;
    const size_t lds = nf::rc_fwd_lds(Kin, Hp);
    static nf::LdsOptIn opted;
    if (nf::opt_in_lds(reinterpret_cast<const void *>(&nf::rc_forward_kernel), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL(nf::rc_forward_kernel, dim3(nf::rc_grid(Bp)), dim3(nf::RC_THREADS), lds, (hipStream_t)stream, (const float *)x,
                       ldx, (const float *)context, ldc, (float *)out, (float *)save, (const float *)blob, (const int *)table, B, Bp);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_resnet_ctx_backward(const void *g_out, const void *save, void *G, void *g_x, void *g_context, const void *blob,
                                      const int32_t *table, int64_t B, int nI, int C, int hidden, int out_features, int num_blocks,
                                      nf_stream_t stream) {
    const int rc = rc_check(B, nI, C, hidden, out_features, num_blocks);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!g_out || !save || !G || !g_x || !g_context || !blob || !table) return NF_EFAULT;
    if (nf_misaligned16(save, G, blob)) return NF_EINVAL;    // 16-byte loads / stores (g_out, g_x, g_context: element by element)
    const int Hp = (hidden + 31) / 32 * 32;
    const int64_t Bp = (B + 63) / 64 * 64;
    const size_t lds = nf::rc_bwd_lds(Hp);
    static nf::LdsOptIn opted;
    if (nf::opt_in_lds(reinterpret_cast<const void *>(&nf::rc_backward_kernel), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL(nf::rc_backward_kernel, dim3(nf::rc_grid(Bp)), dim3(nf::RC_THREADS), lds, (hipStream_t)stream,
                       (const float *)g_out, (const float *)save, (float *)G, (float *)g_x, (float *)g_context, (const float *)blob,
                       (const int *)table, B, Bp);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_resnet_ctx_wgrad(const void *g_out, const void *save, const void *G, void *grads, void *part, const int32_t *jobs,
                                   int njobs, const int32_t *table, int64_t B, int hidden, int num_blocks, nf_stream_t stream) {
    if (B < 0 || njobs < 1 || hidden < 1 || num_blocks < 1) return NF_EINVAL;
    if (hidden > 256 || num_blocks > 4) return NF_ENOTSUP;
    if (B == 0) return NF_OK;
    if (!g_out || !save || !G || !grads || !part || !jobs || !table) return NF_EFAULT;
    const int64_t Bp = (B + 63) / 64 * 64;
    const int nch = nf_resnet_ctx_wgrad_chunks(B, njobs);
    const int64_t chunk = ((B + nch - 1) / nch + 7) / 8 * 8;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nf::rc_wgrad_kernel, dim3((unsigned)njobs, (unsigned)nch), dim3(nf::RC_THREADS), 0, st, (const float *)g_out,
                       (const float *)save, (const float *)G, (const int *)jobs, (const int *)table, (float *)part, njobs, B, Bp, chunk);
    NF_CHECK_LAUNCH();
    hipLaunchKernelGGL(nf::rc_wgrad_reduce_kernel, dim3((unsigned)njobs), dim3(256), 0, st, (const float *)part, (const int *)jobs,
                       (float *)grads, njobs, nch);
    NF_CHECK_LAUNCH();
    return NF_OK;
}
