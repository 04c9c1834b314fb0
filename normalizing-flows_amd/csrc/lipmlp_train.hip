// lipmlp_train.hip -- training of ONE residual-flow layer y = x + g(x), g a LipschitzMLP on 2-D rows, for gfx950: one forward launch
// (value, log-det estimate and the estimate's cotangent of the Jacobian) and one backward launch plus a fixed-order slab reduction.
//
// Reference semantics: normflows/flows/residual.py:143-268 (iResBlock._logdetgrad and its estimators, MemoryEfficientLogDetEstimator).
// On 2-D rows every estimator is a closed-form function of the exact 2 x 2 Jacobian J of g, which lm_net (lipmlp_net.hpp) computes
// with two forward-mode tangent streams; so the forward kernel evaluates the estimator per row in registers and hands the backward
// ONE cotangent per row, Jhat = d ld / d J, whatever the estimator was.
//
// Notation (the Swish comes first; p_0 = x, tau_0^j = e_j; layer l = 0 .. L):
//     a_l = f(p_l; c_l)      alpha_l^j = f'(p_l) tau_l^j      p_{l+1} = W_l a_l + b_l      tau_{l+1}^j = W_l alpha_l^j
//     g = p_{L+1}            J[:, j] = tau_{L+1}^j
// Backward, from phat_{L+1} = gy and tauhat_{L+1}^j = w Jhat[:, j] (w: the row's log-det cotangent):
//     ahat_l = W_l^T phat_{l+1}      alphahat_l^j = W_l^T tauhat_{l+1}^j      tauhat_l^j = f'(p_l) alphahat_l^j
//     phat_l = f'(p_l) ahat_l + f''(p_l) sum_j tau_l^j alphahat_l^j
//     What_l += phat_{l+1} a_l^T + sum_j tauhat_{l+1}^j alpha_l^jT      bhat_l += phat_{l+1}
//     chat_l += sum [df/dc ahat_l + df'/dc sum_j tau_l^j alphahat_l^j]      gx = gy + phat_0
// with s = sigmoid(c p), q = s (1 - s) (2 + c p (1 - 2 s)) / 1.1:  f'' = c q,  df/dc = p^2 s (1 - s) / 1.1,  df'/dc = p q.
//
// Backward mapping (template <HP, VEC>): 256 lanes own a tile of TR = 2048 / HP rows.  LDS holds the pre-activations (p_l, tau_l^0,
// tau_l^1) of up to three hidden layers and one three-stream work buffer C: 12 planes of TR x (HP + 4) floats; 100-113 KiB with the
// row buffers.  The tile's forward is recomputed into them (C carries the activations between products), then C carries the cotangents down.  In a
// transposed hidden product lane (rg, cg) owns rows 2 rg, 2 rg + 1 and columns 4 cg .. 4 cg + 3 of all three streams; the Swish
// backward is lane-local on the same positions and leaves (a_l, alpha_l^j) in place of the pre-activations for the weight gradient.
// The weight gradient of a hidden layer is a (HP x HP) outer-product sum over rows and streams: lane (kg, og) owns a T x T block,
// T = HP / 16.  Parameter gradients are accumulated over the tiles a persistent workgroup walks in that workgroup's own slab of
// blob-many floats (one read-modify-write per element and tile by the lane that owns it; 64 accumulators per hidden layer and lane
// would not stay in registers next to the products), then the slabs are summed in a fixed order (train_reduce.hpp).  Plain fp32
// FMAs, no atomics: bit-identical from run to run.  A row past the batch runs on zeros with zero cotangents.
#include "lipmlp_net.hpp"
#include "train_reduce.hpp"

namespace nf {

constexpr int LT_MAXTERMS = 32;
struct LtCoef { float c[LT_MAXTERMS]; };      // coeff(k) of series term k = 1 .. nterms, by value in the launch arguments

static inline int lt_rows(int hp) { return 2048 / hp; }
static inline size_t lt_lds_bytes(int hp) { return sizeof(float) * ((size_t)12 * lt_rows(hp) * (hp + 4) + 18 * lt_rows(hp) + 16); }

// ---- forward ------------------------------------------------------------------------------------------------------------------
// kind 0: log|det(I + J)|; 1: Hutchinson sum_k a_k v^T J^k v; 2: Neumann n^T J v, n = v + sum_k (-1)^k coeff(k) v^T J^k held constant;
// 3: exact trace sum_k a_k tr(J^k); a_k = (-1)^(k+1) coeff(k) / k.  Jh[2 i + j] = d ld / d J_ij.
__device__ __forceinline__ void lt_estimate(int kind, int nterms, const LtCoef &coef, float J00, float J01, float J10, float J11,
                                            float v0, float v1, float &ld, float *Jh) {
    if (kind == 0) {
        const float det = (J00 + 1.0f) * (J11 + 1.0f) - J01 * J10;
        ld = M<float>::log(fabsf(det));
        const float id = 1.0f / det;
        Jh[0] = (J11 + 1.0f) * id, Jh[1] = -J10 * id, Jh[2] = -J01 * id, Jh[3] = (J00 + 1.0f) * id;
        return;
    }
    ld = 0.0f;
    Jh[0] = Jh[1] = Jh[2] = Jh[3] = 0.0f;
    float sgn = 1.0f;                       // (-1)^(k+1)
    if (kind == 1) {                        // G_k = sum_{m<k} (v^T J^m)^T (J^(k-1-m) v)^T: G_1 = v v^T, G_{k+1} = G_k J^T + L_k^T v^T
        float L0 = v0, L1 = v1, G00 = v0 * v0, G01 = v0 * v1, G10 = v1 * v0, G11 = v1 * v1;
        for (int k = 1; k <= nterms; ++k) {
            const float n0 = fmaf(L1, J10, L0 * J00), n1 = fmaf(L1, J11, L0 * J01);
            L0 = n0, L1 = n1;
            const float a = sgn * coef.c[k - 1] / (float)k;
            ld = fmaf(a, fmaf(L1, v1, L0 * v0), ld);
            Jh[0] = fmaf(a, G00, Jh[0]), Jh[1] = fmaf(a, G01, Jh[1]), Jh[2] = fmaf(a, G10, Jh[2]), Jh[3] = fmaf(a, G11, Jh[3]);
            const float h00 = fmaf(G01, J01, G00 * J00) + L0 * v0, h01 = fmaf(G01, J11, G00 * J10) + L0 * v1;
            const float h10 = fmaf(G11, J01, G10 * J00) + L1 * v0, h11 = fmaf(G11, J11, G10 * J10) + L1 * v1;
            G00 = h00, G01 = h01, G10 = h10, G11 = h11;
            sgn = -sgn;
        }
    } else if (kind == 2) {
        float L0 = v0, L1 = v1, n0 = v0, n1 = v1;
        for (int k = 1; k <= nterms; ++k) {
            const float m0 = fmaf(L1, J10, L0 * J00), m1 = fmaf(L1, J11, L0 * J01);
            L0 = m0, L1 = m1;
            sgn = -sgn;                     // (-1)^k
            n0 = fmaf(sgn * coef.c[k - 1], L0, n0);
            n1 = fmaf(sgn * coef.c[k - 1], L1, n1);
        }
        ld = n0 * fmaf(J01, v1, J00 * v0) + n1 * fmaf(J11, v1, J10 * v0);
        Jh[0] = n0 * v0, Jh[1] = n0 * v1, Jh[2] = n1 * v0, Jh[3] = n1 * v1;
    } else {                                // P = J^(k-1)
        float P00 = 1.0f, P01 = 0.0f, P10 = 0.0f, P11 = 1.0f;
        for (int k = 1; k <= nterms; ++k) {
            const float a = sgn * coef.c[k - 1] / (float)k, ak = a * (float)k;
            Jh[0] = fmaf(ak, P00, Jh[0]), Jh[1] = fmaf(ak, P10, Jh[1]), Jh[2] = fmaf(ak, P01, Jh[2]), Jh[3] = fmaf(ak, P11, Jh[3]);
            const float q00 = fmaf(P01, J10, P00 * J00), q01 = fmaf(P01, J11, P00 * J01);
            const float q10 = fmaf(P11, J10, P10 * J00), q11 = fmaf(P11, J11, P10 * J01);
            P00 = q00, P01 = q01, P10 = q10, P11 = q11;
            ld = fmaf(a, P00 + P11, ld);
            sgn = -sgn;
        }
    }
}

template <int HP, bool VEC>
__global__ void __launch_bounds__(LM_THREADS)
lipmlp_train_fwd_kernel(const float *__restrict__ x, const float *__restrict__ vareps, float *__restrict__ y, float *__restrict__ ld,
                        float *__restrict__ jhat, const float *__restrict__ blob, int64_t B, int kind, int nterms, LtCoef coef) {
    constexpr int R = 4096 / HP, LDH = HP + 4;
    extern __shared__ __attribute__((aligned(16))) float lm_lds[];
    float *H = lm_lds, *xs = H + 3 * R * LDH, *rowA = xs + 2 * R, *res = rowA + 4 * R;
    const int tid = threadIdx.x;
    const int64_t ntiles = (B + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * R + tid;
        const bool valid = tid < R && row < B;         // a row past the batch runs on zeros
        if (tid < R) {
            xs[2 * tid] = valid ? x[2 * row] : 0.0f;
            xs[2 * tid + 1] = valid ? x[2 * row + 1] : 0.0f;
        }
        __syncthreads();
        lm_net<HP, 3, VEC>(H, rowA, res, xs, blob, blob + LM_HDR);
        if (valid) {
            const float *r6 = res + 6 * tid;           // [g_0, g_1, J00, J10, J01, J11]
            const float v0 = vareps ? vareps[2 * row] : 0.0f, v1 = vareps ? vareps[2 * row + 1] : 0.0f;
            float l, Jh[4];
            lt_estimate(kind, nterms, coef, r6[2], r6[4], r6[3], r6[5], v0, v1, l, Jh);
            y[2 * row] = xs[2 * tid] + r6[0];
            y[2 * row + 1] = xs[2 * tid + 1] + r6[1];
            ld[row] = l;
            *reinterpret_cast<float4 *>(jhat + 4 * row) = make_float4(Jh[0], Jh[1], Jh[2], Jh[3]);
        }
        __syncthreads();
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// The Swish at pre-activation p with slope c: value h, derivative dh, q (f'' = c q, df'/dc = p q) and dc = df/dc.
__device__ __forceinline__ void lt_swish2(float p, float c, float &h, float &dh, float &q, float &dc) {
    const float s = 1.0f / (1.0f + M<float>::exp(-c * p));
    const float ss = s * (1.0f - s);
    h = p * s / 1.1f;
    dh = (s + c * p * ss) / 1.1f;
    q = ss * (2.0f + c * p * (1.0f - 2.0f * s)) / 1.1f;
    dc = p * p * ss / 1.1f;
}

// T consecutive floats of LDS at a T-float boundary.
template <int T> __device__ __forceinline__ void lt_ldT(const float *p, float *o) {
    if (T == 8) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
    } else if (T == 4) {
        const float4 a = *reinterpret_cast<const float4 *>(p);
        o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
    } else {
        const float2 a = *reinterpret_cast<const float2 *>(p);
        o[0] = a.x, o[1] = a.y;
    }
}

// cacc[i] += v for a wave-uniform i in 0 .. 3, with static register indexing.
__device__ __forceinline__ void lt_cadd(float *cacc, int i, float v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cacc[k] += k == i ? v : 0.0f;
}

template <int HP, bool VEC>
__global__ void __launch_bounds__(LM_THREADS)
lipmlp_train_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gy, const float *__restrict__ jhat,
                        const float *__restrict__ wld, float *__restrict__ gx, const float *__restrict__ blob,
                        float *__restrict__ slabs, int64_t nblob, int64_t B, int want) {
    constexpr int TR = 2048 / HP, LDH = HP + 4, PL = TR * LDH, CT = HP / 4, T = HP / 16;
    extern __shared__ __attribute__((aligned(16))) float lm_lds[];
    float *S = lm_lds;                      // [3 layers][3 streams][PL]: (p, tau^0, tau^1), later (a, alpha^0, alpha^1)
    float *Cw = S + 9 * PL;                 // [3 streams][PL]: activations going forward, cotangents going backward
    float *xs = Cw + 3 * PL;                // [TR][2]
    float *rowA = xs + 2 * TR;              // [TR][4]: a_0 (2), f'(x) (2)
    float *cot = rowA + 4 * TR;             // [TR][6]: phat_{L+1} (2), tauhat^0 (2), tauhat^1 (2)
    float *rowB = cot + 6 * TR;             // [TR][6]: ahat_0 (2), alphahat_0^0 (2), alphahat_0^1 (2)
    float *red = rowB + 6 * TR;             // [4 waves][4]
    const int tid = threadIdx.x;
    const float *hdr = blob, *W = blob + LM_HDR;
    int nmid = (int)hdr[1];
    nmid = nmid < 0 ? 0 : (nmid > 2 ? 2 : nmid);
    float *slab = want ? slabs + (size_t)blockIdx.x * nblob : nullptr;
    float *sW = want ? slab + LM_HDR : nullptr;
    if (want) {
        for (int64_t e = tid; e < nblob; e += LM_THREADS) slab[e] = 0.0f;
        __threadfence_block();
        __syncthreads();
    }
    const float *W0 = W, *Wl = W + 3 * HP + 2 * (HP * HP + HP);
    constexpr int OFF_L = 3 * HP + 2 * (HP * HP + HP);
    const int cg = tid % CT, rg = tid / CT;
    const int kg = tid / 16, og = tid % 16;
    float cacc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t ntiles = (B + TR - 1) / TR;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * TR + tid;
        const bool valid = tid < TR && row < B;
        if (tid < TR) {                    // the input, its Swish, and the cotangents of g and J; zeros past the batch
            const float x0 = valid ? x[2 * row] : 0.0f, x1 = valid ? x[2 * row + 1] : 0.0f;
            xs[2 * tid] = x0, xs[2 * tid + 1] = x1;
            float a0, a1, d0, d1;
            lm_swish(x0, hdr[2], a0, d0);
            lm_swish(x1, hdr[2], a1, d1);
            rowA[4 * tid] = a0, rowA[4 * tid + 1] = a1, rowA[4 * tid + 2] = d0, rowA[4 * tid + 3] = d1;
            const float wv = (valid && wld) ? wld[row] : 0.0f;
            float4 jh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (valid && wld) jh = *reinterpret_cast<const float4 *>(jhat + 4 * row);
            cot[6 * tid] = (valid && gy) ? gy[2 * row] : 0.0f;
            cot[6 * tid + 1] = (valid && gy) ? gy[2 * row + 1] : 0.0f;
            cot[6 * tid + 2] = wv * jh.x, cot[6 * tid + 3] = wv * jh.z;      // tauhat^0 = w Jhat[:, 0]
            cot[6 * tid + 4] = wv * jh.y, cot[6 * tid + 5] = wv * jh.w;      // tauhat^1 = w Jhat[:, 1]
        }
        __syncthreads();
        // ---- the tile's forward again: S[l] <- pre-activations of hidden layer l + 1
        {
            const float *b0 = W + 2 * HP;
            const float c = hdr[3];
            for (int idx = tid; idx < TR * HP; idx += LM_THREADS) {
                const int r = idx / HP, o = idx % HP;
                const float w0 = W0[o], w1 = W0[HP + o];
                const float pre = fmaf(w1, rowA[4 * r + 1], fmaf(w0, rowA[4 * r], b0[o]));
                const float t0 = w0 * rowA[4 * r + 2], t1 = w1 * rowA[4 * r + 3];
                S[r * LDH + o] = pre, S[PL + r * LDH + o] = t0, S[2 * PL + r * LDH + o] = t1;
                if (nmid > 0) {
                    float h, dh;
                    lm_swish(pre, c, h, dh);
                    Cw[r * LDH + o] = h, Cw[PL + r * LDH + o] = t0 * dh, Cw[2 * PL + r * LDH + o] = t1 * dh;
                }
            }
        }
        __syncthreads();
        for (int m = 0; m < nmid; ++m) {
            const float *Wm = W + 3 * HP + (size_t)m * (HP * HP + HP), *bm = Wm + HP * HP;
            float acc[3][2][4];
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[s][i][j] = 0.0f;
            for (int k = 0; k < HP; k += 4) {
                float4 w[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) w[kk] = lm_ld4<VEC>(Wm + (k + kk) * HP + 4 * cg);
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const float4 a = *reinterpret_cast<const float4 *>(Cw + s * PL + (2 * rg + i) * LDH + k);
                        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            acc[s][i][0] = fmaf(av[kk], w[kk].x, acc[s][i][0]);
                            acc[s][i][1] = fmaf(av[kk], w[kk].y, acc[s][i][1]);
                            acc[s][i][2] = fmaf(av[kk], w[kk].z, acc[s][i][2]);
                            acc[s][i][3] = fmaf(av[kk], w[kk].w, acc[s][i][3]);
                        }
                    }
            }
            __syncthreads();               // every lane has read the layer's input: Cw is free to take the next one
            const float4 b4 = lm_ld4<VEC>(bm + 4 * cg);
            const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
            const float c = hdr[4 + m];
            float *Sm = S + (m + 1) * 3 * PL;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int off = (2 * rg + i) * LDH + 4 * cg;
                const float pv[4] = {acc[0][i][0] + bv[0], acc[0][i][1] + bv[1], acc[0][i][2] + bv[2], acc[0][i][3] + bv[3]};
                *reinterpret_cast<float4 *>(Sm + off) = make_float4(pv[0], pv[1], pv[2], pv[3]);
                *reinterpret_cast<float4 *>(Sm + PL + off) = make_float4(acc[1][i][0], acc[1][i][1], acc[1][i][2], acc[1][i][3]);
                *reinterpret_cast<float4 *>(Sm + 2 * PL + off) = make_float4(acc[2][i][0], acc[2][i][1], acc[2][i][2], acc[2][i][3]);
                if (m + 1 < nmid) {
                    float hv[4], dv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) lm_swish(pv[j], c, hv[j], dv[j]);
                    *reinterpret_cast<float4 *>(Cw + off) = make_float4(hv[0], hv[1], hv[2], hv[3]);
#pragma unroll
                    for (int s = 1; s < 3; ++s)
                        *reinterpret_cast<float4 *>(Cw + s * PL + off) =
                            make_float4(acc[s][i][0] * dv[0], acc[s][i][1] * dv[1], acc[s][i][2] * dv[2], acc[s][i][3] * dv[3]);
                }
            }
            __syncthreads();
        }
        // ---- the last linear layer transposed and the Swish in front of it: Cw <- cotangents of hidden layer nmid + 1
        {
            float *Sl = S + nmid * 3 * PL;
            const float c = hdr[3 + nmid];
            float csum = 0.0f;
            for (int idx = tid; idx < TR * HP; idx += LM_THREADS) {
                const int r = idx / HP, k = idx % HP;
                const float u0 = Wl[k], u1 = Wl[HP + k];
                const float *ct = cot + 6 * r;
                const float ah = fmaf(u1, ct[1], u0 * ct[0]), al0 = fmaf(u1, ct[3], u0 * ct[2]), al1 = fmaf(u1, ct[5], u0 * ct[4]);
                const int off = r * LDH + k;
                const float p = Sl[off], t0 = Sl[PL + off], t1 = Sl[2 * PL + off];
                float h, dh, q, dc;
                lt_swish2(p, c, h, dh, q, dc);
                const float ta = fmaf(t1, al1, t0 * al0);
                Cw[off] = fmaf(c * q, ta, dh * ah), Cw[PL + off] = dh * al0, Cw[2 * PL + off] = dh * al1;
                Sl[off] = h, Sl[PL + off] = dh * t0, Sl[2 * PL + off] = dh * t1;
                csum += fmaf(p * q, ta, dc * ah);
            }
            lt_cadd(cacc, 1 + nmid, csum);
        }
        __syncthreads();
        if (want) {                        // What_last (2, HP), bhat_last (2)
            const float *Sl = S + nmid * 3 * PL;
            for (int idx = tid; idx < 2 * HP; idx += LM_THREADS) {
                const int i = idx / HP, k = idx % HP;
                float g = 0.0f;
                for (int r = 0; r < TR; ++r) {
                    const float *ct = cot + 6 * r;
                    g = fmaf(ct[i], Sl[r * LDH + k], g);
                    g = fmaf(ct[2 + i], Sl[PL + r * LDH + k], g);
                    g = fmaf(ct[4 + i], Sl[2 * PL + r * LDH + k], g);
                }
                sW[OFF_L + idx] += g;
            }
            if (tid < 2) {
                float g = 0.0f;
                for (int r = 0; r < TR; ++r) g += cot[6 * r + tid];
                sW[OFF_L + 2 * HP + tid] += g;
            }
        }
        // ---- the hidden products transposed, last to first
        for (int m = nmid - 1; m >= 0; --m) {
            const float *Wm = W + 3 * HP + (size_t)m * (HP * HP + HP);
            float *Sm = S + m * 3 * PL;
            float acc[3][2][4];
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[s][i][j] = 0.0f;
            for (int o = 0; o < HP; o += 4) {
                float4 w[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) w[kk] = lm_ld4<VEC>(Wm + (4 * cg + kk) * HP + o);
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const float4 a = *reinterpret_cast<const float4 *>(Cw + s * PL + (2 * rg + i) * LDH + o);
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
                            acc[s][i][kk] = fmaf(a.w, w[kk].w, fmaf(a.z, w[kk].z, fmaf(a.y, w[kk].y, fmaf(a.x, w[kk].x, acc[s][i][kk]))));
                    }
            }
            // the Swish in front of this product, lane-local: the new cotangents wait in registers while Cw is still read
            const float c = hdr[3 + m];
            float csum = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int off = (2 * rg + i) * LDH + 4 * cg;
                const float4 p4 = *reinterpret_cast<const float4 *>(Sm + off);
                const float4 t04 = *reinterpret_cast<const float4 *>(Sm + PL + off);
                const float4 t14 = *reinterpret_cast<const float4 *>(Sm + 2 * PL + off);
                const float pv[4] = {p4.x, p4.y, p4.z, p4.w}, t0v[4] = {t04.x, t04.y, t04.z, t04.w}, t1v[4] = {t14.x, t14.y, t14.z, t14.w};
                float hv[4], a0v[4], a1v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float dh, q, dc;
                    lt_swish2(pv[j], c, hv[j], dh, q, dc);
                    const float ah = acc[0][i][j], al0 = acc[1][i][j], al1 = acc[2][i][j];
                    const float ta = fmaf(t1v[j], al1, t0v[j] * al0);
                    acc[0][i][j] = fmaf(c * q, ta, dh * ah), acc[1][i][j] = dh * al0, acc[2][i][j] = dh * al1;
                    a0v[j] = dh * t0v[j], a1v[j] = dh * t1v[j];
                    csum += fmaf(pv[j] * q, ta, dc * ah);
                }
                *reinterpret_cast<float4 *>(Sm + off) = make_float4(hv[0], hv[1], hv[2], hv[3]);
                *reinterpret_cast<float4 *>(Sm + PL + off) = make_float4(a0v[0], a0v[1], a0v[2], a0v[3]);
                *reinterpret_cast<float4 *>(Sm + 2 * PL + off) = make_float4(a1v[0], a1v[1], a1v[2], a1v[3]);
            }
            lt_cadd(cacc, 1 + m, csum);
            __syncthreads();               // Sm holds (a, alpha^j) of every lane; Cw still the cotangents behind the product
            if (want) {                    // What_m (HP, HP) [k][o] and bhat_m (HP)
                float g[T][T];
#pragma unroll
                for (int a = 0; a < T; ++a)
#pragma unroll
                    for (int b = 0; b < T; ++b) g[a][b] = 0.0f;
                for (int r = 0; r < TR; ++r)
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        float av[T], cv[T];
                        lt_ldT<T>(Sm + s * PL + r * LDH + T * kg, av);
                        lt_ldT<T>(Cw + s * PL + r * LDH + T * og, cv);
#pragma unroll
                        for (int a = 0; a < T; ++a)
#pragma unroll
                            for (int b = 0; b < T; ++b) g[a][b] = fmaf(av[a], cv[b], g[a][b]);
                    }
                float *gW = sW + 3 * HP + (size_t)m * (HP * HP + HP);
#pragma unroll
                for (int a = 0; a < T; ++a)
#pragma unroll
                    for (int b = 0; b < T; ++b) gW[(T * kg + a) * HP + T * og + b] += g[a][b];
                if (tid < HP) {
                    float gb = 0.0f;
                    for (int r = 0; r < TR; ++r) gb += Cw[r * LDH + tid];
                    gW[HP * HP + tid] += gb;
                }
            }
            __syncthreads();               // Cw has been read by every lane
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int off = (2 * rg + i) * LDH + 4 * cg;
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    *reinterpret_cast<float4 *>(Cw + s * PL + off) = make_float4(acc[s][i][0], acc[s][i][1], acc[s][i][2], acc[s][i][3]);
            }
            __syncthreads();
        }
        // ---- the first linear layer transposed: rowB <- (ahat_0, alphahat_0^0, alphahat_0^1) per row
        for (int it = tid; it < 6 * TR; it += LM_THREADS) {
            const int s = it / (2 * TR), i = (it / TR) % 2, r = it % TR;
            const float *cp = Cw + s * PL + r * LDH, *wp = W0 + i * HP;
            float o0 = 0.0f;
            for (int k = 0; k < HP; k += 4) {
                const float4 a = *reinterpret_cast<const float4 *>(cp + k);
                const float4 u = lm_ld4<VEC>(wp + k);
                o0 = fmaf(a.w, u.w, fmaf(a.z, u.z, fmaf(a.y, u.y, fmaf(a.x, u.x, o0))));
            }
            rowB[6 * r + 2 * s + i] = o0;
        }
        if (want) {                        // What_0 (2, HP) [i][o] and bhat_0 (HP): alpha_0^j = f'(x_j) e_j
            for (int idx = tid; idx < 2 * HP; idx += LM_THREADS) {
                const int i = idx / HP, o = idx % HP;
                float g = 0.0f;
                for (int r = 0; r < TR; ++r) {
                    g = fmaf(Cw[r * LDH + o], rowA[4 * r + i], g);
                    g = fmaf(Cw[(1 + i) * PL + r * LDH + o], rowA[4 * r + 2 + i], g);
                }
                sW[idx] += g;
            }
            if (tid < HP) {
                float gb = 0.0f;
                for (int r = 0; r < TR; ++r) gb += Cw[r * LDH + tid];
                sW[2 * HP + tid] += gb;
            }
        }
        __syncthreads();
        if (tid < TR) {                    // the input Swish: tau_0^j = e_j
            const float c = hdr[2];
            float csum = 0.0f, ph[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float h, dh, q, dc;
                lt_swish2(xs[2 * tid + i], c, h, dh, q, dc);
                const float ah = rowB[6 * tid + i], ta = rowB[6 * tid + 2 + 3 * i];   // alphahat_0^i[i]
                ph[i] = fmaf(c * q, ta, dh * ah);
                csum += fmaf(xs[2 * tid + i] * q, ta, dc * ah);
            }
            cacc[0] += csum;
            if (valid && gx) {
                gx[2 * row] = cot[6 * tid] + ph[0];
                gx[2 * row + 1] = cot[6 * tid + 1] + ph[1];
            }
        }
        __syncthreads();
    }
    if (want) {                            // chat of the four Swish slopes: lanes of a wave, then the waves, in a fixed order
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cacc[k] += __shfl_xor(cacc[k], o, 64);
            if ((tid & 63) == 0) red[4 * (tid >> 6) + k] = cacc[k];
        }
        __syncthreads();
        if (tid < 4) slab[2 + tid] = (red[tid] + red[4 + tid]) + (red[8 + tid] + red[12 + tid]);
    }
}

// gblob[e] = sum over the workgroups' slabs in a fixed order (train_reduce.hpp: chunk lanes, then lane order).
__global__ void __launch_bounds__(64 * RL)
lipmlp_train_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ gblob, int64_t n, int chunks) {
    __shared__ float sm[RL][64];
    for (int64_t e0 = (int64_t)blockIdx.x * 64; e0 < n; e0 += (int64_t)gridDim.x * 64)
        wgrad_reduce_group(slabs, gblob, nullptr, n, n, n, chunks, 0, 1, 0, nullptr, 0, e0, sm);
}

static int lt_check(int64_t B, int hp, int64_t nblob) {
    if (hp != 32 && hp != 64 && hp != 128) return NF_ENOTSUP;
    if (B < 0) return NF_EINVAL;
    if (nblob != LM_HDR + lm_rstride(hp)) return NF_EINVAL;
    return NF_OK;
}

static inline int lt_bwd_grid(int64_t B, int hp) { return persistent_grid((B + lt_rows(hp) - 1) / lt_rows(hp)); }

static LdsOptIn lt_optin[6];

}  // namespace nf

extern "C" int nf_lipmlp_train_rows(int hp) { return hp != 32 && hp != 64 && hp != 128 ? NF_ENOTSUP : nf::lt_rows(hp); }

extern "C" int64_t nf_lipmlp_train_scratch_floats(int64_t B, int hp) {
    if (hp != 32 && hp != 64 && hp != 128) return NF_ENOTSUP;
    if (B < 0) return NF_EINVAL;
    return (int64_t)nf::lt_bwd_grid(B, hp) * (nf::LM_HDR + nf::lm_rstride(hp));
}

extern "C" int nf_lipmlp_train_fwd(const void *x, const void *vareps, void *y, void *ld, void *jhat, const void *blob, int64_t nblob,
                                   int64_t B, int hp, int kind, int nterms, const float *coef, nf_stream_t stream) {
    const int rc = nf::lt_check(B, hp, nblob);
    if (rc != NF_OK) return rc;
    if (kind < 0 || kind > 3) return NF_EINVAL;
    if (kind != 0 && nterms > nf::LT_MAXTERMS) return NF_ERANGE;
    if (kind != 0 && nterms < 1) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !y || !ld || !jhat || !blob || (kind != 0 && !coef) || ((kind == 1 || kind == 2) && !vareps)) return NF_EFAULT;
    if (nf_misaligned16(jhat)) return NF_EINVAL;
    nf::LtCoef cf;
    for (int k = 0; k < nf::LT_MAXTERMS; ++k) cf.c[k] = (kind != 0 && k < nterms) ? coef[k] : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    const int grid = nf::persistent_grid((B + nf::lm_rows(hp) - 1) / nf::lm_rows(hp));
    const size_t lds = nf::lm_lds_bytes(hp, 3);
    const bool vec = !nf_misaligned16(blob);
#define NF_LT_FWD(HP, VEC)                                                                                                       \
    hipLaunchKernelGGL((nf::lipmlp_train_fwd_kernel<HP, VEC>), dim3(grid), dim3(nf::LM_THREADS), lds, st, (const float *)x,      \
                       (const float *)vareps, (float *)y, (float *)ld, (float *)jhat, (const float *)blob, B, kind,              \
                       kind == 0 ? 0 : nterms, cf)
    if (hp == 32) { if (vec) NF_LT_FWD(32, true); else NF_LT_FWD(32, false); }
    else if (hp == 64) { if (vec) NF_LT_FWD(64, true); else NF_LT_FWD(64, false); }
    else { if (vec) NF_LT_FWD(128, true); else NF_LT_FWD(128, false); }
#undef NF_LT_FWD
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_lipmlp_train_bwd(const void *x, const void *gy, const void *jhat, const void *w, void *gx, const void *blob,
                                   void *slabs, void *gblob, int64_t nblob, int64_t B, int hp, int want, nf_stream_t stream) {
    const int rc = nf::lt_check(B, hp, nblob);
    if (rc != NF_OK) return rc;
    if (want != 0 && want != 1) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !blob || (w && !jhat) || (want && (!slabs || !gblob))) return NF_EFAULT;
    if (nf_misaligned16(jhat)) return NF_EINVAL;
    if (!gx && !want) return NF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int grid = nf::lt_bwd_grid(B, hp);
    const size_t lds = nf::lt_lds_bytes(hp);
    const bool vec = !nf_misaligned16(blob);
#define NF_LT_BWD(HP, VEC, SLOT)                                                                                                 \
    do {                                                                                                                         \
        const int orc = nf::opt_in_lds((const void *)nf::lipmlp_train_bwd_kernel<HP, VEC>, lds, nf::lt_optin[SLOT]);             \
        if (orc != NF_OK) return orc;                                                                                            \
        hipLaunchKernelGGL((nf::lipmlp_train_bwd_kernel<HP, VEC>), dim3(grid), dim3(nf::LM_THREADS), lds, st, (const float *)x,  \
                           (const float *)gy, (const float *)jhat, (const float *)w, (float *)gx, (const float *)blob,           \
                           (float *)slabs, nblob, B, want);                                                                      \
    } while (0)
    if (hp == 32) { if (vec) NF_LT_BWD(32, true, 0); else NF_LT_BWD(32, false, 1); }
    else if (hp == 64) { if (vec) NF_LT_BWD(64, true, 2); else NF_LT_BWD(64, false, 3); }
    else { if (vec) NF_LT_BWD(128, true, 4); else NF_LT_BWD(128, false, 5); }
#undef NF_LT_BWD
    NF_CHECK_LAUNCH();
    if (want) {
        hipLaunchKernelGGL(nf::lipmlp_train_reduce_kernel, dim3(nf::grid_for(nblob, 64)), dim3(64 * nf::RL), 0, st,
                           (const float *)slabs, (float *)gblob, nblob, grid);
        NF_CHECK_LAUNCH();
    }
    return NF_OK;
}
