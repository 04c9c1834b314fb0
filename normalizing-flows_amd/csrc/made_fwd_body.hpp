// made_fwd_body.hpp -- the BODY of the one-launch MADE forward kernels, included between the braces of made_fwd.hip's made_fwd_kernel
// (every epilogue; read its header comment first) and of made_fwd_train_ft.hip's made_fwd_train_ft_kernel (EPI 3 behind a gathered,
// fed x tile).  A text fragment and not a function: inlined through a call the existing instantiations came out with other
// registers (the 128-row tile spilled two more values), and a further template parameter would rename them.  The including kernel
// provides: NSB, EPI, TR, FT (compile-time), x, y, logdet, blob, table, B, acc_mode, p, save, bits, Bp, x_pad, direction.
//
// FT (nf_made_forward_train_ft): the x tile of made_fwd_ft.hip in front of EPI 3 -- the MADE of the autoregressive spline layers with a
// permuted mask and / or the periodic preprocessing of utils/nn.py:64-129 (nets/made.py:250-252) under autograd.  The tile is
// GATHERED in degree order through the training feature table that FOLLOWS the items in `table` (tt = int32 [3][D]: col | scale
// (float bits) | index of the position's periodic feature or -1), the initial layer contracts over the FED values (w_sin sin(s x) +
// w_cos cos(s x) + bias for a periodic position; the three per position follow the streams in `blob` at table[9] = [3][D], gathered
// from the live preprocessing.weights / .bias with the weight streams by nf_pack_gather: flows/made_pack.made_train_structure_ft),
// and besides EPI 3's outputs the kernel leaves the raw values in position order (x_pos (B, D), the spline's input, through the
// `logdet` argument EPI 3 does not use) and the fed values in the padded shape nf_made_wgrad takes (x_pad (Bp, 128), zeros beyond the
// batch and beyond D).  No pointer but x_pad is added to EPI 3's arguments: the 512-slot and the 128-row instantiations have no
// registers to spare.

// EPI 0: z = scale x + shift, logdet = sum log scale (autoregressive.py:101-110, :124-128: rows 2 f = unconstrained scale, 2 f + 1
// = shift);  EPI 1: the raw MADE output (B, mult D) for the callers that apply another element-wise transform;  EPI 2: the
// autoregressive rational-quadratic spline of neural_spline/autoregressive.py:94-134 (density direction: one MADE pass, then
// utils/splines.py:16-219 element-wise with 8 bins and linear tails) on the final layer's accumulators -- the final layer runs in
// groups of four features whose rows are packed so that a lane holds the 2 x 24 parameters of two features (the layout of
// nsf_wide.hip; mlp_tile.hpp mf_final_item), the spline runs in registers (rqs_regs), x is read from the tile and y written into it.
// EPI 3: EPI 1 under autograd (core.py:87-102 through a MADE): every layer's pre-activations are also written row-major to
// save[l][Bp][Hp] (l = 0: the initial layer's h; 2 b + 1: block b's inner t; 2 b + 2: its output h) and the signs of what a ReLU
// follows to bits[tile][2 b | 2 b + 1][item][512 lanes] -- the operands of made_bwd.hip.
// EPI 4 (affine_wide.hip, nf_affine_wide): a RealNVP coupling layer -- MaskedAffineFlow (coupling.py:209-229) or AffineCouplingBlock
// (:117-171, :232-267) -- on EPI 0's skeleton in plain-MLP mode: rows 2 f / 2 f + 1 = feature f's scale / shift parameter, the x tile is
// the whole z row, `direction` (the including kernel's) picks forward / inverse and table[24] the scale map (NF_SCALE_*, or 4 = the
// masked flow's exp with its non-finite -> NaN rule); affine.hip's formulas and signs.  A feature table follows the items (one word
// per 16 features, 2 bits each): 0 = identity, 1 = transformed, 2 = transformed and FED AS ZERO (a block's z2 columns, which its
// param_map never sees: a zero weight would turn an inf there into NaN for the whole row) -- the tile holds 0 for such a feature and
// the epilogue reads its z from global memory again.  Its ReLU keeps NaN (torch's LeakyReLU(0): NaN stays NaN, fmaxf would drop it).

    static_assert(TR == 64 || (TR == 128 && NSB == 1 && EPI == 3), "128-row tiles: the 256-slot training forward only (mf_tr128)");
    static_assert(!FT || EPI == 3, "the gathered / fed x tile: the training forward only");
    constexpr int NSH = TR / 64;             // sample blocks per HALF of a tile (a 256-slot item covers one half, a final-layer item too)
    constexpr int NS = NSB * NSH;            // sample blocks per hidden work item
    constexpr int HP = 256 * NSB;
    constexpr int HRB = 8 * NSB;             // hidden row-blocks
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *acts = lds;                                  // [HRB * 4 k-groups][2][TR][4]
    float *xreg = lds + (size_t)HRB * 4 * 8 * TR;       // [Dp / 8][2][TR][4]
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = table[0], Dp = table[1], NB = table[5], NFB = table[7], nrounds = table[8], nitems = table[10];
    const int MD = table[12] ? table[12] : table[6] * D;       // raw output row length: mult D for a MADE, out_features for a ResidualNet
    const int ldx = table[14] ? table[14] : D;                 // row stride of x (the conv path hands over 128-padded rows)
    const int plain = table[13];     // 1: a plain MLP  x -> W0 -> relu -> W1 -> relu -> Wf  (NB = 1 without the block's second linear and
                                     // its residual; EPI 1 / 3: the 3x3 -> 1x1 -> 3x3 conv conditioner over pixel rows (conv_rows.hip);
                                     // EPI 4: the stacked s / t nets or the param_map of a coupling layer; never EPI 0 / 2)
    const int *mtab = table + MF_HDR + MF_NW * nitems * 2;    // EPI 4: the feature table (Dp / 16 words)
    const int smap = table[24];                               // EPI 4: the scale map
    const int nets = table[25];                               // EPI 4, a masked flow: bit 0 = it has an s-net, bit 1 = a t-net
    const int *items = table + MF_HDR + w * nitems * 2;       // [nitems][nkg, rb]
    const float *stream = blob + table[16 + w];
    const int rbs[2] = {w, HRB - 1 - w};                      // (the packer's wave_items: the hidden row-blocks of this wave)
    const int sb0s[2] = {0, NSB == 2 ? 0 : NSH};
    const int lane_b = (TR * hh + n) * 4;       // the lane's offset inside a k-group of activations (sample block 0)
    const int64_t ntiles = (B + TR - 1) / TR;
    MfRing ring;
    mf_ring_start(ring, stream, lane);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        const int nrows = (int)((B - row0) < TR ? (B - row0) : TR);
        ring.ap = stream + lane * 4;            // (the ring already holds the stream's first entries: the wrap-around copy)
        int tq = tid;                           // per-tile address arithmetic from an index the compiler cannot hoist out of the tile loop
        asm volatile("" : "+v"(tq));            // (round 6, as in nsf_wide.hip: hoisted, those values stayed live across the products)
        asm volatile("" : "+v"(ring.ap));       // (likewise the restarted stream's first request addresses: four 64-bit pairs)
        // ---- x tile -> LDS (B-operand order; rows beyond the batch and features beyond D are zero) ---------------------------------
        if constexpr (FT) {
            // degree order: the wave gathers positions f0, f0 + step, ... (wave-uniform: every table read is a scalar-cache read, none
            // joins the weight ring's vector requests) for its 64 rows; the FED value is the initial layer's B operand, the raw one
            // leaves for the spline.  Rows beyond the batch feed zeros (the weight-gradient operand x_pad is copied from this tile).
            const int r = tq & (TR - 1);
            const bool live = r < nrows;
            const int *tt = table + MF_HDR + MF_NW * nitems * 2;
            const float *feed = blob + table[9];
            const float *xr = x + (row0 + r) * D;
            float *xo = logdet + (row0 + r) * D;
#pragma unroll 1
            for (int f = (TR == 64 ? w : w >> 1); f < Dp; f += 64 * MF_NW / TR) {
                float g = 0.0f;
                if (f < D) {
                    float v = 0.0f;
                    if (live) v = xr[tt[f]];
                    g = v;
                    if (tt[2 * D + f] >= 0) {       // libm's sincosf, not the fast intrinsics: the reference evaluates torch.sin / torch.cos (ft_feed;
                                                    // one call: sinf + cosf cost the 512-slot instantiation four spilled VGPRs)
                        const float a = __int_as_float(tt[D + f]) * v;
                        float sn, cs;
                        sincosf(a, &sn, &cs);
                        g = feed[f] * sn + feed[D + f] * cs + feed[2 * D + f];
                    }
                    if (live) xo[f] = v;
                    else g = 0.0f;
                }
                xreg[((size_t)(f >> 2) * TR + r) * 4 + (f & 3)] = g;
            }
        } else {
            const int r = tq & (TR - 1), cg = tq / TR;
            const float *xr = x + (row0 + r) * ldx;
#pragma unroll 1
            for (int c = cg; c < Dp / 4; c += 64 * MF_NW / TR) {
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (r < nrows && 4 * c < D) {           // (Dp rounds D up to 32: the last chunks may lie wholly beyond the row)
                    if ((D & 3) == 0) v = *reinterpret_cast<const f32x4 *>(xr + 4 * c);
                    else
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (4 * c + i < D) v[i] = xr[4 * c + i];
                }
                if constexpr (EPI == 4) {               // (c is wave-uniform: a scalar read)
                    const unsigned mb = (unsigned)mtab[c >> 2] >> (8 * (c & 3));
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (((mb >> (2 * i)) & 3u) == 2u) v[i] = 0.0f;
                }
                *reinterpret_cast<f32x4 *>(xreg + ((size_t)c * TR + r) * 4) = v;
            }
        }
        f32x16 h[2][NS], t[2][NS];
        MF_BARRIER();
        if constexpr (FT) {      // the fed tile -> x_pad rows (16-byte stores; the tile is not written again before the next tile's barrier)
            const int r = tq & (TR - 1), cg = tq / TR;
            if (row0 + r < Bp) {
                float *xp = x_pad + (row0 + r) * MF_LDP;
#pragma unroll 1
                for (int c = cg; 4 * c < MF_LDP; c += 64 * MF_NW / TR) {
                    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (4 * c < Dp) v = *reinterpret_cast<const f32x4 *>(xreg + ((size_t)c * TR + r) * 4);
                    *reinterpret_cast<f32x4 *>(xp + 4 * c) = v;
                }
            }
        }
        // ---- initial layer: h = b0 + W0 x ----------------------------------------------------------------------------------------------
#pragma unroll
        for (int s = 0; s < 2; ++s) mf_item<NS, false, TR>(ring, items[2 * s], xreg + lane_b + 128 * sb0s[s], h[s]);
        float *stile = nullptr;
        unsigned *btile = nullptr;
        if constexpr (EPI == 3) {
            stile = save + (size_t)row0 * HP;
            btile = bits + ((size_t)tile * 2 * NB * 2) * 512 + tq;
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_save_rows<NS, true>(stile, HP, nrows, rbs[s], sb0s[s], hh, n, h[s]);
        }
        // ---- residual blocks (nets/made.py:196-214): t = b1 + W1 relu(h);  h += b2 + W2 relu(t) -------------------------------
        for (int b = 0; b < NB; ++b) {
            MF_BARRIER();        // (b > 0: every wave has finished reading relu(t) of the previous block)
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_publish<NS, true, TR, EPI == 4>(acts, rbs[s], sb0s[s], hh, n, h[s]);
            if constexpr (EPI == 3)
#pragma unroll
                for (int s = 0; s < 2; ++s) btile[((size_t)(2 * b) * 2 + s) * 512] = mf_sign_bits<NS>(h[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_item<NS, false, TR>(ring, items[2 * (2 + 4 * b + s)], acts + lane_b + 128 * sb0s[s], t[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_publish<NS, true, TR, EPI == 4>(acts, rbs[s], sb0s[s], hh, n, t[s]);
            if constexpr (EPI == 3)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    btile[((size_t)(2 * b + 1) * 2 + s) * 512] = mf_sign_bits<NS>(t[s]);
                    mf_save_rows<NS, true>(stile + (size_t)(2 * b + 1) * Bp * HP, HP, nrows, rbs[s], sb0s[s], hh, n, t[s]);
                }
            MF_BARRIER();
            if (plain) break;            // (relu(t) is published: the final layer's input)
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_item<NS, true, TR>(ring, items[2 * (4 + 4 * b + s)], acts + lane_b + 128 * sb0s[s], h[s]);
            if constexpr (EPI == 3)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    mf_save_rows<NS, true>(stile + (size_t)(2 * b + 2) * Bp * HP, HP, nrows, rbs[s], sb0s[s], hh, n, h[s]);
        }
        // ---- final layer on the RAW block output (:303-304) + epilogue -------------------------------------------------------------
        if (!plain) {
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_publish<NS, false, TR>(acts, rbs[s], sb0s[s], hh, n, h[s]);
            MF_BARRIER();
        }
        if constexpr (EPI == 2) {
            const int G = NFB, nfi = nrounds;                 // (the header slots of the block variants: groups, final items per wave)
            const int *fit = items + 2 * (2 + 4 * NB);
            float ldt[4][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma nounroll
            for (int j = 0; j < nfi; ++j) {
                const int g = fit[2 * j + 1];
                if (g < 0) continue;
                f32x16 o[3][2];
                mf_final_item<MF_ROWS>(ring, fit[2 * j], acts + lane_b, o);
                float lsum[2] = {0.0f, 0.0f};
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        float prm[24];
#pragma unroll
                        for (int v = 0; v < 24; ++v) prm[v] = o[(24 * f + v) >> 4][sb][(24 * f + v) & 15];
                        const int tf = 4 * g + 2 * hh + f;
                        const bool valid = tf < D;
                        const int col = valid ? tf : 0;
                        float *xp = xreg + ((size_t)(col >> 2) * 64 + 32 * sb + n) * 4 + (col & 3);
                        float yv, lad;
                        rqs_regs_h<false>(p, *xp, prm, yv, lad);      // (round 5: binary bin descent; round 6: its first level before the knots exist)
                        if (valid) {
                            *xp = yv;
                            lsum[sb] += lad;
                        }
                        __builtin_amdgcn_sched_barrier(0);      // one evaluation at a time: interleaved, the four cost 7 spilled VGPRs at Hp = 512
                    }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ldt[q][0] = j == q ? lsum[0] : ldt[q][0];
                    ldt[q][1] = j == q ? lsum[1] : ldt[q][1];
                }
            }
            MF_BARRIER();                      // every wave is done with the activations: their region now holds the partial sums
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= nfi) break;
                const int g = fit[2 * j + 1];
                if (g >= 0) {
#pragma unroll
                    for (int sb = 0; sb < 2; ++sb) {
                        const float v = ldt[j][sb] + __shfl_xor(ldt[j][sb], 32);
                        if (hh == 0) acts[g * 64 + 32 * sb + n] = v;
                    }
                }
            }
            MF_BARRIER();
            if (tq < nrows) {
                float v = 0.0f;
                for (int g = 0; g < G; ++g) v += acts[g * 64 + tq];      // fixed order: deterministic
                ld_store(logdet + row0 + tq, v, acc_mode);
            }
            const int r = tq & 63, cg = tq >> 6;
            float *yr = y + (row0 + r) * D;
            if (r < nrows)
                for (int c = cg; 4 * c < D; c += MF_NW) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(xreg + ((size_t)c * 64 + r) * 4);
                    if ((D & 3) == 0) *reinterpret_cast<f32x4 *>(yr + 4 * c) = v;
                    else
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (4 * c + i < D) yr[4 * c + i] = v[i];
                }
            MF_BARRIER();                      // the next tile overwrites the x tile and the activations
            continue;
        }
        float ldsum[2] = {0.0f, 0.0f};
        for (int rd = 0; rd < nrounds; ++rd) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int *it = items + 2 * (2 + 4 * NB + 2 * rd + s);
                const int fb = it[1];                         // sample half s (TR = 64: sample block s)
                if (fb >= 0) {
                    f32x16 o[NSH];
                    mf_item<NSH, false, TR>(ring, it[0], acts + lane_b + 128 * NSH * s, o);
                    if constexpr (EPI == 0) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int f0 = 16 * fb + 4 * q + 2 * hh;
                            float *xp = xreg + ((size_t)((2 * fb + (q >> 1)) * 2 + (q & 1)) * 64 + 32 * s + n) * 4 + 2 * hh;
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                if (f0 + e < D) {
                                    const float scale = 1.0f / (1.0f + __expf(-(o[0][4 * q + 2 * e] + 2.0f))) + 1e-3f;
                                    xp[e] = scale * xp[e] + o[0][4 * q + 2 * e + 1];
                                    ldsum[s] += __logf(scale);
                                }
                            }
                        }
                    } else if constexpr (EPI == 4) {
                        const unsigned mw = (unsigned)mtab[fb];       // the 16 features of this row-block
                        const bool live = 32 * s + n < nrows;
                        const float *zg = x + (row0 + 32 * s + n) * ldx;      // (read only for a live row)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int f0 = 16 * fb + 4 * q + 2 * hh;
                            float *xp = xreg + ((size_t)((2 * fb + (q >> 1)) * 2 + (q & 1)) * 64 + 32 * s + n) * 4 + 2 * hh;
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                const unsigned mode = (mw >> (2 * (4 * q + 2 * hh + e))) & 3u;
                                if (f0 + e < D && (mode != 0u || smap == 4)) {
                                    float sc = o[0][4 * q + 2 * e], sh = o[0][4 * q + 2 * e + 1];
                                    float v = xp[e], yo;
                                    if (mode == 2u) v = live ? zg[f0 + e] : 0.0f;
                                    if (smap == 4) {             // masked_affine_kernel with b = 1 (identity) / 0
                                        const float bi = mode == 0u ? 1.0f : 0.0f;
                                        if (!(nets & 1)) sc = 0.0f;       // a missing net is the constant 0, whatever its zero rows
                                        if (!(nets & 2)) sh = 0.0f;       // made of a non-finite hidden value (0 * inf)
                                        if (!M<float>::finite(sc)) sc = M<float>::nan();
                                        if (!M<float>::finite(sh)) sh = M<float>::nan();
                                        const float zm = bi * v;
                                        if (direction == 0) yo = zm + (1.0f - bi) * (v * M<float>::exp(sc) + sh);
                                        else yo = zm + (1.0f - bi) * (v - sh) * M<float>::exp(-sc);
                                        ldsum[s] += (1.0f - bi) * sc;
                                    } else if (smap == NF_SCALE_NONE) {      // affine_coupling_kernel
                                        yo = direction == 0 ? v + sh : v - sh;
                                    } else if (smap == NF_SCALE_EXP) {
                                        yo = direction == 0 ? v * M<float>::exp(sc) + sh : (v - sh) * M<float>::exp(-sc);
                                        ldsum[s] += sc;
                                    } else {
                                        const float sg = sigmoid(sc + 2.0f);
                                        const float lg = M<float>::log(sg);
                                        if (smap == NF_SCALE_SIGMOID) {
                                            yo = direction == 0 ? v / sg + sh : (v - sh) * sg;
                                            ldsum[s] -= lg;
                                        } else {
                                            yo = direction == 0 ? v * sg + sh : (v - sh) / sg;
                                            ldsum[s] += lg;
                                        }
                                    }
                                    xp[e] = yo;
                                }
                            }
                        }
                    } else {
#pragma unroll
                        for (int ss = 0; ss < NSH; ++ss) {
                            const int rl = 32 * (NSH * s + ss) + n;
                            const int64_t r = row0 + rl;
                            if (rl < nrows) {
                                float *yp = y + r * (int64_t)MD + 32 * fb + 4 * hh;
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const int c = 32 * fb + 8 * q + 4 * hh;
                                    if ((MD & 3) == 0) {
                                        if (c < MD) *reinterpret_cast<f32x4 *>(yp + 8 * q) = f32x4{o[ss][4 * q], o[ss][4 * q + 1], o[ss][4 * q + 2], o[ss][4 * q + 3]};
                                    } else {
#pragma unroll
                                        for (int i = 0; i < 4; ++i) if (c + i < MD) yp[8 * q + i] = o[ss][4 * q + i];
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        MF_BARRIER();                          // every wave is done with the activations (and, EPI 0 / 4, has written its z values)
        if constexpr (EPI == 0 || EPI == 4) {
            // per-sample log-det: the lane-halves' sums, then the 8 row-blocks' in a FIXED order (deterministic)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float v = ldsum[s] + __shfl_xor(ldsum[s], 32);
                if constexpr (EPI == 4) v = direction == 0 ? v : -v;       // (the inverse: the opposite sign, as affine.hip stores it)
                const int fb = (s == 0 ? w : 7 - w);
                if (hh == 0) acts[fb * 64 + 32 * s + n] = v;
            }
            MF_BARRIER();
            if (tq < nrows) {
                float v = 0.0f;
                for (int fb = 0; fb < 8; ++fb) v += acts[fb * 64 + tq];
                ld_store(logdet + row0 + tq, v, acc_mode);
            }
            const int r = tq & 63, cg = tq >> 6;
            float *yr = y + (row0 + r) * D;
            if (r < nrows)
                for (int c = cg; 4 * c < D; c += MF_NW) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(xreg + ((size_t)c * 64 + r) * 4);
                    if ((D & 3) == 0) *reinterpret_cast<f32x4 *>(yr + 4 * c) = v;
                    else
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (4 * c + i < D) yr[4 * c + i] = v[i];
                }
            MF_BARRIER();                      // the next tile overwrites the x tile and the activations
        }
    }
