// nsf_tile_final.hpp -- a FRAGMENT of the tile loop of nsf_wide_kernel and nsf_ctx_kernel, included inside the kernel body (nsf_tile.hpp says why
// it is text and not a function).  Reads ring, items, fin0 (index of the first final entry), nfi, G, acts, xreg, ldp, tabs, p, h, lane_b, hh,
// n, nI, nT, PI, tq, MP / FPL / FPG / NFI; reads and writes ld_ident.  With NSF_TILE_FT (nsf_circ.hip: per-feature tails and bounds) also ftl, the
// kernel's LDS copy of the per-feature table with row stride NSF_FT_STRIDE.
MF_BARRIER();
#pragma unroll
for (int s = 0; s < NHI; ++s) mf_publish<NS, false, TR>(acts, items[3 * s + 1], items[3 * s + 2], hh, n, h[s]);
MF_BARRIER();
float ldt[NFI][2];                                   // [final item][sample block] (nfi <= NFI)
#pragma unroll
for (int q = 0; q < NFI; ++q) ldt[q][0] = ldt[q][1] = 0.0f;
#pragma nounroll
for (int j = 0; j < nfi; ++j) {                       // (rolled: one copy of the item's code; the sums go to their slot by selects)
    const int *it = items + 3 * (fin0 + j);
    const int g = it[1], sbo = it[2];                 // group of four transform features, first of its two sample blocks
    if (g < 0) continue;
    f32x16 o[3][2];
    mf_final_item<TR>(ring, it[0], acts + lane_b + 128 * sbo, o);
    float lsum[2] = {0.0f, 0.0f};
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int f = 0; f < FPL; ++f) {
            float prm[MP];
#pragma unroll
            for (int v = 0; v < MP; ++v) prm[v] = o[(MP * f + v) >> 4][sb][(MP * f + v) & 15];
            const int tf = FPG * g + FPL * hh + f;
            const bool valid = tf < nT;
            float *xp = xreg + nsf_xidx<TR>(PI + (valid ? tf : 0), 32 * (sbo + sb) + n);
            float yv, lad;
            // round 5: binary bin descent (rqs_regs_t; the packed PAIR version of the benchmark kernel spilled 11-23 registers here)
#ifdef NSF_TILE_FT      // list tails: bound and type of the feature from the table; 0 / log-det 0 outside (utils/splines.py:48-57)
            nsf_regs_ft<DIR == 1, KB>(p, ftl[FT_BOUND * NSF_FT_STRIDE + PI + (valid ? tf : 0)],
                                      __float_as_int(ftl[FT_TAILS * NSF_FT_STRIDE + PI + (valid ? tf : 0)]), *xp, prm, yv, lad);
#else           // round 6: first descent level before the knots exist (fused_common.hpp rqs_regs_h): half the live arrays
            rqs_regs_h<DIR == 1, KB>(p, *xp, prm, yv, lad);
#endif
            if (valid) {
                *xp = yv;
                lsum[sb] += lad;
            }
        }
#pragma unroll
    for (int q = 0; q < NFI; ++q) {
        ldt[q][0] = j == q ? lsum[0] : ldt[q][0];
        ldt[q][1] = j == q ? lsum[1] : ldt[q][1];
    }
}
MF_BARRIER();                                        // every wave is done with the activations
if constexpr (DIR == 0) {
#pragma unroll 1
    for (int i = tq; i < nI * nsf_tabw(KB); i += 64 * MF_NW) acts[i] = tabs[i];
}
#pragma unroll
for (int j = 0; j < NFI; ++j) {
    if (j >= nfi) break;
    const int *it = items + 3 * (fin0 + j);
    const int g = it[1], sbo = it[2];
    if (g >= 0) {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            const float v = ldt[j][sb] + __shfl_xor(ldt[j][sb], 32);
            if (hh == 0) ldp[g * TR + 32 * (sbo + sb) + n] = v;
        }
    }
}
if constexpr (DIR == 0) {                            // density: the identity half's spline after the conditioner (:88-92)
    MF_BARRIER();
#ifdef NSF_TILE_FT
    ld_ident = nsf_identity_ft<false, TR, KB>(xreg, acts, nI, tq);
#else
    ld_ident = nsf_identity<false, TR, KB>(xreg, acts, p, nI, tq);
#endif
}
ldp[(G + tq / TR) * TR + tq % TR] = ld_ident;
MF_BARRIER();
