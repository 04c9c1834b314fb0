// nsf_tile_load.hpp -- a FRAGMENT of the tile loop of nsf_wide_kernel and nsf_ctx_kernel, included inside the kernel body (nsf_tile.hpp says why
// it is text and not a function).  Reads x, xreg, row0, nrows, D, Dp, nI, nT, par_i, PI, tq, NIG (+ ctx, ldc, C, PC with NSF_TILE_CONTEXT).
{   // x tile -> LDS, columns sorted into positions (rows beyond the batch and the padding positions are zero)
    const int r = tq % TR, cg = tq / TR;
    const float *xr = x + (row0 + r) * D;
#pragma unroll 1        // (runtime trip counts: the unroller's remainder bookkeeping stayed live across the whole tile -- 1-8 spilled registers)
    for (int c = cg; 4 * c < D; c += NIG) {
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < nrows) {
            if ((D & 3) == 0) v = *reinterpret_cast<const f32x4 *>(xr + 4 * c);
            else
#pragma unroll
                for (int i = 0; i < 4; ++i) if (4 * c + i < D) v[i] = xr[4 * c + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = 4 * c + i;
            if (col < D) xreg[nsf_xidx<TR>(((col ^ par_i) & 1) ? PI + (col >> 1) : (col >> 1), r)] = v[i];
        }
    }
#pragma unroll 1
    for (int ps = nI + cg; ps < PI; ps += NIG) xreg[nsf_xidx<TR>(ps, r)] = 0.0f;
#pragma unroll 1
    for (int ps = PI + nT + cg; ps < Dp; ps += NIG) xreg[nsf_xidx<TR>(ps, r)] = 0.0f;
#ifdef NSF_TILE_CONTEXT                                      // nsf_ctx.hip: then the row's context at [Dp, Dp + PC)
    const float *cr = ctx + (row0 + r) * ldc;         // (ldc = 0: every row reads row 0)
#pragma unroll 1
    for (int ps = cg; ps < PC; ps += NIG) xreg[nsf_xidx<TR>(Dp + ps, r)] = (r < nrows && ps < C) ? cr[ps] : 0.0f;
#endif
}
