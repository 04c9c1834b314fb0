// nsf_tile_store.hpp -- a FRAGMENT of the tile loop of nsf_wide_kernel and nsf_ctx_kernel, included inside the kernel body (nsf_tile.hpp says why
// it is text and not a function).  Reads y, logdet, xreg, ldp, row0, nrows, D, G, par_i, PI, ld_const (the LU log-det, or 0), acc_mode, tq, NIG.
if (tq < nrows) {
    float v = ld_const;
#pragma unroll 1
    for (int s = 0; s < G + NIG; ++s) v += ldp[s * TR + tq];      // fixed order: deterministic
    ld_store(logdet + row0 + tq, v, acc_mode);
}
{
    const int r = tq % TR, cg = tq / TR;
    float *yr = y + (row0 + r) * D;
    if (r < nrows) {
#pragma unroll 1
        for (int c = cg; 4 * c < D; c += NIG) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = 4 * c + i < D ? 4 * c + i : D - 1;
                v[i] = xreg[nsf_xidx<TR>(((col ^ par_i) & 1) ? PI + (col >> 1) : (col >> 1), r)];
            }
            if ((D & 3) == 0) *reinterpret_cast<f32x4 *>(yr + 4 * c) = v;
            else
#pragma unroll
                for (int i = 0; i < 4; ++i) if (4 * c + i < D) yr[4 * c + i] = v[i];
        }
    }
}
