// density2d_row_body.hpp -- the statements that evaluate one row of a closed-form 2-D density: a FRAGMENT, #included inside a
// function body (no include guard, no namespace).  In scope at the point of inclusion: `KIND` (compile-time kind code), z0, z1
// (the row), p (the parameter record), n (modes / rings), cx, cy (kind 6: the centres), inv2s2, lognorm (kind 6:
// d2_circ_setup's).  It declares and sets v = log p(z) and g0, g1 = d log p / d z.
//
// Why statements and not a function: nf_density2d must keep its results bit for bit.  Called as an inlined function from
// density2d_kernel, hipcc's SLP vectorizer pairs the two products of kinds 2 and 3 into one packed multiply, they no longer contract
// into the FMAs of the sum, and the log-density's last bits change.  Included in place, density2d_kernel's instruction stream is
// the one it had before the body was shared (compare the disassembly, not the register counts).  density2d_row.hpp wraps the same
// fragment into d2_row<KIND>() for the kernels that evaluate several densities per launch (hmc2d.hip).
        float v, g0, g1;
        if (KIND == D2_TWO_MODES) {
            // p: loc, 1 / (2 scale), |loc|, 1 / (3 scale), 2 / (3 scale)^2
            v = d2_ring(z0, z1, p[0], p[1], g0, g1);
            float da, deps;
            v += d2_two_bumps(fabsf(z0), p[2], p[3], p[4], da, deps);
            g0 += da * d2_sign(z0);
        } else if (KIND == D2_SMILEY) {
            // p: loc, 1 / (2 scale), 0.8, 1.2
            v = d2_ring(z0, z1, p[0], p[1], g0, g1);
            const float y = z1 + p[2];
            const float u = (fabsf(y) - p[3]) * p[1];
            v -= 0.5f * u * u;
            g1 -= u * p[1] * d2_sign(y);
        } else if (KIND == D2_SINUSOIDAL || KIND == D2_SIN_GAP || KIND == D2_SIN_SPLIT) {
            // p: 2 pi / period, 1 / scale, (20 scale)^-4, 2 / scale^2, w amplitude, w centre, w scale
            v = d2_envelope(z0, z1, p[2], g0, g1);
            float sn, cs;
            ::sincosf(p[0] * z0, &sn, &cs);
            const float dw1 = p[0] * cs;
            if (KIND == D2_SINUSOIDAL) {
                const float u = (z1 - sn) * p[1];
                v -= 0.5f * u * u;
                g1 -= u * p[1];
                g0 += u * p[1] * dw1;
            } else {
                const float t = (z0 - p[5]) / p[6];
                float h, dh;                            // h = w / 2 and its derivative in z0
                if (KIND == D2_SIN_GAP) {
                    h = p[4] * M<float>::exp(-0.5f * t * t) * 0.5f;
                    dh = -h * t / p[6];
                } else {
                    const float sg = 1.0f / (1.0f + M<float>::exp(-t));
                    h = p[4] * sg * 0.5f;
                    dh = h * (1.0f - sg) / p[6];
                }
                const float y = z1 - sn + h;
                float da, deps;
                v += d2_two_bumps(fabsf(y), fabsf(h), p[1], p[3], da, deps);
                const float dy = da * d2_sign(y);
                g1 += dy;
                g0 += dy * (dh - dw1) + deps * d2_sign(h) * dh;
            }
        } else {
            // streaming log-sum-exp over the modes: running maximum mx, S = sum exp(t_i - mx), T0 / T1 = sum exp(t_i - mx) d t_i / d z
            float mx = 0.0f, S = 0.0f, T0 = 0.0f, T1 = 0.0f, nrm = 0.0f;
            if (KIND == D2_RINGS) nrm = M<float>::sqrt(z0 * z0 + z1 * z1);
            for (int i = 0; i < n; ++i) {
                float t, d0, d1;
                if (KIND == D2_RINGS) {                 // p: 2 / n_rings, 1 / (2 scale^2)
                    const float u = nrm - p[0] * (float)(i + 1);
                    t = -(u * u) * p[1];
                    d0 = -2.0f * u * p[1];              // d t / d |z|
                    d1 = 0.0f;
                } else {
                    const float u0 = z0 - cx[i], u1 = z1 - cy[i];
                    t = -(u0 * u0 + u1 * u1) * inv2s2;
                    d0 = -2.0f * u0 * inv2s2;
                    d1 = -2.0f * u1 * inv2s2;
                }
                if (i == 0 || t > mx) {
                    const float f = i == 0 ? 0.0f : M<float>::exp(mx - t);
                    S = S * f + 1.0f; T0 = T0 * f + d0; T1 = T1 * f + d1;
                    mx = t;
                } else {
                    const float e = M<float>::exp(t - mx);
                    S += e; T0 = fmaf(e, d0, T0); T1 = fmaf(e, d1, T1);
                }
            }
            v = mx + M<float>::log(S) + lognorm;
            if (KIND == D2_RINGS) {
                const float gn = nrm > 0.0f ? T0 / S / nrm : 0.0f;
                g0 = gn * z0;
                g1 = gn * z1;
            } else {
                g0 = T0 / S;
                g1 = T1 / S;
            }
        }
