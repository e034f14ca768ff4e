// Device-side target log-densities evaluated on the 16-chain tile of a workgroup.
// ManyWell: fab/target_distributions/many_well.py:81-90 -> double_well.py:44-58
// GMM:      fab/target_distributions/gmm.py:57-66 (MixtureSameFamily of diagonal normals, -inf mask)
// Quartic:  log p = -sum_j (a_j x_j + b_j x_j^2 + c_j x_j^4) - 1/2 x^T J x - log_norm, J symmetric (tests/quartic_cases.py)
// Rotor:    log p = sum_j [sum_m (A_mj cos m th_j + B_mj sin m th_j) - l_j x_j - q_j x_j^2] + 1/2 sum_j sum_n kap_jn cos 2 pi d_jn
//           - log_norm, th_j = 2 pi w_j, w_j = x_j r_j reduced to [-1/2, 1/2], d_jn = w_j - w_k reduced (tests/rotor_cases.py)
#pragma once
#include "flow_device.h"

namespace fab {

struct TargetDev {
    int kind, dim;
    float a, b, c, log_norm;
    int n_mix;
    const float* locs;
    const float* scales;
};

static inline TargetDev make_target_dev(const fabhip_target& t) {
    TargetDev d;
    d.kind = t.kind; d.dim = t.dim; d.a = t.a; d.b = t.b; d.c = t.c; d.log_norm = t.log_norm;
    d.n_mix = t.n_mix; d.locs = t.locs; d.scales = t.scales;
    return d;
}

static inline int check_target(const fabhip_target* t, int dim) {
    if (!t) return FABHIP_EINVAL;
    if (t->dim != dim) return FABHIP_EINVAL;
    if (t->kind == FABHIP_TARGET_MANYWELL) return (dim % 2 == 0) ? FABHIP_OK : FABHIP_EINVAL;
    if (t->kind == FABHIP_TARGET_GMM) return (t->n_mix > 0 && t->locs && t->scales) ? FABHIP_OK : FABHIP_EINVAL;
    if (t->kind == FABHIP_TARGET_QUARTIC)
        return (t->locs && t->scales && dim >= 1 && dim <= FABHIP_MAX_DIM) ? FABHIP_OK : FABHIP_EINVAL;
    if (t->kind == FABHIP_TARGET_ROTOR)
        return (t->locs && t->scales && dim >= 1 && dim <= FABHIP_MAX_DIM && t->n_mix >= 1 && t->n_mix <= FABHIP_MAX_DIM - 1)
                   ? FABHIP_OK : FABHIP_EINVAL;
    return FABHIP_ENOTSUP;
}

__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, row_ror<8>(v));
    v = fmaxf(v, row_ror<4>(v));
    v = fmaxf(v, row_ror<2>(v));
    v = fmaxf(v, row_ror<1>(v));
    return v;
}

// sin and cos of 2 pi w for w in [-1/2, 1/2] (revolutions, already reduced): y = 4 w quarter turns, q = rint(y) in -2 .. 2,
// r = y - q exact in [-1/2, 1/2], then the Taylor polynomials of sin / cos (pi / 2 r) on |angle| <= pi / 4 (both below one ulp
// of truncation error there) and the quadrant by float compares: a NaN fails every compare and leaves the NaN polynomials.
// No table, no private array (sinf / cosf on 2 pi t would bring their large-argument path and its scratch).
__device__ __forceinline__ void sincos_rev(float w, float& s, float& c) {
    const float y = 4.f * w;
    const float q = rintf(y);
    const float a = (y - q) * 1.5707963267948966f;
    const float a2 = a * a;
    float ps = 2.7557319223985893e-6f;
    ps = ps * a2 - 1.9841269841269841e-4f;
    ps = ps * a2 + 8.3333333333333333e-3f;
    ps = ps * a2 - 1.6666666666666667e-1f;
    ps = a + a * (a2 * ps);
    float pc = 2.4801587301587302e-5f;
    pc = pc * a2 - 1.3888888888888889e-3f;
    pc = pc * a2 + 4.1666666666666667e-2f;
    pc = pc * a2 - 0.5f;
    pc = 1.f + a2 * pc;
    const bool odd = fabsf(q) == 1.f;
    const float ss = odd ? pc : ps, cc = odd ? ps : pc;
    s = (q == -1.f || fabsf(q) == 2.f) ? -ss : ss;
    c = (q == 1.f || fabsf(q) == 2.f) ? -cc : cc;
}

// X: LDS [16][ldx] positions; GP: LDS [16][ldg] receives d log p / dx when GRAD.
// Returns log p of this thread's row (replicated over its 16 lanes).
template <bool GRAD>
__device__ float target_tile(const TargetDev& tg, const float* X, int ldx, float* GP, int ldg, const Tid& t) {
    const int D = tg.dim;
    if (tg.kind == FABHIP_TARGET_MANYWELL) {
        float acc = 0.f;
        for (int j = t.c; j < D; j += 16) {
            const float x = X[t.row * ldx + j];
            const float x2 = x * x;
            float e, g;
            if ((j & 1) == 0) {
                e = tg.a * x + tg.b * x2 + tg.c * (x2 * x2);
                g = -(tg.a + 2.f * tg.b * x + 4.f * tg.c * (x2 * x));
            } else {
                e = 0.5f * x2;
                g = -x;
            }
            acc += -e;
            if (GRAD) GP[t.row * ldg + j] = g;
        }
        return row16_sum(acc) - tg.log_norm;
    }
    if (tg.kind == FABHIP_TARGET_QUARTIC) {
        // Lane c owns sites j = c, c + 16, ... (D <= 64: at most four).  J = locs [D][D] is symmetric, so (J x)_j is read as
        // sum_k J[k][j] x_k in ascending k: the 16 lanes of a row read consecutive floats of row k, x_k is an LDS broadcast.
        // The site loop is rolled as ManyWell's and the k loop sits INSIDE it, unrolled by 4 only: a lane walks one column of J
        // per site it owns (every element of J is read once per row; the row's x is re-read from LDS once per owned site), and
        // the live state is one accumulator and the four loads in flight.  (k outer with the four site accumulators live cost the HMC kernels 12 - 24 VGPRs and
        // one of them scratch: DESIGN section 18.)
        const float* J = tg.locs;
        const float* S = tg.scales;            // [3][D]: rows a, b, c
        float acc = 0.f;
#pragma unroll 1
        for (int j = t.c; j < D; j += 16) {
            float jx = 0.f;
#pragma unroll 4
            for (int k = 0; k < D; ++k) jx += J[k * D + j] * X[t.row * ldx + k];
            const float x = X[t.row * ldx + j];
            const float x2 = x * x;
            const float sa = S[j], sb = S[D + j], sc = S[2 * D + j];
            acc += -(sa * x + sb * x2 + sc * (x2 * x2) + 0.5f * x * jx);
            if (GRAD) GP[t.row * ldg + j] = -(sa + 2.f * sb * x + 4.f * sc * (x2 * x)) - jx;
        }
        return row16_sum(acc) - tg.log_norm;
    }
    if (tg.kind == FABHIP_TARGET_ROTOR) {
        // Lane c owns sites j = c, c + 16, ... as above; the site loop is rolled and the neighbour loop sits inside it.  T = locs
        // [2 NB][D]: rows 0 .. NB - 1 the neighbour indices k_jn as floats, rows NB .. 2 NB - 1 the couplings; for one n the 16
        // lanes of a row read consecutive floats of both.  x_k comes from the tile in LDS and is reduced again per neighbour (its
        // rate is a gathered read of row 6 of S): no staging of the reduced revolutions, no exchange between lanes.  One
        // sin / cos pair per site (harmonics 2 and 3 by angle addition) and one per listed neighbour; the live state across the
        // neighbour loop is one energy and one gradient accumulator.  An index is clamped to the tile (the class builds the
        // table; a raw caller's wrong index then reads a wrong site, never beyond the row - index entries must be finite floats,
        // include/fabhip.h says so: the conversion of a NaN or an inf is not defined).
        const float* T = tg.locs;
        const float* S = tg.scales;            // [9][D]: rows A1 A2 A3 B1 B2 B3 r l q
        const int NB = tg.n_mix;
        const float TWO_PI = 6.283185307179586f;
        float acc = 0.f;
#pragma unroll 1
        for (int j = t.c; j < D; j += 16) {
            const float x = X[t.row * ldx + j];
            const float r = S[6 * D + j];
            const float w = fmaf(x, r, -rintf(x * r));     // one rounding of x r - n: the revolution keeps its low bits
            float ce = 0.f, cg = 0.f;
#pragma unroll 1
            for (int n = 0; n < NB; ++n) {
                const int k = min(max((int)T[n * D + j], 0), D - 1);
                const float kap = T[(NB + n) * D + j];
                const float xk = X[t.row * ldx + k], rk = S[6 * D + k];
                float d = w - fmaf(xk, rk, -rintf(xk * rk));
                d = d - rintf(d);
                float sd, cd;
                sincos_rev(d, sd, cd);
                ce += kap * cd;
                cg += kap * sd;
            }
            float s1, c1;
            sincos_rev(w, s1, c1);
            const float c2 = c1 * c1 - s1 * s1, s2 = 2.f * (s1 * c1);
            const float c3 = c2 * c1 - s2 * s1, s3 = s2 * c1 + c2 * s1;
            const float l = S[7 * D + j], q = S[8 * D + j];
            const float A1 = S[j], A2 = S[D + j], A3 = S[2 * D + j], B1 = S[3 * D + j], B2 = S[4 * D + j], B3 = S[5 * D + j];
            acc += (A1 * c1 + B1 * s1) + (A2 * c2 + B2 * s2) + (A3 * c3 + B3 * s3) - l * x - q * (x * x) + 0.5f * ce;
            if (GRAD) {
                const float gs = (B1 * c1 - A1 * s1) + 2.f * (B2 * c2 - A2 * s2) + 3.f * (B3 * c3 - A3 * s3);
                GP[t.row * ldg + j] = TWO_PI * r * (gs - cg) - l - 2.f * q * x;
            }
        }
        return row16_sum(acc) - tg.log_norm;
    }
    // ---- GMM: lane c handles components k = c, c+16, ... ----------------------------------------
    const float LOG2PI = 1.8378770664093453f;
    const float log_mix = -logf((float)tg.n_mix);
    float best = -INFINITY;
    bool any_nan = false;
    for (int k = t.c; k < tg.n_mix; k += 16) {
        float m = 0.f, hld = 0.f;
        for (int j = 0; j < D; ++j) {
            const float sc = tg.scales[k * D + j];
            const float z = (X[t.row * ldx + j] - tg.locs[k * D + j]) / sc;
            m += z * z;
            hld += logf(sc);
        }
        const float comp = -0.5f * ((float)D * LOG2PI + m) - hld + log_mix;
        any_nan |= (comp != comp);
        best = fmaxf(best, comp);
    }
    const float mx = row16_max(best);
    float se = 0.f;
    for (int k = t.c; k < tg.n_mix; k += 16) {
        float m = 0.f, hld = 0.f;
        for (int j = 0; j < D; ++j) {
            const float sc = tg.scales[k * D + j];
            const float z = (X[t.row * ldx + j] - tg.locs[k * D + j]) / sc;
            m += z * z;
            hld += logf(sc);
        }
        const float comp = -0.5f * ((float)D * LOG2PI + m) - hld + log_mix;
        se += (mx == -INFINITY) ? 0.f : expf(comp - mx);
    }
    const float stot = row16_sum(se);
    const float nanflag = row16_sum(any_nan ? 1.f : 0.f);
    float lp = (mx == -INFINITY) ? -INFINITY : mx + logf(stot);
    if (nanflag > 0.f) lp = NAN;
    if (GRAD) {
        for (int j = 0; j < D; ++j) {
            float gj = 0.f;
            for (int k = t.c; k < tg.n_mix; k += 16) {
                float m = 0.f, hld = 0.f;
                for (int jj = 0; jj < D; ++jj) {
                    const float sc = tg.scales[k * D + jj];
                    const float z = (X[t.row * ldx + jj] - tg.locs[k * D + jj]) / sc;
                    m += z * z;
                    hld += logf(sc);
                }
                const float comp = -0.5f * ((float)D * LOG2PI + m) - hld + log_mix;
                const float w = expf(comp - lp);
                const float sc = tg.scales[k * D + j];
                gj += w * (-(X[t.row * ldx + j] - tg.locs[k * D + j]) / (sc * sc));
            }
            gj = row16_sum(gj);
            GP[t.row * ldg + j] = gj;          // all 16 lanes of the row store the same value
        }
    }
    if (lp < -1e4f) lp = -INFINITY;       // gmm.py:63-65
    return lp - tg.log_norm;
}

}  // namespace fab
