// fe_modinv.cuh -- field inversion by batched divsteps (Bernstein-Yang "safegcd") for the two Pasta fields, host and gfx950.
//
// fe_inv_gcd<F>(a, k) has fe_inv's contract exactly (groupmap.cuh): Montgomery words below p in, the Montgomery words of the inverse out, below p, and 0 -> 0.  The
// inverse of a field element is unique, so the two routines agree on every byte (tests/test_modinv_host.py on the host, tests/test_gpu_fast_inverse.py on the
// device); tests/modinv_model.py restates this file limb by limb on integers.  fe_inv walks 254 dependent squarings and ~65 products; this file walks at most 25
// batches of 30 branch-free divsteps and two 2 x 2 matrix updates over nine limbs.  Opt-in callers only: mina_field_inv_gcd and, under mina_ctx_set_fast_inverse,
// the MSM finishes (msm.cuh), and under mina_ctx_set_chain_inverse the `_gcd` twins of the chain's scalar stages and the Lagrange set-up (FeInvGcd, at the end).
//
// THE ITERATION.  delta = 1, f = p, g = a (the Montgomery words read as an integer), d = 0, e = 1; f stays odd.  One divstep:
//     delta > 0 and g odd:   (delta, f, g) <- (1 - delta, g, (g - f) / 2)
//     otherwise:             (delta, f, g) <- (1 + delta, f, (g + (g mod 2) f) / 2)
// A batch runs 30 divsteps on the LOW 30 BITS of f and g alone (mi_divsteps30) and yields delta and the integer matrix t = (u v; q r) = 2^30 * (the product of the
// 30 transition matrices), |u| + |v| <= 2^30 and |q| + |r| <= 2^30.  Then, both divisions exact,
//     (f, g) <- (u f + v g, q f + r g) / 2^30                                                                                      (mi_update_fg)
//     (d, e) <- (u d + v e + md p, q d + r e + me p) / 2^30      md, me: what makes the low 30 bits zero, see below                   (mi_update_de)
// which keeps  d a = f  and  e a = g  (mod p).  When g = 0, f = +-gcd(p, a) = +-1 (+-p for a = 0) and the inverse of the integer a is sign(f) d mod p.
// 750 divsteps are above the published bound floor((49 * 256 + 57) / 17) = 741 for inputs below 2^256: THE OUTER LOOP HAS THE FIXED TRIP COUNT MI_BATCHES = 25 and
// may leave early, once per batch, when g = 0 (inputs below p were seen to take 19 batches at most).  No other loop here depends on data.
//
// LIMBS AND BOUNDS.  f, g, d, e: nine signed limbs, value = sum v[i] 2^(30 i); after every update limbs 0..7 lie in [0, 2^30) and limb 8 carries the sign.
//     |f|, |g| < 2^256 throughout (a divstep never grows max(|f|, |g|) beyond the larger of the two before it): |limb 8| <= 2^16.
//     INVARIANT of d, e:  -2p < d, e < p  after every batch (it holds at the start: 0 and 1).  Proof: with d' = d + p if d < 0 else d (e' alike), d', e' lie in
//     (-p, p) and  u d + v e + (u [d < 0] + v [e < 0]) p = u d' + v e', of magnitude below 2^30 p.  The low 30 bits are then cleared by SUBTRACTING k p,
//     0 <= k < 2^30 (k = the low 30 bits times p^-1 mod 2^30): the sum lies in (-2^31 p, 2^30 p), a multiple of 2^30; divided, in (-2p, p).  So |limb 8| of d, e
//     is at most 2^15 + 1 (p = 2^254 + ..: limb 8 of p is 2^14), md and me lie in (-2^31, 2^30].
//     Every 64-bit accumulator is a sum of two products of a matrix entry by a limb, |u x| + |v y| <= 2^30 * 2^30 = 2^60, at most one product md p_i < 2^61,
//     and the carry of the limb before, < 2^33: below 2^62 in magnitude.  No signed operation overflows; the divsteps run on unsigned words.
//     Right shifts of signed values go through mi_sar, which never shifts a negative number.
#pragma once
#include "groupmap.cuh"

namespace mb {

struct mi30_t { int32_t v[9]; };                  // nine signed 30-bit limbs
struct mi_mat_t { int32_t u, v, q, r; };           // a batch's matrix, entries of magnitude <= 2^30

static constexpr int MI_BATCHES = 25, MI_STEPS = 30;
static constexpr uint32_t MI_M30 = 0x3fffffffu;

// the modulus in 30-bit limbs and p^-1 mod 2^30: compile-time constants from the modulus words of fp.cuh
template <int F> constexpr uint32_t mi_p_word(int i) { return i == 0 ? 1u : i == 1 ? FieldP<F>::P1 : i == 2 ? FieldP<F>::P2 : i == 3 ? FieldP<F>::P3 : i == 7 ? P7 : 0u; }
template <int F> constexpr int32_t mi_p_limb(int i) {
    const int w = (30 * i) >> 5, s = (30 * i) & 31;
    const uint64_t x = (uint64_t)mi_p_word<F>(w) | (w + 1 < 8 ? (uint64_t)mi_p_word<F>(w + 1) << 32 : 0);
    return (int32_t)((x >> s) & MI_M30);
}
template <int F> constexpr uint32_t mi_p_inv30() {
    const uint32_t p0 = mi_p_word<F>(0);
    uint32_t x = 1;                                // Newton: the number of correct low bits doubles, 1 -> 32
    for (int i = 0; i < 5; ++i) x *= 2u - p0 * x;
    return x & MI_M30;
}
static_assert(mi_p_limb<FIELD_FP>(8) == (1 << 14) && mi_p_limb<FIELD_FQ>(8) == (1 << 14) && mi_p_limb<FIELD_FP>(0) == 1 && mi_p_limb<FIELD_FQ>(7) == 0, "p = 2^254 + t, t < 2^126, p = 1 mod 2^32");
static_assert(((mi_p_inv30<FIELD_FP>() * mi_p_word<FIELD_FP>(0)) & MI_M30) == 1 && ((mi_p_inv30<FIELD_FQ>() * mi_p_word<FIELD_FQ>(0)) & MI_M30) == 1, "p^-1 mod 2^30");

// floor(x / 2^n) without shifting a negative value
MB_HD int64_t mi_sar(int64_t x, int n) { return x < 0 ? ~(~x >> n) : x >> n; }
MB_HD int32_t mi_low30(int64_t x) { return (int32_t)((uint64_t)x & MI_M30); }

// 30 divsteps on the low 30 bits of f and g; branch-free: masks only.  -> the new delta; t = the batch's matrix.
// Bit 0 of g at step i is a function of the low i + 1 bits of f0 and g0, so nothing above bit 29 is read, and the words wrap as unsigned numbers do.
MB_HD int32_t mi_divsteps30(int32_t delta, uint32_t f0, uint32_t g0, mi_mat_t &t) {
    uint32_t u = 1, v = 0, q = 0, r = 1, f = f0, g = g0, dl = (uint32_t)delta;
#pragma unroll
    for (int i = 0; i < MI_STEPS; ++i) {
        uint32_t c1 = 0u - (uint32_t)((int32_t)dl > 0);          // delta > 0
        const uint32_t c2 = 0u - (g & 1u);                       // g odd
        const uint32_t x = (f ^ c1) - c1, y = (u ^ c1) - c1, z = (v ^ c1) - c1;      // -f, -u, -v where delta > 0
        g += x & c2; q += y & c2; r += z & c2;                   // g odd: g +- f, and the matrix row with it
        c1 &= c2;                                                // the swap: delta > 0 and g odd
        dl = ((dl ^ c1) - c1) + 1u;                              // 1 - delta | 1 + delta
        f += g & c1; u += q & c1; v += r & c1;                   // f <- the old g = (g - f) + f
        g >>= 1; u <<= 1; v <<= 1;
    }
    t.u = (int32_t)u; t.v = (int32_t)v; t.q = (int32_t)q; t.r = (int32_t)r;
    return (int32_t)dl;
}

// (f, g) <- t (f, g) / 2^30
MB_HD void mi_update_fg(mi30_t &f, mi30_t &g, const mi_mat_t &t) {
    const int64_t u = t.u, v = t.v, q = t.q, r = t.r;
    int64_t cf = u * f.v[0] + v * g.v[0], cg = q * f.v[0] + r * g.v[0];
    cf = mi_sar(cf, 30); cg = mi_sar(cg, 30);                    // the low 30 bits are zero
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const int64_t fi = f.v[i], gi = g.v[i];
        cf += u * fi + v * gi; cg += q * fi + r * gi;
        f.v[i - 1] = mi_low30(cf); cf = mi_sar(cf, 30);
        g.v[i - 1] = mi_low30(cg); cg = mi_sar(cg, 30);
    }
    f.v[8] = (int32_t)cf; g.v[8] = (int32_t)cg;
}

// (d, e) <- (t (d, e) + (md, me) p) / 2^30, -2p < d, e < p before and after (the proof: at the top of the file)
template <int F> MB_HD void mi_update_de(mi30_t &d, mi30_t &e, const mi_mat_t &t) {
    const int64_t u = t.u, v = t.v, q = t.q, r = t.r;
    const int32_t sd = d.v[8] < 0 ? -1 : 0, se = e.v[8] < 0 ? -1 : 0;
    int32_t md = (t.u & sd) + (t.v & se), me = (t.q & sd) + (t.r & se);          // + p per negative operand: t (d', e')
    int64_t cd = u * d.v[0] + v * e.v[0], ce = q * d.v[0] + r * e.v[0];
    md -= (int32_t)((mi_p_inv30<F>() * (uint32_t)(uint64_t)cd + (uint32_t)md) & MI_M30);     // - k p, 0 <= k < 2^30: the low 30 bits of cd + md p_0 become zero
    me -= (int32_t)((mi_p_inv30<F>() * (uint32_t)(uint64_t)ce + (uint32_t)me) & MI_M30);
    cd += (int64_t)mi_p_limb<F>(0) * md; ce += (int64_t)mi_p_limb<F>(0) * me;
    cd = mi_sar(cd, 30); ce = mi_sar(ce, 30);
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const int64_t di = d.v[i], ei = e.v[i];
        cd += u * di + v * ei; ce += q * di + r * ei;
        if (mi_p_limb<F>(i) != 0) { cd += (int64_t)mi_p_limb<F>(i) * md; ce += (int64_t)mi_p_limb<F>(i) * me; }      // (limbs 5, 6, 7 of p are zero)
        d.v[i - 1] = mi_low30(cd); cd = mi_sar(cd, 30);
        e.v[i - 1] = mi_low30(ce); ce = mi_sar(ce, 30);
    }
    d.v[8] = (int32_t)cd; e.v[8] = (int32_t)ce;
}

// d in (-2p, p) -> sign(f) d mod p in [0, p), limbs in [0, 2^30)
template <int F> MB_HD void mi_normalize(mi30_t &d, int32_t f_top) {
    const int32_t add = d.v[8] < 0 ? -1 : 0, neg = f_top < 0 ? -1 : 0;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {                                // + p where negative: (-p, p); then the sign of f; carries
        int32_t x = d.v[i] + (mi_p_limb<F>(i) & add);
        x = (x ^ neg) - neg;
        x += c;
        c = (int32_t)mi_sar(x, 30);
        d.v[i] = i < 8 ? (int32_t)((uint32_t)x & MI_M30) : x;
    }
    const int32_t add2 = d.v[8] < 0 ? -1 : 0;
    c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {                                // + p where still negative: [0, p)
        int32_t x = d.v[i] + (mi_p_limb<F>(i) & add2) + c;
        c = (int32_t)mi_sar(x, 30);
        d.v[i] = i < 8 ? (int32_t)((uint32_t)x & MI_M30) : x;
    }
}

MB_HD mi30_t mi_from_words(const fe_t &a) {
    mi30_t r;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int w = (30 * i) >> 5, s = (30 * i) & 31;
        const uint64_t x = (uint64_t)a.v[w] | (w + 1 < 8 ? (uint64_t)a.v[w + 1] << 32 : 0);
        r.v[i] = (int32_t)((x >> s) & MI_M30);
    }
    return r;
}
MB_HD fe_t mi_to_words(const mi30_t &a) {           // limbs in [0, 2^30), value below 2^256
    fe_t r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = (32 * i) / 30, s = (32 * i) % 30;
        const uint64_t x = ((uint64_t)(uint32_t)a.v[k] >> s) | ((uint64_t)(uint32_t)a.v[k + 1] << (30 - s));
        r.v[i] = (uint32_t)x;
    }
    return r;
}
template <int F> MB_HD mi30_t mi_modulus() {
    mi30_t r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] = mi_p_limb<F>(i);
    return r;
}

struct mi_no_trace { MB_HD void operator()(int, int32_t, const mi30_t &, const mi30_t &, const mi30_t &, const mi30_t &) const {} };

// the inverse of the INTEGER a modulo p, words in, words below p out; `trace` sees delta, f, g, d, e at the end of every batch that ran (the host tests' hook)
template <int F, class Trace> MB_HD fe_t mi_inverse_words(const fe_t &a, const Trace &trace) {
    mi30_t f = mi_modulus<F>(), g = mi_from_words(a), d, e;
#pragma unroll
    for (int i = 0; i < 9; ++i) { d.v[i] = 0; e.v[i] = 0; }
    e.v[0] = 1;
    int32_t delta = 1;
#pragma unroll 1
    for (int b = 0; b < MI_BATCHES; ++b) {
        int32_t nz = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) nz |= g.v[i];
        if (nz == 0) break;
        mi_mat_t t;
        delta = mi_divsteps30(delta, (uint32_t)f.v[0], (uint32_t)g.v[0], t);
        mi_update_de<F>(d, e, t);
        mi_update_fg(f, g, t);
        trace(b, delta, f, g, d, e);
    }
    mi_normalize<F>(d, f.v[8]);
    return mi_to_words(d);
}

// fe_inv's contract on the divstep iteration: what comes out of the loop is (a_plain R)^-1 = a_plain^-1 R^-1, and two Montgomery products by R^2 make it
// a_plain^-1 R.  r2: FieldK::r2.
template <int F> MB_HD fe_t fe_inv_gcd_r2(const fe_t &a, const fe_t &r2) {
    const fe_t x = mi_inverse_words<F>(a, mi_no_trace{});
    return fe_mul<F>(fe_mul<F>(x, r2), r2);
}
template <int F> MB_HD fe_t fe_inv_gcd(const fe_t &a, const FieldK &k) { return fe_inv_gcd_r2<F>(a, k.r2); }

// A kernel body's inversion as a type, over the FieldK the kernel already has (mina_ctx_set_chain_inverse): `foo_kernel` is its body with FeInvPow, `foo_gcd_kernel`
// the same body with FeInvGcd; the host picks one per launch.  A kernel holds ONE of the two routines.
struct FeInvPow { template <int F> static MB_HD fe_t inv(const fe_t &a, const FieldK &k) { return fe_inv<F>(a, k); } };
struct FeInvGcd { template <int F> static MB_HD fe_t inv(const fe_t &a, const FieldK &k) { return fe_inv_gcd<F>(a, k); } };

}  // namespace mb
