/* hbls_dev.hip — MI355X-native (gfx950/CDNA4) BLS12-381 library: device field
 * arithmetic, curve/pairing kernels, and the C-ABI host layer (include/hbls.h).
 *
 * THE PRODUCT PATH.  No CPU fallback: every entry point fails with
 * HBLS_ERR_NOGPU when no AMD GPU is present (the CPU oracle under oracle/ is
 * test infrastructure only and is never linked here).
 *
 * Semantics: herumi bls/mcl with BLS_SWAP_G=1, restated from the reference's
 * FFI usage (see include/hbls.h per-function cites and oracle/pyref.py
 * provenance notes).  Parity: bit-exact vs oracle/ on serialized outputs;
 * accept/reject-exact on verifies (tests/test_gpu_parity.py).
 *
 * Design notes (round 1 — correctness-first, VALU-bound):
 *  - Fp = 6x64-bit limbs, Montgomery (R=2^384), CIOS via unsigned __int128
 *    (lowers to v_mad_u64_u32 chains on gfx950).
 *  - one THREAD per independent crypto item (hash/sign/pairing); one BLOCK
 *    (256 threads, LDS tree) per masked-aggregate item.  EC point sums are
 *    associative, so the tree reduction is bit-exact vs the reference's
 *    sequential Mask.SetMask loop after normalization.
 *  - this is wide-integer VALU work: no MFMA (BASELINE.json north_star).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../oracle/bls_consts.h"
#include "../../include/hbls.h"

typedef unsigned __int128 u128;

#define DEV __device__ __forceinline__
/* Heavyweight primitives are real calls: full inlining of the fp_mul ->
 * fp2 -> fp6 -> fp12 -> pairing chain makes the verify kernels explode to
 * O(100k) instructions and hipcc compile time to tens of minutes.  Call
 * overhead is negligible against their instruction counts. */
#define DEVN __device__ __noinline__

/* ================================================================ Fp */
struct fp_t { uint64_t l[6]; };
struct fp2_t { fp_t a, b; };

DEV bool fp_is_zero(const fp_t &x) {
    return (x.l[0] | x.l[1] | x.l[2] | x.l[3] | x.l[4] | x.l[5]) == 0;
}
DEV bool fp_eq(const fp_t &x, const fp_t &y) {
    uint64_t d = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) d |= x.l[i] ^ y.l[i];
    return d == 0;
}
DEV bool fp_geq_p(const uint64_t t[6]) {
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        if (t[i] > BLS_P[i]) return true;
        if (t[i] < BLS_P[i]) return false;
    }
    return true;
}
DEV void fp_cond_sub_p(fp_t &r, const uint64_t t[6], uint64_t hi) {
    if (hi || fp_geq_p(t)) {
        u128 bw = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            u128 d = (u128)t[i] - BLS_P[i] - (uint64_t)bw;
            r.l[i] = (uint64_t)d;
            bw = (d >> 64) & 1;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++) r.l[i] = t[i];
    }
}
DEV void fp_add(fp_t &r, const fp_t &x, const fp_t &y) {
    uint64_t t[6];
    u128 c = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        c += (u128)x.l[i] + y.l[i];
        t[i] = (uint64_t)c;
        c >>= 64;
    }
    fp_cond_sub_p(r, t, (uint64_t)c);
}
DEV void fp_sub(fp_t &r, const fp_t &x, const fp_t &y) {
    uint64_t t[6];
    u128 bw = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        u128 d = (u128)x.l[i] - y.l[i] - (uint64_t)bw;
        t[i] = (uint64_t)d;
        bw = (d >> 64) & 1;
    }
    if (bw) {
        u128 c = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            c += (u128)t[i] + BLS_P[i];
            t[i] = (uint64_t)c;
            c >>= 64;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) r.l[i] = t[i];
}
DEV void fp_neg(fp_t &r, const fp_t &x) {
    if (fp_is_zero(x)) { r = x; return; }
    u128 bw = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        u128 d = (u128)BLS_P[i] - x.l[i] - (uint64_t)bw;
        r.l[i] = (uint64_t)d;
        bw = (d >> 64) & 1;
    }
}
DEV void fp_dbl(fp_t &r, const fp_t &x) { fp_add(r, x, x); }

/* 12x32-limb CIOS — every product is one v_mad_u64_u32 (32x32+64); measured
 * 1.29x the 6x64/u128 form on gfx950 (hbls_fpmul_bench_ops A/B).  The u64
 * interface/layout is unchanged; split/repack is ~5% of the mads.
 * The body is shared between the default CALL form (noinline: a fully
 * inlined build thrashes the instruction cache and ran pathologically
 * slow) and an inline clone used only inside fp2_mul/fp2_sqr. */
/* optional per-call fp_mul counter (perf-instrumentation builds only:
 * -DHBLS_COUNT_MULS; settles the roofline's algorithmic-mul denominator
 * with the GPU path's OWN count instead of the oracle's) */
#ifdef HBLS_COUNT_MULS
__device__ unsigned long long g_fp_mul_count;
#define MULCOUNT() atomicAdd(&g_fp_mul_count, 1ull)
#else
#define MULCOUNT()
#endif

#define FP_MUL_BODY(r, x, y) do { \
    MULCOUNT(); \
    uint32_t a_[12], b_[12], t_[13]; \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < 6; i_++) { \
        a_[2 * i_] = (uint32_t)(x).l[i_]; \
        a_[2 * i_ + 1] = (uint32_t)((x).l[i_] >> 32); \
        b_[2 * i_] = (uint32_t)(y).l[i_]; \
        b_[2 * i_ + 1] = (uint32_t)((y).l[i_] >> 32); \
    } \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < 13; i_++) t_[i_] = 0; \
    uint32_t t13_ = 0; \
    const uint32_t pinv32_ = (uint32_t)BLS_P_INV; \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < 12; i_++) { \
        uint64_t acc_ = 0; \
        uint32_t ai_ = a_[i_]; \
        _Pragma("unroll") \
        for (int j_ = 0; j_ < 12; j_++) { \
            acc_ = (uint64_t)ai_ * b_[j_] + t_[j_] + (uint32_t)(acc_ >> 32); \
            t_[j_] = (uint32_t)acc_; \
        } \
        acc_ = (uint64_t)t_[12] + (uint32_t)(acc_ >> 32); \
        t_[12] = (uint32_t)acc_; \
        t13_ = (uint32_t)(acc_ >> 32); \
        uint32_t m_ = t_[0] * pinv32_; \
        acc_ = (uint64_t)m_ * (uint32_t)BLS_P[0] + t_[0]; \
        _Pragma("unroll") \
        for (int j_ = 1; j_ < 12; j_++) { \
            uint32_t pj_ = (uint32_t)(BLS_P[j_ >> 1] >> ((j_ & 1) * 32)); \
            acc_ = (uint64_t)m_ * pj_ + t_[j_] + (uint32_t)(acc_ >> 32); \
            t_[j_ - 1] = (uint32_t)acc_; \
        } \
        acc_ = (uint64_t)t_[12] + (uint32_t)(acc_ >> 32); \
        t_[11] = (uint32_t)acc_; \
        t_[12] = t13_ + (uint32_t)(acc_ >> 32); \
    } \
    uint64_t w_[6]; \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < 6; i_++) \
        w_[i_] = (uint64_t)t_[2 * i_] | ((uint64_t)t_[2 * i_ + 1] << 32); \
    fp_cond_sub_p(r, w_, t_[12]); \
} while (0)

/* Hand-allocated asm CIOS core (generated: gen_fp_mul_asm.py) — same
 * semantics as FP_MUL_BODY, 938 instrs vs the compiler's 1415 (the pinned
 * t-register pairs let each v_mad_u64_u32 write (limb, carry) directly,
 * killing the pair-shuffle movs). */
#include "fp_mul_asm.inc"
#define FP_MUL_ASM_BODY(r, x, y) do { \
    MULCOUNT(); \
    uint32_t a_[12], b_[12], t_[13]; \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < 6; i_++) { \
        a_[2 * i_] = (uint32_t)(x).l[i_]; \
        a_[2 * i_ + 1] = (uint32_t)((x).l[i_] >> 32); \
        b_[2 * i_] = (uint32_t)(y).l[i_]; \
        b_[2 * i_ + 1] = (uint32_t)((y).l[i_] >> 32); \
    } \
    fp_mul_asm_core(t_, a_, b_); \
    uint64_t w_[6]; \
    _Pragma("unroll") \
    for (int i_ = 0; i_ < 6; i_++) \
        w_[i_] = (uint64_t)t_[2 * i_] | ((uint64_t)t_[2 * i_ + 1] << 32); \
    fp_cond_sub_p(r, w_, t_[12]); \
} while (0)

/* Measured verdict (see ROUND2_NOTES.md): the asm core is bit-exact and
 * cuts issue count 1415->1158, but fp_mul is BOUND BY v_mad_u64_u32
 * EXECUTION, not issue — +4.7% on the called-form µbench, +-0% end to end
 * (inline sites regress: register pins cost shuffle movs).  Default stays
 * the compiler body; -DHBLS_ASM_FPMUL switches the called form to asm for
 * future A/Bs. */
#ifdef HBLS_ASM_FPMUL
DEV void fp_mul_inl(fp_t &r, const fp_t &x, const fp_t &y) { FP_MUL_BODY(r, x, y); }
DEV void fp_sqr_inl(fp_t &r, const fp_t &x) { FP_MUL_BODY(r, x, x); }
DEVN void fp_mul(fp_t &r, const fp_t &x, const fp_t &y) { FP_MUL_ASM_BODY(r, x, y); }
#else
DEV void fp_mul_inl(fp_t &r, const fp_t &x, const fp_t &y) { FP_MUL_BODY(r, x, y); }
DEV void fp_sqr_inl(fp_t &r, const fp_t &x) { FP_MUL_BODY(r, x, x); }
DEVN void fp_mul(fp_t &r, const fp_t &x, const fp_t &y) { FP_MUL_BODY(r, x, y); }
#endif
DEVN void fp_mul_asm(fp_t &r, const fp_t &x, const fp_t &y) { FP_MUL_ASM_BODY(r, x, y); }
DEVN void fp_mul_c(fp_t &r, const fp_t &x, const fp_t &y) { FP_MUL_BODY(r, x, y); }
DEV void fp_sqr(fp_t &r, const fp_t &x) { fp_mul(r, x, x); }

DEV void fp_one(fp_t &r) {
#pragma unroll
    for (int i = 0; i < 6; i++) r.l[i] = BLS_ONE_P[i];
}
DEV void fp_zero(fp_t &r) {
#pragma unroll
    for (int i = 0; i < 6; i++) r.l[i] = 0;
}
DEV void fp_load(fp_t &r, const uint64_t v[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) r.l[i] = v[i];
}
DEV void fp_to_mont(fp_t &r, const uint64_t raw[6]) {
    fp_t t, r2;
#pragma unroll
    for (int i = 0; i < 6; i++) { t.l[i] = raw[i]; r2.l[i] = BLS_R2P[i]; }
    fp_mul(r, t, r2);
}
DEVN void fp_from_mont(uint64_t raw[6], const fp_t &x) {
    fp_t one, t;
    fp_zero(one);
    one.l[0] = 1;
    fp_mul(t, x, one);
#pragma unroll
    for (int i = 0; i < 6; i++) raw[i] = t.l[i];
}
/* s = x^((p-3)/4): the one exponentiation behind sqrt, legendre and inverse
 * (p = 3 mod 4).  (p-3)/4 = p >> 2, so bit k of p drives step k-2; bit 380
 * is p's top bit.  With c = s*x: c^2 = x iff x is a square, and then
 * 1/c = s — a root and its inverse from one chain (fp2_sqrt_tail). */
#ifdef HBLS_POW_BINARY
DEVN void fp_pow_pm3o4(fp_t &s, const fp_t &x) {
    fp_t acc = x;
    for (int k = 379; k >= 2; k--) {
        fp_sqr_inl(acc, acc);
        if ((BLS_P[k >> 6] >> (k & 63)) & 1) fp_mul_inl(acc, acc, x);
    }
    s = acc;
}
#else
/* Sliding-window schedule for the fixed exponent, derived from the modulus
 * at compile time: 4-bit windows over the odd powers x^1..x^15.  Entry i
 * says "square nsq[i] times, then multiply by tab[idx[i]]"; idx 8 means no
 * multiply (the exponent's trailing zero bits).  461 fp-mul against 570 for
 * the binary chain (-DHBLS_POW_BINARY keeps that one for A/Bs); one shared
 * inlined squaring and one inlined multiply, the 8 table entries through
 * the called fp_mul. */
#define POW_WIN 4
#define POW_NOMUL (1 << (POW_WIN - 1))
struct pow_sched_t { uint8_t nsq[128], idx[128]; int n, first; };
/* BLS_P again, as a constexpr (the generated header's copy is a plain const
 * array, which a constant expression may not read) */
static constexpr uint64_t POW_P[6] = { 0xb9feffffffffaaabULL, 0x1eabfffeb153ffffULL, 0x6730d2a0f6b0f624ULL, 0x64774b84f38512bfULL, 0x4b1ba7b6434bacd7ULL, 0x1a0111ea397fe69aULL };
constexpr int pm3o4_bit(int k) { return (int)((POW_P[(k + 2) >> 6] >> ((k + 2) & 63)) & 1); }
constexpr pow_sched_t pm3o4_sched() {
    pow_sched_t s{};
    int k = 378, pending = 0;
    bool first = true;
    while (k >= 0) {
        if (!pm3o4_bit(k)) { pending++; k--; continue; }
        int l = k - (POW_WIN - 1) < 0 ? 0 : k - (POW_WIN - 1);
        while (!pm3o4_bit(l)) l++;
        int v = 0;
        for (int j = k; j >= l; j--) v = 2 * v + pm3o4_bit(j);
        if (first) { s.first = v >> 1; first = false; }
        else { s.nsq[s.n] = (uint8_t)(pending + k - l + 1); s.idx[s.n] = (uint8_t)(v >> 1); s.n++; }
        pending = 0;
        k = l - 1;
    }
    if (pending) { s.nsq[s.n] = (uint8_t)pending; s.idx[s.n] = POW_NOMUL; s.n++; }
    return s;
}
static constexpr pow_sched_t PM3O4 = pm3o4_sched();
DEVN void fp_pow_pm3o4(fp_t &s, const fp_t &x) {
    fp_t tab[POW_NOMUL], x2, acc;
    tab[0] = x;
    fp_sqr(x2, x);
    for (int i = 1; i < POW_NOMUL; i++) fp_mul(tab[i], tab[i - 1], x2);
    acc = tab[PM3O4.first];
    for (int i = 0; i < PM3O4.n; i++) {
        for (int j = PM3O4.nsq[i]; j > 0; j--) fp_sqr_inl(acc, acc);
        if (PM3O4.idx[i] != POW_NOMUL) fp_mul_inl(acc, acc, tab[PM3O4.idx[i]]);
    }
    s = acc;
}
#endif
/* x^(p-2) = s^4 x */
DEVN void fp_inv(fp_t &r, const fp_t &x) {
    fp_t s;
    fp_pow_pm3o4(s, x);
    fp_sqr(s, s);
    fp_sqr(s, s);
    fp_mul(r, s, x);
}
/* x^((p+1)/4) = s x, then check */
DEVN bool fp_sqrt(fp_t &r, const fp_t &x) {
    fp_t y, y2;
    fp_pow_pm3o4(y, x);
    fp_mul(y, y, x);
    fp_sqr(y2, y);
    if (!fp_eq(y2, x)) return false;
    r = y;
    return true;
}
/* x^((p-1)/2) = s^2 x */
DEVN int fp_legendre(const fp_t &x) {
    if (fp_is_zero(x)) return 0;
    fp_t y, one;
    fp_pow_pm3o4(y, x);
    fp_sqr(y, y);
    fp_mul(y, y, x);
    fp_one(one);
    return fp_eq(y, one) ? 1 : -1;
}
/* x/2: add p when odd, shift right (x + p < 2^382, no carry out).  Holds on
 * Montgomery form unchanged. */
DEV void fp_half(fp_t &r, const fp_t &x) {
    uint64_t t[6];
    const uint64_t m = 0 - (x.l[0] & 1);
    u128 c = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        c += (u128)x.l[i] + (BLS_P[i] & m);
        t[i] = (uint64_t)c;
        c >>= 64;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) r.l[i] = (t[i] >> 1) | (t[i + 1] << 63);
    r.l[5] = t[5] >> 1;
}
DEVN bool fp_is_odd(const fp_t &x) {
    uint64_t raw[6];
    fp_from_mont(raw, x);
    return raw[0] & 1;
}


/* register-ABI multiplier: 12 scalar u64 args + 12-dword struct return ride
 * entirely in VGPRs (zero scratch at the call boundary — measured, see
 * DESIGN.md §4b).  Shared by the HBLS_FP2_RS compact-code experiment and
 * the opt-in rf build. */
DEVN fp_t fp_mul_rs(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t x3,
                    uint64_t x4, uint64_t x5,
                    uint64_t y0, uint64_t y1, uint64_t y2, uint64_t y3,
                    uint64_t y4, uint64_t y5) {
    fp_t x, y, r;
    x.l[0] = x0; x.l[1] = x1; x.l[2] = x2; x.l[3] = x3; x.l[4] = x4; x.l[5] = x5;
    y.l[0] = y0; y.l[1] = y1; y.l[2] = y2; y.l[3] = y3; y.l[4] = y4; y.l[5] = y5;
    FP_MUL_BODY(r, x, y);
    return r;
}
#define RFM(r, x, y) (r) = fp_mul_rs((x).l[0], (x).l[1], (x).l[2], (x).l[3], (x).l[4], (x).l[5], \
                                     (y).l[0], (y).l[1], (y).l[2], (y).l[3], (y).l[4], (y).l[5])

/* ================================================================ Fp2 */
DEV bool fp2_is_zero(const fp2_t &x) { return fp_is_zero(x.a) && fp_is_zero(x.b); }
DEV bool fp2_eq(const fp2_t &x, const fp2_t &y) { return fp_eq(x.a, y.a) && fp_eq(x.b, y.b); }
DEV void fp2_add(fp2_t &r, const fp2_t &x, const fp2_t &y) { fp_add(r.a, x.a, y.a); fp_add(r.b, x.b, y.b); }
DEV void fp2_sub(fp2_t &r, const fp2_t &x, const fp2_t &y) { fp_sub(r.a, x.a, y.a); fp_sub(r.b, x.b, y.b); }
DEV void fp2_neg(fp2_t &r, const fp2_t &x) { fp_neg(r.a, x.a); fp_neg(r.b, x.b); }
DEV void fp2_conj(fp2_t &r, const fp2_t &x) { r.a = x.a; fp_neg(r.b, x.b); }
DEV void fp2_dbl(fp2_t &r, const fp2_t &x) { fp2_add(r, x, x); }
DEV void fp2_half(fp2_t &r, const fp2_t &x) { fp_half(r.a, x.a); fp_half(r.b, x.b); }
DEVN void fp2_mul(fp2_t &r, const fp2_t &x, const fp2_t &y) {
#ifdef HBLS_FP2_RS
    /* compact-code variant: ~400-instr body + calls into the shared
     * register-ABI CIOS, instead of three inlined ~1.4k-instr CIOS copies
     * (the inlined form makes fp2_mul a 5k-instr function and the Miller
     * call set ~240 KB vs the 32 KB I-cache) */
    fp_t ac, bd, ab, cd, t;
    RFM(ac, x.a, y.a);
    RFM(bd, x.b, y.b);
    fp_add(ab, x.a, x.b);
    fp_add(cd, y.a, y.b);
    RFM(t, ab, cd);
    fp_sub(t, t, ac);
    fp_sub(t, t, bd);
    fp_sub(r.a, ac, bd);
    r.b = t;
#else
    fp_t ac, bd, ab, cd, t;
    fp_mul_inl(ac, x.a, y.a);
    fp_mul_inl(bd, x.b, y.b);
    fp_add(ab, x.a, x.b);
    fp_add(cd, y.a, y.b);
    fp_mul_inl(t, ab, cd);
    fp_sub(t, t, ac);
    fp_sub(t, t, bd);
    fp_sub(r.a, ac, bd);
    r.b = t;
#endif
}
DEVN void fp2_sqr(fp2_t &r, const fp2_t &x) {
#ifdef HBLS_FP2_RS
    fp_t s, d, m;
    fp_add(s, x.a, x.b);
    fp_sub(d, x.a, x.b);
    RFM(m, x.a, x.b);
    RFM(r.a, s, d);
    fp_dbl(r.b, m);
#else
    fp_t s, d, m;
    fp_add(s, x.a, x.b);
    fp_sub(d, x.a, x.b);
    fp_mul_inl(m, x.a, x.b);
    fp_mul_inl(r.a, s, d);
    fp_dbl(r.b, m);
#endif
}
DEV void fp2_mul_fp(fp2_t &r, const fp2_t &x, const fp_t &s) {
    fp_mul(r.a, x.a, s);
    fp_mul(r.b, x.b, s);
}
DEV void fp2_mul_xi(fp2_t &r, const fp2_t &x) {
    fp_t na, nb;
    fp_sub(na, x.a, x.b);
    fp_add(nb, x.a, x.b);
    r.a = na; r.b = nb;
}
DEVN void fp2_inv(fp2_t &r, const fp2_t &x) {
    fp_t n, t, ia, ib;
    fp_sqr(n, x.a);
    fp_sqr(t, x.b);
    fp_add(n, n, t);
    fp_inv(n, n);
    fp_mul(ia, x.a, n);
    fp_mul(t, x.b, n);
    fp_neg(ib, t);
    r.a = ia; r.b = ib;
}
DEV void fp2_one(fp2_t &r) { fp_one(r.a); fp_zero(r.b); }
DEV void fp2_zero(fp2_t &r) { fp_zero(r.a); fp_zero(r.b); }
/* b != 0 half of fp2_sqrt, given w = sqrt(a^2 + b^2): t = (a+w)/2, else
 * (a-w)/2; c = sqrt t; d = b/(2c).  t != 0 because b != 0, so with
 * s = t^((p-3)/4) and c = s t, c^2 = t gives 1/c = s and d = b s / 2: one
 * exponentiation per attempt and no inversion. */
DEVN bool fp2_sqrt_tail(fp2_t &r, const fp2_t &x, const fp_t &w) {
    fp_t t, s, c, c2, d;
    fp_add(t, x.a, w);
    fp_half(t, t);
    fp_pow_pm3o4(s, t);
    fp_mul(c, s, t);
    fp_sqr(c2, c);
    if (!fp_eq(c2, t)) {
        fp_sub(t, x.a, w);
        fp_half(t, t);
        fp_pow_pm3o4(s, t);
        fp_mul(c, s, t);
        fp_sqr(c2, c);
        if (!fp_eq(c2, t)) return false;
    }
    fp_mul(d, x.b, s);
    fp_half(d, d);
    r.a = c; r.b = d;
    return true;
}
DEVN bool fp2_sqrt(fp2_t &r, const fp2_t &x) {
    if (fp_is_zero(x.b)) {
        fp_t s, na;
        if (fp_sqrt(s, x.a)) { r.a = s; fp_zero(r.b); return true; }
        fp_neg(na, x.a);
        if (fp_sqrt(s, na)) { fp_zero(r.a); r.b = s; return true; }
        return false;
    }
    fp_t n, t, w;
    fp_sqr(n, x.a);
    fp_sqr(t, x.b);
    fp_add(n, n, t);
    if (!fp_sqrt(w, n)) return false;
    return fp2_sqrt_tail(r, x, w);
}
/* Either root of x, for callers that fix the sign afterwards by parity
 * (g2_deserialize).  Same accept/reject as fp2_sqrt; the b != 0 path needs
 * no second attempt: with t = (a+w)/2, s = t^((p-3)/4), c = s t, c^2 is t
 * or -t.  If -t, then t' = (a-w)/2 = -b^2/(4t) is the square, s^2 = -1/t
 * and s c = -1, so (b s / 2, -c) is a root: its square is
 * (t' + t) + (-b s c) u = a + b u.  Both components are non-zero on this
 * path, so the parity of the result decides the sign. */
DEVN bool fp2_sqrt_any(fp2_t &r, const fp2_t &x) {
    if (fp_is_zero(x.b)) return fp2_sqrt(r, x);
    fp_t n, t, w, s, c, c2, d;
    fp_sqr(n, x.a);
    fp_sqr(t, x.b);
    fp_add(n, n, t);
    if (!fp_sqrt(w, n)) return false;
    fp_add(t, x.a, w);
    fp_half(t, t);
    fp_pow_pm3o4(s, t);
    fp_mul(c, s, t);
    fp_sqr(c2, c);
    fp_mul(d, x.b, s);
    fp_half(d, d);
    if (fp_eq(c2, t)) { r.a = c; r.b = d; return true; }
    fp_neg(c2, c2);
    if (!fp_eq(c2, t)) return false;
    r.a = d; fp_neg(r.b, c);
    return true;
}
DEV bool fp2_is_odd(const fp2_t &x) { return fp_is_odd(x.a); }

/* ================================================================ G1 */
struct g1_t { fp_t x, y, z; };
struct g1aff_t { fp_t x, y; };
struct g2_t { fp2_t x, y, z; };
struct g2aff_t { fp2_t x, y; };

DEV void g1_set_inf(g1_t &p) { fp_one(p.x); fp_one(p.y); fp_zero(p.z); }
DEV bool g1_is_inf(const g1_t &p) { return fp_is_zero(p.z); }
DEVN void g1_dbl(g1_t &r, const g1_t &p) {
    if (g1_is_inf(p)) { r = p; return; }
    fp_t A, B, C, D, E, F, t;
    fp_sqr_inl(A, p.x);
    fp_sqr_inl(B, p.y);
    fp_sqr_inl(C, B);
    fp_add(t, p.x, B);
    fp_sqr_inl(t, t);
    fp_sub(t, t, A);
    fp_sub(t, t, C);
    fp_dbl(D, t);
    fp_dbl(E, A);
    fp_add(E, E, A);
    fp_sqr_inl(F, E);
    fp_t nx, nz;
    fp_sub(nx, F, D);
    fp_sub(nx, nx, D);
    fp_mul_inl(t, p.y, p.z);
    fp_dbl(nz, t);
    fp_sub(t, D, nx);
    fp_mul_inl(t, E, t);
    fp_dbl(C, C); fp_dbl(C, C); fp_dbl(C, C);
    fp_sub(r.y, t, C);
    r.x = nx;
    r.z = nz;
}
DEVN void g1_add(g1_t &r, const g1_t &p, const g1_t &q) {
    if (g1_is_inf(p)) { r = q; return; }
    if (g1_is_inf(q)) { r = p; return; }
    fp_t z1z1, z2z2, u1, u2, s1, s2, h, rr, hh, hhh, v, t;
    fp_sqr_inl(z1z1, p.z);
    fp_sqr_inl(z2z2, q.z);
    fp_mul_inl(u1, p.x, z2z2);
    fp_mul_inl(u2, q.x, z1z1);
    fp_mul_inl(s1, p.y, q.z); fp_mul_inl(s1, s1, z2z2);
    fp_mul_inl(s2, q.y, p.z); fp_mul_inl(s2, s2, z1z1);
    fp_sub(h, u2, u1);
    fp_sub(rr, s2, s1);
    if (fp_is_zero(h)) {
        if (fp_is_zero(rr)) { g1_dbl(r, p); return; }
        g1_set_inf(r); return;
    }
    fp_sqr_inl(hh, h);
    fp_mul_inl(hhh, hh, h);
    fp_mul_inl(v, u1, hh);
    fp_sqr_inl(t, rr);
    fp_sub(t, t, hhh);
    fp_sub(t, t, v);
    fp_sub(r.x, t, v);
    fp_sub(t, v, r.x);
    fp_mul_inl(t, rr, t);
    fp_mul_inl(v, s1, hhh);
    fp_sub(r.y, t, v);
    fp_mul_inl(t, p.z, q.z);
    fp_mul_inl(r.z, t, h);
}
/* mixed add: r = p + affine q (q never infinity — table keys) */
#define G1_MADD_BODY(r, p, q) do { \
    if (g1_is_inf(p)) { (r).x = (q).x; (r).y = (q).y; fp_one((r).z); break; } \
    fp_t z1z1, u2, s2, h, rr, hh, hhh, v, t; \
    fp_sqr_inl(z1z1, (p).z); \
    fp_mul_inl(u2, (q).x, z1z1); \
    fp_mul_inl(s2, (q).y, (p).z); \
    fp_mul_inl(s2, s2, z1z1); \
    fp_sub(h, u2, (p).x); \
    fp_sub(rr, s2, (p).y); \
    if (fp_is_zero(h)) { \
        if (fp_is_zero(rr)) { g1_dbl(r, p); break; } \
        g1_set_inf(r); break; \
    } \
    fp_sqr_inl(hh, h); \
    fp_mul_inl(hhh, hh, h); \
    fp_mul_inl(v, (p).x, hh); \
    fp_sqr_inl(t, rr); \
    fp_sub(t, t, hhh); \
    fp_sub(t, t, v); \
    fp_sub((r).x, t, v); \
    fp_sub(t, v, (r).x); \
    fp_mul_inl(t, rr, t); \
    fp_mul_inl(v, (p).y, hhh); \
    fp_sub((r).y, t, v); \
    fp_mul_inl((r).z, (p).z, h); \
} while (0)
DEVN void g1_madd(g1_t &r, const g1_t &p, const g1aff_t &q) { G1_MADD_BODY(r, p, q); }
/* inline clone for the mask kernel's accumulate loop: the DEVN call passes
 * the accumulator by reference, costing a 144 B scratch round-trip per
 * point addition; the kernel has exactly one call site so inlining
 * duplicates nothing. */
DEV void g1_madd_i(g1_t &r, const g1_t &p, const g1aff_t &q) { G1_MADD_BODY(r, p, q); }
DEV void g1_neg(g1_t &r, const g1_t &p) { r.x = p.x; fp_neg(r.y, p.y); r.z = p.z; }
DEVN void g1_to_affine(g1aff_t &r, const g1_t &p) {
    fp_t zi, zi2, zi3;
    fp_inv(zi, p.z);
    fp_sqr(zi2, zi);
    fp_mul(zi3, zi2, zi);
    fp_mul(r.x, p.x, zi2);
    fp_mul(r.y, p.y, zi3);
}
DEVN void g1_mul(g1_t &r, const g1_t &p, const uint64_t *k, int n) {
    g1_t acc;
    g1_set_inf(acc);
    bool started = false;
    for (int i = n - 1; i >= 0; i--)
        for (int b = 63; b >= 0; b--) {
            if (started) g1_dbl(acc, acc);
            if ((k[i] >> b) & 1) { g1_add(acc, acc, p); started = true; }
        }
    r = acc;
}

/* ================================================================ G2 */
DEV void g2_set_inf(g2_t &p) { fp2_one(p.x); fp2_one(p.y); fp2_zero(p.z); }
DEV bool g2_is_inf(const g2_t &p) { return fp2_is_zero(p.z); }
DEVN void g2_dbl(g2_t &r, const g2_t &p) {
    if (g2_is_inf(p)) { r = p; return; }
    fp2_t A, B, C, D, E, F, t, nx, nz;
    fp2_sqr(A, p.x);
    fp2_sqr(B, p.y);
    fp2_sqr(C, B);
    fp2_add(t, p.x, B);
    fp2_sqr(t, t);
    fp2_sub(t, t, A);
    fp2_sub(t, t, C);
    fp2_dbl(D, t);
    fp2_dbl(E, A);
    fp2_add(E, E, A);
    fp2_sqr(F, E);
    fp2_sub(nx, F, D);
    fp2_sub(nx, nx, D);
    fp2_mul(t, p.y, p.z);
    fp2_dbl(nz, t);
    fp2_sub(t, D, nx);
    fp2_mul(t, E, t);
    fp2_dbl(C, C); fp2_dbl(C, C); fp2_dbl(C, C);
    fp2_sub(r.y, t, C);
    r.x = nx;
    r.z = nz;
}
DEVN void g2_add(g2_t &r, const g2_t &p, const g2_t &q) {
    if (g2_is_inf(p)) { r = q; return; }
    if (g2_is_inf(q)) { r = p; return; }
    fp2_t z1z1, z2z2, u1, u2, s1, s2, h, rr, hh, hhh, v, t;
    fp2_sqr(z1z1, p.z);
    fp2_sqr(z2z2, q.z);
    fp2_mul(u1, p.x, z2z2);
    fp2_mul(u2, q.x, z1z1);
    fp2_mul(s1, p.y, q.z); fp2_mul(s1, s1, z2z2);
    fp2_mul(s2, q.y, p.z); fp2_mul(s2, s2, z1z1);
    fp2_sub(h, u2, u1);
    fp2_sub(rr, s2, s1);
    if (fp2_is_zero(h)) {
        if (fp2_is_zero(rr)) { g2_dbl(r, p); return; }
        g2_set_inf(r); return;
    }
    fp2_sqr(hh, h);
    fp2_mul(hhh, hh, h);
    fp2_mul(v, u1, hh);
    fp2_sqr(t, rr);
    fp2_sub(t, t, hhh);
    fp2_sub(t, t, v);
    fp2_sub(r.x, t, v);
    fp2_sub(t, v, r.x);
    fp2_mul(t, rr, t);
    fp2_mul(v, s1, hhh);
    fp2_sub(r.y, t, v);
    fp2_mul(t, p.z, q.z);
    fp2_mul(r.z, t, h);
}
DEV void g2_neg(g2_t &r, const g2_t &p) { r.x = p.x; fp2_neg(r.y, p.y); r.z = p.z; }
DEVN void g2_to_affine(g2aff_t &r, const g2_t &p) {
    fp2_t zi, zi2, zi3;
    fp2_inv(zi, p.z);
    fp2_sqr(zi2, zi);
    fp2_mul(zi3, zi2, zi);
    fp2_mul(r.x, p.x, zi2);
    fp2_mul(r.y, p.y, zi3);
}
DEV void g2_from_affine(g2_t &r, const g2aff_t &p) { r.x = p.x; r.y = p.y; fp2_one(r.z); }
DEVN void g2_mul(g2_t &r, const g2_t &p, const uint64_t *k, int n) {
    g2_t acc;
    g2_set_inf(acc);
    bool started = false;
    for (int i = n - 1; i >= 0; i--)
        for (int b = 63; b >= 0; b--) {
            if (started) g2_dbl(acc, acc);
            if ((k[i] >> b) & 1) { g2_add(acc, acc, p); started = true; }
        }
    r = acc;
}
DEVN void g2_psi(g2_t &r, const g2_t &p) {
    /* psi on Jacobian coords directly: x=X/Z^2, y=Y/Z^3 ->
     * (cx*conj(X), cy*conj(Y), conj(Z)) — no inversion needed. */
    if (g2_is_inf(p)) { r = p; return; }
    fp2_t cx, cy, t;
    fp_load(cx.a, BLS_PSI_CX_A); fp_load(cx.b, BLS_PSI_CX_B);
    fp_load(cy.a, BLS_PSI_CY_A); fp_load(cy.b, BLS_PSI_CY_B);
    fp2_conj(t, p.x); fp2_mul(r.x, t, cx);
    fp2_conj(t, p.y); fp2_mul(r.y, t, cy);
    fp2_conj(r.z, p.z);
}

/* ================================================================ serialization */
DEVN void fp_to_le48(uint8_t out[48], const fp_t &x) {
    uint64_t raw[6];
    fp_from_mont(raw, x);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 8; j++)
            out[i * 8 + j] = (uint8_t)(raw[i] >> (8 * j));
}
DEVN bool fp_from_le48(fp_t &x, const uint8_t in[48]) {
    uint64_t raw[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        raw[i] = 0;
#pragma unroll
        for (int j = 0; j < 8; j++)
            raw[i] |= (uint64_t)in[i * 8 + j] << (8 * j);
    }
    if (fp_geq_p(raw)) return false;
    fp_t t, r2;
    fp_load(t, raw);
    fp_load(r2, BLS_R2P);
    fp_mul(x, t, r2);
    return true;
}
DEV bool bytes_all_zero(const uint8_t *b, int n) {
    uint8_t acc = 0;
    for (int i = 0; i < n; i++) acc |= b[i];
    return acc == 0;
}
DEVN void g1_serialize(uint8_t out[48], const g1_t &p) {
    if (g1_is_inf(p)) {
        for (int i = 0; i < 48; i++) out[i] = 0;
        return;
    }
    g1aff_t a;
    g1_to_affine(a, p);
    fp_to_le48(out, a.x);
    if (fp_is_odd(a.y)) out[47] |= 0x80;
}
DEVN void g2_serialize(uint8_t out[96], const g2_t &p) {
    if (g2_is_inf(p)) {
        for (int i = 0; i < 96; i++) out[i] = 0;
        return;
    }
    g2aff_t a;
    g2_to_affine(a, p);
    fp_to_le48(out, a.x.a);
    fp_to_le48(out + 48, a.x.b);
    if (fp2_is_odd(a.y)) out[95] |= 0x80;
}
DEV void g1_b(fp_t &b) { fp_load(b, BLS_B1); }
DEV void g2_b(fp2_t &b) { fp_load(b.a, BLS_B2_A); fp_load(b.b, BLS_B2_B); }

DEV bool g1_in_subgroup(const g1_t &p) {
    g1_t t;
    g1_mul(t, p, BLS_R, 4);
    return g1_is_inf(t);
}
DEV bool g2_in_subgroup(const g2_t &p) {
    g2_t t;
    g2_mul(t, p, BLS_R, 4);
    return g2_is_inf(t);
}
DEV bool g2_eq_jac(const g2_t &p, const g2_t &q) {
    if (g2_is_inf(p) || g2_is_inf(q)) return g2_is_inf(p) && g2_is_inf(q);
    fp2_t z1z1, z2z2, a, b;
    fp2_sqr(z1z1, p.z); fp2_sqr(z2z2, q.z);
    fp2_mul(a, p.x, z2z2); fp2_mul(b, q.x, z1z1);
    if (!fp2_eq(a, b)) return false;
    fp2_mul(a, p.y, q.z); fp2_mul(a, a, z2z2);
    fp2_mul(b, q.y, p.z); fp2_mul(b, b, z1z1);
    return fp2_eq(a, b);
}
/* Scott's G2 membership criterion for BLS12-381: Q in E'(Fp2) is in the
 * order-r subgroup iff psi(Q) == [z]Q  (z negative: [z]Q = -[|z|]Q).
 * ~4x cheaper than the full [r]Q == inf check; equivalence property-tested
 * against the r-mult on valid and out-of-subgroup points (GPU tests). */
DEVN bool g2_in_subgroup_fast(const g2_t &p) {
    if (g2_is_inf(p)) return true;
    g2_t lhs, rhs;
    g2_psi(lhs, p);
    uint64_t u = BLS_U;
    g2_mul(rhs, p, &u, 1);
    g2_neg(rhs, rhs);
    return g2_eq_jac(lhs, rhs);
}
/* 1 ok; 0 bad; infinity accepted (idx==inf flag via out z=0) */
DEVN bool g1_deserialize(g1_t &p, const uint8_t in[48], bool check_subgroup) {
    if (bytes_all_zero(in, 48)) { g1_set_inf(p); return true; }
    uint8_t buf[48];
    for (int i = 0; i < 48; i++) buf[i] = in[i];
    bool odd = (buf[47] & 0x80) != 0;
    buf[47] &= 0x7F;
    g1aff_t a;
    if (!fp_from_le48(a.x, buf)) return false;
    fp_t y2, b;
    fp_sqr(y2, a.x); fp_mul(y2, y2, a.x);
    g1_b(b);
    fp_add(y2, y2, b);
    if (!fp_sqrt(a.y, y2)) return false;
    if (fp_is_odd(a.y) != odd) fp_neg(a.y, a.y);
    p.x = a.x; p.y = a.y; fp_one(p.z);
    if (check_subgroup && !g1_in_subgroup(p)) return false;
    return true;
}
DEVN bool g2_deserialize(g2_t &p, const uint8_t in[96], bool check_subgroup) {
    if (bytes_all_zero(in, 96)) { g2_set_inf(p); return true; }
    uint8_t buf[96];
    for (int i = 0; i < 96; i++) buf[i] = in[i];
    bool odd = (buf[95] & 0x80) != 0;
    buf[95] &= 0x7F;
    g2aff_t a;
    if (!fp_from_le48(a.x.a, buf)) return false;
    if (!fp_from_le48(a.x.b, buf + 48)) return false;
    fp2_t y2, b;
    fp2_sqr(y2, a.x); fp2_mul(y2, y2, a.x);
    g2_b(b);
    fp2_add(y2, y2, b);
    if (!fp2_sqrt_any(a.y, y2)) return false;
    if (fp2_is_odd(a.y) != odd) fp2_neg(a.y, a.y);
    g2_from_affine(p, a);
    if (check_subgroup && !g2_in_subgroup_fast(p)) return false;
    return true;
}

/* ================================================================ FT map + cofactor */
/* 1/c1^2 = -1/3 (Montgomery form) */
static const uint64_t FT_NEG_INV3[6] = { 0x6bfcaaaaaaa98e3aULL, 0x10e7fffba46d5554ULL, 0xad4d68c3364ddf23ULL, 0xa43851108110e928ULL, 0xa506d9b4e0519578ULL, 0x0158e66214ffab57ULL };
DEVN bool ft_map_g2(g2aff_t &r, const fp2_t &t) {
    if (fp2_is_zero(t)) return false;
    /* neg = legendre(norm t) < 0.  For t in Fp (what hash_to_g2_point feeds)
     * the norm is a non-zero square: no exponentiation. */
    bool neg = false;
    if (!fp_is_zero(t.b)) {
        fp_t norm, tmp;
        fp_sqr(norm, t.a);
        fp_sqr(tmp, t.b);
        fp_add(norm, norm, tmp);
        neg = fp_legendre(norm) < 0;
    }
    /* Thread-per-item: a wave pays for every lane's path, so the control
     * flow is kept uniform.  One inversion of w0*t serves 1/w0 and 1/t
     * (x3 = 1 + 1/w^2 = 1 + w0^2 (1/t)^2 / c1^2, c1^2 = -3); each candidate
     * gets one norm-sqrt attempt in order x1 -> x2 -> x3; the sqrt tail
     * runs once, on the chosen candidate.  Same field elements as the
     * candidate-by-candidate fp2_sqrt form. */
    fp2_t tt, w0, iv, w, b2, xc[3], x, y2, y;
    fp_t one, wn;
    fp_one(one);
    g2_b(b2);
    fp2_sqr(tt, t);
    fp2_add(w0, tt, b2);
    fp_add(w0.a, w0.a, one);
    if (fp2_is_zero(w0)) return false;
    fp2_mul(iv, w0, t);
    fp2_inv(iv, iv);                              /* 1/(w0 t) */
    fp2_mul(w, iv, tt);                           /* t/w0 */
    { fp_t c1; fp_load(c1, BLS_FT_C1); fp2_mul_fp(w, w, c1); }
    fp2_mul(x, t, w);
    fp2_neg(xc[0], x);
    { fp_t c2; fp_load(c2, BLS_FT_C2); fp_add(xc[0].a, xc[0].a, c2); }
    fp2_neg(xc[1], xc[0]);
    fp_sub(xc[1].a, xc[1].a, one);
    fp2_sqr(x, w0);
    fp2_mul(x, x, iv);                            /* w0/t */
    fp2_sqr(x, x);
    { fp_t c; fp_load(c, FT_NEG_INV3); fp2_mul_fp(xc[2], x, c); }
    fp_add(xc[2].a, xc[2].a, one);
    bool found = false;
    for (int i = 0; i < 3; i++) {
        if (found) continue;
        fp2_t xi = xc[i], g;
        fp_t n, u;
        fp2_sqr(g, xi); fp2_mul(g, g, xi);
        fp2_add(g, g, b2);
        fp_sqr(n, g.a);
        fp_sqr(u, g.b);
        fp_add(n, n, u);
        if (fp_sqrt(u, n)) { found = true; x = xi; y2 = g; wn = u; }
    }
    if (!found) return false;
    /* b == 0 (negligible) keeps fp2_sqrt's own path */
    bool ok = fp_is_zero(y2.b) ? fp2_sqrt(y, y2) : fp2_sqrt_tail(y, y2, wn);
    if (!ok) return false;
    if (neg) fp2_neg(y, y);
    r.x = x; r.y = y;
    return true;
}
DEV void g2_mul_u64(g2_t &r, const g2_t &p, uint64_t k) { g2_mul(r, p, &k, 1); }
DEVN void g2_clear_cofactor(g2_t &r, const g2_t &p, int fast) {
    if (!fast) {
        g2_mul(r, p, BLS_H2, BLS_H2_LIMBS);
        return;
    }
    g2_t t1, t2, t3, t2a, acc, tn;
    g2_mul_u64(t1, p, BLS_U); g2_neg(t1, t1);
    g2_psi(t2, p);
    g2_dbl(t3, p);
    g2_psi(t3, t3); g2_psi(t3, t3);
    g2_neg(tn, t2);
    g2_add(t3, t3, tn);
    g2_add(t2a, t1, t2);
    g2_mul_u64(t2a, t2a, BLS_U); g2_neg(t2a, t2a);
    g2_add(acc, t3, t2a);
    g2_neg(tn, t1);
    g2_add(acc, acc, tn);
    g2_neg(tn, p);
    g2_add(r, acc, tn);
}
DEVN bool hash_to_g2_point(g2_t &r, const uint8_t *msg, int len, int fast_cofactor) {
    uint8_t buf[48];
    for (int i = 0; i < 48; i++) buf[i] = 0;
    int n = len < 48 ? len : 48;
    for (int i = 0; i < n; i++) buf[i] = msg[i];
    buf[47] &= 0x0F;
    uint64_t raw[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        raw[i] = 0;
#pragma unroll
        for (int j = 0; j < 8; j++)
            raw[i] |= (uint64_t)buf[i * 8 + j] << (8 * j);
    }
    fp2_t t;
    { fp_t tr, r2; fp_load(tr, raw); fp_load(r2, BLS_R2P); fp_mul(t.a, tr, r2); }
    fp_zero(t.b);
    g2aff_t m;
    if (!ft_map_g2(m, t)) return false;
    g2_t mp;
    g2_from_affine(mp, m);
    g2_clear_cofactor(r, mp, fast_cofactor);
    return true;
}

/* ================================================================ Fp6/Fp12/pairing */
struct fp6_t { fp2_t c0, c1, c2; };
struct fp12_t { fp6_t c0, c1; };

DEV void fp6_add(fp6_t &r, const fp6_t &x, const fp6_t &y) { fp2_add(r.c0, x.c0, y.c0); fp2_add(r.c1, x.c1, y.c1); fp2_add(r.c2, x.c2, y.c2); }
DEV void fp6_sub(fp6_t &r, const fp6_t &x, const fp6_t &y) { fp2_sub(r.c0, x.c0, y.c0); fp2_sub(r.c1, x.c1, y.c1); fp2_sub(r.c2, x.c2, y.c2); }
DEV void fp6_neg(fp6_t &r, const fp6_t &x) { fp2_neg(r.c0, x.c0); fp2_neg(r.c1, x.c1); fp2_neg(r.c2, x.c2); }
DEVN void fp6_mul(fp6_t &r, const fp6_t &x, const fp6_t &y) {
    fp2_t t0, t1, t2, s0, s1, tt, r0, r1;
    fp2_mul(t0, x.c0, y.c0);
    fp2_mul(t1, x.c1, y.c1);
    fp2_mul(t2, x.c2, y.c2);
    fp2_add(s0, x.c1, x.c2);
    fp2_add(s1, y.c1, y.c2);
    fp2_mul(tt, s0, s1);
    fp2_sub(tt, tt, t1);
    fp2_sub(tt, tt, t2);
    fp2_mul_xi(tt, tt);
    fp2_add(r0, t0, tt);
    fp2_add(s0, x.c0, x.c1);
    fp2_add(s1, y.c0, y.c1);
    fp2_mul(tt, s0, s1);
    fp2_sub(tt, tt, t0);
    fp2_sub(tt, tt, t1);
    fp2_t xt2;
    fp2_mul_xi(xt2, t2);
    fp2_add(r1, tt, xt2);
    fp2_add(s0, x.c0, x.c2);
    fp2_add(s1, y.c0, y.c2);
    fp2_mul(tt, s0, s1);
    fp2_sub(tt, tt, t0);
    fp2_sub(tt, tt, t2);
    fp2_add(r.c2, tt, t1);
    r.c0 = r0; r.c1 = r1;
}
DEV void fp6_mul_v(fp6_t &r, const fp6_t &x) {
    fp2_t t;
    fp2_mul_xi(t, x.c2);
    r.c2 = x.c1; r.c1 = x.c0; r.c0 = t;
}
DEVN void fp6_inv(fp6_t &r, const fp6_t &x) {
    fp2_t c0, c1, c2, t, norm, tmp, tmp2;
    fp2_sqr(c0, x.c0);
    fp2_mul(t, x.c1, x.c2);
    fp2_mul_xi(t, t);
    fp2_sub(c0, c0, t);
    fp2_sqr(c1, x.c2);
    fp2_mul_xi(c1, c1);
    fp2_mul(t, x.c0, x.c1);
    fp2_sub(c1, c1, t);
    fp2_sqr(c2, x.c1);
    fp2_mul(t, x.c0, x.c2);
    fp2_sub(c2, c2, t);
    fp2_mul(norm, x.c0, c0);
    fp2_mul(tmp, x.c2, c1);
    fp2_mul(tmp2, x.c1, c2);
    fp2_add(tmp, tmp, tmp2);
    fp2_mul_xi(tmp, tmp);
    fp2_add(norm, norm, tmp);
    fp2_inv(norm, norm);
    fp2_mul(r.c0, c0, norm);
    fp2_mul(r.c1, c1, norm);
    fp2_mul(r.c2, c2, norm);
}
DEVN void fp12_mul(fp12_t &r, const fp12_t &x, const fp12_t &y) {
    fp6_t t0, t1, s0, s1, tt, vt1;
    fp6_mul(t0, x.c0, y.c0);
    fp6_mul(t1, x.c1, y.c1);
    fp6_add(s0, x.c0, x.c1);
    fp6_add(s1, y.c0, y.c1);
    fp6_mul(tt, s0, s1);
    fp6_sub(tt, tt, t0);
    fp6_sub(tt, tt, t1);
    fp6_mul_v(vt1, t1);
    fp6_add(r.c0, t0, vt1);
    r.c1 = tt;
}
DEVN void fp12_sqr(fp12_t &r, const fp12_t &x) {
    fp6_t ab, apb, avb, t0, vab;
    fp6_mul(ab, x.c0, x.c1);
    fp6_add(apb, x.c0, x.c1);
    fp6_mul_v(avb, x.c1);
    fp6_add(avb, x.c0, avb);
    fp6_mul(t0, apb, avb);
    fp6_sub(t0, t0, ab);
    fp6_mul_v(vab, ab);
    fp6_sub(r.c0, t0, vab);
    fp6_add(r.c1, ab, ab);
}
DEV void fp12_conj(fp12_t &r, const fp12_t &x) { r.c0 = x.c0; fp6_neg(r.c1, x.c1); }
DEVN void fp12_inv(fp12_t &r, const fp12_t &x) {
    fp6_t t, t1;
    fp6_mul(t, x.c0, x.c0);
    fp6_mul(t1, x.c1, x.c1);
    fp6_mul_v(t1, t1);
    fp6_sub(t, t, t1);
    fp6_inv(t, t);
    fp6_mul(r.c0, x.c0, t);
    fp6_mul(t1, x.c1, t);
    fp6_neg(r.c1, t1);
}
DEV void fp12_one(fp12_t &r) {
    fp2_one(r.c0.c0); fp2_zero(r.c0.c1); fp2_zero(r.c0.c2);
    fp2_zero(r.c1.c0); fp2_zero(r.c1.c1); fp2_zero(r.c1.c2);
}
DEV bool fp12_is_one(const fp12_t &x) {
    fp_t one;
    fp_one(one);
    if (!fp_eq(x.c0.c0.a, one)) return false;
    if (!fp_is_zero(x.c0.c0.b)) return false;
    if (!fp2_is_zero(x.c0.c1) || !fp2_is_zero(x.c0.c2)) return false;
    if (!fp2_is_zero(x.c1.c0) || !fp2_is_zero(x.c1.c1) || !fp2_is_zero(x.c1.c2)) return false;
    return true;
}
DEV void frob_coeff1(fp2_t &g, int i) {
    switch (i) {
    case 0: fp_load(g.a, BLS_FROB1_0_A); fp_load(g.b, BLS_FROB1_0_B); break;
    case 1: fp_load(g.a, BLS_FROB1_1_A); fp_load(g.b, BLS_FROB1_1_B); break;
    case 2: fp_load(g.a, BLS_FROB1_2_A); fp_load(g.b, BLS_FROB1_2_B); break;
    case 3: fp_load(g.a, BLS_FROB1_3_A); fp_load(g.b, BLS_FROB1_3_B); break;
    case 4: fp_load(g.a, BLS_FROB1_4_A); fp_load(g.b, BLS_FROB1_4_B); break;
    default: fp_load(g.a, BLS_FROB1_5_A); fp_load(g.b, BLS_FROB1_5_B); break;
    }
}
DEV void frob_coeff2(fp_t &g, int i) {
    switch (i) {
    case 0: fp_load(g, BLS_FROB2_0); break;
    case 1: fp_load(g, BLS_FROB2_1); break;
    case 2: fp_load(g, BLS_FROB2_2); break;
    case 3: fp_load(g, BLS_FROB2_3); break;
    case 4: fp_load(g, BLS_FROB2_4); break;
    default: fp_load(g, BLS_FROB2_5); break;
    }
}
DEVN void fp12_frob(fp12_t &r, const fp12_t &x) {
    const fp2_t *in[6] = { &x.c0.c0, &x.c1.c0, &x.c0.c1, &x.c1.c1, &x.c0.c2, &x.c1.c2 };
    fp12_t tmp;
    fp2_t *out[6] = { &tmp.c0.c0, &tmp.c1.c0, &tmp.c0.c1, &tmp.c1.c1, &tmp.c0.c2, &tmp.c1.c2 };
    for (int i = 0; i < 6; i++) {
        fp2_t g, c;
        frob_coeff1(g, i);
        fp2_conj(c, *in[i]);
        fp2_mul(*out[i], c, g);
    }
    r = tmp;
}
DEVN void fp12_frob2(fp12_t &r, const fp12_t &x) {
    const fp2_t *in[6] = { &x.c0.c0, &x.c1.c0, &x.c0.c1, &x.c1.c1, &x.c0.c2, &x.c1.c2 };
    fp12_t tmp;
    fp2_t *out[6] = { &tmp.c0.c0, &tmp.c1.c0, &tmp.c0.c1, &tmp.c1.c1, &tmp.c0.c2, &tmp.c1.c2 };
    for (int i = 0; i < 6; i++) {
        fp_t g;
        frob_coeff2(g, i);
        fp2_mul_fp(*out[i], *in[i], g);
    }
    r = tmp;
}
DEVN void fp12_mul_line(fp12_t &f, const fp2_t &c0, const fp2_t &c3, const fp2_t &c5) {
    fp6_t t0, t1, l01, tt, vt1, fs, l;
    fp2_mul(t0.c0, f.c0.c0, c0);
    fp2_mul(t0.c1, f.c0.c1, c0);
    fp2_mul(t0.c2, f.c0.c2, c0);
    {
        const fp2_t &a0 = f.c1.c0, &a1 = f.c1.c1, &a2 = f.c1.c2;
        fp2_t p1, p2, q;
        fp2_mul(p1, a1, c5);
        fp2_mul(p2, a2, c3);
        fp2_add(q, p1, p2);
        fp2_mul_xi(t1.c0, q);
        fp2_mul(p1, a0, c3);
        fp2_mul(p2, a2, c5);
        fp2_mul_xi(p2, p2);
        fp2_add(t1.c1, p1, p2);
        fp2_mul(p1, a0, c5);
        fp2_mul(p2, a1, c3);
        fp2_add(t1.c2, p1, p2);
    }
    fp6_add(fs, f.c0, f.c1);
    l.c0 = c0; l.c1 = c3; l.c2 = c5;
    fp6_mul(l01, fs, l);
    fp6_sub(tt, l01, t0);
    fp6_sub(tt, tt, t1);
    fp6_mul_v(vt1, t1);
    fp6_add(f.c0, t0, vt1);
    f.c1 = tt;
}
/* Miller-loop step helpers: line coefficients from the Jacobian formulas
 * (derivation in DESIGN.md §4), point updated in place. */
DEVN void ml_dbl_step(g2_t &T, const g1aff_t &Pa, fp2_t &c0, fp2_t &c3, fp2_t &c5) {
    fp2_t A, B, ZZ, t, t2, newz;
    fp2_sqr(A, T.x);
    fp2_sqr(B, T.y);
    fp2_sqr(ZZ, T.z);
    fp2_mul(t, A, T.x);
    fp2_dbl(t2, t); fp2_add(t, t, t2);
    fp2_dbl(t2, B);
    fp2_sub(c3, t, t2);                  /* 3X^3 - 2Y^2 */
    fp2_dbl(t, A); fp2_add(t, t, A);
    fp2_mul(t, t, ZZ);
    fp2_mul_fp(t, t, Pa.x);
    fp2_neg(c5, t);                      /* -3X^2 Z^2 xP */
    fp2_mul(newz, T.y, T.z);
    fp2_dbl(newz, newz);
    fp2_mul(t, newz, ZZ);
    fp2_mul_fp(t, t, Pa.y);
    fp2_mul_xi(c0, t);                   /* xi yP 2YZ^3 */
    g2_dbl(T, T);
}
DEVN void ml_add_step(g2_t &T, const g2aff_t &Q, const g1aff_t &Pa,
                      fp2_t &c0, fp2_t &c3, fp2_t &c5) {
    fp2_t zz, u2, s2, h, rr, zh, hh, hhh, v, newx, t, t2;
    fp2_sqr(zz, T.z);
    fp2_mul(u2, Q.x, zz);
    fp2_mul(s2, Q.y, zz);
    fp2_mul(s2, s2, T.z);
    fp2_sub(h, u2, T.x);
    fp2_sub(rr, s2, T.y);
    fp2_mul(zh, T.z, h);
    fp2_mul_fp(t, zh, Pa.y);
    fp2_mul_xi(c0, t);                   /* xi yP ZH */
    fp2_mul(t, rr, Q.x);
    fp2_mul(t2, Q.y, zh);
    fp2_sub(c3, t, t2);                  /* r x2 - y2 ZH */
    fp2_mul_fp(t, rr, Pa.x);
    fp2_neg(c5, t);                      /* -r xP */
    fp2_sqr(hh, h);
    fp2_mul(hhh, hh, h);
    fp2_mul(v, T.x, hh);
    fp2_sqr(t, rr);
    fp2_sub(t, t, hhh);
    fp2_sub(t, t, v);
    fp2_sub(newx, t, v);
    fp2_sub(t, v, newx);
    fp2_mul(t, rr, t);
    fp2_mul(t2, T.y, hhh);
    fp2_sub(T.y, t, t2);
    T.x = newx;
    fp2_mul(T.z, T.z, h);
}
/* f_{|z|,Q}(P); f must start at 1 */
DEVN void miller_loop_acc(fp12_t &f, const g2aff_t &Q, const g1aff_t &Pa) {
    g2_t T;
    g2_from_affine(T, Q);
    fp2_t c0, c3, c5;
    for (int bit = 62; bit >= 0; bit--) {
        fp12_sqr(f, f);
        ml_dbl_step(T, Pa, c0, c3, c5);
        fp12_mul_line(f, c0, c3, c5);
        if ((BLS_U >> bit) & 1) {
            ml_add_step(T, Q, Pa, c0, c3, c5);
            fp12_mul_line(f, c0, c3, c5);
        }
    }
}
/* ---- homogeneous-projective Miller steps (executable spec
 * in tests/test_miller_formulas.py).  T = (X, Y, Z) with x = X/Z, y = Y/Z on
 * y^2 = x^3 + b', b' = 4 xi.  The doubling shares every square between the
 * line and the point (3 mul + 6 sqr + 2 mul_fp against the Jacobian step's
 * recomputation through g2_dbl); lines land in the same (c0, c3, c5) slots,
 * scaled by an Fp2 factor that the final exponentiation removes. */
DEVN void ml_dbl_step_h(g2_t &T, const g1aff_t &Pa, fp2_t &c0, fp2_t &c3, fp2_t &c5) {
    fp2_t A, B, C, E, F, G, H, XX, t, t2;
    fp2_mul(A, T.x, T.y);
    fp2_half(A, A);                      /* XY/2 */
    fp2_sqr(B, T.y);
    fp2_sqr(C, T.z);
    fp2_mul_xi(E, C);
    fp2_dbl(E, E); fp2_dbl(E, E);        /* b' Z^2 */
    fp2_dbl(t, E); fp2_add(E, E, t);     /* E = 3b' Z^2 */
    fp2_dbl(t, E); fp2_add(F, E, t);     /* F = 3E */
    fp2_add(G, B, F);
    fp2_half(G, G);
    fp2_add(H, T.y, T.z);
    fp2_sqr(H, H);
    fp2_add(t, B, C);
    fp2_sub(H, H, t);                    /* 2YZ */
    fp2_sqr(XX, T.x);
    fp2_mul_fp(t, H, Pa.y);
    fp2_mul_xi(c0, t);                   /* xi yP 2YZ */
    fp2_sub(c3, B, E);                   /* Y^2 - 3b' Z^2 */
    fp2_dbl(t, XX); fp2_add(t, t, XX);
    fp2_mul_fp(t, t, Pa.x);
    fp2_neg(c5, t);                      /* -3X^2 xP */
    fp2_sub(t, B, F);
    fp2_mul(T.x, A, t);
    fp2_sqr(t, G);
    fp2_sqr(t2, E);
    fp2_dbl(G, t2); fp2_add(t2, t2, G);
    fp2_sub(T.y, t, t2);                 /* G^2 - 3E^2 */
    fp2_mul(T.z, B, H);
}
/* mixed addition T += Q, Q affine; theta = Y - y2 Z, lambda = X - x2 Z */
DEVN void ml_add_step_h(g2_t &T, const g2aff_t &Q, const g1aff_t &Pa,
                        fp2_t &c0, fp2_t &c3, fp2_t &c5) {
    fp2_t th, la, C, D, E, F, G, H, t, t2;
    fp2_mul(t, Q.y, T.z);
    fp2_sub(th, T.y, t);
    fp2_mul(t, Q.x, T.z);
    fp2_sub(la, T.x, t);
    fp2_mul_fp(t, la, Pa.y);
    fp2_mul_xi(c0, t);                   /* xi yP lambda */
    fp2_mul(t, Q.x, th);
    fp2_mul(t2, Q.y, la);
    fp2_sub(c3, t, t2);                  /* x2 theta - y2 lambda */
    fp2_mul_fp(t, th, Pa.x);
    fp2_neg(c5, t);                      /* -theta xP */
    fp2_sqr(C, th);
    fp2_sqr(D, la);
    fp2_mul(E, la, D);
    fp2_mul(F, T.z, C);
    fp2_mul(G, T.x, D);
    fp2_add(H, E, F);
    fp2_dbl(t, G);
    fp2_sub(H, H, t);
    fp2_mul(T.x, la, H);
    fp2_sub(t, G, H);
    fp2_mul(t, th, t);
    fp2_mul(t2, E, T.y);
    fp2_sub(T.y, t, t2);
    fp2_mul(T.z, T.z, E);
}
/* ---- the same steps on arguments that were never made affine (DESIGN.md
 * §4m; executable spec in tests/test_miller_jac_formulas.py).
 * Full addition T += Q2 with Q2 = (X2, Y2, Z2) homogeneous:
 *   theta' = Y Z2 - Y2 Z = Z2 theta,  lambda' = X Z2 - X2 Z = Z2 lambda,
 * the line of ml_add_step_h scaled by Z2^2 and the point by Z2^4 (the same
 * projective point).  Pp = (xP k, yP k) for a k in Fp, and c3 is multiplied
 * by the same k: the whole line is k times ml_add_step_h's. */
DEVN void ml_add_step_hj(g2_t &T, const g2_t &Q2, const g1aff_t &Pp, const fp_t &k,
                         fp2_t &c0, fp2_t &c3, fp2_t &c5) {
    fp2_t th, la, yz, xz, zz, C, D, E, F, G, H, t, t2;
    fp2_mul(yz, T.y, Q2.z);
    fp2_mul(t, Q2.y, T.z);
    fp2_sub(th, yz, t);
    fp2_mul(xz, T.x, Q2.z);
    fp2_mul(t, Q2.x, T.z);
    fp2_sub(la, xz, t);
    fp2_mul(zz, T.z, Q2.z);
    fp2_mul(t, la, Q2.z);
    fp2_mul_fp(t, t, Pp.y);
    fp2_mul_xi(c0, t);                   /* xi yP lambda' Z2 */
    fp2_mul(t, Q2.x, th);
    fp2_mul(t2, Q2.y, la);
    fp2_sub(t, t, t2);
    fp2_mul_fp(c3, t, k);                /* X2 theta' - Y2 lambda' */
    fp2_mul(t, th, Q2.z);
    fp2_mul_fp(t, t, Pp.x);
    fp2_neg(c5, t);                      /* -theta' Z2 xP */
    fp2_sqr(C, th);
    fp2_sqr(D, la);
    fp2_mul(E, la, D);
    fp2_mul(F, zz, C);
    fp2_mul(G, xz, D);
    fp2_add(H, E, F);
    fp2_dbl(t, G);
    fp2_sub(H, H, t);
    fp2_mul(T.x, la, H);
    fp2_sub(t, G, H);
    fp2_mul(t, th, t);
    fp2_mul(t2, E, yz);
    fp2_sub(T.y, t, t2);
    fp2_mul(T.z, zz, E);
}
/* f = f_{|z|,Q}(P) up to subfield factors for Jacobian Q = (X, Y, Z) and
 * P = (x, y, z), both with a nonzero third coordinate: no inversion.
 * G1: xP = x/z^2, yP = y/z^3; every line is multiplied by k = z^3 in Fp, so
 * the steps get (x z, y) where they use (xP, yP) and c3 is multiplied by k.
 * G2: T starts at the homogeneous form (X Z, Y, Z^3) of Q, which the
 * additions use as it is. */
DEVN void miller_loop1_hj(fp12_t &f, const g2_t &Qj, const g1_t &Pj) {
    g1aff_t Pp;
    fp_t k;
    fp_sqr(k, Pj.z);
    fp_mul(k, k, Pj.z);
    fp_mul(Pp.x, Pj.x, Pj.z);
    Pp.y = Pj.y;
    g2_t Q2, T;
    fp2_t c0, c3, c5;
    fp2_sqr(c0, Qj.z);
    fp2_mul(Q2.z, c0, Qj.z);
    fp2_mul(Q2.x, Qj.x, Qj.z);
    Q2.y = Qj.y;
    T = Q2;
    fp12_one(f);
    for (int bit = 62; bit >= 0; bit--) {
        fp12_sqr(f, f);
        ml_dbl_step_h(T, Pp, c0, c3, c5);
        fp2_mul_fp(c3, c3, k);
        fp12_mul_line(f, c0, c3, c5);
        if ((BLS_U >> bit) & 1) {
            ml_add_step_hj(T, Q2, Pp, k, c0, c3, c5);
            fp12_mul_line(f, c0, c3, c5);
        }
    }
}
/* f *= l1 * l2 for two lines a0 + (a3 v + a5 v^2) w, b0 + (b3 v + b5 v^2) w.
 * Their product m = m0 + m1 w has m0 full and m1 = (0, x, y): 6 fp2-mul.
 * Folding m into f takes f0*m0 (6), f1*m1 (5, Karatsuba on the 2-sparse
 * operand) and (f0+f1)(m0+m1) (6): 23 fp2-mul and one pass over f, against
 * 30 and two passes for two fp12_mul_line calls. */
DEVN void fp12_mul_line2(fp12_t &f, const fp2_t &a0, const fp2_t &a3, const fp2_t &a5,
                         const fp2_t &b0, const fp2_t &b3, const fp2_t &b5) {
    fp6_t m0, t0, t1, fs, tt, vt1;
    fp2_t p00, p33, p55, x, y, s, u, q1, q2, q3;
    fp2_mul(p00, a0, b0);
    fp2_mul(p33, a3, b3);
    fp2_mul(p55, a5, b5);
    fp2_add(s, a3, a5);
    fp2_add(u, b3, b5);
    fp2_mul(q1, s, u);
    fp2_sub(q1, q1, p33);
    fp2_sub(q1, q1, p55);
    fp2_mul_xi(m0.c1, q1);               /* xi (a3 b5 + a5 b3) */
    fp2_mul_xi(s, p33);
    fp2_add(m0.c0, p00, s);              /* a0 b0 + xi a3 b3 */
    fp2_mul_xi(m0.c2, p55);              /* xi a5 b5 */
    fp2_add(s, a0, a3);
    fp2_add(u, b0, b3);
    fp2_mul(x, s, u);
    fp2_sub(x, x, p00);
    fp2_sub(x, x, p33);                  /* a0 b3 + a3 b0 */
    fp2_add(s, a0, a5);
    fp2_add(u, b0, b5);
    fp2_mul(y, s, u);
    fp2_sub(y, y, p00);
    fp2_sub(y, y, p55);                  /* a0 b5 + a5 b0 */
    fp6_mul(t0, f.c0, m0);
    {
        const fp2_t &g0 = f.c1.c0, &g1 = f.c1.c1, &g2 = f.c1.c2;
        fp2_mul(q1, g1, x);
        fp2_mul(q2, g2, y);
        fp2_add(s, g1, g2);
        fp2_add(u, x, y);
        fp2_mul(q3, s, u);
        fp2_sub(q3, q3, q1);
        fp2_sub(q3, q3, q2);             /* g1 y + g2 x */
        fp2_mul_xi(t1.c0, q3);
        fp2_mul(s, g0, x);
        fp2_mul_xi(u, q2);
        fp2_add(t1.c1, s, u);
        fp2_mul(s, g0, y);
        fp2_add(t1.c2, s, q1);
    }
    fp6_add(fs, f.c0, f.c1);
    fp2_add(m0.c1, m0.c1, x);            /* m0 + m1 */
    fp2_add(m0.c2, m0.c2, y);
    fp6_mul(tt, fs, m0);
    fp6_sub(tt, tt, t0);
    fp6_sub(tt, tt, t1);
    fp6_mul_v(vt1, t1);
    fp6_add(f.c0, t0, vt1);
    f.c1 = tt;
}
/* fused two-pairing Miller loop: f = f_{|z|,Q1}(P1) * f_{|z|,Q2}(P2), one
 * shared squaring chain (the standard multi-pairing product trick), the
 * two legs' lines folded into f together */
DEVN void miller_loop2(fp12_t &f, const g2aff_t &Q1, const g1aff_t &P1,
                       const g2aff_t &Q2, const g1aff_t &P2) {
    g2_t T1, T2;
    g2_from_affine(T1, Q1);
    g2_from_affine(T2, Q2);
    fp2_t a0, a3, a5, b0, b3, b5;
    fp12_one(f);
    for (int bit = 62; bit >= 0; bit--) {
        fp12_sqr(f, f);
        ml_dbl_step_h(T1, P1, a0, a3, a5);
        ml_dbl_step_h(T2, P2, b0, b3, b5);
        fp12_mul_line2(f, a0, a3, a5, b0, b3, b5);
        if ((BLS_U >> bit) & 1) {
            ml_add_step_h(T1, Q1, P1, a0, a3, a5);
            ml_add_step_h(T2, Q2, P2, b0, b3, b5);
            fp12_mul_line2(f, a0, a3, a5, b0, b3, b5);
        }
    }
}
DEV void fp4_sqr_gs(fp2_t &c, fp2_t &d, const fp2_t &a, const fp2_t &b) {
    fp2_t a2, b2, t;
    fp2_sqr(a2, a);
    fp2_sqr(b2, b);
    fp2_mul_xi(t, b2);
    fp2_add(c, a2, t);
    fp2_add(t, a, b);
    fp2_sqr(t, t);
    fp2_sub(t, t, a2);
    fp2_sub(d, t, b2);
}
DEVN void fp12_cyc_sqr(fp12_t &r, const fp12_t &x) {
    const fp2_t &a0 = x.c0.c0, &a1 = x.c1.c0, &a2 = x.c0.c1,
                &a3 = x.c1.c1, &a4 = x.c0.c2, &a5 = x.c1.c2;
    fp2_t t00, t03, t01, t04, t02, t05, tmp, x05;
    fp4_sqr_gs(t00, t03, a0, a3);
    fp4_sqr_gs(t01, t04, a1, a4);
    fp4_sqr_gs(t02, t05, a2, a5);
    fp12_t out;
    fp2_sub(tmp, t00, a0); fp2_dbl(tmp, tmp); fp2_add(out.c0.c0, tmp, t00);
    fp2_sub(tmp, t01, a2); fp2_dbl(tmp, tmp); fp2_add(out.c0.c1, tmp, t01);
    fp2_sub(tmp, t02, a4); fp2_dbl(tmp, tmp); fp2_add(out.c0.c2, tmp, t02);
    fp2_mul_xi(x05, t05);
    fp2_add(tmp, x05, a1); fp2_dbl(tmp, tmp); fp2_add(out.c1.c0, tmp, x05);
    fp2_add(tmp, t03, a3); fp2_dbl(tmp, tmp); fp2_add(out.c1.c1, tmp, t03);
    fp2_add(tmp, t04, a5); fp2_dbl(tmp, tmp); fp2_add(out.c1.c2, tmp, t04);
    r = out;
}
DEVN void fp12_pow_u(fp12_t &r, const fp12_t &x) {
    fp12_t acc = x;
    for (int bit = 62; bit >= 0; bit--) {
        fp12_cyc_sqr(acc, acc);
        if ((BLS_U >> bit) & 1) fp12_mul(acc, acc, x);
    }
    r = acc;
}
DEVN void final_exp(fp12_t &r, const fp12_t &f_in) {
    fp12_t f, t, inv;
    fp12_conj(t, f_in);
    fp12_inv(inv, f_in);
    fp12_mul(f, t, inv);
    fp12_frob2(t, f);
    fp12_mul(f, t, f);
    fp12_t a, b, c, d, u1, u2;
    fp12_pow_u(u1, f);
    fp12_mul(a, u1, f);
    fp12_conj(a, a);
    fp12_pow_u(u1, a);
    fp12_mul(b, u1, a);
    fp12_conj(b, b);
    fp12_pow_u(u1, b);
    fp12_conj(u1, u1);
    fp12_frob(u2, b);
    fp12_mul(c, u1, u2);
    fp12_pow_u(u1, c);
    fp12_pow_u(u1, u1);
    fp12_frob2(u2, c);
    fp12_mul(d, u1, u2);
    fp12_conj(u1, c);
    fp12_mul(d, d, u1);
    fp12_cyc_sqr(t, f);                  /* f is cyclotomic after the easy part */
    fp12_mul(t, t, f);
    fp12_mul(r, d, t);
}
/* verify core: pub (G1 jac), sig (G2 affine, pre-checked), hm (G2 jac) */
/* ---- fp6-granularity called layer (traffic experiment, HBLS_VERIFY_RF=5):
 * the verify kernel's scratch traffic is ~proportional to the number of
 * by-ref field-op calls (each fp2-level call round-trips ~290 B of
 * operands).  Coarsening the called unit to fp6 (864 B per fp6-mul vs
 * ~1.7 KB for its six fp2 calls) with ALL internal multiplies through the
 * zero-traffic register-ABI CIOS should cut the fp6-shaped ~60% of the
 * traffic nearly in half — IF the traffic model is right. */
DEV void fp2_mul_ri(fp2_t &r, const fp2_t &x, const fp2_t &y) {
    fp_t ac, bd, ab, cd, t;
    RFM(ac, x.a, y.a);
    RFM(bd, x.b, y.b);
    fp_add(ab, x.a, x.b);
    fp_add(cd, y.a, y.b);
    RFM(t, ab, cd);
    fp_sub(t, t, ac);
    fp_sub(t, t, bd);
    fp_sub(r.a, ac, bd);
    r.b = t;
}
DEVN void fp6_mul_rs6(fp6_t &r, const fp6_t &x, const fp6_t &y) {
    fp2_t t0, t1, t2, s0, s1, tt, r0, r1;
    fp2_mul_ri(t0, x.c0, y.c0);
    fp2_mul_ri(t1, x.c1, y.c1);
    fp2_mul_ri(t2, x.c2, y.c2);
    fp2_add(s0, x.c1, x.c2);
    fp2_add(s1, y.c1, y.c2);
    fp2_mul_ri(tt, s0, s1);
    fp2_sub(tt, tt, t1);
    fp2_sub(tt, tt, t2);
    fp2_mul_xi(tt, tt);
    fp2_add(r0, t0, tt);
    fp2_add(s0, x.c0, x.c1);
    fp2_add(s1, y.c0, y.c1);
    fp2_mul_ri(tt, s0, s1);
    fp2_sub(tt, tt, t0);
    fp2_sub(tt, tt, t1);
    fp2_t xt2;
    fp2_mul_xi(xt2, t2);
    fp2_add(r1, tt, xt2);
    fp2_add(s0, x.c0, x.c2);
    fp2_add(s1, y.c0, y.c2);
    fp2_mul_ri(tt, s0, s1);
    fp2_sub(tt, tt, t0);
    fp2_sub(tt, tt, t2);
    fp2_add(r.c2, tt, t1);
    r.c0 = r0; r.c1 = r1;
}
DEVN void fp12_mul_6(fp12_t &r, const fp12_t &x, const fp12_t &y) {
    fp6_t t0, t1, s0, s1, tt, vt1;
    fp6_mul_rs6(t0, x.c0, y.c0);
    fp6_mul_rs6(t1, x.c1, y.c1);
    fp6_add(s0, x.c0, x.c1);
    fp6_add(s1, y.c0, y.c1);
    fp6_mul_rs6(tt, s0, s1);
    fp6_sub(tt, tt, t0);
    fp6_sub(tt, tt, t1);
    fp6_mul_v(vt1, t1);
    fp6_add(r.c0, t0, vt1);
    r.c1 = tt;
}
DEVN void fp12_sqr_6(fp12_t &r, const fp12_t &x) {
    fp6_t ab, apb, avb, t0, vab;
    fp6_mul_rs6(ab, x.c0, x.c1);
    fp6_add(apb, x.c0, x.c1);
    fp6_mul_v(avb, x.c1);
    fp6_add(avb, x.c0, avb);
    fp6_mul_rs6(t0, apb, avb);
    fp6_sub(t0, t0, ab);
    fp6_mul_v(vab, ab);
    fp6_sub(r.c0, t0, vab);
    fp6_add(r.c1, ab, ab);
}
DEVN void fp12_mul_line_6(fp12_t &f, const fp2_t &c0, const fp2_t &c3, const fp2_t &c5) {
    fp6_t t0, t1, l01, tt, vt1, fs, l;
    fp2_mul(t0.c0, f.c0.c0, c0);
    fp2_mul(t0.c1, f.c0.c1, c0);
    fp2_mul(t0.c2, f.c0.c2, c0);
    {
        const fp2_t &a0 = f.c1.c0, &a1 = f.c1.c1, &a2 = f.c1.c2;
        fp2_t p1, p2, q;
        fp2_mul(p1, a1, c5);
        fp2_mul(p2, a2, c3);
        fp2_add(q, p1, p2);
        fp2_mul_xi(t1.c0, q);
        fp2_mul(p1, a0, c3);
        fp2_mul(p2, a2, c5);
        fp2_mul_xi(p2, p2);
        fp2_add(t1.c1, p1, p2);
        fp2_mul(p1, a0, c5);
        fp2_mul(p2, a1, c3);
        fp2_add(t1.c2, p1, p2);
    }
    fp6_add(fs, f.c0, f.c1);
    l.c0 = c0; l.c1 = c3; l.c2 = c5;
    fp6_mul_rs6(l01, fs, l);
    fp6_sub(tt, l01, t0);
    fp6_sub(tt, tt, t1);
    fp6_mul_v(vt1, t1);
    fp6_add(f.c0, t0, vt1);
    f.c1 = tt;
}
DEVN void miller_loop2_6(fp12_t &f, const g2aff_t &Q1, const g1aff_t &P1,
                         const g2aff_t &Q2, const g1aff_t &P2) {
    g2_t T1, T2;
    g2_from_affine(T1, Q1);
    g2_from_affine(T2, Q2);
    fp2_t c0, c3, c5;
    fp12_one(f);
    for (int bit = 62; bit >= 0; bit--) {
        fp12_sqr_6(f, f);
        ml_dbl_step(T1, P1, c0, c3, c5);
        fp12_mul_line_6(f, c0, c3, c5);
        ml_dbl_step(T2, P2, c0, c3, c5);
        fp12_mul_line_6(f, c0, c3, c5);
        if ((BLS_U >> bit) & 1) {
            ml_add_step(T1, Q1, P1, c0, c3, c5);
            fp12_mul_line_6(f, c0, c3, c5);
            ml_add_step(T2, Q2, P2, c0, c3, c5);
            fp12_mul_line_6(f, c0, c3, c5);
        }
    }
}
DEVN void fp12_pow_u_6(fp12_t &r, const fp12_t &x) {
    fp12_t acc = x;
    for (int bit = 62; bit >= 0; bit--) {
        fp12_cyc_sqr(acc, acc);
        if ((BLS_U >> bit) & 1) fp12_mul_6(acc, acc, x);
    }
    r = acc;
}
DEVN void final_exp_6(fp12_t &r, const fp12_t &f_in) {
    fp12_t f, t, inv;
    fp12_conj(t, f_in);
    fp12_inv(inv, f_in);
    fp12_mul_6(f, t, inv);
    fp12_frob2(t, f);
    fp12_mul_6(f, t, f);
    fp12_t a, b, c, d, u1, u2;
    fp12_pow_u_6(u1, f);
    fp12_mul_6(a, u1, f);
    fp12_conj(a, a);
    fp12_pow_u_6(u1, a);
    fp12_mul_6(b, u1, a);
    fp12_conj(b, b);
    fp12_pow_u_6(u1, b);
    fp12_conj(u1, u1);
    fp12_frob(u2, b);
    fp12_mul_6(c, u1, u2);
    fp12_pow_u_6(u1, c);
    fp12_pow_u_6(u1, u1);
    fp12_frob2(u2, c);
    fp12_mul_6(d, u1, u2);
    fp12_conj(u1, c);
    fp12_mul_6(d, d, u1);
    fp12_sqr_6(t, f);
    fp12_mul_6(t, t, f);
    fp12_mul_6(r, d, t);
}
DEVN int verify_pairing_6(const g1_t &pub, const g2_t &hm, const g2aff_t &sig_aff,
                          bool sig_inf) {
    bool pub_inf = g1_is_inf(pub);
    if (pub_inf && sig_inf) return 1;
    if (pub_inf || sig_inf) return 0;
    g1aff_t pa, ba;
    g2aff_t ha;
    g1_to_affine(pa, pub);
    { g1_t base, nb;
      fp_load(base.x, BLS_G1_X); fp_load(base.y, BLS_G1_Y); fp_one(base.z);
      g1_neg(nb, base);
      ba.x = nb.x; ba.y = nb.y; }
    g2_t hmc = hm;
    g2_to_affine(ha, hmc);
    fp12_t f;
    miller_loop2_6(f, ha, pa, sig_aff, ba);
    fp12_conj(f, f);
    final_exp_6(f, f);
    return fp12_is_one(f) ? 1 : 0;
}
__global__ void k_verify_6(const g1_t *aggpubs, const g2_t *hms, const g2aff_t *sigs,
                           const int32_t *sig_flags, const int32_t *hm_ok,
                           int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (!hm_ok[i] || sig_flags[i] == 0) { results[i] = HBLS_ERR_BADINPUT; return; }
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing_6(aggpubs[i], hms[i], sig_inf ? dummy : sigs[i], sig_inf);
}

/* affine-input pairing: identical math to verify_pairing below, with the
 * per-item fp_inv/fp2_inv conversions hoisted into the batched Montgomery-
 * inversion kernels (k_g1_batch_affine / k_g2_batch_affine) — ~1.1k of the
 * 21.9k fp-muls per item amortize to ~60 (exact, oracle-checked). */
DEVN int verify_pairing_aff(const g1aff_t &pa, bool pub_inf, const g2aff_t &ha,
                            const g2aff_t &sig_aff, bool sig_inf) {
    if (pub_inf && sig_inf) return 1;   /* herumi edge: both identity accepts */
    if (pub_inf || sig_inf) return 0;
    g1aff_t ba;
    { g1_t base, nb;
      fp_load(base.x, BLS_G1_X); fp_load(base.y, BLS_G1_Y); fp_one(base.z);
      g1_neg(nb, base);
      ba.x = nb.x; ba.y = nb.y; }
    fp12_t f;
    miller_loop2(f, ha, pa, sig_aff, ba);
    fp12_conj(f, f);
    final_exp(f, f);
    return fp12_is_one(f) ? 1 : 0;
}

/* batched Jacobian->affine via Montgomery inversion: each thread chains
 * K=16 items' z (or z-norm) products, pays ONE fp_inv, and walks back.
 * Infinity items are flagged and skipped with z=1 placeholders. */
#define BA_K 16
__global__ void k_g1_batch_affine(const g1_t *in, g1aff_t *out, int32_t *infflag,
                                  int batch) {
    int base = (blockIdx.x * blockDim.x + threadIdx.x) * BA_K;
    if (base >= batch) return;
    int m = batch - base < BA_K ? batch - base : BA_K;
    fp_t zs[BA_K], prod[BA_K], acc;
    fp_one(acc);
    for (int i = 0; i < m; i++) {
        fp_t z = in[base + i].z;
        bool inf = fp_is_zero(z);
        infflag[base + i] = inf ? 1 : 0;
        if (inf) fp_one(z);
        zs[i] = z;
        fp_mul(acc, acc, z);
        prod[i] = acc;
    }
    fp_t inv;
    fp_inv(inv, acc);
    for (int i = m - 1; i >= 0; i--) {
        fp_t zinv;
        if (i > 0) fp_mul(zinv, inv, prod[i - 1]);
        else zinv = inv;
        fp_mul(inv, inv, zs[i]);
        fp_t zi2, zi3;
        fp_sqr_inl(zi2, zinv);
        fp_mul(zi3, zi2, zinv);
        fp_mul(out[base + i].x, in[base + i].x, zi2);
        fp_mul(out[base + i].y, in[base + i].y, zi3);
    }
}
__global__ void k_g2_batch_affine(const g2_t *in, g2aff_t *out, const int32_t *ok_in,
                                  int batch) {
    int base = (blockIdx.x * blockDim.x + threadIdx.x) * BA_K;
    if (base >= batch) return;
    int m = batch - base < BA_K ? batch - base : BA_K;
    /* fp2_inv(z) = conj(z) / (za^2 + zb^2): batch-invert the Fp norms */
    fp_t ns[BA_K], prod[BA_K], acc;
    fp_one(acc);
    for (int i = 0; i < m; i++) {
        fp2_t z = in[base + i].z;
        fp_t n, t;
        fp_sqr_inl(n, z.a);
        fp_sqr_inl(t, z.b);
        fp_add(n, n, t);
        /* invalid/infinity items (ok_in==0 or z==0) use norm=1 placeholders;
         * their outputs are never read (verify gates on the flags) */
        if (fp_is_zero(n)) fp_one(n);
        ns[i] = n;
        fp_mul(acc, acc, n);
        prod[i] = acc;
    }
    fp_t inv;
    fp_inv(inv, acc);
    for (int i = m - 1; i >= 0; i--) {
        fp_t ninv;
        if (i > 0) fp_mul(ninv, inv, prod[i - 1]);
        else ninv = inv;
        fp_mul(inv, inv, ns[i]);
        fp2_t z = in[base + i].z, zi, zi2, zi3;
        fp_mul(zi.a, z.a, ninv);
        fp_t t;
        fp_mul(t, z.b, ninv);
        fp_neg(zi.b, t);
        fp2_sqr(zi2, zi);
        fp2_mul(zi3, zi2, zi);
        fp2_mul(out[base + i].x, in[base + i].x, zi2);
        fp2_mul(out[base + i].y, in[base + i].y, zi3);
    }
    (void)ok_in;
}
__global__ void k_verify_aff(const g1aff_t *pubs, const int32_t *pub_inf,
                             const g2aff_t *hms_aff, const g2aff_t *sigs,
                             const int32_t *sig_flags, const int32_t *hm_ok,
                             int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (!hm_ok[i] || sig_flags[i] == 0) { results[i] = HBLS_ERR_BADINPUT; return; }
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing_aff(pubs[i], pub_inf[i] != 0, hms_aff[i],
                                    sig_inf ? dummy : sigs[i], sig_inf);
}

DEVN int verify_pairing(const g1_t &pub, const g2_t &hm, const g2aff_t &sig_aff, bool sig_inf) {
    bool pub_inf = g1_is_inf(pub);
    if (pub_inf && sig_inf) return 1;   /* herumi edge: both identity accepts */
    if (pub_inf || sig_inf) return 0;
    g1aff_t pa, ba;
    g2aff_t ha;
    g1_to_affine(pa, pub);
    { g1_t base, nb;
      fp_load(base.x, BLS_G1_X); fp_load(base.y, BLS_G1_Y); fp_one(base.z);
      g1_neg(nb, base);
      ba.x = nb.x; ba.y = nb.y; }
    g2_t hmc = hm;
    g2_to_affine(ha, hmc);
    fp12_t f;
    miller_loop2(f, ha, pa, sig_aff, ba);
    fp12_conj(f, f);
    final_exp(f, f);
    return fp12_is_one(f) ? 1 : 0;
}

/* split-leg pairing: two single-leg Miller loops (f = f1 * f2) instead of
 * the fused shared-squaring loop.  +63 fp12_sqr of work (~10%) but the live
 * state drops by T2/Q2/P2 (~680 B/thread of hot scratch) — an A/B against
 * the scratch-bandwidth bound (HBLS_VERIFY_RF=4). */
DEVN int verify_pairing_2p(const g1_t &pub, const g2_t &hm, const g2aff_t &sig_aff,
                           bool sig_inf) {
    bool pub_inf = g1_is_inf(pub);
    if (pub_inf && sig_inf) return 1;
    if (pub_inf || sig_inf) return 0;
    g1aff_t pa, ba;
    g2aff_t ha;
    g1_to_affine(pa, pub);
    { g1_t base, nb;
      fp_load(base.x, BLS_G1_X); fp_load(base.y, BLS_G1_Y); fp_one(base.z);
      g1_neg(nb, base);
      ba.x = nb.x; ba.y = nb.y; }
    g2_t hmc = hm;
    g2_to_affine(ha, hmc);
    fp12_t f1, f2;
    fp12_one(f1);
    miller_loop_acc(f1, ha, pa);
    fp12_one(f2);
    miller_loop_acc(f2, sig_aff, ba);
    fp12_mul(f1, f1, f2);
    fp12_conj(f1, f1);
    final_exp(f1, f1);
    return fp12_is_one(f1) ? 1 : 0;
}
__global__ void k_verify_2p(const g1_t *aggpubs, const g2_t *hms, const g2aff_t *sigs,
                            const int32_t *sig_flags, const int32_t *hm_ok,
                            int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (!hm_ok[i] || sig_flags[i] == 0) { results[i] = HBLS_ERR_BADINPUT; return; }
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing_2p(aggpubs[i], hms[i], sig_inf ? dummy : sigs[i], sig_inf);
}

#ifdef HBLS_RF
#include "hbls_rf.inc"
#endif

/* ================================================================ Keccak-256 */
__constant__ uint64_t D_KECCAK_RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
    0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
    0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
    0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL };
DEV uint64_t rol64(uint64_t v, int s) { return s ? (v << s) | (v >> (64 - s)) : v; }
DEVN void keccak_f(uint64_t st[25]) {
    const int rot[25] = { 0,1,62,28,27, 36,44,6,55,20, 3,10,43,25,39, 41,45,15,21,8, 18,2,61,56,14 };
    const int pi[25] = { 0,6,12,18,24, 3,9,10,16,22, 1,7,13,19,20, 4,5,11,17,23, 2,8,14,15,21 };
    for (int rnd = 0; rnd < 24; rnd++) {
        uint64_t C[5], Dd[5], B[25];
#pragma unroll
        for (int x = 0; x < 5; x++)
            C[x] = st[x] ^ st[x + 5] ^ st[x + 10] ^ st[x + 15] ^ st[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++)
            Dd[x] = C[(x + 4) % 5] ^ rol64(C[(x + 1) % 5], 1);
#pragma unroll
        for (int i = 0; i < 25; i++) st[i] ^= Dd[i % 5];
#pragma unroll
        for (int i = 0; i < 25; i++) B[i] = rol64(st[pi[i]], rot[pi[i]]);
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++)
                st[y * 5 + x] = B[y * 5 + x] ^ ((~B[y * 5 + (x + 1) % 5]) & B[y * 5 + (x + 2) % 5]);
        st[0] ^= D_KECCAK_RC[rnd];
    }
}
DEVN void keccak256_dev(const uint8_t *in, int len, uint8_t out[32]) {
    uint64_t st[25];
#pragma unroll
    for (int i = 0; i < 25; i++) st[i] = 0;
    const int rate = 136;
    while (len >= rate) {
        for (int i = 0; i < rate / 8; i++) {
            uint64_t v = 0;
            for (int j = 0; j < 8; j++) v |= (uint64_t)in[8 * i + j] << (8 * j);
            st[i] ^= v;
        }
        keccak_f(st);
        in += rate; len -= rate;
    }
    uint8_t blk[136];
    for (int i = 0; i < rate; i++) blk[i] = 0;
    for (int i = 0; i < len; i++) blk[i] = in[i];
    blk[len] = 0x01;
    blk[rate - 1] |= 0x80;
    for (int i = 0; i < rate / 8; i++) {
        uint64_t v = 0;
        for (int j = 0; j < 8; j++) v |= (uint64_t)blk[8 * i + j] << (8 * j);
        st[i] ^= v;
    }
    keccak_f(st);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 8; j++)
            out[8 * i + j] = (uint8_t)(st[i] >> (8 * j));
}

/* ================================================================ kernels */
/* fr scalar check: value < r, return limbs */
DEV bool fr_from_le32(uint64_t k[4], const uint8_t in[32]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        k[i] = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) k[i] |= (uint64_t)in[i * 8 + j] << (8 * j);
    }
    for (int i = 3; i >= 0; i--) {
        if (k[i] > BLS_R[i]) return false;
        if (k[i] < BLS_R[i]) return true;
    }
    return false;
}

__global__ void k_pk_from_sk(const uint8_t *sks, uint8_t *pks, int32_t *ok, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    uint64_t k[4];
    if (!fr_from_le32(k, sks + 32 * i)) { ok[i] = 0; return; }
    g1_t base, pk;
    fp_load(base.x, BLS_G1_X); fp_load(base.y, BLS_G1_Y); fp_one(base.z);
    g1_mul(pk, base, k, 4);
    g1_serialize(pks + 48 * i, pk);
    ok[i] = 1;
}

__global__ void k_g1_table_build(const uint8_t *pks48, g1aff_t *table, int32_t *ok, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g1_t p;
    if (!g1_deserialize(p, pks48 + 48 * i, true) || g1_is_inf(p)) { ok[i] = 0; return; }
    g1aff_t a;
    a.x = p.x; a.y = p.y;  /* z==1 after deserialize */
    table[i] = a;
    ok[i] = 1;
}

/* masked aggregate: one block (256 threads) per batch item.
 * Each thread sums its strided subset with mixed adds; LDS tree of Jacobian
 * adds reduces to one point (group law is associative => bit-exact). */
#define MASK_BLOCK 64
#define MASK_SUBS 4            /* items per block */
#define MASK_LANES 16          /* lanes per item (small-committee instance) */
#define MASK_IDX_CAP 1024      /* segment length = compacted capacity, bits */
/* Masked committee sum, MASK_SUBS items per block, LANES lanes per item
 * (16 for small committees; 64 — a full wave per item — when n >= 16384,
 * where 16 lanes x batch leaves most of the chip idle).
 * 1) popcount the bitmap; if participation > 1/2 and the committee full-sum
 *    is available, work on the COMPLEMENT side (full - sum(unset)): the
 *    FBFT norm is ~90% participation, so the minority side is ~10% of keys.
 * 2) walk the bitmap in 1024-bit segments, compacting each segment's
 *    minority-side indices into LDS word-by-word (one atomic per nonzero
 *    word), so the point additions run with every lane active — the
 *    strided bit-test form at 10-33% minority density leaves most of each
 *    wave idle (measured 45x off the chip's fp_mul rate at 10%).
 * EC addition is associative: any order/tree is bit-exact after
 * normalization (parity tests vs the oracle's sequential loop). */
template <int LANES>
__global__ void __launch_bounds__(LANES * MASK_SUBS)
k_mask_aggregate(const g1aff_t *table, int n, const uint8_t *bitmaps,
                 int bm_stride, const g1_t *full_sum, g1_t *out, int batch) {
    __shared__ g1_t red[MASK_SUBS][LANES];
    __shared__ uint32_t idx[MASK_SUBS][MASK_IDX_CAP];
    __shared__ int cnt[MASK_SUBS];
    const int sub = threadIdx.x / LANES;
    const int lane = threadIdx.x % LANES;
    const int item = blockIdx.x * MASK_SUBS + sub;
    const bool active = item < batch;
    const uint8_t *bm = active ? bitmaps + (size_t)item * bm_stride : nullptr;

    if (lane == 0) cnt[sub] = 0;
    __syncthreads();
    if (active) {
        int c = 0;
        for (int i = lane; i < bm_stride; i += LANES) c += __popc(bm[i]);
        if (c) atomicAdd(&cnt[sub], c);
    }
    __syncthreads();
    const int set_count = cnt[sub];
    const bool complement = active && full_sum != nullptr && set_count > n / 2;
    g1_t acc;
    g1_set_inf(acc);
    for (int base = 0; base < n; base += MASK_IDX_CAP) {
        __syncthreads();
        if (lane == 0) cnt[sub] = 0;
        __syncthreads();
        if (active) {
            const int end = base + MASK_IDX_CAP < n ? base + MASK_IDX_CAP : n;
            for (int w = base / 32 + lane; w * 32 < end; w += LANES) {
                uint32_t word = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int byte = w * 4 + k;
                    if (byte < bm_stride) word |= (uint32_t)bm[byte] << (8 * k);
                }
                if (complement) word = ~word;
                const int lo = w * 32;
                /* clip past n: bitmap padding must not enter the complement */
                if (n - lo < 32) word &= (1u << (n - lo)) - 1;
                int c = __popc(word);
                if (c) {
                    int pos = atomicAdd(&cnt[sub], c);
                    while (word) {
                        int b = __ffs(word) - 1;
                        word &= word - 1;
                        idx[sub][pos++] = (uint32_t)(lo + b);
                    }
                }
            }
        }
        __syncthreads();
        if (active) {
            const int m = cnt[sub];
            for (int k = lane; k < m; k += LANES)
                g1_madd_i(acc, acc, table[idx[sub][k]]);
        }
    }
    __syncthreads();
    red[sub][lane] = acc;
    __syncthreads();
    for (int s = LANES / 2; s > 0; s >>= 1) {
        if (lane < s) {
            g1_t t;
            g1_add(t, red[sub][lane], red[sub][lane + s]);
            red[sub][lane] = t;
        }
        __syncthreads();
    }
    if (active && lane == 0) {
        if (complement) {
            g1_t nsum, res;
            g1_neg(nsum, red[sub][0]);
            g1_add(res, *full_sum, nsum);
            out[item] = res;
        } else {
            out[item] = red[sub][0];
        }
    }
}
/* ---- 8-bit windowed mask path (large committees) ----
 * wtab[g*255 + b-1] = sum of table[8g+j] for bits j of b (affine); winf
 * flags the (adversarially possible) infinity sums an affine entry cannot
 * represent.  One point-add per nonzero bitmap byte: ~2.7x fewer adds than
 * per-key accumulation at the FBFT's 1/10-1/3 minority densities. */
__global__ void k_wtab_build_jac(const g1aff_t *table, int n, g1_t *wj,
                                 int groups) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    for (int b = 1; b < 256; b++) {
        int j = __ffs(b) - 1, rest = b & (b - 1);
        g1_t base, o;
        if (rest) base = wj[(size_t)g * 255 + rest - 1];
        else g1_set_inf(base);
        if (8 * g + j < n) g1_madd(o, base, table[8 * g + j]);
        else o = base;
        wj[(size_t)g * 255 + b - 1] = o;
    }
}
__global__ void k_wtab_to_affine(const g1_t *wj, g1aff_t *wtab, uint8_t *winf,
                                 size_t m) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    g1_t p = wj[e];
    if (g1_is_inf(p)) { winf[e] = 1; return; }
    winf[e] = 0;
    g1aff_t a;
    g1_to_affine(a, p);
    wtab[e] = a;
}
/* windowed masked sum: one g1_madd per nonzero minority byte.  At ~1/3
 * minority density ~96% of bytes are nonzero, so no compaction is needed —
 * lanes stride bytes directly with negligible divergence. */
template <int LANES>
__global__ void __launch_bounds__(LANES * MASK_SUBS)
k_mask_aggregate_w(const g1aff_t *wtab, const uint8_t *winf, int n,
                   const uint8_t *bitmaps, int bm_stride,
                   const g1_t *full_sum, g1_t *out, int batch) {
    __shared__ g1_t red[MASK_SUBS][LANES];
    __shared__ int cnt[MASK_SUBS];
    const int sub = threadIdx.x / LANES;
    const int lane = threadIdx.x % LANES;
    const int item = blockIdx.x * MASK_SUBS + sub;
    const bool active = item < batch;
    const uint8_t *bm = active ? bitmaps + (size_t)item * bm_stride : nullptr;

    if (lane == 0) cnt[sub] = 0;
    __syncthreads();
    if (active) {
        int c = 0;
        for (int i = lane; i < bm_stride; i += LANES) c += __popc(bm[i]);
        if (c) atomicAdd(&cnt[sub], c);
    }
    __syncthreads();
    const int set_count = cnt[sub];
    const bool complement = active && full_sum != nullptr && set_count > n / 2;
    g1_t acc;
    g1_set_inf(acc);
    if (active) {
        for (int i = lane; i < bm_stride; i += LANES) {
            uint32_t v = bm[i];
            if (complement) v = ~v & 0xffu;
            const int tail = n - 8 * i;
            if (tail < 8) v &= (1u << tail) - 1;
            if (v) {
                size_t e = (size_t)i * 255 + v - 1;
                if (!winf[e]) g1_madd_i(acc, acc, wtab[e]);
            }
        }
    }
    red[sub][lane] = acc;
    __syncthreads();
    for (int ss = LANES / 2; ss > 0; ss >>= 1) {
        if (lane < ss) {
            g1_t t;
            g1_add(t, red[sub][lane], red[sub][lane + ss]);
            red[sub][lane] = t;
        }
        __syncthreads();
    }
    if (active && lane == 0) {
        if (complement) {
            g1_t nsum, res;
            g1_neg(nsum, red[sub][0]);
            g1_add(res, *full_sum, nsum);
            out[item] = res;
        } else {
            out[item] = red[sub][0];
        }
    }
}

/* LANES dispatch: a full wave per item once the per-item scan is long
 * enough to keep it busy (n >= 16384 also covers config4's 65536). */
static inline void launch_mask_aggregate(const g1aff_t *table, int n,
        const uint8_t *bm, int bm_stride, const g1_t *full_sum,
        g1_t *out, int batch,
        const g1aff_t *wtab = nullptr, const uint8_t *winf = nullptr,
        hipStream_t stream = 0) {
    int blocks = (batch + MASK_SUBS - 1) / MASK_SUBS;
    if (wtab != nullptr) {
        /* small bitmaps leave 64 lanes with so few byte-adds that the
         * reduction tree dominates: use 16 lanes below 2048 bytes */
        if (bm_stride >= 2048)
            hipLaunchKernelGGL((k_mask_aggregate_w<64>), dim3(blocks),
                               dim3(64 * MASK_SUBS), 0, stream,
                               wtab, winf, n, bm, bm_stride, full_sum, out, batch);
        else
            hipLaunchKernelGGL((k_mask_aggregate_w<16>), dim3(blocks),
                               dim3(16 * MASK_SUBS), 0, stream,
                               wtab, winf, n, bm, bm_stride, full_sum, out, batch);
        return;
    }
    if (n >= 16384)
        hipLaunchKernelGGL((k_mask_aggregate<64>), dim3(blocks),
                           dim3(64 * MASK_SUBS), 0, stream,
                           table, n, bm, bm_stride, full_sum, out, batch);
    else
        hipLaunchKernelGGL((k_mask_aggregate<MASK_LANES>), dim3(blocks),
                           dim3(MASK_BLOCK), 0, stream,
                           table, n, bm, bm_stride, full_sum, out, batch);
}

__global__ void k_hash_to_g2(const uint8_t *msgs, int mlen, g2_t *out,
                             int32_t *ok, int batch, int fast_cofactor) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    g2_t h;
    if (!hash_to_g2_point(h, msgs + (size_t)i * mlen, mlen, fast_cofactor)) { ok[i] = 0; return; }
    out[i] = h;
    ok[i] = 1;
}

__global__ void k_g2_decompress(const uint8_t *sigs96, g2aff_t *out, int32_t *flags, int batch) {
    /* flags: 1 ok, 0 bad, 2 infinity */
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    g2_t p;
    if (!g2_deserialize(p, sigs96 + (size_t)i * 96, true)) { flags[i] = 0; return; }
    if (g2_is_inf(p)) { flags[i] = 2; return; }
    out[i].x = p.x;
    out[i].y = p.y;
    flags[i] = 1;
}

__global__ void k_verify(const g1_t *aggpubs, const g2_t *hms, const g2aff_t *sigs,
                         const int32_t *sig_flags, const int32_t *hm_ok,
                         int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (!hm_ok[i] || sig_flags[i] == 0) { results[i] = HBLS_ERR_BADINPUT; return; }
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing(aggpubs[i], hms[i], sig_inf ? dummy : sigs[i], sig_inf);
}

/* per-signer vote verify: pub = table[key_idx[i]]; hm_idx (optional) maps
 * each vote to a shared per-round hash point (stream path: 16 rounds share
 * 16 hash-to-G2 results across thousands of votes) — null means hms[i]. */
__global__ void k_verify_votes(const g1aff_t *table, int n, const uint32_t *key_idx,
                               const g2_t *hms, const uint32_t *hm_idx,
                               const g2aff_t *sigs,
                               const int32_t *sig_flags, const int32_t *hm_ok,
                               int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    int h = hm_idx ? (int)hm_idx[i] : i;
    if (!hm_ok[h] || sig_flags[i] == 0 || key_idx[i] >= (uint32_t)n) {
        results[i] = HBLS_ERR_BADINPUT; return;
    }
    g1_t pub;
    pub.x = table[key_idx[i]].x;
    pub.y = table[key_idx[i]].y;
    fp_one(pub.z);
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing(pub, hms[h], sig_inf ? dummy : sigs[i], sig_inf);
}

__global__ void k_g2_serialize(const g2_t *pts, uint8_t *out96, const int32_t *ok, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (!ok[i]) { for (int j = 0; j < 96; j++) out96[96 * i + j] = 0; return; }
    g2_t p = pts[i];
    g2_serialize(out96 + (size_t)i * 96, p);
}
__global__ void k_g1_serialize(const g1_t *pts, uint8_t *out48, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    g1_t p = pts[i];
    g1_serialize(out48 + (size_t)i * 48, p);
}

__global__ void k_sign(const uint8_t *sks, const uint8_t *msgs, int mlen,
                       uint8_t *sigs, int32_t *ok, int batch, int fast_cofactor) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    uint64_t k[4];
    if (!fr_from_le32(k, sks + 32 * i)) { ok[i] = 0; return; }
    g2_t h, sig;
    if (!hash_to_g2_point(h, msgs + (size_t)i * mlen, mlen, fast_cofactor)) { ok[i] = 0; return; }
    g2_mul(sig, h, k, 4);
    g2_serialize(sigs + (size_t)i * 96, sig);
    ok[i] = 1;
}

/* generic G1 ops for the scalar drop-ins (1-thread kernels) */
__global__ void k_g1_addsub(const uint8_t *a48, const uint8_t *b48, uint8_t *out48,
                            int32_t *ok, int sub) {
    g1_t a, b;
    if (!g1_deserialize(a, a48, true) || !g1_deserialize(b, b48, true)) { *ok = 0; return; }
    if (sub) g1_neg(b, b);
    g1_add(a, a, b);
    g1_serialize(out48, a);
    *ok = 1;
}
__global__ void k_g2_addsub(const uint8_t *a96, const uint8_t *b96, uint8_t *out96,
                            int32_t *ok, int sub) {
    g2_t a, b;
    if (!g2_deserialize(a, a96, true) || !g2_deserialize(b, b96, true)) { *ok = 0; return; }
    if (sub) g2_neg(b, b);
    g2_add(a, a, b);
    g2_serialize(out96, a);
    *ok = 1;
}
__global__ void k_g1_check(const uint8_t *p48, int32_t *ok) {
    g1_t p;
    *ok = g1_deserialize(p, p48, true) ? 1 : 0;
}
__global__ void k_g2_check(const uint8_t *p96, int32_t *ok) {
    g2_t p;
    *ok = g2_deserialize(p, p96, true) ? 1 : 0;
}
/* test support: decompress WITHOUT subgroup check, then report both
 * membership methods (full [r]Q and psi-criterion) for equivalence tests */
__global__ void k_g2_subgroup_methods(const uint8_t *p96, int32_t *out2) {
    g2_t p;
    if (!g2_deserialize(p, p96, false)) { out2[0] = out2[1] = -1; return; }
    out2[0] = g2_in_subgroup(p) ? 1 : 0;
    out2[1] = g2_in_subgroup_fast(p) ? 1 : 0;
}

/* MSM v1: blocks of 256 threads; thread t of block b handles point b*256+t,
 * does full scalar mult, LDS tree reduce; second kernel reduces block results. */
/* config-4 support: add n_ext serialized G1 partials (from other ranks'
 * committee slices) into each item's aggregate before the pairing check.
 * Partials are internal products (no subgroup check; identity = 48 zeros). */
__global__ void k_add_partials(g1_t *aggs, const uint8_t *ext48s, int n_ext,
                               int32_t *ok, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    g1_t acc = aggs[i];
    for (int e = 0; e < n_ext; e++) {
        const uint8_t *p = ext48s + ((size_t)e * batch + i) * 48;
        g1_t q;
        if (!g1_deserialize(q, p, false)) { ok[i] = 0; return; }
        g1_add(acc, acc, q);
    }
    aggs[i] = acc;
    ok[i] = 1;
}

/* sync-path seal-blob split (§8f-3): commitSigAndBitmap blobs
 * (96B sig || ceil(n/8)B bitmap each, internal/chain/sig.go:22-35) are
 * uploaded raw and parsed on-device — coalesced byte-granular grid-stride
 * over the blob buffer, no host-side per-item copies. */
__global__ void k_seal_split(const uint8_t *blobs, size_t blob_len, size_t bm,
                             uint8_t *sigs96, uint8_t *bms, size_t batch) {
    size_t total = batch * blob_len;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        size_t j = t / blob_len, off = t - j * blob_len;
        uint8_t v = blobs[t];
        if (off < 96) sigs96[j * 96 + off] = v;
        else bms[j * bm + (off - 96)] = v;
    }
}

/* config-4 epilogue: an item whose external partial failed to deserialize
 * (ok[i]==0 from k_add_partials) must report bad input, not a verify result
 * computed against the local-slice-only key sum. */
__global__ void k_merge_pok(int32_t *results, const int32_t *pok, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (!pok[i]) results[i] = HBLS_ERR_BADINPUT;
}

/* sum of n serialized G2 signatures (AggregateSig batch form,
 * crypto/bls/mask.go:57-64): one 64-thread block, strided deserialize+add,
 * LDS tree.  flags: 1 ok, 0 bad input. */
__global__ void __launch_bounds__(64) k_g2_sum(const uint8_t *sigs96, int n,
                                               uint8_t *out96, int32_t *ok) {
    __shared__ g2_t red[64];
    g2_t acc;
    g2_set_inf(acc);
    bool good = true;
    for (int i = threadIdx.x; i < n; i += 64) {
        g2_t q;
        if (!g2_deserialize(q, sigs96 + (size_t)i * 96, true)) { good = false; break; }
        g2_add(acc, acc, q);
    }
    if (!good) atomicExch(ok, 0);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            g2_t t;
            g2_add(t, red[threadIdx.x], red[threadIdx.x + st]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && *ok) g2_serialize(out96, red[0]);
}

__global__ void k_keccak(const uint8_t *msgs, int mlen, uint8_t *outs, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    keccak256_dev(msgs + (size_t)i * mlen, mlen, outs + (size_t)i * 32);
}

#include "hbls_coop.inc"

/* ================================================================ host layer */
#include <memory>
#include <mutex>
#include <vector>

static int g_device = -1;
static int g_fast_cofactor = 1;
static int g_coop_threshold = -1;   /* -1: read env on first use; 0: disabled */
static int coop_threshold(void) {
    if (g_coop_threshold < 0) {
        const char *e = getenv("HBLS_COOP_THRESHOLD");
        g_coop_threshold = e ? atoi(e) : 8192;
    }
    return g_coop_threshold;
}
extern "C" void hbls_set_coop_threshold(int n) { g_coop_threshold = n; }
static thread_local uint64_t g_last_ns = 0;
static thread_local uint64_t g_stage_ns[9] = {0};
static std::once_flag g_init_flag;
static int g_init_rc = HBLS_ERR_NOGPU;
/* combined aggregate verify (hbls_aggrlc.inc, included below) */
static int aggrlc_init_tables(void);
static void aggrlc_stats_reset(void);

#define HIP_OK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    fprintf(stderr, "hbls: %s failed: %s\n", #expr, hipGetErrorString(_e)); return HBLS_ERR; } } while (0)
#define HIP_OKP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    fprintf(stderr, "hbls: %s failed: %s\n", #expr, hipGetErrorString(_e)); return nullptr; } } while (0)

extern "C" int hbls_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int hbls_init(int device) {
    int n = hbls_device_count();
    if (n <= 0) return HBLS_ERR_NOGPU;
    if (device >= 0) {
        if (device >= n) return HBLS_ERR_BADINPUT;
        if (hipSetDevice(device) != hipSuccess) return HBLS_ERR;
        g_device = device;
    } else {
        hipGetDevice(&g_device);
    }
    /* warm up: trivial alloc/free to initialize the context */
    void *p = nullptr;
    if (hipMalloc(&p, 64) != hipSuccess) return HBLS_ERR;
    hipFree(p);
    g_init_rc = HBLS_OK;
    /* fixed-base table of -G1 for the combined aggregate verify; without it
     * every call takes the exact path */
    (void)aggrlc_init_tables();
    return HBLS_OK;
}

extern "C" void hbls_set_g2_cofactor_mode(int fast) { g_fast_cofactor = fast; }
extern "C" const char *hbls_version(void) { return "hbls 0.1 (gfx950)"; }
extern "C" uint64_t hbls_last_kernel_ns(void) { return g_last_ns; }
extern "C" uint64_t hbls_last_stage_ns(int i) { return (i >= 0 && i < 9) ? g_stage_ns[i] : 0; }

static int require_gpu(void) {
    if (g_init_rc != HBLS_OK) {
        /* allow implicit init on first call */
        if (hbls_init(-1) != HBLS_OK) return HBLS_ERR_NOGPU;
    }
    return HBLS_OK;
}

/* RAII device buffer */
struct DevBuf {
    void *p = nullptr;
    hipError_t err = hipSuccess;
    explicit DevBuf(size_t n) { err = hipMalloc(&p, n ? n : 1); }
    /* a buffer that only some callers of a shared body need: none unless wanted */
    DevBuf(size_t n, bool wanted) { if (wanted) err = hipMalloc(&p, n ? n : 1); }
    ~DevBuf() { if (p) hipFree(p); }
    template <typename T> T *as() const { return (T *)p; }
};

/* ---- host-side accounting of the last aggregate-verify call on this thread
 * (steady_clock): 0 device allocations, 1 time inside upload calls, 2 first
 * launch to results on the host, 3 frees, 4 the whole call */
#include <chrono>
static thread_local uint64_t g_host_ns[5] = {0};
static thread_local bool g_host_open = false;
static inline uint64_t host_now_ns(void) {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
        std::chrono::steady_clock::now().time_since_epoch()).count();
}
extern "C" uint64_t hbls_last_host_ns(int i) { return (i >= 0 && i < 5) ? g_host_ns[i] : 0; }
/* adds its own lifetime to counter i */
struct HostSpan {
    int i; uint64_t t0;
    explicit HostSpan(int idx) : i(idx), t0(host_now_ns()) {}
    ~HostSpan() { g_host_ns[i] += host_now_ns() - t0; }
};
/* the outermost one on a thread resets the counters and owns counter 4 */
struct HostCall {
    bool owner; uint64_t t0;
    HostCall() : owner(!g_host_open), t0(0) {
        if (!owner) return;
        g_host_open = true;
        for (int i = 0; i < 5; i++) g_host_ns[i] = 0;
        t0 = host_now_ns();
    }
    ~HostCall() {
        if (!owner) return;
        g_host_ns[4] = host_now_ns() - t0;
        g_host_open = false;
    }
};
/* times the destructors of the DevBufs declared between the two: FreeClock
 * before the first of them, FreeClockArm after the last (locals die in
 * reverse order, so the arm fires first and the clock stops last) */
struct FreeClock {
    uint64_t t0 = 0; bool armed = false;
    ~FreeClock() { if (armed) g_host_ns[3] += host_now_ns() - t0; }
};
struct FreeClockArm {
    FreeClock &fc;
    explicit FreeClockArm(FreeClock &f) : fc(f) {}
    ~FreeClockArm() { fc.t0 = host_now_ns(); fc.armed = true; }
};

/* ---- uploads off the compute stream.  Kernels run on the null stream; a
 * host buffer goes up on one non-blocking stream of its own (created on
 * first use, kept for the life of the process) with an event behind it, and
 * the null stream waits on that event ahead of the first kernel that reads
 * the buffer — so a kernel waits only for the bytes it reads.  The sources
 * are pageable: the copy call returns once the runtime has staged them, and
 * the host issues the next launch only then, which is why the callers
 * interleave uploads and launches instead of queueing every upload first. */
static hipStream_t g_upload_stream = nullptr;
static std::once_flag g_upload_flag;
static hipStream_t upload_stream(void) {
    std::call_once(g_upload_flag, [] {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess)
            g_upload_stream = s;
        else
            (void)hipGetLastError();    /* no stream: uploads fall to the null stream */
    });
    return g_upload_stream;
}
/* dst <- src on the upload stream, `done` recorded behind it, and the null
 * stream made to wait on `done` */
static hipError_t upload_then_wait(void *dst, const void *src, size_t n, hipEvent_t done) {
    HostSpan sp(1);
    hipStream_t s = upload_stream();
    hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(done, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(0, done, 0);
    return e;
}
/* a fixed set of events, destroyed on every return path */
template <int N> struct EventSet {
    hipEvent_t e[N];
    hipError_t err = hipSuccess;
    EventSet() {
        for (int i = 0; i < N; i++) {
            e[i] = nullptr;
            hipError_t r = hipEventCreate(&e[i]);
            if (r != hipSuccess) err = r;
        }
    }
    ~EventSet() { for (int i = 0; i < N; i++) if (e[i]) (void)hipEventDestroy(e[i]); }
    hipEvent_t operator[](int i) const { return e[i]; }
};

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    Timer() { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, 0); }
    void stop_and_store() {
        hipEventRecord(b, 0);
        hipEventSynchronize(b);
        float ms = 0;
        hipEventElapsedTime(&ms, a, b);
        g_last_ns = (uint64_t)(ms * 1e6);
        destroy();
    }
    /* a caller that returns before stop_and_store() leaves both alive */
    ~Timer() { destroy(); }
    void destroy() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
    }
};

/* the tail of the batch entries that report per-item ok-flags: download them,
 * HBLS_ERR_BADINPUT if any is 0 */
static int check_ok_flags(const int32_t *d_ok, size_t batch) {
    std::vector<int32_t> ok(batch);
    HIP_OK(hipMemcpy(ok.data(), d_ok, batch * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < batch; i++)
        if (!ok[i]) return HBLS_ERR_BADINPUT;
    return HBLS_OK;
}

extern "C" int hbls_batch_pk_from_sk(const uint8_t *sks32, size_t batch, uint8_t *pks48) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dsk(batch * 32), dpk(batch * 48), dok(batch * 4);
    if (dsk.err || dpk.err || dok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dsk.p, sks32, batch * 32, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_pk_from_sk, dim3(nb), dim3(64), 0, 0,
                       dsk.as<uint8_t>(), dpk.as<uint8_t>(), dok.as<int32_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(pks48, dpk.p, batch * 48, hipMemcpyDeviceToHost));
    return check_ok_flags(dok.as<int32_t>(), batch);
}

extern "C" int hbls_pk_from_sk(const uint8_t sk32[32], uint8_t pk48[48]) {
    return hbls_batch_pk_from_sk(sk32, 1, pk48);
}

extern "C" int hbls_batch_hash_to_g2(const uint8_t *msgs, size_t msg_len, size_t batch,
                                     uint8_t *out96s) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dm(batch * msg_len), dout(batch * sizeof(g2_t)), dok(batch * 4), dser(batch * 96);
    if (dm.err || dout.err || dok.err || dser.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dm.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    /* exception: no verify stage; the thread-per-item hash whatever the threshold */
    hipLaunchKernelGGL(k_hash_to_g2, dim3(nb), dim3(64), 0, 0,
                       dm.as<uint8_t>(), (int)msg_len, dout.as<g2_t>(), dok.as<int32_t>(),
                       (int)batch, g_fast_cofactor);
    hipLaunchKernelGGL(k_g2_serialize, dim3(nb), dim3(64), 0, 0,
                       dout.as<g2_t>(), dser.as<uint8_t>(), dok.as<int32_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out96s, dser.p, batch * 96, hipMemcpyDeviceToHost));
    return check_ok_flags(dok.as<int32_t>(), batch);
}
extern "C" int hbls_hash_to_g2(const uint8_t *msg, size_t msg_len, uint8_t out96[96]) {
    return hbls_batch_hash_to_g2(msg, msg_len, 1, out96);
}

extern "C" int hbls_batch_sign(const uint8_t *sks32, const uint8_t *msgs, size_t msg_len,
                               size_t batch, uint8_t *sigs96) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dsk(batch * 32), dm(batch * msg_len), dsig(batch * 96), dok(batch * 4);
    if (dsk.err || dm.err || dsig.err || dok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dsk.p, sks32, batch * 32, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dm.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_sign, dim3(nb), dim3(64), 0, 0,
                       dsk.as<uint8_t>(), dm.as<uint8_t>(), (int)msg_len,
                       dsig.as<uint8_t>(), dok.as<int32_t>(), (int)batch, g_fast_cofactor);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(sigs96, dsig.p, batch * 96, hipMemcpyDeviceToHost));
    return check_ok_flags(dok.as<int32_t>(), batch);
}
extern "C" int hbls_sign_hash(const uint8_t sk32[32], const uint8_t *msg, size_t msg_len,
                              uint8_t sig96[96]) {
    return hbls_batch_sign(sk32, msg, msg_len, 1, sig96);
}

/* ---- committee ---- */


#ifndef HBLS_RF_DEFAULT
#define HBLS_RF_DEFAULT 0
#endif
#ifdef HBLS_RF_ALL_LB
#define HBLS_RF_W2_KERN k_verify_rf_w2
#define HBLS_RF_W1_KERN k_verify_rf_w1
#else
#define HBLS_RF_W2_KERN k_verify_rf
#define HBLS_RF_W1_KERN k_verify_rf
#endif
/* register-file verify dispatch (HBLS_VERIFY_RF: 0 round-1 kernel,
 * 1 rf compiler-occupancy, 2 rf 256-reg, 3 rf 512-reg) */
static int g_rf_override = -1;
static int rf_mode(void) {
    if (g_rf_override >= 0) return g_rf_override;
    static int m = -1;
    if (m < 0) { const char *e = getenv("HBLS_VERIFY_RF"); m = e ? atoi(e) : HBLS_RF_DEFAULT; }
    return m;
}
extern "C" void hbls_set_verify_rf(int mode) { g_rf_override = mode; }
/* batched Montgomery-inversion affine conversion ahead of the scalar verify
 * kernel.  MEASURED WALL-NEUTRAL (+1.7 ms on a 197 ms launch at batch
 * 131072, profiles/r02_data/r2o_affine_*.json) despite removing ~5% of the
 * multiplies — the fifth datapoint confirming the pairing kernel is bound
 * by scratch traffic, not arithmetic (with r1's fused-Miller neutrality
 * and the four r2 falsifications).  Default OFF; HBLS_BATCH_AFFINE=1
 * enables for A/Bs. */
static int use_batch_affine(void) {
    static int m = -1;
    if (m < 0) { const char *e = getenv("HBLS_BATCH_AFFINE"); m = (e && atoi(e)) ? 1 : 0; }
    return m;
}
/* coop items-per-block dispatch.  MEASURED (profiles/r02_data/r2g_coopab.log):
 * the 8-item/32-thread variant (38 KB arena, 4 blocks/CU) is WORSE at every
 * batch (e.g. 116 vs 82 ms at 4096, stream 17.9k vs 19.2k msgs/s) — the
 * half-empty waves double the per-item instruction issue, which costs more
 * than the extra co-residency hides.  Default is therefore 16 items
 * everywhere; HBLS_COOP_ITEMS=8 keeps the losing variant reproducible. */
static int coop_items(size_t batch) {
    static int force = -2;
    if (force == -2) {
        const char *e = getenv("HBLS_COOP_ITEMS");
        force = e ? atoi(e) : 0;
    }
    if (force == 8 || force == 16) return force;
    (void)batch;
    return 16;
}

/* ---- one launcher per stage of the verify pipelines.  Every
 * entry point goes through these.  Each takes the wave-cooperative kernel when
 * the n it is given is at or below coop_threshold() and the thread-per-item
 * kernel above it, on the null stream; the caller chooses the n. */
#define LAUNCH_COOP(kern, n, ...) do { \
    int it_ = coop_items(n); \
    int nbc_ = (int)(((n) + it_ - 1) / it_); \
    if (it_ == 16) hipLaunchKernelGGL(kern<16>, dim3(nbc_), dim3(64), 0, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(kern<8>, dim3(nbc_), dim3(32), 0, 0, __VA_ARGS__); \
} while (0)
static inline bool coop_wanted(size_t n) { return (int)n <= coop_threshold(); }
static inline int scalar_blocks(size_t n) { return (int)((n + 63) / 64); }

/* the cooperative hash whatever the threshold: launch_hash_to_g2's first
 * branch, and what hbls_stream_set_rounds always takes */
static void launch_hash_to_g2_coop(const uint8_t *d_msg, size_t msg_len, g2_t *d_hm,
                                   int32_t *d_hok, size_t n) {
    LAUNCH_COOP(k_hash_to_g2_coop, n, d_msg, (int)msg_len, d_hm, d_hok, (int)n,
                g_fast_cofactor);
}
/* n messages of msg_len bytes -> n hash points and their ok-flags */
static void launch_hash_to_g2(const uint8_t *d_msg, size_t msg_len, g2_t *d_hm,
                              int32_t *d_hok, size_t n) {
    if (coop_wanted(n))
        launch_hash_to_g2_coop(d_msg, msg_len, d_hm, d_hok, n);
    else
        hipLaunchKernelGGL(k_hash_to_g2, dim3(scalar_blocks(n)), dim3(64), 0, 0,
                           d_msg, (int)msg_len, d_hm, d_hok, (int)n, g_fast_cofactor);
}
/* n serialized signatures -> affine points and their flags */
static void launch_g2_decompress(const uint8_t *d_sig, g2aff_t *d_saff, int32_t *d_sflags,
                                 size_t n) {
    if (coop_wanted(n))
        LAUNCH_COOP(k_g2_decompress_coop, n, d_sig, d_saff, d_sflags, (int)n);
    else
        hipLaunchKernelGGL(k_g2_decompress, dim3(scalar_blocks(n)), dim3(64), 0, 0,
                           d_sig, d_saff, d_sflags, (int)n);
}
/* the thread-per-item pairing check, by rf_mode() */
static void launch_verify_scalar(const g1_t *d_pub, const g2_t *d_hm, const g2aff_t *d_saff,
                                 const int32_t *d_sflags, const int32_t *d_hok,
                                 int32_t *d_res, size_t n) {
    void (*kern)(const g1_t *, const g2_t *, const g2aff_t *, const int32_t *,
                 const int32_t *, int32_t *, int) = k_verify;
    switch (rf_mode()) {
#ifdef HBLS_RF
    case 1: kern = k_verify_rf; break;
    case 2: kern = HBLS_RF_W2_KERN; break;
    case 3: kern = HBLS_RF_W1_KERN; break;
#endif
    case 4: kern = k_verify_2p; break;
    case 5: kern = k_verify_6; break;
    }
    hipLaunchKernelGGL(kern, dim3(scalar_blocks(n)), dim3(64), 0, 0,
                       d_pub, d_hm, d_saff, d_sflags, d_hok, d_res, (int)n);
}
/* pairing check of n prepared (key sum, hash point, signature) triples */
static void launch_verify(const g1_t *d_pub, const g2_t *d_hm, const g2aff_t *d_saff,
                          const int32_t *d_sflags, const int32_t *d_hok, int32_t *d_res,
                          size_t n) {
    if (coop_wanted(n))
        LAUNCH_COOP(k_verify_coop, n, d_pub, d_hm, d_saff, d_sflags, d_hok, d_res, (int)n);
    else
        launch_verify_scalar(d_pub, d_hm, d_saff, d_sflags, d_hok, d_res, n);
}
/* gather buffers of the rf votes path: the caller declares one ahead of its
 * Timer and hands it to launch_verify_votes.  One element each unless
 * rf_mode() is on. */
struct RfGather {
    DevBuf pub, hm, ok;
    explicit RfGather(size_t n)
        : pub((rf_mode() ? n : 1) * sizeof(g1_t)), hm((rf_mode() ? n : 1) * sizeof(g2_t)),
          ok((rf_mode() ? n : 1) * 4) {}
    bool err() const { return pub.err || hm.err || ok.err; }
};
/* per-vote check against the key table: vote i is key d_idx[i] on hash point
 * d_hm[d_hm_idx ? d_hm_idx[i] : i].  Above the threshold rf modes 1..3 go
 * gather (keys and per-vote hash points) -> k_verify_rf. */
static void launch_verify_votes(const g1aff_t *table, size_t n_keys, const uint32_t *d_idx,
                                const g2_t *d_hm, const uint32_t *d_hm_idx,
                                const g2aff_t *d_saff, const int32_t *d_sflags,
                                const int32_t *d_hok, int32_t *d_res, size_t n,
                                const RfGather &g) {
    if (coop_wanted(n)) {
        LAUNCH_COOP(k_verify_votes_coop, n, table, (int)n_keys, d_idx, d_hm, d_hm_idx,
                    d_saff, d_sflags, d_hok, d_res, (int)n);
        return;
    }
    int nb = scalar_blocks(n);
#ifdef HBLS_RF
    if (rf_mode() >= 1 && rf_mode() <= 3) {
        hipLaunchKernelGGL(k_gather_votes_rf, dim3(nb), dim3(64), 0, 0,
                           table, (int)n_keys, d_idx, d_hm, d_hm_idx, d_hok,
                           g.pub.as<g1_t>(), g.hm.as<g2_t>(), g.ok.as<int32_t>(), (int)n);
        hipLaunchKernelGGL(k_verify_rf, dim3(nb), dim3(64), 0, 0,
                           g.pub.as<g1_t>(), g.hm.as<g2_t>(), d_saff, d_sflags,
                           g.ok.as<int32_t>(), d_res, (int)n);
        return;
    }
#endif
    (void)g;
    hipLaunchKernelGGL(k_verify_votes, dim3(nb), dim3(64), 0, 0,
                       table, (int)n_keys, d_idx, d_hm, d_hm_idx, d_saff, d_sflags, d_hok,
                       d_res, (int)n);
}

struct hbls_committee {
    g1aff_t *d_table;
    g1_t *d_full_sum;   /* committee-wide key sum, for the dense-mask path */
    g1aff_t *d_wtab;    /* 8-bit window table (n >= 16384): groups x 255 */
    uint8_t *d_winf;    /* per-entry infinity flags for d_wtab */
    size_t n;
    /* quorum by mask (hbls_quorum.inc): voting power per key in 1e-18 units,
     * quorum <=> masked sum > q_threshold */
    uint64_t *d_power;
    uint64_t q_threshold;
    int q_uniform;      /* all weights 1: popcount path */
    int q_set;          /* hbls_committee_set_quorum was called */
};
extern "C" hbls_committee_t *hbls_committee_build(const uint8_t *pks48, size_t n) {
    if (require_gpu() != HBLS_OK) return nullptr;
    g1aff_t *d_table = nullptr;
    HIP_OKP(hipMalloc(&d_table, n * sizeof(g1aff_t)));
    DevBuf dpk(n * 48), dok(n * 4);
    if (dpk.err || dok.err) { hipFree(d_table); return nullptr; }
    if (hipMemcpy(dpk.p, pks48, n * 48, hipMemcpyHostToDevice) != hipSuccess) { hipFree(d_table); return nullptr; }
    int nb = (int)((n + 63) / 64);
    hipLaunchKernelGGL(k_g1_table_build, dim3(nb), dim3(64), 0, 0,
                       dpk.as<uint8_t>(), d_table, dok.as<int32_t>(), (int)n);
    if (hipDeviceSynchronize() != hipSuccess) { hipFree(d_table); return nullptr; }
    std::vector<int32_t> ok(n);
    if (hipMemcpy(ok.data(), dok.p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { hipFree(d_table); return nullptr; }
    for (size_t i = 0; i < n; i++)
        if (!ok[i]) { hipFree(d_table); return nullptr; }
    hbls_committee_t *c = new hbls_committee_t;
    c->d_table = d_table;
    c->n = n;
    c->d_full_sum = nullptr;
    c->d_wtab = nullptr;
    c->d_winf = nullptr;
    /* uniform voting power until hbls_committee_set_quorum says otherwise */
    c->d_power = nullptr;
    c->q_threshold = (uint64_t)(2 * n / 3);
    c->q_uniform = 1;
    c->q_set = 0;
    {
        std::vector<uint64_t> ones(n, 1);
        if (hipMalloc(&c->d_power, n ? n * 8 : 8) != hipSuccess ||
            hipMemcpy(c->d_power, ones.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess) {
            if (c->d_power) hipFree(c->d_power);
            hipFree(d_table);
            delete c;
            return nullptr;
        }
    }
    /* 8-bit window table: 255 subset sums per 8-key group (n x 3060 B:
     * ~12.5 MB at n=4096, ~200 MB at n=65536; skipped silently if the
     * transient allocations fail) */
    if (n >= 2048) {
        size_t groups = (n + 7) / 8, m = groups * 255;
        g1_t *d_wj = nullptr;
        g1aff_t *d_wt = nullptr;
        uint8_t *d_wi = nullptr;
        if (hipMalloc(&d_wj, m * sizeof(g1_t)) == hipSuccess &&
            hipMalloc(&d_wt, m * sizeof(g1aff_t)) == hipSuccess &&
            hipMalloc(&d_wi, m) == hipSuccess) {
            hipLaunchKernelGGL(k_wtab_build_jac, dim3((int)((groups + 63) / 64)),
                               dim3(64), 0, 0, d_table, (int)n, d_wj, (int)groups);
            hipLaunchKernelGGL(k_wtab_to_affine, dim3((int)((m + 255) / 256)),
                               dim3(256), 0, 0, d_wj, d_wt, d_wi, m);
            if (hipDeviceSynchronize() == hipSuccess) {
                c->d_wtab = d_wt;
                c->d_winf = d_wi;
            }
        }
        if (d_wj) hipFree(d_wj);
        if (c->d_wtab == nullptr) {
            if (d_wt) hipFree(d_wt);
            if (d_wi) hipFree(d_wi);
        }
    }
    /* committee-wide sum for the dense-mask complement path */
    g1_t *d_fs = nullptr;
    if (hipMalloc(&d_fs, sizeof(g1_t)) == hipSuccess) {
        size_t bm = (n + 7) / 8;
        DevBuf ones(bm);
        if (!ones.err) {
            std::vector<uint8_t> host_ones(bm, 0);
            for (size_t i = 0; i < n; i++) host_ones[i >> 3] |= 1 << (i & 7);
            if (hipMemcpy(ones.p, host_ones.data(), bm, hipMemcpyHostToDevice) == hipSuccess) {
                launch_mask_aggregate(c->d_table, (int)n, ones.as<uint8_t>(),
                                      (int)bm, (const g1_t *)nullptr, d_fs, 1,
                                      c->d_wtab, c->d_winf);
                if (hipDeviceSynchronize() == hipSuccess)
                    c->d_full_sum = d_fs;
            }
        }
        if (c->d_full_sum == nullptr) hipFree(d_fs);
    }
    return c;
}
extern "C" void hbls_committee_free(hbls_committee_t *c) {
    if (c) {
        hipFree(c->d_table);
        if (c->d_full_sum) hipFree(c->d_full_sum);
        if (c->d_wtab) hipFree(c->d_wtab);
        if (c->d_winf) hipFree(c->d_winf);
        if (c->d_power) hipFree(c->d_power);
        delete c;
    }
}
extern "C" size_t hbls_committee_size(const hbls_committee_t *c) { return c->n; }

extern "C" int hbls_mask_aggregate_g1(const hbls_committee_t *c, const uint8_t *bitmap,
                                      uint8_t out48[48]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    size_t bm = (c->n + 7) / 8;
    DevBuf dbm(bm), dout(sizeof(g1_t)), dser(48);
    if (dbm.err || dout.err || dser.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dbm.p, bitmap, bm, hipMemcpyHostToDevice));
    Timer tm;
    launch_mask_aggregate(c->d_table, (int)c->n, dbm.as<uint8_t>(), (int)bm,
                          c->d_full_sum, dout.as<g1_t>(), 1,
                          c->d_wtab, c->d_winf);
    hipLaunchKernelGGL(k_g1_serialize, dim3(1), dim3(1), 0, 0,
                       dout.as<g1_t>(), dser.as<uint8_t>(), 1);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out48, dser.p, 48, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* the hoisted schedule of the combined path (hbls_aggrlc.inc, DESIGN.md
 * §4l): the state its early part hands to aggrlc_verify, null when nothing
 * was hoisted */
struct AggrlcEarly;
/* what one call does on the combined path, resolved from the switches once
 * (aggrlc_plan) and read by everything after: combined or exact, where the
 * signature leg is paired (0 per item, 1 per chunk), whether the chunk-level
 * leg is hoisted, the item kernel's level, the final and chunk-leg kernels */
struct AggrlcPlan { bool combined; int leg; bool hoisted; int level, final_kernel, chunkleg_kernel; };
static AggrlcPlan aggrlc_plan(size_t batch, size_t mode_batch, bool may_hoist);
static AggrlcEarly *aggrlc_early_begin(AggrlcPlan &plan, const g2aff_t *d_saff,
                                       const int32_t *d_sflags, const int32_t *d_hok,
                                       int32_t *d_res, size_t batch);
static void aggrlc_early_free(AggrlcEarly *e);
struct AggrlcEarlyHold {
    AggrlcEarly *p = nullptr;
    ~AggrlcEarlyHold() { if (p) aggrlc_early_free(p); }
};
static int aggrlc_verify(const AggrlcPlan &plan, const g1_t *d_agg, const g2_t *d_hm,
                         const g2aff_t *d_saff, const int32_t *d_sflags, const int32_t *d_hok,
                         int32_t *d_res, size_t batch, AggrlcEarly *early);
#define AGGRLC_FALLBACK 2       /* aggrlc_verify wrote nothing: run the exact path */

/* host copies of the three inputs, for the entry point whose inputs are not
 * on the device yet */
struct AggHostSrc { const uint8_t *bitmaps, *sigs, *msgs; };

/* the pairing stage of the aggregate-verify pipeline and its epilogue: the
 * exact or the combined check over masked key sums, hash points and
 * decompressed signatures already enqueued on the null stream, then the
 * stage intervals (ev[2s], ev[2s+1] around stage s; ev[2] is the call's
 * first event) and the verdicts to the host.  plan is the caller's, resolved
 * once for the call (aggrlc_plan).  Shared by run_agg_verify_pipeline
 * and the epoch-context entry (hbls_ctxset.inc).  With `early` the pipeline
 * has hoisted the combined path's signature chain, so the combined path it
 * is; that chain's interval lies ahead of the verify events and is added to
 * stage 3, so the four stages still add up to the call's kernel time. */
static int run_agg_verify_pairing(const g1_t *d_agg, g2_t *d_hm, g2aff_t *d_saff,
                                  int32_t *d_sflags, int32_t *d_hok, int32_t *d_res,
                                  size_t batch, const AggrlcPlan &plan, const EventSet<8> &ev,
                                  uint64_t t_launch, int32_t *results,
                                  AggrlcEarly *early = nullptr) {
    (void)hipEventRecord(ev[6], 0);
    int arc = AGGRLC_FALLBACK;
    if (plan.combined) {
        arc = aggrlc_verify(plan, d_agg, d_hm, d_saff, d_sflags, d_hok, d_res, batch, early);
        if (arc != HBLS_OK && arc != AGGRLC_FALLBACK) return arc;
    }
    if (arc == HBLS_OK) {
        /* combined path wrote every result */
    } else if ((int)batch > coop_threshold() && rf_mode() == 0 && use_batch_affine()) {
        /* exception: HBLS_BATCH_AFFINE is honoured here and by no other caller */
        DevBuf dpa(batch * sizeof(g1aff_t)), dpi(batch * 4), dha(batch * sizeof(g2aff_t));
        if (dpa.err || dpi.err || dha.err) return HBLS_ERR;
        int nba = (int)((batch + 64 * BA_K - 1) / (64 * BA_K));
        hipLaunchKernelGGL(k_g1_batch_affine, dim3(nba), dim3(64), 0, 0,
                           d_agg, dpa.as<g1aff_t>(), dpi.as<int32_t>(), (int)batch);
        hipLaunchKernelGGL(k_g2_batch_affine, dim3(nba), dim3(64), 0, 0,
                           d_hm, dha.as<g2aff_t>(), d_hok, (int)batch);
        hipLaunchKernelGGL(k_verify_aff, dim3(scalar_blocks(batch)), dim3(64), 0, 0,
                           dpa.as<g1aff_t>(), dpi.as<int32_t>(), dha.as<g2aff_t>(),
                           d_saff, d_sflags, d_hok, d_res, (int)batch);
        HIP_OK(hipDeviceSynchronize());   /* dpa/dha freed at scope exit */
    } else {
        launch_verify(d_agg, d_hm, d_saff, d_sflags, d_hok, d_res, batch);
    }
    (void)hipEventRecord(ev[7], 0);
    HIP_OK(hipEventSynchronize(ev[7]));
    float ms_total = 0, ms = 0;
    (void)hipEventElapsedTime(&ms_total, ev[2], ev[7]);
    g_last_ns = (uint64_t)(ms_total * 1e6);
    for (int i = 0; i < 4; i++) {
        (void)hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
        g_stage_ns[i] = (uint64_t)(ms * 1e6);
    }
    if (early && arc == HBLS_OK) g_stage_ns[3] += g_stage_ns[7];
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, d_res, batch * 4, hipMemcpyDeviceToHost));
    g_host_ns[2] += host_now_ns() - t_launch;
    return HBLS_OK;
}

/* the four-stage aggregate-verify pipeline over DEVICE-resident inputs
 * (bitmaps, serialized sigs, messages) — shared by the host-buffer entry
 * points and the HBM-direct seal-blob path.  Launch order: hash (reads the
 * messages), decompress (the signatures), mask (the bitmaps), verify.  With
 * `src` the three device buffers are still empty and each is uploaded just
 * ahead of the stage that reads it, so the large bitmap upload arrives
 * behind the hash and decompress kernels instead of in front of them.
 * g_stage_ns[0..3] stay mask, hash, decompress, verify: each the interval
 * between events recorded around that stage's launches (an upload wait sits
 * before the stage's first event).  Where the combined path hoists its
 * signature chain (aggrlc_early_begin) that chain runs between
 * decompress and mask, outside the four intervals, and the chunk legs run
 * beside the mask kernel on a side stream. */
static int run_agg_verify_pipeline(const hbls_committee_t *c, const uint8_t *d_bm,
                                   const uint8_t *d_sig, const uint8_t *d_msg,
                                   size_t msg_len, size_t batch, int32_t *results,
                                   const AggHostSrc *src = nullptr) {
    HostCall hcall;
    size_t bm = (c->n + 7) / 8;
    FreeClock fclk;
    uint64_t t_alloc = host_now_ns();
    DevBuf dagg(batch * sizeof(g1_t)), dhm(batch * sizeof(g2_t));
    DevBuf dsaff(batch * sizeof(g2aff_t)), dsflags(batch * 4), dhok(batch * 4), dres(batch * 4);
    g_host_ns[0] += host_now_ns() - t_alloc;
    FreeClockArm farm(fclk);
    if (dagg.err || dhm.err || dsaff.err || dsflags.err || dhok.err || dres.err)
        return HBLS_ERR;
    aggrlc_stats_reset();
    for (int i = 4; i < 9; i++) g_stage_ns[i] = 0;    /* the combined path's own, if it runs */
    /* ev[2s], ev[2s+1] around stage s (0 mask, 1 hash, 2 decompress, 3 verify) */
    EventSet<8> ev;
    EventSet<3> up;
    if (ev.err != hipSuccess || up.err != hipSuccess) return HBLS_ERR;
    uint64_t t_launch = host_now_ns();

    if (src) HIP_OK(upload_then_wait((void *)d_msg, src->msgs, batch * msg_len, up[0]));
    (void)hipEventRecord(ev[2], 0);
    launch_hash_to_g2(d_msg, msg_len, dhm.as<g2_t>(), dhok.as<int32_t>(), batch);
    (void)hipEventRecord(ev[3], 0);

    if (src) HIP_OK(upload_then_wait((void *)d_sig, src->sigs, batch * 96, up[1]));
    (void)hipEventRecord(ev[4], 0);
    launch_g2_decompress(d_sig, dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    (void)hipEventRecord(ev[5], 0);

    /* the combined path's signature chain and chunk legs, ahead of and
     * beside the mask kernel (declared after the buffers and events above:
     * it waits for its side stream before they go) */
    AggrlcPlan plan = aggrlc_plan(batch, batch, true);
    AggrlcEarlyHold early;
    early.p = aggrlc_early_begin(plan, dsaff.as<g2aff_t>(), dsflags.as<int32_t>(),
                                 dhok.as<int32_t>(), dres.as<int32_t>(), batch);

    if (src) HIP_OK(upload_then_wait((void *)d_bm, src->bitmaps, batch * bm, up[2]));
    (void)hipEventRecord(ev[0], 0);
    launch_mask_aggregate(c->d_table, (int)c->n, d_bm, (int)bm,
                                         c->d_full_sum, dagg.as<g1_t>(), (int)batch,
                                         c->d_wtab, c->d_winf);
    (void)hipEventRecord(ev[1], 0);

    return run_agg_verify_pairing(dagg.as<g1_t>(), dhm.as<g2_t>(), dsaff.as<g2aff_t>(),
                                  dsflags.as<int32_t>(), dhok.as<int32_t>(), dres.as<int32_t>(),
                                  batch, plan, ev, t_launch, results, early.p);
}

extern "C" int hbls_batch_agg_verify(const hbls_committee_t *c, const uint8_t *bitmaps,
                                     const uint8_t *sigs96, const uint8_t *msgs,
                                     size_t msg_len, size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    HostCall hcall;
    size_t bm = (c->n + 7) / 8;
    FreeClock fclk;
    uint64_t t_alloc = host_now_ns();
    DevBuf dbm(batch * bm), dsig(batch * 96), dmsg(batch * msg_len);
    g_host_ns[0] += host_now_ns() - t_alloc;
    FreeClockArm farm(fclk);
    if (dbm.err || dsig.err || dmsg.err) return HBLS_ERR;
    /* the pipeline uploads each buffer ahead of the stage that reads it */
    AggHostSrc src = { bitmaps, sigs96, msgs };
    return run_agg_verify_pipeline(c, dbm.as<uint8_t>(), dsig.as<uint8_t>(),
                                   dmsg.as<uint8_t>(), msg_len, batch, results, &src);
}

extern "C" int hbls_agg_verify(const hbls_committee_t *c, const uint8_t *bitmap,
                               const uint8_t sig96[96], const uint8_t *msg, size_t msg_len) {
    int32_t r;
    int rc = hbls_batch_agg_verify(c, bitmap, sig96, msg, msg_len, 1, &r);
    if (rc != HBLS_OK) return rc;
    return r;
}

extern "C" int hbls_batch_verify_votes(const hbls_committee_t *c, const uint32_t *key_idx,
                                       const uint8_t *sigs96, const uint8_t *msgs,
                                       size_t msg_len, size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf didx(batch * 4), dsig(batch * 96), dmsg(batch * msg_len);
    DevBuf dhm(batch * sizeof(g2_t)), dsaff(batch * sizeof(g2aff_t));
    DevBuf dsflags(batch * 4), dhok(batch * 4), dres(batch * 4);
    RfGather rfg(batch);
    if (didx.err || dsig.err || dmsg.err || dhm.err || dsaff.err || dsflags.err ||
        dhok.err || dres.err || rfg.err()) return HBLS_ERR;
    HIP_OK(hipMemcpy(didx.p, key_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmsg.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    launch_hash_to_g2(dmsg.as<uint8_t>(), msg_len, dhm.as<g2_t>(), dhok.as<int32_t>(), batch);
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    launch_verify_votes(c->d_table, c->n, didx.as<uint32_t>(), dhm.as<g2_t>(), nullptr,
                        dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), dhok.as<int32_t>(),
                        dres.as<int32_t>(), batch, rfg);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_verify_hash(const uint8_t pk48[48], const uint8_t sig96[96],
                                const uint8_t *msg, size_t msg_len) {
    /* single drop-in verify: committee of one + all-ones mask of 1 bit.
     * Identity pub (48 zero bytes) is legal here (zero-value struct), so it
     * bypasses the table path. */
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    int zero_pk = 1;
    for (int i = 0; i < 48; i++) if (pk48[i]) { zero_pk = 0; break; }
    if (zero_pk) {
        int zero_sig = 1;
        for (int i = 0; i < 96; i++) if (sig96[i]) { zero_sig = 0; break; }
        if (zero_sig) return HBLS_OK;           /* herumi: both identity accepts */
        if (hbls_g2_check(sig96) != HBLS_OK) return HBLS_ERR_BADINPUT;
        return HBLS_FALSE;
    }
    hbls_committee_t *c = hbls_committee_build(pk48, 1);
    if (!c) return HBLS_ERR_BADINPUT;
    uint8_t bitmap = 1;
    int r = hbls_agg_verify(c, &bitmap, sig96, msg, msg_len);
    hbls_committee_free(c);
    return r;
}

/* scalar G1/G2 ops */
/* the body of the single-point entries: upload one point of len bytes, or two
 * (b), launch one thread, read its flag, and download the result (out) only
 * when the flag is set; unset_rc is what an unset flag returns.  launch gets
 * the device copies of a, b and out (null where there is none) and the flag. */
template <typename Launch>
static int run_point_op(const uint8_t *a, const uint8_t *b, uint8_t *out, size_t len,
                        int unset_rc, Launch launch) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf da(len), db(len, b != nullptr), dout(len, out != nullptr), dok(4);
    if (da.err || db.err || dout.err || dok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(da.p, a, len, hipMemcpyHostToDevice));
    if (b) HIP_OK(hipMemcpy(db.p, b, len, hipMemcpyHostToDevice));
    launch(da.as<uint8_t>(), db.as<uint8_t>(), dout.as<uint8_t>(), dok.as<int32_t>());
    HIP_OK(hipDeviceSynchronize());
    int32_t ok;
    HIP_OK(hipMemcpy(&ok, dok.p, 4, hipMemcpyDeviceToHost));
    if (!ok) return unset_rc;
    if (out) HIP_OK(hipMemcpy(out, dout.p, len, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
extern "C" int hbls_g1_add_impl(const uint8_t *a, const uint8_t *b, uint8_t *out, int sub) {
    return run_point_op(a, b, out, 48, HBLS_ERR_BADINPUT,
                        [sub](uint8_t *da, uint8_t *db, uint8_t *dout, int32_t *dok) {
        hipLaunchKernelGGL(k_g1_addsub, dim3(1), dim3(1), 0, 0, da, db, dout, dok, sub);
    });
}
extern "C" int hbls_g1_add(const uint8_t a48[48], const uint8_t b48[48], uint8_t out48[48]) {
    return hbls_g1_add_impl(a48, b48, out48, 0);
}
extern "C" int hbls_g1_sub(const uint8_t a48[48], const uint8_t b48[48], uint8_t out48[48]) {
    return hbls_g1_add_impl(a48, b48, out48, 1);
}
extern "C" int hbls_g2_add(const uint8_t a96[96], const uint8_t b96[96], uint8_t out96[96]) {
    return run_point_op(a96, b96, out96, 96, HBLS_ERR_BADINPUT,
                        [](uint8_t *da, uint8_t *db, uint8_t *dout, int32_t *dok) {
        hipLaunchKernelGGL(k_g2_addsub, dim3(1), dim3(1), 0, 0, da, db, dout, dok, 0);
    });
}
extern "C" int hbls_g1_check(const uint8_t p48[48]) {
    return run_point_op(p48, nullptr, nullptr, 48, HBLS_FALSE,
                        [](uint8_t *dp, uint8_t *, uint8_t *, int32_t *dok) {
        hipLaunchKernelGGL(k_g1_check, dim3(1), dim3(1), 0, 0, dp, dok);
    });
}
extern "C" int hbls_g2_subgroup_methods(const uint8_t p96[96], int32_t out2[2]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dp(96), dout(8);
    if (dp.err || dout.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dp.p, p96, 96, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_g2_subgroup_methods, dim3(1), dim3(1), 0, 0,
                       dp.as<uint8_t>(), dout.as<int32_t>());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out2, dout.p, 8, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
extern "C" int hbls_g2_check(const uint8_t p96[96]) {
    return run_point_op(p96, nullptr, nullptr, 96, HBLS_FALSE,
                        [](uint8_t *dp, uint8_t *, uint8_t *, int32_t *dok) {
        hipLaunchKernelGGL(k_g2_check, dim3(1), dim3(1), 0, 0, dp, dok);
    });
}

/* round-1 per-thread double-and-add MSM, kept ONLY as the A/B reference for
 * the Pippenger kernel (hbls_msm_g1_naive; never on the product path) */
__global__ void __launch_bounds__(256)
k_msm_naive(const uint8_t *points48, const uint8_t *scalars32, int n,
            g1_t *partials, int32_t *ok) {
    __shared__ g1_t red[256];
    int i = blockIdx.x * 256 + threadIdx.x;
    g1_t acc;
    g1_set_inf(acc);
    if (i < n) {
        g1_t p;
        uint64_t k[4];
        if (!g1_deserialize(p, points48 + (size_t)i * 48, true) ||
            !fr_from_le32(k, scalars32 + (size_t)i * 32)) {
            atomicExch(ok, 0);
        } else {
            g1_mul(acc, p, k, 4);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            g1_t t;
            g1_add(t, red[threadIdx.x], red[threadIdx.x + s]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}
__global__ void k_g1_reduce_seq(const g1_t *partials, int n, uint8_t *out48) {
    g1_t acc;
    g1_set_inf(acc);
    for (int i = 0; i < n; i++) g1_add(acc, acc, partials[i]);
    g1_serialize(out48, acc);
}
extern "C" int hbls_msm_g1_naive(const uint8_t *points48, const uint8_t *scalars32,
                                 size_t n, uint8_t out48[48]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    int nblocks = (int)((n + 255) / 256);
    DevBuf dp(n * 48), ds(n * 32), dpart(nblocks * sizeof(g1_t)), dok(4), dout(48);
    if (dp.err || ds.err || dpart.err || dok.err || dout.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dp.p, points48, n * 48, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(ds.p, scalars32, n * 32, hipMemcpyHostToDevice));
    int32_t one = 1;
    HIP_OK(hipMemcpy(dok.p, &one, 4, hipMemcpyHostToDevice));
    Timer tm;
    hipLaunchKernelGGL(k_msm_naive, dim3(nblocks), dim3(256), 0, 0,
                       dp.as<uint8_t>(), ds.as<uint8_t>(), (int)n,
                       dpart.as<g1_t>(), dok.as<int32_t>());
    hipLaunchKernelGGL(k_g1_reduce_seq, dim3(1), dim3(1), 0, 0,
                       dpart.as<g1_t>(), nblocks, dout.as<uint8_t>());
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    int32_t ok;
    HIP_OK(hipMemcpy(&ok, dok.p, 4, hipMemcpyDeviceToHost));
    if (!ok) return HBLS_ERR_BADINPUT;
    HIP_OK(hipMemcpy(out48, dout.p, 48, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* ---- Pippenger bucket MSM (the `north_star`'s general-scalar MSM) ----
 * radix-256 digits (c = 8): 32 windows x 255 buckets.  GPU shape:
 *   prep     — thread/point: decompress + subgroup-check + digit transpose
 *   buckets  — one WAVE per (window, bucket): lanes stride the digit row
 *              (coalesced byte reads), accumulate matching points (mixed
 *              adds; identity fast paths make empty lanes cheap), LDS tree
 *   wreduce  — one thread per window: suffix sums S_w = sum b * B_b
 *   combine  — Horner over windows (248 doublings + 31 adds), one thread
 * Work ~ 32n mixed adds + 8160-wave trees vs n * (255 dbl + ~128 add) for
 * the round-1 per-thread double-and-add. */
__global__ void k_msm_prep(const uint8_t *points48, const uint8_t *scalars32, int n,
                           g1aff_t *pts, uint8_t *digits /* 32 x n */, int32_t *ok) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g1_t p;
    uint64_t k[4];
    if (!g1_deserialize(p, points48 + (size_t)i * 48, true) ||
        !fr_from_le32(k, scalars32 + (size_t)i * 32)) {
        atomicExch(ok, 0);
        return;
    }
    /* serialized points are affine (z=1) after deserialize */
    g1aff_t a;
    a.x = p.x;
    a.y = p.y;
    bool inf = g1_is_inf(p);
    pts[i] = a;
    for (int w = 0; w < 32; w++) {
        uint8_t d = (uint8_t)(k[w >> 3] >> (8 * (w & 7)));
        /* infinity contributes nothing: digit 0 is never bucketed */
        digits[(size_t)w * n + i] = inf ? 0 : d;
    }
}

/* counting sort of (window, digit) -> point-index lists, so each bucket
 * wave touches exactly its own points: no digit scans, no divergence
 * (the first bucket design scanned all n digits per wave and lost to the
 * naive kernel — profiles/r02_data/r2i_msm_ab.json) */
__global__ void k_msm_hist(const uint8_t *digits, int n, uint32_t *cnt /* 32*256 */) {
    size_t total = (size_t)32 * n;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride)
        atomicAdd(&cnt[(t / n) * 256 + digits[t]], 1u);
}
__global__ void __launch_bounds__(64) k_msm_prefix(const uint32_t *cnt,
                                                   uint32_t *off /* 32*257 */,
                                                   uint32_t *cursor /* 32*256 */) {
    int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 32) return;
    uint32_t acc = 0;
    for (int b = 0; b < 256; b++) {
        off[w * 257 + b] = acc;
        cursor[w * 256 + b] = acc;
        acc += cnt[w * 256 + b];
    }
    off[w * 257 + 256] = acc;
}
__global__ void k_msm_scatter(const uint8_t *digits, int n, uint32_t *cursor,
                              uint32_t *list /* 32*n */) {
    size_t total = (size_t)32 * n;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        size_t w = t / n;
        uint32_t slot = atomicAdd(&cursor[w * 256 + digits[t]], 1u);
        list[w * n + slot] = (uint32_t)(t - w * n);
    }
}
__global__ void __launch_bounds__(64) k_msm_buckets(
        const g1aff_t *pts, const uint32_t *list, const uint32_t *off, int n,
        g1_t *buckets /* 32*255 */) {
    int w = blockIdx.x / 255;
    int b = blockIdx.x % 255 + 1;
    uint32_t lo = off[w * 257 + b], hi = off[w * 257 + b + 1];
    g1_t acc;
    g1_set_inf(acc);
    for (uint32_t k = lo + threadIdx.x; k < hi; k += 64)
        g1_madd_i(acc, acc, pts[list[(size_t)w * n + k]]);
    __shared__ g1_t red[64];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            g1_t t;
            g1_add(t, red[threadIdx.x], red[threadIdx.x + s]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) buckets[w * 255 + b - 1] = red[0];
}

/* window reduction, parallelized (the serial 510-add suffix sum per window
 * was a 23 ms tail — profiles/r02_data/r2k_msm_kernels.txt).  Chunked:
 *   S_w = sum_b b*B_b = sum_c [ P_c + (lo_c - 1)*T_c ]
 * with P_c the chunk-local weighted suffix sum and T_c the chunk total;
 * (lo_c - 1) = 16c, and sum_c 16c*T_c = 16 * sum of T-suffix sums. */
__global__ void __launch_bounds__(64) k_msm_wreduce(const g1_t *buckets,
                                                    g1_t *chunkP, g1_t *chunkT) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;   /* 32 windows x 16 chunks */
    if (t >= 32 * 16) return;
    int w = t / 16, c = t % 16;
    int lo = c * 16 + 1;
    int hi = lo + 16 < 256 ? lo + 16 : 256;
    g1_t run, wsum;
    g1_set_inf(run);
    g1_set_inf(wsum);
    for (int b = hi - 1; b >= lo; b--) {
        g1_t t1;
        g1_add(t1, run, buckets[w * 255 + b - 1]);
        run = t1;
        g1_add(t1, wsum, run);
        wsum = t1;
    }
    chunkP[t] = wsum;
    chunkT[t] = run;
}
__global__ void __launch_bounds__(64) k_msm_wcombine(const g1_t *chunkP,
                                                     const g1_t *chunkT, g1_t *wsums) {
    int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 32) return;
    g1_t acc, t;
    g1_set_inf(acc);
    for (int c = 0; c < 16; c++) { g1_add(t, acc, chunkP[w * 16 + c]); acc = t; }
    g1_t run, ssum;
    g1_set_inf(run);
    g1_set_inf(ssum);
    for (int c = 15; c >= 1; c--) {
        g1_add(t, run, chunkT[w * 16 + c]);
        run = t;
        g1_add(t, ssum, run);
        ssum = t;
    }
    for (int d = 0; d < 4; d++) { g1_dbl(t, ssum); ssum = t; }   /* x16 */
    g1_add(t, acc, ssum);
    wsums[w] = t;
}
/* Horner combine, parallelized: each window shifts by its own 8w doublings
 * (longest chain 248, all windows concurrent), then one 32-add fold. */
__global__ void __launch_bounds__(64) k_msm_shift(const g1_t *wsums, g1_t *shifted) {
    int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 32) return;
    g1_t acc = wsums[w], t;
    for (int d = 0; d < 8 * w; d++) { g1_dbl(t, acc); acc = t; }
    shifted[w] = acc;
}
__global__ void k_msm_final(const g1_t *shifted, uint8_t *out48) {
    g1_t acc, t;
    g1_set_inf(acc);
    for (int w = 0; w < 32; w++) { g1_add(t, acc, shifted[w]); acc = t; }
    g1_serialize(out48, acc);
}

/* digits-only prep against an already-validated resident point table
 * (committee handle): the serialized-input entry below spends most of its
 * time decompressing + subgroup-checking points (~4.5k fp-muls each, same
 * cost the naive kernel pays) — production callers hold the committee
 * table resident (UpdateParticipants, quorum.go:326-334), so the MSM core
 * should be callable without re-validating points. */
__global__ void k_msm_digits(const uint8_t *scalars32, int n, uint8_t *digits,
                             int32_t *ok) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t k[4];
    if (!fr_from_le32(k, scalars32 + (size_t)i * 32)) {
        atomicExch(ok, 0);
        return;
    }
    for (int w = 0; w < 32; w++)
        digits[(size_t)w * n + i] = (uint8_t)(k[w >> 3] >> (8 * (w & 7)));
}

static int msm_core(const g1aff_t *d_pts, const uint8_t *d_digits, size_t n,
                    uint8_t *d_out48) {
    DevBuf dcnt(32 * 256 * 4), doff(32 * 257 * 4), dcur(32 * 256 * 4), dlist(n * 32 * 4);
    DevBuf dbuck(32 * 255 * sizeof(g1_t)), dws(32 * sizeof(g1_t));
    if (dcnt.err || doff.err || dcur.err || dlist.err || dbuck.err || dws.err)
        return HBLS_ERR;
    HIP_OK(hipMemset(dcnt.p, 0, 32 * 256 * 4));
    int nb_sc = (int)(((size_t)32 * n + 255) / 256);
    if (nb_sc > 4096) nb_sc = 4096;
    hipLaunchKernelGGL(k_msm_hist, dim3(nb_sc), dim3(256), 0, 0,
                       d_digits, (int)n, dcnt.as<uint32_t>());
    hipLaunchKernelGGL(k_msm_prefix, dim3(1), dim3(64), 0, 0,
                       dcnt.as<uint32_t>(), doff.as<uint32_t>(), dcur.as<uint32_t>());
    hipLaunchKernelGGL(k_msm_scatter, dim3(nb_sc), dim3(256), 0, 0,
                       d_digits, (int)n, dcur.as<uint32_t>(), dlist.as<uint32_t>());
    DevBuf dcp(32 * 16 * sizeof(g1_t)), dct(32 * 16 * sizeof(g1_t)), dsh(32 * sizeof(g1_t));
    if (dcp.err || dct.err || dsh.err) return HBLS_ERR;
    hipLaunchKernelGGL(k_msm_buckets, dim3(32 * 255), dim3(64), 0, 0,
                       d_pts, dlist.as<uint32_t>(), doff.as<uint32_t>(),
                       (int)n, dbuck.as<g1_t>());
    hipLaunchKernelGGL(k_msm_wreduce, dim3(8), dim3(64), 0, 0,
                       dbuck.as<g1_t>(), dcp.as<g1_t>(), dct.as<g1_t>());
    hipLaunchKernelGGL(k_msm_wcombine, dim3(1), dim3(64), 0, 0,
                       dcp.as<g1_t>(), dct.as<g1_t>(), dws.as<g1_t>());
    hipLaunchKernelGGL(k_msm_shift, dim3(1), dim3(64), 0, 0,
                       dws.as<g1_t>(), dsh.as<g1_t>());
    hipLaunchKernelGGL(k_msm_final, dim3(1), dim3(1), 0, 0,
                       dsh.as<g1_t>(), d_out48);
    HIP_OK(hipGetLastError());
    /* keep the intermediate buffers alive until the chain completes (hipFree
     * in ~DevBuf synchronizes, but be explicit about the dependency) */
    HIP_OK(hipDeviceSynchronize());
    return HBLS_OK;
}

/* MSM against the resident committee table: out = sum scalar_i * table[i].
 * Points were decompressed + subgroup-checked once at committee build. */
extern "C" int hbls_msm_g1_committee(const hbls_committee_t *c, const uint8_t *scalars32,
                                     uint8_t out48[48]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    size_t n = c->n;
    DevBuf ds(n * 32), ddig(n * 32), dok(4), dout(48);
    if (ds.err || ddig.err || dok.err || dout.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(ds.p, scalars32, n * 32, hipMemcpyHostToDevice));
    int32_t one = 1;
    HIP_OK(hipMemcpy(dok.p, &one, 4, hipMemcpyHostToDevice));
    Timer tm;
    hipLaunchKernelGGL(k_msm_digits, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, 0,
                       ds.as<uint8_t>(), (int)n, ddig.as<uint8_t>(), dok.as<int32_t>());
    rc = msm_core(c->d_table, ddig.as<uint8_t>(), n, dout.as<uint8_t>());
    tm.stop_and_store();
    if (rc != HBLS_OK) return rc;
    int32_t ok;
    HIP_OK(hipMemcpy(&ok, dok.p, 4, hipMemcpyDeviceToHost));
    if (!ok) return HBLS_ERR_BADINPUT;
    HIP_OK(hipMemcpy(out48, dout.p, 48, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_msm_g1(const uint8_t *points48, const uint8_t *scalars32, size_t n,
                           uint8_t out48[48]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (n == 0) return HBLS_ERR_BADINPUT;
    DevBuf dp(n * 48), ds(n * 32), dpts(n * sizeof(g1aff_t)), ddig(n * 32);
    DevBuf dok(4), dout(48);
    if (dp.err || ds.err || dpts.err || ddig.err || dok.err || dout.err)
        return HBLS_ERR;
    HIP_OK(hipMemcpy(dp.p, points48, n * 48, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(ds.p, scalars32, n * 32, hipMemcpyHostToDevice));
    int32_t one = 1;
    HIP_OK(hipMemcpy(dok.p, &one, 4, hipMemcpyHostToDevice));
    Timer tm;
    hipLaunchKernelGGL(k_msm_prep, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, 0,
                       dp.as<uint8_t>(), ds.as<uint8_t>(), (int)n,
                       dpts.as<g1aff_t>(), ddig.as<uint8_t>(), dok.as<int32_t>());
    rc = msm_core(dpts.as<g1aff_t>(), ddig.as<uint8_t>(), n, dout.as<uint8_t>());
    tm.stop_and_store();
    if (rc != HBLS_OK) return rc;
    HIP_OK(hipGetLastError());
    int32_t ok;
    HIP_OK(hipMemcpy(&ok, dok.p, 4, hipMemcpyDeviceToHost));
    if (!ok) return HBLS_ERR_BADINPUT;
    HIP_OK(hipMemcpy(out48, dout.p, 48, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* ---- fp_mul representation A/B microbenchmark ----
 * Variant 0: the shipping 6x64-limb CIOS (u128 accumulators).
 * Variant 1: 12x32-limb CIOS — every product is a 32x32+64 mad, the native
 *   v_mad_u64_u32 shape; more mads (288 vs 72 wider ones) but no carry
 *   juggling beyond the accumulator flow. */
DEV void fp_mul32(uint32_t r[12], const uint32_t a[12], const uint32_t b[12],
                  const uint32_t p32[12], uint32_t pinv32) {
    uint32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = 0;
    uint32_t t13 = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        uint64_t acc = 0;
        uint32_t ai = a[i];
#pragma unroll
        for (int j = 0; j < 12; j++) {
            acc = (uint64_t)ai * b[j] + t[j] + (uint32_t)(acc >> 32);
            t[j] = (uint32_t)acc;
        }
        acc = (uint64_t)t[12] + (uint32_t)(acc >> 32);
        t[12] = (uint32_t)acc;
        t13 = (uint32_t)(acc >> 32);
        uint32_t m = t[0] * pinv32;
        acc = (uint64_t)m * p32[0] + t[0];
#pragma unroll
        for (int j = 1; j < 12; j++) {
            acc = (uint64_t)m * p32[j] + t[j] + (uint32_t)(acc >> 32);
            t[j - 1] = (uint32_t)acc;
        }
        acc = (uint64_t)t[12] + (uint32_t)(acc >> 32);
        t[11] = (uint32_t)acc;
        t[12] = t13 + (uint32_t)(acc >> 32);
    }
    /* conditional subtract p */
    bool ge = t[12] != 0;
    if (!ge) {
        ge = true;
        for (int i = 11; i >= 0; i--) {
            if (t[i] > p32[i]) { ge = true; break; }
            if (t[i] < p32[i]) { ge = false; break; }
        }
    }
    if (ge) {
        uint64_t bw = 0;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            uint64_t d = (uint64_t)t[i] - p32[i] - (uint32_t)bw;
            r[i] = (uint32_t)d;
            bw = (d >> 32) & 1;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) r[i] = t[i];
    }
}
/* forceinline clone of the 12x32 CIOS — probes whether inlining the core
 * multiplier is safe/profitable before re-attempting it in the real kernels */
DEV void fp_mul32_fi(uint32_t r[12], const uint32_t a[12], const uint32_t b[12],
                     const uint32_t p32[12], uint32_t pinv32) {
    uint32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = 0;
    uint32_t t13 = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        uint64_t acc = 0;
        uint32_t ai = a[i];
#pragma unroll
        for (int j = 0; j < 12; j++) {
            acc = (uint64_t)ai * b[j] + t[j] + (uint32_t)(acc >> 32);
            t[j] = (uint32_t)acc;
        }
        acc = (uint64_t)t[12] + (uint32_t)(acc >> 32);
        t[12] = (uint32_t)acc;
        t13 = (uint32_t)(acc >> 32);
        uint32_t m = t[0] * pinv32;
        acc = (uint64_t)m * p32[0] + t[0];
#pragma unroll
        for (int j = 1; j < 12; j++) {
            acc = (uint64_t)m * p32[j] + t[j] + (uint32_t)(acc >> 32);
            t[j - 1] = (uint32_t)acc;
        }
        acc = (uint64_t)t[12] + (uint32_t)(acc >> 32);
        t[11] = (uint32_t)acc;
        t[12] = t13 + (uint32_t)(acc >> 32);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) r[i] = t[i];   /* skip cond-sub: timing probe */
    (void)p32;
}
/* variant 3: 12x32 CIOS with the outer row loop NOT unrolled (smaller code,
 * loop-carried schedule); variant 4: two rows interleaved per iteration. */
DEV void fp_mul32_noun(uint32_t r[12], const uint32_t a[12], const uint32_t b[12],
                       const uint32_t p32[12], uint32_t pinv32) {
    uint32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = 0;
    uint32_t t13 = 0;
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        uint64_t acc = 0;
        uint32_t ai = a[i];
#pragma unroll
        for (int j = 0; j < 12; j++) {
            acc = (uint64_t)ai * b[j] + t[j] + (uint32_t)(acc >> 32);
            t[j] = (uint32_t)acc;
        }
        acc = (uint64_t)t[12] + (uint32_t)(acc >> 32);
        t[12] = (uint32_t)acc;
        t13 = (uint32_t)(acc >> 32);
        uint32_t m = t[0] * pinv32;
        acc = (uint64_t)m * p32[0] + t[0];
#pragma unroll
        for (int j = 1; j < 12; j++) {
            acc = (uint64_t)m * p32[j] + t[j] + (uint32_t)(acc >> 32);
            t[j - 1] = (uint32_t)acc;
        }
        acc = (uint64_t)t[12] + (uint32_t)(acc >> 32);
        t[11] = (uint32_t)acc;
        t[12] = t13 + (uint32_t)(acc >> 32);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) r[i] = t[i];
    (void)p32;
}

/* variant 5: comba (product-scanning) interleaved Montgomery — every product
 * chains into ONE 64-bit accumulator via mad, with a carry-overflow counter
 * (96-bit column accumulator); no per-limb hi/lo pair shuffling. */
DEV void fp_mul32_comba(uint32_t r[13], const uint32_t a[12], const uint32_t b[12],
                        const uint32_t p32[12], uint32_t pinv32) {
    uint64_t acc = 0;
    uint32_t extra = 0;
    uint32_t m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            if (i <= k) {
                uint64_t nacc = acc + (uint64_t)a[i] * b[k - i];
                extra += (nacc < acc);
                acc = nacc;
            }
        }
#pragma unroll
        for (int i = 0; i < 12; i++) {
            if (i < k) {
                uint64_t nacc = acc + (uint64_t)m[i] * p32[k - i];
                extra += (nacc < acc);
                acc = nacc;
            }
        }
        uint32_t mk = (uint32_t)acc * pinv32;
        m[k] = mk;
        {
            uint64_t nacc = acc + (uint64_t)mk * p32[0];
            extra += (nacc < acc);
            acc = nacc;
        }
        acc = (acc >> 32) | ((uint64_t)extra << 32);
        extra = 0;
    }
#pragma unroll
    for (int k = 12; k < 24; k++) {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            if (i >= k - 11) {
                if (k - i < 12) {
                    uint64_t nacc = acc + (uint64_t)a[i] * b[k - i];
                    extra += (nacc < acc);
                    acc = nacc;
                    nacc = acc + (uint64_t)m[i] * p32[k - i];
                    extra += (nacc < acc);
                    acc = nacc;
                }
            }
        }
        r[k - 12] = (uint32_t)acc;
        acc = (acc >> 32) | ((uint64_t)extra << 32);
        extra = 0;
    }
    r[12] = (uint32_t)acc;
}

__global__ void __launch_bounds__(256) k_fpmul_bench(uint64_t *sink, int iters, int variant) {
    /* independent 4-chain per thread to expose ILP, like the real kernels */
    fp_t a, b;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a.l[i] = BLS_ONE_P[i] ^ (blockIdx.x * 256 + threadIdx.x);
        b.l[i] = BLS_R2P[i] ^ (i * 1234567u);
    }
    a.l[5] &= 0x0fffffffffffffffULL;
    b.l[5] &= 0x0fffffffffffffffULL;
    if (variant == 0) {
        fp_t x0 = a, x1 = b, x2 = a, x3 = b;
        for (int it = 0; it < iters; it++) {
            fp_mul_c(x0, x0, a);
            fp_mul_c(x1, x1, b);
            fp_mul_c(x2, x2, a);
            fp_mul_c(x3, x3, b);
        }
        if (x0.l[0] == 0xdeadbeef) sink[threadIdx.x] = x0.l[0] + x1.l[1] + x2.l[2] + x3.l[3];
    } else if (variant == 1) {
        uint32_t p32[12], a32[12], b32[12], x0[12], x1[12], x2[12], x3[12];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            p32[2 * i] = (uint32_t)BLS_P[i];
            p32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
            a32[2 * i] = (uint32_t)a.l[i];
            a32[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
            b32[2 * i] = (uint32_t)b.l[i];
            b32[2 * i + 1] = (uint32_t)(b.l[i] >> 32);
        }
        uint32_t pinv32 = (uint32_t)BLS_P_INV;   /* -p^-1 mod 2^32 = low word */
#pragma unroll
        for (int i = 0; i < 12; i++) { x0[i] = a32[i]; x1[i] = b32[i]; x2[i] = a32[i]; x3[i] = b32[i]; }
        for (int it = 0; it < iters; it++) {
            fp_mul32(x0, x0, a32, p32, pinv32);
            fp_mul32(x1, x1, b32, p32, pinv32);
            fp_mul32(x2, x2, a32, p32, pinv32);
            fp_mul32(x3, x3, b32, p32, pinv32);
        }
        if (x0[0] == 0xdeadbeef) sink[threadIdx.x] = x0[0] + x1[1] + x2[2] + x3[3];
    }
    if (variant == 6) {
        fp_t x0 = a, x1 = b, x2 = a, x3 = b;
        for (int it = 0; it < iters; it++) {
            fp_mul_asm(x0, x0, a);
            fp_mul_asm(x1, x1, b);
            fp_mul_asm(x2, x2, a);
            fp_mul_asm(x3, x3, b);
        }
        if (x0.l[0] == 0xdeadbeef) sink[threadIdx.x] = x0.l[0] + x1.l[1] + x2.l[2] + x3.l[3];
    }
    if (variant == 3) {
        uint32_t p32[12], a32[12], b32[12], x0[12], x1[12], x2[12], x3[12];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            p32[2 * i] = (uint32_t)BLS_P[i];
            p32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
            a32[2 * i] = (uint32_t)a.l[i];
            a32[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
            b32[2 * i] = (uint32_t)b.l[i];
            b32[2 * i + 1] = (uint32_t)(b.l[i] >> 32);
        }
        uint32_t pinv32 = (uint32_t)BLS_P_INV;
#pragma unroll
        for (int i = 0; i < 12; i++) { x0[i] = a32[i]; x1[i] = b32[i]; x2[i] = a32[i]; x3[i] = b32[i]; }
        for (int it = 0; it < iters; it++) {
            fp_mul32_noun(x0, x0, a32, p32, pinv32);
            fp_mul32_noun(x1, x1, b32, p32, pinv32);
            fp_mul32_noun(x2, x2, a32, p32, pinv32);
            fp_mul32_noun(x3, x3, b32, p32, pinv32);
        }
        if (x0[0] == 0xdeadbeef) sink[threadIdx.x] = x0[0] + x1[1] + x2[2] + x3[3];
    }
    if (variant == 5) {
        uint32_t p32[12], a32[12], b32[12], x0[13], x1[13], x2[13], x3[13];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            p32[2 * i] = (uint32_t)BLS_P[i];
            p32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
            a32[2 * i] = (uint32_t)a.l[i];
            a32[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
            b32[2 * i] = (uint32_t)b.l[i];
            b32[2 * i + 1] = (uint32_t)(b.l[i] >> 32);
        }
        uint32_t pinv32 = (uint32_t)BLS_P_INV;
#pragma unroll
        for (int i = 0; i < 12; i++) { x0[i] = a32[i]; x1[i] = b32[i]; x2[i] = a32[i]; x3[i] = b32[i]; }
        x0[12] = x1[12] = x2[12] = x3[12] = 0;
        for (int it = 0; it < iters; it++) {
            fp_mul32_comba(x0, x0, a32, p32, pinv32);
            fp_mul32_comba(x1, x1, b32, p32, pinv32);
            fp_mul32_comba(x2, x2, a32, p32, pinv32);
            fp_mul32_comba(x3, x3, b32, p32, pinv32);
        }
        if (x0[0] == 0xdeadbeef) sink[threadIdx.x] = x0[0] + x1[1] + x2[2] + x3[3];
    }
    if (variant == 2) {
        uint32_t p32[12], a32[12], b32[12], x0[12], x1[12], x2[12], x3[12];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            p32[2 * i] = (uint32_t)BLS_P[i];
            p32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
            a32[2 * i] = (uint32_t)a.l[i];
            a32[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
            b32[2 * i] = (uint32_t)b.l[i];
            b32[2 * i + 1] = (uint32_t)(b.l[i] >> 32);
        }
        uint32_t pinv32 = (uint32_t)BLS_P_INV;
#pragma unroll
        for (int i = 0; i < 12; i++) { x0[i] = a32[i]; x1[i] = b32[i]; x2[i] = a32[i]; x3[i] = b32[i]; }
        for (int it = 0; it < iters; it++) {
            fp_mul32_fi(x0, x0, a32, p32, pinv32);
            fp_mul32_fi(x1, x1, b32, p32, pinv32);
            fp_mul32_fi(x2, x2, a32, p32, pinv32);
            fp_mul32_fi(x3, x3, b32, p32, pinv32);
        }
        if (x0[0] == 0xdeadbeef) sink[threadIdx.x] = x0[0] + x1[1] + x2[2] + x3[3];
    }
}
/* asm-vs-C fp_mul equivalence: each thread runs a dependent chain through
 * both bodies on xorshift-derived inputs (< p via top-limb mask) and counts
 * bitwise mismatches at every step. */
__global__ void k_fpmul_asm_check(uint32_t *mism, int iters) {
    uint64_t s = 0x9e3779b97f4a7c15ULL * (blockIdx.x * 256 + threadIdx.x + 1);
    fp_t a, b;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17; a.l[i] = s;
        s ^= s << 13; s ^= s >> 7; s ^= s << 17; b.l[i] = s;
    }
    a.l[5] &= 0x19999999ffffffffULL;   /* < p: top 32-bit limb < 0x1a0111ea */
    b.l[5] &= 0x19999999ffffffffULL;
    fp_t xc = a, xa = a;
    uint32_t bad = 0;
    for (int it = 0; it < iters; it++) {
        fp_mul_c(xc, xc, b);
        fp_mul_asm(xa, xa, b);
#pragma unroll
        for (int i = 0; i < 6; i++) bad += (xc.l[i] != xa.l[i]);
        fp_mul_c(xc, xc, xc);
        fp_mul_asm(xa, xa, xa);
#pragma unroll
        for (int i = 0; i < 6; i++) bad += (xc.l[i] != xa.l[i]);
    }
    if (bad) atomicAdd(mism, bad);
}
/* returns mismatch count (-1 on launch failure); 0 = asm core bit-exact */
extern "C" long long hbls_fpmul_asm_check(void) {
    if (require_gpu() != HBLS_OK) return -1;
    DevBuf mism(4);
    if (mism.err) return -1;
    (void)hipMemset(mism.p, 0, 4);
    hipLaunchKernelGGL(k_fpmul_asm_check, dim3(512), dim3(256), 0, 0,
                       mism.as<uint32_t>(), 64);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    uint32_t h = 0;
    (void)hipMemcpy(&h, mism.p, 4, hipMemcpyDeviceToHost);
    return (long long)h;
}

/* measured fp_mul throughput (muls/s) for the given variant */
/* occupancy-sweep twin of the fp_mul µbench: 64-thread blocks so the host
 * can dial waves/SIMD exactly (de-risks the 1-wave register-file verify
 * kernel design — how much dependent-mad latency is exposed with no
 * co-resident waves when the stream is pure register VALU code?).
 * chains: number of independent 4-limb... independent mul chains per lane
 * (3 matches Karatsuba fp2_mul ILP, 1 is worst-case serial). */
__global__ void __launch_bounds__(64) k_fpmul_bench_w(uint64_t *sink, int iters, int chains) {
    fp_t a, b;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a.l[i] = BLS_ONE_P[i] ^ (blockIdx.x * 64 + threadIdx.x);
        b.l[i] = BLS_R2P[i] ^ (i * 1234567u);
    }
    a.l[5] &= 0x0fffffffffffffffULL;
    b.l[5] &= 0x0fffffffffffffffULL;
    uint32_t p32[12], a32[12], b32[12], x0[12], x1[12], x2[12], x3[12];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        p32[2 * i] = (uint32_t)BLS_P[i];
        p32[2 * i + 1] = (uint32_t)(BLS_P[i] >> 32);
        a32[2 * i] = (uint32_t)a.l[i];
        a32[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
        b32[2 * i] = (uint32_t)b.l[i];
        b32[2 * i + 1] = (uint32_t)(b.l[i] >> 32);
    }
    uint32_t pinv32 = (uint32_t)BLS_P_INV;
#pragma unroll
    for (int i = 0; i < 12; i++) { x0[i] = a32[i]; x1[i] = b32[i]; x2[i] = a32[i]; x3[i] = b32[i]; }
    if (chains == 4) {
        for (int it = 0; it < iters; it++) {
            fp_mul32(x0, x0, a32, p32, pinv32);
            fp_mul32(x1, x1, b32, p32, pinv32);
            fp_mul32(x2, x2, a32, p32, pinv32);
            fp_mul32(x3, x3, b32, p32, pinv32);
        }
    } else if (chains == 3) {
        for (int it = 0; it < iters; it++) {
            fp_mul32(x0, x0, a32, p32, pinv32);
            fp_mul32(x1, x1, b32, p32, pinv32);
            fp_mul32(x2, x2, a32, p32, pinv32);
        }
    } else if (chains == 5) {
        /* hand-allocated asm CIOS body inlined, 3 chains (the register-file
         * kernel's candidate multiplier; pinned regs serialize across
         * chains — measures the 1-wave issue-rate story) */
        fp_t y0 = a, y1 = b, y2 = a;
        for (int it = 0; it < iters; it++) {
            FP_MUL_ASM_BODY(y0, y0, a);
            FP_MUL_ASM_BODY(y1, y1, b);
            FP_MUL_ASM_BODY(y2, y2, a);
        }
        if (y0.l[0] == 0xdeadbeef) sink[threadIdx.x] = y0.l[0] + y1.l[1] + y2.l[2];
    } else if (chains == 6) {
        /* asm CIOS in called form, 3 chains */
        fp_t y0 = a, y1 = b, y2 = a;
        for (int it = 0; it < iters; it++) {
            fp_mul_asm(y0, y0, a);
            fp_mul_asm(y1, y1, b);
            fp_mul_asm(y2, y2, a);
        }
        if (y0.l[0] == 0xdeadbeef) sink[threadIdx.x] = y0.l[0] + y1.l[1] + y2.l[2];
    } else {
        for (int it = 0; it < iters; it++)
            fp_mul32(x0, x0, a32, p32, pinv32);
    }
    if (x0[0] == 0xdeadbeef) sink[threadIdx.x] = x0[0] + x1[1] + x2[2] + x3[3];
}

/* rate in mul/s at a chosen occupancy: blocks64 64-thread blocks in flight.
 * blocks64 = 1024 -> 1 wave/SIMD chip-wide, 8192 -> 8 waves/SIMD. */
extern "C" double hbls_fpmul_bench_waves(int blocks64, int chains) {
    if (require_gpu() != HBLS_OK) return 0.0;
    DevBuf sink(64 * 8);
    if (sink.err) return 0.0;
    int iters = 4000;
    int ch = chains;
    if (chains < 3) ch = 1; else if (chains == 4) ch = 4; else if (chains > 6) ch = 3;
    hipLaunchKernelGGL(k_fpmul_bench_w, dim3(blocks64), dim3(64), 0, 0,
                       sink.as<uint64_t>(), 200, ch);
    (void)hipDeviceSynchronize();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(k_fpmul_bench_w, dim3(blocks64), dim3(64), 0, 0,
                       sink.as<uint64_t>(), iters, ch);
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess) return 0.0;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    double muls_per_iter = (ch == 4) ? 4.0 : (ch == 1 ? 1.0 : 3.0);
    return (double)blocks64 * 64.0 * iters * muls_per_iter / (ms * 1e-3);
}

extern "C" double hbls_fpmul_bench_ops(int variant) {
    if (require_gpu() != HBLS_OK) return 0.0;
    DevBuf sink(256 * 8);
    if (sink.err) return 0.0;
    int blocks = 256 * 8, iters = 4000;
    hipLaunchKernelGGL(k_fpmul_bench, dim3(blocks), dim3(256), 0, 0,
                       sink.as<uint64_t>(), 200, variant);
    (void)hipDeviceSynchronize();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(k_fpmul_bench, dim3(blocks), dim3(256), 0, 0,
                       sink.as<uint64_t>(), iters, variant);
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess) return 0.0;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return (double)blocks * 256.0 * iters * 4.0 / (ms * 1e-3);
}

/* ---- VALU integer-MAD throughput microbenchmark ----
 * The hot path is wide-integer modular arithmetic: the roofline peak is the
 * device's 64x64->128 multiply-accumulate rate, which no datasheet quotes.
 * This kernel measures it: each thread runs UNROLL independent u128 mads per
 * iteration (the same primitive the CIOS fp_mul lowers to: v_mad_u64_u32
 * chains).  bench.py reports roofline.peak from this measured ceiling. */
__global__ void __launch_bounds__(256) k_mad_bench(uint64_t *sink, int iters) {
    uint64_t a0 = blockIdx.x * 256 + threadIdx.x + 1;
    uint64_t a1 = a0 * 2654435761u + 1;
    uint64_t a2 = a1 ^ 0x9e3779b97f4a7c15ull;
    uint64_t a3 = a2 + 12345;
    uint64_t b = a0 | 1;
    for (int it = 0; it < iters; it++) {
#pragma unroll 8
        for (int u = 0; u < 8; u++) {
            u128 p0 = (u128)a0 * b + a1;
            u128 p1 = (u128)a1 * b + a2;
            u128 p2 = (u128)a2 * b + a3;
            u128 p3 = (u128)a3 * b + a0;
            a0 = (uint64_t)p0 ^ (uint64_t)(p0 >> 64);
            a1 = (uint64_t)p1 ^ (uint64_t)(p1 >> 64);
            a2 = (uint64_t)p2 ^ (uint64_t)(p2 >> 64);
            a3 = (uint64_t)p3 ^ (uint64_t)(p3 >> 64);
        }
    }
    if (a0 == 0xdeadbeef) sink[threadIdx.x] = a0 + a1 + a2 + a3;  /* keep live */
    (void)sink;
}
/* returns measured 64x64->128 mad ops/sec (each inner op = one u128 mad) */
extern "C" double hbls_mad_peak_ops(void) {
    if (require_gpu() != HBLS_OK) return 0.0;
    DevBuf sink(256 * 8);
    if (sink.err) return 0.0;
    int blocks = 256 * 8;         /* 8 workgroups per CU */
    int iters = 2000;
    /* warmup */
    hipLaunchKernelGGL(k_mad_bench, dim3(blocks), dim3(256), 0, 0, sink.as<uint64_t>(), 100);
    (void)hipDeviceSynchronize();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(k_mad_bench, dim3(blocks), dim3(256), 0, 0, sink.as<uint64_t>(), iters);
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess) return 0.0;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    double total_ops = (double)blocks * 256.0 * (double)iters * 8.0 * 4.0;
    return total_ops / (ms * 1e-3);
}

/* config-4: local masked partial sums, serialized (one 48B point per item) */
extern "C" int hbls_mask_partials(const hbls_committee_t *c, const uint8_t *bitmaps,
                                  size_t batch, uint8_t *out48s) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    size_t bm = (c->n + 7) / 8;
    DevBuf dbm(batch * bm), dagg(batch * sizeof(g1_t)), dser(batch * 48);
    if (dbm.err || dagg.err || dser.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dbm.p, bitmaps, batch * bm, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    launch_mask_aggregate(c->d_table, (int)c->n, dbm.as<uint8_t>(), (int)bm,
                                         c->d_full_sum, dagg.as<g1_t>(), (int)batch,
                                         c->d_wtab, c->d_winf);
    hipLaunchKernelGGL(k_g1_serialize, dim3(nb), dim3(64), 0, 0,
                       dagg.as<g1_t>(), dser.as<uint8_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out48s, dser.p, batch * 48, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* config-4: aggregate-verify where this rank holds ONE SLICE of the
 * committee; ext48s carries the other ranks' per-item partial sums
 * (n_ext blocks of batch x 48 B, layout [ext][item]). */
extern "C" int hbls_batch_agg_verify_partials(
        const hbls_committee_t *c, const uint8_t *bitmaps,
        const uint8_t *ext48s, size_t n_ext,
        const uint8_t *sigs96, const uint8_t *msgs,
        size_t msg_len, size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    size_t bm = (c->n + 7) / 8;
    DevBuf dbm(batch * bm), dext(batch * 48 * (n_ext ? n_ext : 1));
    DevBuf dsig(batch * 96), dmsg(batch * msg_len);
    DevBuf dagg(batch * sizeof(g1_t)), dhm(batch * sizeof(g2_t));
    DevBuf dsaff(batch * sizeof(g2aff_t)), dsflags(batch * 4), dhok(batch * 4);
    DevBuf dres(batch * 4), dpok(batch * 4);
    if (dbm.err || dext.err || dsig.err || dmsg.err || dagg.err || dhm.err ||
        dsaff.err || dsflags.err || dhok.err || dres.err || dpok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dbm.p, bitmaps, batch * bm, hipMemcpyHostToDevice));
    if (n_ext)
        HIP_OK(hipMemcpy(dext.p, ext48s, batch * 48 * n_ext, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmsg.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    launch_mask_aggregate(c->d_table, (int)c->n, dbm.as<uint8_t>(), (int)bm,
                                         c->d_full_sum, dagg.as<g1_t>(), (int)batch,
                                         c->d_wtab, c->d_winf);
    if (n_ext)
        hipLaunchKernelGGL(k_add_partials, dim3(nb), dim3(64), 0, 0,
                           dagg.as<g1_t>(), dext.as<uint8_t>(), (int)n_ext,
                           dpok.as<int32_t>(), (int)batch);
    launch_hash_to_g2(dmsg.as<uint8_t>(), msg_len, dhm.as<g2_t>(), dhok.as<int32_t>(), batch);
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    launch_verify(dagg.as<g1_t>(), dhm.as<g2_t>(), dsaff.as<g2aff_t>(),
                  dsflags.as<int32_t>(), dhok.as<int32_t>(), dres.as<int32_t>(), batch);
    if (n_ext)
        hipLaunchKernelGGL(k_merge_pok, dim3(nb), dim3(64), 0, 0,
                           dres.as<int32_t>(), dpok.as<int32_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* sync-path batch seal verification (stagedstreamsync/sig_verify.go:23-59,
 * legacysync/syncing.go:857): each item is a raw commitSigAndBitmap blob
 * (96B sig || ceil(n/8)B bitmap, internal/chain/sig.go:22-35) plus its
 * commit payload; the raw blob window travels to HBM ONCE and is split
 * on-device (k_seal_split) — no host-side per-item copies (§8f-3). */
extern "C" int hbls_batch_seal_verify(const hbls_committee_t *c,
                                      const uint8_t *sig_bitmaps, size_t blob_len,
                                      const uint8_t *msgs, size_t msg_len,
                                      size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    size_t bm = (c->n + 7) / 8;
    if (blob_len != 96 + bm) return HBLS_ERR_BADINPUT;
    DevBuf dblob(batch * blob_len), dsig(batch * 96), dbm(batch * bm);
    DevBuf dmsg(batch * msg_len);
    if (dblob.err || dsig.err || dbm.err || dmsg.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dblob.p, sig_bitmaps, batch * blob_len, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmsg.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    size_t total = batch * blob_len;
    int nb = (int)((total + 255) / 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_seal_split, dim3(nb), dim3(256), 0, 0,
                       dblob.as<uint8_t>(), blob_len, bm,
                       dsig.as<uint8_t>(), dbm.as<uint8_t>(), batch);
    HIP_OK(hipGetLastError());
    return run_agg_verify_pipeline(c, dbm.as<uint8_t>(), dsig.as<uint8_t>(),
                                   dmsg.as<uint8_t>(), msg_len, batch, results);
}

/* ConstructCommitPayload (consensus/signature/signature.go:12-24):
 * LE64(blockNum) || blockHash(32) || [LE64(viewID) if staking].
 * Host-side byte assembly — returns payload length (40 or 48). */
extern "C" int hbls_construct_commit_payload(uint64_t block_num, const uint8_t hash32[32],
                                             uint64_t view_id, int staking, uint8_t out[48]) {
    for (int i = 0; i < 8; i++) out[i] = (uint8_t)(block_num >> (8 * i));
    memcpy(out + 8, hash32, 32);
    if (!staking) return 40;
    for (int i = 0; i < 8; i++) out[40 + i] = (uint8_t)(view_id >> (8 * i));
    return 48;
}
/* ParseCommitSigAndBitmap (internal/chain/sig.go:22-35): payload = 96B sig || bitmap.
 * Returns bitmap length, or HBLS_ERR_BADINPUT if payload < 96 bytes. */
extern "C" int hbls_parse_commit_sig_bitmap(const uint8_t *payload, size_t len,
                                            uint8_t sig96[96], uint8_t *bitmap,
                                            size_t bitmap_cap) {
    if (len < 96) return HBLS_ERR_BADINPUT;
    size_t bl = len - 96;
    if (bl > bitmap_cap) return HBLS_ERR_BADINPUT;
    memcpy(sig96, payload, 96);
    memcpy(bitmap, payload + 96, bl);
    return (int)bl;
}

/* AggregateSig batch form: out = sum of n serialized signatures */
extern "C" int hbls_g2_aggregate(const uint8_t *sigs96, size_t n, uint8_t out96[96]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf ds(n * 96), dout(96), dok(4);
    if (ds.err || dout.err || dok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(ds.p, sigs96, n * 96, hipMemcpyHostToDevice));
    int32_t one = 1;
    HIP_OK(hipMemcpy(dok.p, &one, 4, hipMemcpyHostToDevice));
    Timer tm;
    hipLaunchKernelGGL(k_g2_sum, dim3(1), dim3(64), 0, 0,
                       ds.as<uint8_t>(), (int)n, dout.as<uint8_t>(), dok.as<int32_t>());
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    int32_t ok;
    HIP_OK(hipMemcpy(&ok, dok.p, 4, hipMemcpyDeviceToHost));
    if (!ok) return HBLS_ERR_BADINPUT;
    HIP_OK(hipMemcpy(out96, dout.p, 96, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_hash_edge_count(void) {
    int32_t v = -1;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_cv_edge_count), 4) != hipSuccess) return -1;
    return v;
}
extern "C" int hbls_hash_edge_reset(void) {
    int32_t z = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_cv_edge_count), &z, 4) == hipSuccess ? 1 : 0;
}
extern "C" int hbls_coop_selftest(void) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return -100;
    DevBuf dout(4);
    if (dout.err) return -101;
    int32_t zero = 0;
    HIP_OK(hipMemcpy(dout.p, &zero, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_coop_selftest, dim3(1), dim3(64), 0, 0, dout.as<int32_t>());
    if (hipDeviceSynchronize() != hipSuccess) return -102;
    int32_t bad;
    HIP_OK(hipMemcpy(&bad, dout.p, 4, hipMemcpyDeviceToHost));
    return bad;
}

extern "C" int hbls_batch_keccak256(const uint8_t *msgs, size_t msg_len, size_t batch,
                                    uint8_t *out32s) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dm(batch * msg_len), dout(batch * 32);
    if (dm.err || dout.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dm.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_keccak, dim3(nb), dim3(64), 0, 0,
                       dm.as<uint8_t>(), (int)msg_len, dout.as<uint8_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out32s, dout.p, batch * 32, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* ======================== device-resident vote stream ========================
 * Config-5 streaming FBFT rounds (consensus/leader.go:221-309 per-message
 * loop) as a DEVICE-RESIDENT context: the committee table, per-round
 * hash-to-G2 points, participation bitmaps and running G2 aggregates all
 * live in HBM; one tick = one upload (key/round indices + signatures), a
 * fixed launch chain (decompress -> verify -> dedup -> per-round
 * accumulate), one 4B/vote download.  This replaces the round-1 python
 * shape (per-call copies + per-round k_g2_sum launches) that capped the
 * stream at ~3.4k msgs/s. */

struct hbls_stream {
    const hbls_committee_t *c;
    int max_rounds;
    int nwords;           /* committee bitmap words (32-bit) per round */
    g2_t *d_hm;           /* per-round hash point */
    int32_t *d_hm_ok;
    uint32_t *d_bitmap;   /* max_rounds x nwords, little-endian bit order */
    g2_t *d_agg;          /* per-round aggregate signature (jacobian) */
    /* async check lane: the periodic window checks (a latency-bound
     * 1-block pairing for <=16 rounds) run on their own HIP stream against
     * SNAPSHOTS of the rounds' state, overlapping the next ticks */
    hipStream_t check_stream;
    uint8_t *ck_bm;       /* snapshots + scratch, sized max_rounds */
    g2_t *ck_hm;
    int32_t *ck_hok;
    g2aff_t *ck_saff;
    int32_t *ck_sflags;
    g1_t *ck_agg;
    int32_t *ck_res;
    uint32_t *ck_slots;
    int ck_pending;       /* rounds in the in-flight check (0 = none) */
    int verify_mode;      /* 0 per-item (default), 1 random-combination batched */
};

__global__ void k_stream_reset(uint32_t *bitmap, g2_t *agg, const uint32_t *slots,
                               int k, int nwords) {
    int s = blockIdx.x;
    if (s >= k) return;
    uint32_t r = slots[s];
    for (int w = threadIdx.x; w < nwords; w += blockDim.x)
        bitmap[(size_t)r * nwords + w] = 0;
    if (threadIdx.x == 0) g2_set_inf(agg[r]);
}

/* scatter freshly hashed round payloads into the per-round slots */
__global__ void k_stream_scatter_hm(g2_t *hm, int32_t *hm_ok, const g2_t *src,
                                    const int32_t *src_ok, const uint32_t *slots, int k) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= k) return;
    hm[slots[s]] = src[s];
    hm_ok[slots[s]] = src_ok[s];
}

/* round-index validation + clamp (an OOB round index must not fault the
 * verify kernel's hm gather; flagged items report HBLS_ERR_BADINPUT) */
__global__ void k_stream_clamp(const uint32_t *round_idx, int max_rounds,
                               uint32_t *clamped, int32_t *okflag, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    uint32_t r = round_idx[i];
    int ok = r < (uint32_t)max_rounds;
    clamped[i] = ok ? r : 0;
    okflag[i] = ok;
}

/* dedup: first valid vote per (round, key) wins the bitmap bit; later valid
 * votes become result=2 (valid duplicate — the reference's quorum dedup,
 * quorum.go:354-394; within one tick the winner is unordered, as the
 * reference's concurrent pubsub validators are). */
__global__ void k_stream_dedup(uint32_t *bitmap, int nwords, const uint32_t *key_idx,
                               const uint32_t *round_idx, int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    if (results[i] != 1) return;
    uint32_t k = key_idx[i], r = round_idx[i];
    uint32_t bit = 1u << (k & 31);
    uint32_t old = atomicOr(&bitmap[(size_t)r * nwords + (k >> 5)], bit);
    if (old & bit) results[i] = 2;
}

/* per-round accumulate of accepted signatures: one 64-thread block per
 * active round slot, strided G2 adds + LDS tree (k_g2_sum shape), folded
 * into the resident aggregate. */
__global__ void __launch_bounds__(64) k_stream_accum(
        g2_t *agg, const uint32_t *slots, int kslots, const uint32_t *round_idx,
        const g2aff_t *sigs, const int32_t *results, int batch) {
    int s = blockIdx.x;
    if (s >= kslots) return;
    uint32_t r = slots[s];
    __shared__ g2_t red[64];
    g2_t acc;
    g2_set_inf(acc);
    for (int i = threadIdx.x; i < batch; i += 64) {
        if (round_idx[i] == r && results[i] == 1) {
            g2_t q;
            g2_from_affine(q, sigs[i]);
            g2_add(acc, acc, q);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            g2_t t;
            g2_add(t, red[threadIdx.x], red[threadIdx.x + st]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        g2_t t;
        g2_add(t, agg[r], red[0]);
        agg[r] = t;
    }
}

/* gather per-round check inputs: byte bitmaps (the word array IS the LE
 * byte layout), hm points, and the aggregate as affine + inf flag */
__global__ void k_stream_gather_check(const uint32_t *bitmap, int nwords, int bmbytes,
                                      const g2_t *hm, const int32_t *hm_ok,
                                      const g2_t *agg, const uint32_t *slots, int k,
                                      uint8_t *bm_out, g2_t *hm_out, int32_t *hmok_out,
                                      g2aff_t *sig_out, int32_t *sflags_out) {
    int s = blockIdx.x;
    if (s >= k) return;
    uint32_t r = slots[s];
    const uint8_t *src = (const uint8_t *)(bitmap + (size_t)r * nwords);
    for (int j = threadIdx.x; j < bmbytes; j += blockDim.x)
        bm_out[(size_t)s * bmbytes + j] = src[j];
    if (threadIdx.x == 0) {
        hm_out[s] = hm[r];
        hmok_out[s] = hm_ok[r];
        g2_t a = agg[r];
        if (g2_is_inf(a)) {
            sflags_out[s] = 2;
        } else {
            sflags_out[s] = 1;
            g2_to_affine(sig_out[s], a);
        }
    }
}

#include "hbls_rlc.inc"
#include "hbls_aggrlc.inc"
#include "hbls_quorum.inc"
#include "hbls_ctxset.inc"
#include "hbls_multikey.inc"
#include "hbls_msgs.inc"
#include "hbls_probe.inc"

extern "C" void hbls_stream_free(hbls_stream *s);

extern "C" hbls_stream *hbls_stream_create(const hbls_committee_t *c, int max_rounds) {
    if (require_gpu() != HBLS_OK || !c || max_rounds <= 0) return nullptr;
    hbls_stream *s = new hbls_stream();
    s->c = c;
    s->max_rounds = max_rounds;
    s->nwords = (int)((c->n + 31) / 32);
    size_t R = (size_t)max_rounds;
    if (hipMalloc(&s->d_hm, R * sizeof(g2_t)) != hipSuccess ||
        hipMalloc(&s->d_hm_ok, R * 4) != hipSuccess ||
        hipMalloc(&s->d_bitmap, R * s->nwords * 4) != hipSuccess ||
        hipMalloc(&s->d_agg, R * sizeof(g2_t)) != hipSuccess) {
        hbls_stream_free(s);
        return nullptr;
    }
    (void)hipMemset(s->d_hm_ok, 0, R * 4);
    (void)hipMemset(s->d_bitmap, 0, R * s->nwords * 4);
    /* aggregates start at the identity */
    std::vector<uint32_t> all(R);
    for (size_t i = 0; i < R; i++) all[i] = (uint32_t)i;
    DevBuf dslots(R * 4);
    if (dslots.err) { hbls_stream_free(s); return nullptr; }
    (void)hipMemcpy(dslots.p, all.data(), R * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_stream_reset, dim3((uint32_t)R), dim3(64), 0, 0,
                       s->d_bitmap, s->d_agg, dslots.as<uint32_t>(), (int)R, s->nwords);
    size_t bm = (c->n + 7) / 8;
    if (hipStreamCreate(&s->check_stream) != hipSuccess ||
        hipMalloc(&s->ck_bm, R * bm) != hipSuccess ||
        hipMalloc(&s->ck_hm, R * sizeof(g2_t)) != hipSuccess ||
        hipMalloc(&s->ck_hok, R * 4) != hipSuccess ||
        hipMalloc(&s->ck_saff, R * sizeof(g2aff_t)) != hipSuccess ||
        hipMalloc(&s->ck_sflags, R * 4) != hipSuccess ||
        hipMalloc(&s->ck_agg, R * sizeof(g1_t)) != hipSuccess ||
        hipMalloc(&s->ck_res, R * 4) != hipSuccess ||
        hipMalloc(&s->ck_slots, R * 4) != hipSuccess) {
        hbls_stream_free(s);
        return nullptr;
    }
    s->ck_pending = 0;
    s->verify_mode = 0;
    if (hipDeviceSynchronize() != hipSuccess) { hbls_stream_free(s); return nullptr; }
    return s;
}

extern "C" void hbls_stream_free(hbls_stream *s) {
    if (!s) return;
    if (s->check_stream) {
        (void)hipStreamSynchronize(s->check_stream);
        (void)hipStreamDestroy(s->check_stream);
    }
    if (s->d_hm) (void)hipFree(s->d_hm);
    if (s->d_hm_ok) (void)hipFree(s->d_hm_ok);
    if (s->d_bitmap) (void)hipFree(s->d_bitmap);
    if (s->d_agg) (void)hipFree(s->d_agg);
    if (s->ck_bm) (void)hipFree(s->ck_bm);
    if (s->ck_hm) (void)hipFree(s->ck_hm);
    if (s->ck_hok) (void)hipFree(s->ck_hok);
    if (s->ck_saff) (void)hipFree(s->ck_saff);
    if (s->ck_sflags) (void)hipFree(s->ck_sflags);
    if (s->ck_agg) (void)hipFree(s->ck_agg);
    if (s->ck_res) (void)hipFree(s->ck_res);
    if (s->ck_slots) (void)hipFree(s->ck_slots);
    delete s;
}

/* (re)open round slots: hash the payloads on device (one batched launch),
 * clear bitmaps + aggregates.  payloads: k x plen bytes. */
extern "C" int hbls_stream_set_rounds(hbls_stream *s, const uint32_t *slots, int k,
                                      const uint8_t *payloads, size_t plen) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (k <= 0 || k > s->max_rounds) return HBLS_ERR_BADINPUT;
    for (int i = 0; i < k; i++)
        if (slots[i] >= (uint32_t)s->max_rounds) return HBLS_ERR_BADINPUT;
    DevBuf dslots(k * 4), dpl((size_t)k * plen), dhm(k * sizeof(g2_t)), dok(k * 4);
    if (dslots.err || dpl.err || dhm.err || dok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dslots.p, slots, k * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dpl.p, payloads, (size_t)k * plen, hipMemcpyHostToDevice));
    Timer tm;
    /* exception: the cooperative hash whatever the threshold */
    launch_hash_to_g2_coop(dpl.as<uint8_t>(), plen, dhm.as<g2_t>(), dok.as<int32_t>(), (size_t)k);
    hipLaunchKernelGGL(k_stream_scatter_hm, dim3((k + 63) / 64), dim3(64), 0, 0,
                       s->d_hm, s->d_hm_ok, dhm.as<g2_t>(), dok.as<int32_t>(),
                       dslots.as<uint32_t>(), k);
    hipLaunchKernelGGL(k_stream_reset, dim3(k), dim3(64), 0, 0,
                       s->d_bitmap, s->d_agg, dslots.as<uint32_t>(), k, s->nwords);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    return HBLS_OK;
}

/* one tick: verify a batch of votes against (key_idx, round_idx), dedup via
 * the resident bitmaps, fold accepted signatures into the resident
 * aggregates.  results per vote: 1 accepted, 2 valid duplicate, 0 invalid
 * signature, HBLS_ERR_BADINPUT malformed.  active_slots: the distinct round
 * slots present in this batch (hosts know; keeps the accumulate launch
 * exact). */
extern "C" int hbls_stream_process(hbls_stream *s, const uint32_t *key_idx,
                                   const uint32_t *round_idx, const uint8_t *sigs96,
                                   const uint32_t *active_slots, int n_active,
                                   size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    rlc_stats_reset();
    if (batch == 0 || n_active <= 0) return HBLS_ERR_BADINPUT;
    if (s->verify_mode == 1 && batch > RLC_MAX_ITEMS) return HBLS_ERR_BADINPUT;
    for (int i = 0; i < n_active; i++)
        if (active_slots[i] >= (uint32_t)s->max_rounds) return HBLS_ERR_BADINPUT;
    DevBuf didx(batch * 4), dridx(batch * 4), dsig(batch * 96);
    DevBuf dclamp(batch * 4), dpok(batch * 4);
    DevBuf dsaff(batch * sizeof(g2aff_t)), dsflags(batch * 4), dres(batch * 4);
    DevBuf dact(n_active * 4);
    RfGather rfg(batch);
    if (didx.err || dridx.err || dsig.err || dclamp.err || dpok.err ||
        dsaff.err || dsflags.err || dres.err || dact.err || rfg.err()) return HBLS_ERR;
    HIP_OK(hipMemcpy(didx.p, key_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dridx.p, round_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dact.p, active_slots, n_active * 4, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_stream_clamp, dim3(nb), dim3(64), 0, 0,
                       dridx.as<uint32_t>(), s->max_rounds,
                       dclamp.as<uint32_t>(), dpok.as<int32_t>(), (int)batch);
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    if (s->verify_mode == 1) {
        /* batched: one pairing per round slot present in the tick, grouped
         * by the clamped round index (never by active_slots) */
        rc = rlc_verify_chain(s->c, s->d_hm, s->d_hm_ok, (size_t)s->max_rounds, round_idx,
                              didx.as<uint32_t>(), dclamp.as<uint32_t>(), dpok.as<int32_t>(),
                              dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), dres.as<int32_t>(),
                              batch);
        if (rc != HBLS_OK) { tm.stop_and_store(); return rc; }
    } else {
        launch_verify_votes(s->c->d_table, s->c->n, didx.as<uint32_t>(), s->d_hm,
                            dclamp.as<uint32_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(),
                            s->d_hm_ok, dres.as<int32_t>(), batch, rfg);
    }
    hipLaunchKernelGGL(k_merge_pok, dim3(nb), dim3(64), 0, 0,
                       dres.as<int32_t>(), dpok.as<int32_t>(), (int)batch);
    hipLaunchKernelGGL(k_stream_dedup, dim3(nb), dim3(64), 0, 0,
                       s->d_bitmap, s->nwords, didx.as<uint32_t>(),
                       dclamp.as<uint32_t>(), dres.as<int32_t>(), (int)batch);
    hipLaunchKernelGGL(k_stream_accum, dim3(n_active), dim3(64), 0, 0,
                       s->d_agg, dact.as<uint32_t>(), n_active, dclamp.as<uint32_t>(),
                       dsaff.as<g2aff_t>(), dres.as<int32_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* pairing-check the given rounds' resident aggregates against their
 * resident masks (validator.go:224-228 shape).  ok[i]: 1/0. */
extern "C" int hbls_stream_check(hbls_stream *s, const uint32_t *slots, int k,
                                 int32_t *ok) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (k <= 0) return HBLS_ERR_BADINPUT;
    for (int i = 0; i < k; i++)
        if (slots[i] >= (uint32_t)s->max_rounds) return HBLS_ERR_BADINPUT;
    size_t bm = (s->c->n + 7) / 8;
    DevBuf dslots(k * 4), dbm((size_t)k * bm), dhm(k * sizeof(g2_t)), dhok(k * 4);
    DevBuf dsaff(k * sizeof(g2aff_t)), dsflags(k * 4);
    DevBuf dagg(k * sizeof(g1_t)), dres(k * 4);
    if (dslots.err || dbm.err || dhm.err || dhok.err || dsaff.err ||
        dsflags.err || dagg.err || dres.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dslots.p, slots, k * 4, hipMemcpyHostToDevice));
    Timer tm;
    hipLaunchKernelGGL(k_stream_gather_check, dim3(k), dim3(64), 0, 0,
                       s->d_bitmap, s->nwords, (int)bm, s->d_hm, s->d_hm_ok,
                       s->d_agg, dslots.as<uint32_t>(), k,
                       dbm.as<uint8_t>(), dhm.as<g2_t>(), dhok.as<int32_t>(),
                       dsaff.as<g2aff_t>(), dsflags.as<int32_t>());
    launch_mask_aggregate(s->c->d_table, (int)s->c->n, dbm.as<uint8_t>(), (int)bm,
                          s->c->d_full_sum, dagg.as<g1_t>(), k,
                          s->c->d_wtab, s->c->d_winf);
    launch_verify(dagg.as<g1_t>(), dhm.as<g2_t>(), dsaff.as<g2aff_t>(),
                  dsflags.as<int32_t>(), dhok.as<int32_t>(), dres.as<int32_t>(), (size_t)k);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(ok, dres.p, k * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* async window check: snapshot the rounds' state on the DEFAULT stream
 * (ordered after the ticks that built it), then run the latency-bound
 * mask+pairing chain on a dedicated HIP stream so it overlaps subsequent
 * ticks.  Poll with hbls_stream_check_poll; at most one check in flight. */
extern "C" int hbls_stream_check_submit(hbls_stream *s, const uint32_t *slots, int k) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (k <= 0 || k > s->max_rounds || s->ck_pending) return HBLS_ERR_BADINPUT;
    for (int i = 0; i < k; i++)
        if (slots[i] >= (uint32_t)s->max_rounds) return HBLS_ERR_BADINPUT;
    size_t bm = (s->c->n + 7) / 8;
    HIP_OK(hipMemcpy(s->ck_slots, slots, k * 4, hipMemcpyHostToDevice));
    /* snapshot on stream 0 (after the ticks) into the persistent ck_* bufs */
    hipLaunchKernelGGL(k_stream_gather_check, dim3(k), dim3(64), 0, 0,
                       s->d_bitmap, s->nwords, (int)bm, s->d_hm, s->d_hm_ok,
                       s->d_agg, s->ck_slots, k,
                       s->ck_bm, s->ck_hm, s->ck_hok, s->ck_saff, s->ck_sflags);
    hipEvent_t ev;
    HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(ev, 0));
    HIP_OK(hipStreamWaitEvent(s->check_stream, ev, 0));
    (void)hipEventDestroy(ev);
    launch_mask_aggregate(s->c->d_table, (int)s->c->n, s->ck_bm, (int)bm,
                          s->c->d_full_sum, s->ck_agg, k,
                          s->c->d_wtab, s->c->d_winf, s->check_stream);
    /* exception: always the 16-item cooperative kernel, on the check's own stream */
    hipLaunchKernelGGL(k_verify_coop<16>, dim3((k + CV_ITEMS - 1) / CV_ITEMS), dim3(64), 0,
                       s->check_stream,
                       s->ck_agg, s->ck_hm, s->ck_saff,
                       s->ck_sflags, s->ck_hok, s->ck_res, k);
    HIP_OK(hipGetLastError());
    s->ck_pending = k;
    return HBLS_OK;
}

/* wait for the in-flight check and return its per-round verdicts.
 * ok must hold at least the submitted k entries; returns that k. */
extern "C" int hbls_stream_check_poll(hbls_stream *s, int32_t *ok) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!s->ck_pending) return 0;
    HIP_OK(hipStreamSynchronize(s->check_stream));
    int k = s->ck_pending;
    HIP_OK(hipMemcpy(ok, s->ck_res, k * 4, hipMemcpyDeviceToHost));
    s->ck_pending = 0;
    return k;
}

/* export one round's state: byte bitmap + serialized aggregate (the shape
 * consensus_service.go:305-322 signs into the block) */
extern "C" int hbls_stream_get(hbls_stream *s, uint32_t slot, uint8_t *bitmap_out,
                               uint8_t agg96_out[96]) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (slot >= (uint32_t)s->max_rounds) return HBLS_ERR_BADINPUT;
    size_t bm = (s->c->n + 7) / 8;
    HIP_OK(hipMemcpy(bitmap_out, (uint8_t *)(s->d_bitmap + (size_t)slot * s->nwords),
                     bm, hipMemcpyDeviceToHost));
    DevBuf dser(96), dok(4);
    if (dser.err || dok.err) return HBLS_ERR;
    int32_t one = 1;
    HIP_OK(hipMemcpy(dok.p, &one, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_g2_serialize, dim3(1), dim3(64), 0, 0,
                       s->d_agg + slot, dser.as<uint8_t>(), dok.as<int32_t>(), 1);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(agg96_out, dser.p, 96, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_mulcount_reset(void) {
#ifdef HBLS_COUNT_MULS
    unsigned long long z = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_fp_mul_count), &z, 8) == hipSuccess ? 1 : 0;
#else
    return 0;
#endif
}
extern "C" unsigned long long hbls_mulcount_read(void) {
#ifdef HBLS_COUNT_MULS
    unsigned long long v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_fp_mul_count), 8) != hipSuccess) return 0;
    return v;
#else
    return 0;
#endif
}

extern "C" int hbls_has_rf(void) {
#ifdef HBLS_RF
    return 1;
#else
    return 0;
#endif
}
