/* hbls_aggrlc.inc — one final exponentiation per chunk of aggregate-verify
 * items (included from hbls_dev.hip after hbls_rlc.inc).
 *
 * Every item of hbls_batch_agg_verify is its own two-leg pairing check
 *       e(aggpk_i, H_i) * e(-G1, sig_i) == 1
 * and the final exponentiation FE is a homomorphism onto the order-r group,
 * so for secret nonzero 64-bit scalars r_i
 *       FE( prod_i f_{u,H_i}(r_i*aggpk_i) * f_{u,sig_i}(r_i*(-G1)) ) == 1
 * holds when every item of the chunk verifies and fails except with
 * probability ~2^-64 when one does not (each factor is the item's pairing
 * product raised to r_i; all points lie in the prime-order subgroups: the
 * committee build checks the keys, the decompress checks the signatures, the
 * hash point is cofactor-cleared).  The per-item Miller loop stays at full
 * occupancy; the final exponentiation runs once per AGGRLC_CHUNK items.
 *
 * Accept/reject parity with the per-item kernel is by construction: items
 * that k_verify classifies without a pairing get that classification here
 * and enter no product, and the eligible items of a failing chunk are
 * re-checked by the exact per-item pairing (k_verify_sel). */

#define AGGRLC_CHUNK 64         /* items per product == threads per block */
#define AGGRLC_WINDOWS 8        /* 8-bit windows of a 64-bit scalar */

/* ---- the signature leg once per chunk (DESIGN.md §4k).  The pairing is
 * bilinear, so after the final exponentiation the signature factors of a
 * chunk multiply to e(-G1, S_c) with S_c = sum_i r_i*sig_i: one Miller leg on
 * S_c per chunk replaces one per item.  The group element checked is the
 * same as above, so is the soundness argument.  Each item pays a 64-bit G2
 * scalar multiplication (k_aggrlc_sigscale) and a G2 addition in a tree
 * (k_aggrlc_sigsum) instead; its own Miller loop keeps one leg. */

/* signed 4-bit digits of a 64-bit scalar: k = sum_j d_j 16^j, j = 0..16,
 * -8 <= d_j <= 8.  mag holds |d_0|..|d_15| as nibbles, neg their signs as
 * bits, top is d_16 (0 or 1: the carry out of the last window).  A window
 * value above 8 becomes value-16 with a carry; exactly 8 goes to -8 with a
 * carry when the next window carries anyway (its nibble is 8 or more) and
 * stays +8 otherwise. */
DEV void aggrlc_recode64(uint64_t k, uint64_t &mag, uint32_t &neg, uint32_t &top) {
    uint32_t c = 0;
    mag = 0; neg = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        uint32_t v = ((uint32_t)(k >> (4 * j)) & 15u) + c;
        uint32_t nx = j < 15 ? ((uint32_t)(k >> (4 * j + 4)) & 15u) : 0u;
        c = (v > 8u || (v == 8u && nx >= 8u)) ? 1u : 0u;
        uint32_t m = c ? 16u - v : v;
        mag |= (uint64_t)m << (4 * j);
        neg |= (c && m) ? (1u << j) : 0u;
    }
    top = c;
}

/* r = k*p for a 64-bit k, fixed 4-bit signed windows over a per-lane table
 * of 1p..8p: 64 doublings and at most 16 additions after the table's 4 + 3,
 * with control flow that depends on the scalar only through the "digit is
 * zero" skip — a wave of 64 independent scalars runs g1_mul's 63 additions,
 * here 16.  The same group element as g1_mul for every k, p = identity
 * included (g1_add and g1_dbl carry the identity and the doubling case).
 * One body for both groups, over the point type's double, add, negate-y and
 * set-identity. */
DEV void pt_dbl(g1_t &r, const g1_t &p) { g1_dbl(r, p); }
DEV void pt_dbl(g2_t &r, const g2_t &p) { g2_dbl(r, p); }
DEV void pt_add(g1_t &r, const g1_t &p, const g1_t &q) { g1_add(r, p, q); }
DEV void pt_add(g2_t &r, const g2_t &p, const g2_t &q) { g2_add(r, p, q); }
DEV void pt_neg_y(g1_t &p) { fp_neg(p.y, p.y); }
DEV void pt_neg_y(g2_t &p) { fp2_neg(p.y, p.y); }
DEV void pt_set_inf(g1_t &p) { g1_set_inf(p); }
DEV void pt_set_inf(g2_t &p) { g2_set_inf(p); }
template <typename PT> DEV void pt_mul64w(PT &r, const PT &p, uint64_t k) {
    PT tab[8];
    tab[0] = p;
    pt_dbl(tab[1], tab[0]);
    pt_add(tab[2], tab[1], tab[0]);
    pt_dbl(tab[3], tab[1]);
    pt_add(tab[4], tab[3], tab[0]);
    pt_dbl(tab[5], tab[2]);
    pt_add(tab[6], tab[5], tab[0]);
    pt_dbl(tab[7], tab[3]);
    uint64_t mag; uint32_t neg, top;
    aggrlc_recode64(k, mag, neg, top);
    PT acc;
    if (top) acc = p; else pt_set_inf(acc);
    for (int j = 15; j >= 0; j--) {
        for (int s = 0; s < 4; s++) pt_dbl(acc, acc);
        uint32_t m = (uint32_t)(mag >> (4 * j)) & 15u;
        if (m) {
            PT t = tab[m - 1];
            if ((neg >> j) & 1u) pt_neg_y(t);
            pt_add(acc, acc, t);
        }
    }
    r = acc;
}
DEVN void g1_mul64w(g1_t &r, const g1_t &p, uint64_t k) { pt_mul64w(r, p, k); }
DEVN void g2_mul64w(g2_t &r, const g2_t &p, uint64_t k) { pt_mul64w(r, p, k); }

/* f = f_{|z|,Q}(P): one leg of miller_loop2, the same homogeneous steps */
DEVN void miller_loop1_h(fp12_t &f, const g2aff_t &Q, const g1aff_t &P) {
    g2_t T;
    g2_from_affine(T, Q);
    fp2_t c0, c3, c5;
    fp12_one(f);
    for (int bit = 62; bit >= 0; bit--) {
        fp12_sqr(f, f);
        ml_dbl_step_h(T, P, c0, c3, c5);
        fp12_mul_line(f, c0, c3, c5);
        if ((BLS_U >> bit) & 1) {
            ml_add_step_h(T, Q, P, c0, c3, c5);
            fp12_mul_line(f, c0, c3, c5);
        }
    }
}

/* -G1, affine: the fixed G1 argument of every signature leg */
DEV void aggrlc_neg_g1(g1aff_t &P) {
    fp_load(P.x, BLS_G1_X);
    fp_t gy;
    fp_load(gy, BLS_G1_Y);
    fp_neg(P.y, gy);
}

/* p2[k] = 2^k * (-G1), affine (thread k: k doublings, one inversion): the
 * 64 "keys" whose 8-key subset sums (k_wtab_build_jac) are the fixed-base
 * window table of -G1 */
__global__ void k_aggrlc_pow2(g1aff_t *p2) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 64) return;
    g1aff_t n;
    aggrlc_neg_g1(n);
    g1_t p;
    p.x = n.x; p.y = n.y; fp_one(p.z);
    for (int j = 0; j < k; j++) g1_dbl(p, p);
    g1aff_t a;
    g1_to_affine(a, p);
    p2[k] = a;
}

/* ---- the verdict rule, in k_verify's guard order — the one place it is
 * written.  An item is bad input (hash or signature undecodable), decided
 * without a pairing (identity key sum or identity signature: the herumi
 * verdict, accepted only when both are), or eligible for the combined check;
 * `verdict` is what results[i] gets (for an eligible item the 1 that stands
 * unless its chunk fails and is re-checked).
 * pub == nullptr: the key sum does not exist yet (the hoisted schedule, ahead
 * of the mask kernel).  An identity signature then stays open, verdict
 * untouched, and a real one is eligible for now; the same function with the
 * key sum at hand closes both. */
enum { AGGRLC_CLS_BAD = 0, AGGRLC_CLS_DECIDED, AGGRLC_CLS_ELIGIBLE, AGGRLC_CLS_OPEN };
DEV int aggrlc_classify(int32_t hm_ok, int32_t sig_flag, const g1_t *pub, int32_t &verdict) {
    if (!hm_ok || sig_flag == 0) { verdict = HBLS_ERR_BADINPUT; return AGGRLC_CLS_BAD; }
    bool sig_inf = sig_flag == 2;
    if (!pub) {
        if (sig_inf) return AGGRLC_CLS_OPEN;
    } else {
        bool pub_inf = g1_is_inf(*pub);
        if (pub_inf || sig_inf) {
            verdict = (pub_inf && sig_inf) ? 1 : 0;   /* herumi edge */
            return AGGRLC_CLS_DECIDED;
        }
    }
    verdict = 1;
    return AGGRLC_CLS_ELIGIBLE;
}
/* the item's scalar: a drawn zero would drop the item from the product */
DEV uint64_t aggrlc_scalar(const uint64_t *scalars, size_t i) {
    uint64_t r = scalars[i];
    return r ? r : 1;
}

/* thread per item: verify_pairing up to (and without) the final
 * exponentiation, on the scaled G1 arguments.  elig: 0 classified here,
 * 1 f stored and part of its chunk's product, 2 needs the exact path (the
 * scaled key sum came out as the identity — impossible for subgroup keys,
 * kept so that no input can skip its pairing). */
__global__ void k_aggrlc_miller(const g1_t *aggpubs, const g2_t *hms, const g2aff_t *sigs,
                                const int32_t *sig_flags, const int32_t *hm_ok,
                                const uint64_t *scalars, const g1aff_t *gtab,
                                fp12_t *F, int32_t *elig, int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    fp12_t f;
    fp12_one(f);
    elig[i] = 0;
    int32_t v = 0;
    int cls = aggrlc_classify(hm_ok[i], sig_flags[i], aggpubs + i, v);
    results[i] = v;
    if (cls != AGGRLC_CLS_ELIGIBLE) { F[i] = f; return; }
    uint64_t r = aggrlc_scalar(scalars, i);
    g1_t A, C;
    g1_mul64w(A, aggpubs[i], r);
    g1_set_inf(C);
    for (int w = 0; w < AGGRLC_WINDOWS; w++) {
        uint32_t b = (uint32_t)(r >> (8 * w)) & 255u;
        if (b) g1_madd(C, C, gtab[w * 255 + b - 1]);
    }
    if (g1_is_inf(A) || g1_is_inf(C)) {
        elig[i] = 2; results[i] = 0; F[i] = f; return;
    }
    g1aff_t pa, ca;
    { fp_t t, ti, zi, zi2, zi3;          /* one inversion for both points */
      fp_mul(t, A.z, C.z);
      fp_inv(ti, t);
      fp_mul(zi, ti, C.z);
      fp_sqr(zi2, zi);
      fp_mul(zi3, zi2, zi);
      fp_mul(pa.x, A.x, zi2);
      fp_mul(pa.y, A.y, zi3);
      fp_mul(zi, ti, A.z);
      fp_sqr(zi2, zi);
      fp_mul(zi3, zi2, zi);
      fp_mul(ca.x, C.x, zi2);
      fp_mul(ca.y, C.y, zi3); }
    g2aff_t ha;
    g2_t hmc = hms[i];
    g2_to_affine(ha, hmc);
    miller_loop2(f, ha, pa, sigs[i], ca);
    F[i] = f;
    elig[i] = 1;
}

/* elig value of the hoisted schedule only (DESIGN.md §4l), between
 * k_aggrlc_sigscale<true> and k_aggrlc_item<true, *>: an identity signature
 * whose verdict waits for the key sum.  No later kernel sees it. */
#define AGGRLC_ELIG_OPEN 3

/* chunk-level signature leg, step 1 — thread per item: the classification
 * (aggpubs[i] is read for g1_is_inf only), then B_i = r_i*sig_i, Jacobian.
 * Classified items get elig 0 and B_i = identity, so the chunk sum needs no
 * flags.
 * HOISTED: the launch runs ahead of the mask kernel, so aggpubs does not
 * exist yet and is not read: an identity signature is left open
 * (AGGRLC_ELIG_OPEN, B_i = identity), an item with a real signature is scaled
 * whatever its key sum will be, and k_aggrlc_item<true, *> finishes both once
 * it has the key sums. */
template <bool HOISTED>
__global__ void k_aggrlc_sigscale(const g1_t *aggpubs, const g2aff_t *sigs,
                                  const int32_t *sig_flags, const int32_t *hm_ok,
                                  const uint64_t *scalars, g2_t *B, int32_t *elig,
                                  int32_t *results, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    g2_t b;
    g2_set_inf(b);
    int32_t v = 0;
    int cls = aggrlc_classify(hm_ok[i], sig_flags[i], HOISTED ? nullptr : aggpubs + i, v);
    if (cls != AGGRLC_CLS_OPEN) results[i] = v;
    if (cls != AGGRLC_CLS_ELIGIBLE) {
        elig[i] = cls == AGGRLC_CLS_OPEN ? AGGRLC_ELIG_OPEN : 0;
        B[i] = b; return;
    }
    g2_t s;
    g2_from_affine(s, sigs[i]);
    g2_mul64w(b, s, aggrlc_scalar(scalars, i));
    B[i] = b;
    elig[i] = 1;
}

/* step 2 — one block per chunk (k_rlc_chunk_sum's shape): LDS tree over the
 * chunk's B_i, then lane 0 stores S_c affine.  sflag[c]: 1 = S[c] is an
 * affine point, 0 = the sum is the identity (no eligible item, or signatures
 * that cancel): its pairing value is one and the chunk entry contributes one;
 * the chunk's verdict still comes from the items' own factors.
 * REPAIR (the hoisted schedule, after the Miller kernel): only the chunks
 * marked dirty are summed again, over the items that are still eligible —
 * the B_i of an item whose key sum turned out to be the identity drops out. */
template <bool REPAIR>
__global__ void __launch_bounds__(AGGRLC_CHUNK) k_aggrlc_sigsum(
        const g2_t *B, int batch, int nchunks, g2aff_t *S, int32_t *sflag,
        const int32_t *elig, const int32_t *dirty) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    if (REPAIR && !dirty[c]) return;            /* uniform over the block */
    __shared__ g2_t red[AGGRLC_CHUNK];
    size_t i = (size_t)c * AGGRLC_CHUNK + threadIdx.x;
    if (i < (size_t)batch && (!REPAIR || elig[i] != 0)) red[threadIdx.x] = B[i];
    else g2_set_inf(red[threadIdx.x]);
    __syncthreads();
    for (int s = AGGRLC_CHUNK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            g2_t t;
            g2_add(t, red[threadIdx.x], red[threadIdx.x + s]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        g2_t sum = red[0];
        if (g2_is_inf(sum)) {
            sflag[c] = 0;
        } else {
            g2aff_t a;
            g2_to_affine(a, sum);
            S[c] = a;
            sflag[c] = 1;
        }
    }
}

/* product of f over the 64 lanes of a wave, without LDS: six butterfly
 * rounds (partner lane ^ 1, 2, 4, 8, 16, 32), each an exchange of the 72
 * limbs and one multiplication in Fp12.  Every lane must be active.  Field
 * results are canonical and the product commutes, so after round k the 2^k
 * lanes of a group hold the same limbs and every lane ends with the wave's
 * product.
 * The first round is a whole fp12_mul per lane.  From the second round on
 * the four lanes of an aligned quad hold the same unordered pair {x, y}, so
 * the three Fp6 products of fp12_mul's Karatsuba step go one to a lane —
 * lane 0 of the quad x0 y0, lane 1 x1 y1, lanes 2 and 3 (x0+x1)(y0+y1), each
 * symmetric in x and y — and the quad reads them back: 18 fp-mul a round and
 * lane in place of 54.
 * Callers launch blocks of exactly 64 threads (blockDim.x == 64: the block is
 * one wave and threadIdx.x the lane), and the result relies on every field
 * operation returning the canonical representative below p, which the probe
 * test pins limb for limb. */
DEVN void fp12_wave_prod(fp12_t &f) {
    union { fp12_t v; uint32_t w[144]; } a, b;
    union { fp6_t v; uint32_t w[72]; } u, t0, t1, tt;
    a.v = f;
#pragma unroll
    for (int i = 0; i < 144; i++) b.w[i] = (uint32_t)__shfl_xor((int)a.w[i], 1, 64);
    fp12_mul(a.v, a.v, b.v);
    const int lane = (int)(threadIdx.x & 63u), role = lane & 3, quad = lane & ~3;
    for (int m = 2; m < 64; m <<= 1) {
#pragma unroll
        for (int i = 0; i < 144; i++) b.w[i] = (uint32_t)__shfl_xor((int)a.w[i], m, 64);
        fp6_t p, q;
        fp6_add(p, a.v.c0, a.v.c1);
        fp6_add(q, b.v.c0, b.v.c1);
        if (role == 0) { p = a.v.c0; q = b.v.c0; }
        if (role == 1) { p = a.v.c1; q = b.v.c1; }
        fp6_mul(u.v, p, q);
#pragma unroll
        for (int i = 0; i < 72; i++) {
            t0.w[i] = (uint32_t)__shfl((int)u.w[i], quad, 64);
            t1.w[i] = (uint32_t)__shfl((int)u.w[i], quad + 1, 64);
            tt.w[i] = (uint32_t)__shfl((int)u.w[i], quad + 2, 64);
        }
        fp6_sub(tt.v, tt.v, t0.v);
        fp6_sub(a.v.c1, tt.v, t1.v);
        fp6_mul_v(u.v, t1.v);
        fp6_add(a.v.c0, t0.v, u.v);
    }
    f = a.v;
}

/* the chunk entry f(S_c; -G1).  As arguments for miller_loop1_h: false, and
 * nothing written, when the chunk sum is the identity (sflag[c] == 0) and the
 * entry is one.  As a value: the loop run, or one. */
DEV bool aggrlc_entry_args(const g2aff_t *S, const int32_t *sflag, size_t c,
                           g2aff_t &Q, g1aff_t &P) {
    if (!sflag[c]) return false;
    Q = S[c];
    aggrlc_neg_g1(P);
    return true;
}
DEV void aggrlc_chunk_entry(fp12_t &f, const g2aff_t *S, const int32_t *sflag, size_t c) {
    g2aff_t Q;
    g1aff_t P;
    if (aggrlc_entry_args(S, sflag, c, Q, P)) miller_loop1_h(f, Q, P);
    else fp12_one(f);
}

/* what an item thread of k_aggrlc_item does ahead of its loop; returns the
 * item's elig, and with 1 also A = r_i*aggpk_i.
 * HOISTED: first what k_aggrlc_sigscale<true> left for the key sum — the same
 * rule, now with it.  An open identity signature gets the herumi verdict.  An
 * eligible item whose key sum is the identity is rejected, and since its B_i
 * is already inside S_c it marks the chunk dirty (every writer stores the
 * same value) for the repair launches.
 * Then the scaled key sum; the identity there is elig 2, as in k_aggrlc_miller. */
template <bool HOISTED>
DEV int32_t aggrlc_item_prologue(const g1_t *aggpubs, const uint64_t *scalars, int32_t *elig,
                                 int32_t *results, int32_t *dirty, size_t i, g1_t &A) {
    int32_t e = elig[i];
    if (HOISTED && (e == AGGRLC_ELIG_OPEN || e == 1)) {
        int32_t v;
        int cls = aggrlc_classify(1, e == AGGRLC_ELIG_OPEN ? 2 : 1, aggpubs + i, v);
        if (cls == AGGRLC_CLS_DECIDED) {
            results[i] = v;
            elig[i] = 0;
            if (e == 1) dirty[i / AGGRLC_CHUNK] = 1;
            e = 0;
        }
    }
    if (e != 1) return e;
    g1_mul64w(A, aggpubs[i], aggrlc_scalar(scalars, i));
    if (g1_is_inf(A)) { elig[i] = e = 2; results[i] = 0; }
    return e;
}

/* step 3 — one Miller leg per thread: item i with elig 1 computes
 * f(H_i; r_i*aggpk_i), the entry thread of chunk c f(S_c; -G1) into FX[c].
 * Not HOISTED, the entries ride behind the items in the same launch; HOISTED,
 * they have a kernel of their own (k_aggrlc_chunkleg) and no threads here.
 * LEVEL 0: batch + nchunks threads; the arguments go to affine and both
 * kinds meet in one call of miller_loop1_h, so the block that holds the
 * boundary does not run it twice.  F[i] for k_aggrlc_chunk_prod.
 * LEVEL 1 (DESIGN.md §4m): no inversion — r_i*aggpk_i and H_i go to
 * miller_loop1_hj as they are, Jacobian.  A hash point with Z = 0, which
 * hashing cannot produce, is elig 2 like an identity key sum, so that no
 * input skips its pairing.  The entries (affine S_c, -G1) keep
 * miller_loop1_h: the one wave that holds the last items and the first
 * entries runs the two loops one after the other.
 * LEVEL 2: that, and the block is the chunk: lane l of block c < nchunks is
 * item 64c + l, and no thread leaves before the product — lanes past the
 * batch, classified and demoted items hold one.  fp12_wave_prod takes it and
 * lane 0 stores FC[c], ccnt[c], cforce[c] with k_aggrlc_chunk_prod's meaning;
 * F does not exist.  The entries, when not hoisted, are the blocks from
 * nchunks on, thread per chunk. */
template <bool HOISTED, int LEVEL>
__global__ void k_aggrlc_item(const g1_t *aggpubs, const g2_t *hms, const uint64_t *scalars,
                              const g2aff_t *S, const int32_t *sflag, fp12_t *F, fp12_t *FX,
                              int32_t *elig, int32_t *results, int batch, int nchunks,
                              int32_t *dirty, fp12_t *FC, int32_t *ccnt, int32_t *cforce) {
    constexpr bool FUSED = LEVEL == 2;
    /* the entry threads, when there are any, start at this thread index */
    const size_t first_entry = FUSED ? (size_t)nchunks * blockDim.x : (size_t)batch;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, c = i - first_entry;
    const bool is_entry = !HOISTED && i >= first_entry;
    const bool is_item = !is_entry && i < (size_t)batch;
    if (is_entry ? c >= (size_t)nchunks : !FUSED && !is_item) return;
    fp12_t *dst = is_entry ? FX + c : F + i;    /* one store for both kinds */
    fp12_t f;
    g2aff_t Q; g1aff_t P;               /* level 0: the one loop's arguments */
    int32_t e = 0;
    bool run = false;
    if (is_item) {
        g1_t A;
        e = aggrlc_item_prologue<HOISTED>(aggpubs, scalars, elig, results, dirty, i, A);
        if (e == 1) {
            if constexpr (LEVEL == 0) {
                g1_to_affine(P, A);
                g2_t hmc = hms[i];
                g2_to_affine(Q, hmc);
                run = true;
            } else {
                g2_t hmc = hms[i];
                if (g2_is_inf(hmc)) {
                    elig[i] = e = 2; results[i] = 0;
                } else {
                    miller_loop1_hj(f, hmc, A);
                    run = true;
                }
            }
        }
    } else if (is_entry) {
        if constexpr (LEVEL == 0) {
            run = aggrlc_entry_args(S, sflag, c, Q, P);
        } else {
            aggrlc_chunk_entry(f, S, sflag, c);
            run = true;
        }
    }
    if constexpr (LEVEL == 0) {
        if (run) miller_loop1_h(f, Q, P);
    }
    if (!run) fp12_one(f);
    if (!FUSED || is_entry) {
        *dst = f;
    } else {
        fp12_wave_prod(f);
        unsigned long long any = __ballot(e != 0), force = __ballot(e == 2);
        if (threadIdx.x == 0) {
            FC[blockIdx.x] = f;
            ccnt[blockIdx.x] = __popcll(any);
            cforce[blockIdx.x] = force ? 1 : 0;
        }
    }
}

/* thread per chunk: the chunk's own entry into the product the fused Miller
 * kernel left in FC — what lane 0 of k_aggrlc_chunk_prod does after its tree */
__global__ void k_aggrlc_chunk_fold(fp12_t *FC, const fp12_t *FX, int nchunks) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    fp12_t a = FC[c], b = FX[c];
    fp12_mul(a, a, b);
    FC[c] = a;
}

/* the chunk entries of k_aggrlc_item as a kernel of their own — thread
 * per chunk: FX[c] = f(S_c; -G1), one when sflag[c] is 0.  The hoisted
 * schedule runs it on a side stream beside the mask kernel, where its 64
 * long waves take slots the short mask blocks leave, instead of behind a
 * Miller grid that fills the chip exactly.  With `dirty` (the repair launch)
 * only the chunks marked there are written again. */
__global__ void k_aggrlc_chunkleg(const g2aff_t *S, const int32_t *sflag,
                                  const int32_t *dirty, fp12_t *FX, int nchunks) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    if (dirty && !dirty[c]) return;
    fp12_t f;
    aggrlc_chunk_entry(f, S, sflag, (size_t)c);
    FX[c] = f;
}

/* one leg of cv_miller2 (hbls_coop.inc): Q at CV_Q1 and P at CV_PP
 * pre-loaded, result f at CV_F0 */
DEVN void cv_miller1(lds_fp2 *A, int q) {
    if (q == 0) {
        lds_st(A + CV_T1, lds_ld(A + CV_Q1));
        lds_st(A + (CV_T1 + 1), lds_ld(A + (CV_Q1 + 1)));
        fp2_t one; fp_one(one.a); fp_zero(one.b);
        lds_st(A + (CV_T1 + 2), one);
    }
    __syncthreads();
    cv_fp12_set_one(A, q, CV_F0);
    int cur = CV_F0, oth = CV_F1;
    for (int bit = 62; bit >= 0; bit--) {
        cv_fp12_sqr(A, q, oth, cur);
        { int s = cur; cur = oth; oth = s; }
        cv_ml_dbl_step(A, q, CV_T1, CV_PP);
        cv_fp12_mul_line(A, q, oth, cur);
        { int s = cur; cur = oth; oth = s; }
        if ((BLS_U >> bit) & 1) {
            cv_ml_add_step(A, q, CV_T1, CV_Q1, CV_PP);
            cv_fp12_mul_line(A, q, oth, cur);
            { int s = cur; cur = oth; oth = s; }
        }
    }
    if (cur != CV_F0) cv_fp12_copy(A, q, CV_F0, cur);
}

/* the chunk entries on four lanes per chunk, ITEMS chunks per one-wave block
 * in the arena layout of k_verify_coop: nchunks/ITEMS blocks spread over the
 * chip and each leg's latency is a quarter-lane chain's, so the entries are
 * done while the mask kernel still runs (DESIGN.md §4l).  The cooperative
 * line functions scale their lines by subfield factors the one-lane steps do
 * not, so FX[c] differs from k_aggrlc_chunkleg's by a factor the final
 * exponentiation sends to one: the verdicts are the same.  Chunks with an
 * identity sum, and the dummy sub-items of the last block, march through the
 * loop on the G2 generator: control flow stays uniform across every barrier. */
template <int ITEMS>
__global__ void __launch_bounds__(ITEMS * CV_LANES) k_aggrlc_chunkleg_coop(
        const g2aff_t *S, const int32_t *sflag, fp12_t *FX, int nchunks) {
    __shared__ uint64_t arena[ITEMS][CV_STRIDE64];
    __shared__ int32_t pre[ITEMS];   /* 1 computed; 0 one; -1 dummy */
    const int sub = threadIdx.x / CV_LANES;
    const int q = threadIdx.x % CV_LANES;
    const int c = blockIdx.x * ITEMS + sub;
    lds_fp2 *A = (lds_fp2 *)arena[sub];
    if (q == 0) {
        int32_t r = -1;
        if (c < nchunks) r = sflag[c] ? 1 : 0;
        pre[sub] = r;
        g2aff_t Q;
        if (r == 1) {
            Q = S[c];
        } else {
            fp_load(Q.x.a, BLS_G2_XA); fp_load(Q.x.b, BLS_G2_XB);
            fp_load(Q.y.a, BLS_G2_YA); fp_load(Q.y.b, BLS_G2_YB);
        }
        lds_st(A + (CV_Q1), Q.x); lds_st(A + (CV_Q1 + 1), Q.y);
        g1aff_t n;
        aggrlc_neg_g1(n);
        fp2_t p;
        p.a = n.x; p.b = n.y;
        lds_st(A + (CV_PP), p);
    }
    __syncthreads();
    cv_miller1(A, q);
    if (q == 0) {
        int32_t r = pre[sub];
        if (r != -1) {
            fp12_t f;
            if (r == 1) cv_ld_fp12(A, CV_F0, f);
            else fp12_one(f);
            FX[c] = f;
        }
    }
}

/* one block per chunk: LDS tree product of the chunk's eligible f values
 * (the ragged tail and the classified items contribute one).  ccnt[c] =
 * eligible items, cforce[c] = some item asked for the exact path.  FX, when
 * given, holds the chunks' own entries (the chunk-level signature leg), which
 * lane 0 multiplies in after the tree. */
__global__ void __launch_bounds__(AGGRLC_CHUNK) k_aggrlc_chunk_prod(
        const fp12_t *F, const int32_t *elig, int batch, int nchunks,
        fp12_t *FC, int32_t *ccnt, int32_t *cforce, const fp12_t *FX) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    __shared__ fp12_t red[AGGRLC_CHUNK];
    size_t i = (size_t)c * AGGRLC_CHUNK + threadIdx.x;
    int e = i < (size_t)batch ? elig[i] : 0;
    if (e == 1) red[threadIdx.x] = F[i];
    else fp12_one(red[threadIdx.x]);
    int cnt = __syncthreads_count(e != 0);
    int force = __syncthreads_or(e == 2);
    for (int s = AGGRLC_CHUNK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            fp12_t t;
            fp12_mul(t, red[threadIdx.x], red[threadIdx.x + s]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (FX) {
            fp12_t t;
            fp12_mul(t, red[0], FX[c]);
            FC[c] = t;
        } else {
            FC[c] = red[0];
        }
        ccnt[c] = cnt;
        cforce[c] = force ? 1 : 0;
    }
}

/* one lane per chunk: the shared final exponentiation and the verdict */
__global__ void k_aggrlc_final(const fp12_t *FC, const int32_t *ccnt,
                               const int32_t *cforce, int32_t *verdict, int nchunks) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    if (cforce[c]) { verdict[c] = 0; return; }
    if (ccnt[c] == 0) { verdict[c] = 1; return; }
    fp12_t f = FC[c];
    fp12_conj(f, f);
    final_exp(f, f);
    verdict[c] = fp12_is_one(f) ? 1 : 0;
}

/* the same contract on four lanes per chunk (hbls_coop.inc): ITEMS chunks per
 * block in the arena layout of k_verify_coop.  The thread-per-chunk kernel
 * above costs one whole final exponentiation's latency on nchunks/64 lone
 * waves; here nchunks/ITEMS one-wave blocks spread over the chip and each
 * runs the cooperative chain.  cv_final_exp returns the same field element
 * as final_exp, so the verdicts are identical.  Chunks that need no
 * exponentiation, and the dummy sub-items of the last block, march through
 * the chain on fp12 one: control flow stays uniform across every barrier. */
template <int ITEMS>
__global__ void __launch_bounds__(ITEMS * CV_LANES) k_aggrlc_final_coop(
        const fp12_t *FC, const int32_t *ccnt, const int32_t *cforce,
        int32_t *verdict, int nchunks) {
    __shared__ uint64_t arena[ITEMS][CV_STRIDE64];
    __shared__ int32_t pre[ITEMS];   /* -2 compute; -1 dummy; else the verdict */
    const int sub = threadIdx.x / CV_LANES;
    const int q = threadIdx.x % CV_LANES;
    const int c = blockIdx.x * ITEMS + sub;
    lds_fp2 *A = (lds_fp2 *)arena[sub];
    if (q == 0) {
        int32_t r = -2;
        if (c >= nchunks) r = -1;
        else if (cforce[c]) r = 0;
        else if (ccnt[c] == 0) r = 1;
        pre[sub] = r;
        fp12_t f;
        if (r == -2) f = FC[c];
        else fp12_one(f);
        cv_st_fp12(A, CV_F0, f);
    }
    __syncthreads();
    cv_fp12_conj(A, q, CV_F0, CV_F0);
    cv_final_exp(A, q);
    if (q == 0) {
        int32_t r = pre[sub];
        if (r == -2) {
            fp12_t f;
            cv_ld_fp12(A, CV_F0, f);
            r = fp12_is_one(f) ? 1 : 0;
        }
        if (r != -1) verdict[c] = r;
    }
}

/* k_verify over a compacted index list (the eligible items of failing chunks) */
__global__ void k_verify_sel(const uint32_t *sel, int nsel, const g1_t *aggpubs,
                             const g2_t *hms, const g2aff_t *sigs,
                             const int32_t *sig_flags, const int32_t *hm_ok,
                             int32_t *results, int batch) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nsel) return;
    uint32_t i = sel[j];
    if (i >= (uint32_t)batch) return;
    /* the rule's first guard; verify_pairing holds the rest of it */
    int32_t v;
    if (aggrlc_classify(hm_ok[i], sig_flags[i], nullptr, v) == AGGRLC_CLS_BAD) {
        results[i] = v; return;
    }
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing(aggpubs[i], hms[i], sig_inf ? dummy : sigs[i], sig_inf);
}

/* ---------------------------------------------------------------- host side */

/* chunks checked, chunks failed, items sent to the per-item path — of the
 * last aggregate-verify call on this thread (all zero on the exact path) */
static thread_local uint32_t g_aggrlc_stats[3] = {0, 0, 0};
extern "C" void hbls_aggrlc_last_stats(uint32_t out[3]) {
    for (int i = 0; i < 3; i++) out[i] = g_aggrlc_stats[i];
}
static void aggrlc_stats_reset(void) {
    for (int i = 0; i < 3; i++) g_aggrlc_stats[i] = 0;
}
extern "C" int hbls_aggrlc_chunk_size(void) { return AGGRLC_CHUNK; }

/* smallest batch the auto mode sends to the combined path: the smallest one
 * measured, with the cooperative tail (DESIGN.md §4h; 131072 with the
 * one-lane tail, §4e) */
#define AGGRLC_DEFAULT_THRESHOLD 16384
static int g_aggrlc_threshold = AGGRLC_DEFAULT_THRESHOLD;
extern "C" void hbls_set_aggrlc_threshold(int n) {
    g_aggrlc_threshold = n < 0 ? AGGRLC_DEFAULT_THRESHOLD : n;
}

/* ---- the switches of the combined path, process-global.  Each has an
 * environment variable read on first use, a default, the values it accepts,
 * and a setter that takes those, or -1 for the default.  A default of -1 is
 * a setting too: "auto" for the mode, and for sigleg and early "the rule", 1
 * from the smallest measured batch at which the variant stops losing the wall
 * clock (DESIGN.md §4k, §4l: for early the largest one measured).
 *   mode      0 exact, 1 combined from the threshold up, auto: aggrlc_wanted
 *   final     the chunks' final exponentiations: 16 or 8 = cooperative, that
 *             many chunks per block; 0 = one lane per chunk (§4h's measured
 *             loser at 4096 chunks, kept reproducible)
 *   sigleg    the signature leg: 0 = per item (k_aggrlc_miller, two legs),
 *             1 = per chunk (k_aggrlc_sigscale, _sigsum, _item)
 *   early     the chunk-level leg (§4l): 0 = inside the item kernel, behind
 *             the items; 1 = hoisted (AggrlcEarly)
 *   miller    the item kernel's level (§4m): 0 = affine arguments, F to
 *             memory, k_aggrlc_chunk_prod; 1 = Jacobian arguments; 2 = that
 *             and the product in the kernel (k_aggrlc_chunk_fold); default
 *             the highest level that won §4m's sweep.  The variable must be
 *             exactly one digit; anything else, a typo included, is the default
 *   chunkleg  the hoisted chunk legs: 16 = k_aggrlc_chunkleg_coop; 0 = one
 *             lane per chunk (k_aggrlc_chunkleg, which outlasts the mask
 *             kernel at the benchmark's size, §4l, kept reproducible).  The
 *             repair launch is always the one-lane kernel */
#define AGGRLC_SIGLEG_MIN_BATCH 16384
#define AGGRLC_EARLY_MIN_BATCH 262144
enum { AGGRLC_SW_MODE = 0, AGGRLC_SW_FINAL, AGGRLC_SW_SIGLEG, AGGRLC_SW_EARLY,
       AGGRLC_SW_MILLER, AGGRLC_SW_CHUNKLEG, AGGRLC_SW_N };
struct AggrlcSwitch {
    const char *env;
    int dflt, accepted[3], n_accepted;
    bool one_digit;         /* the variable is one digit character, no atoi */
    size_t rule_min_batch;  /* dflt == -1: 1 from this batch size on, 0 = no rule */
    int value;              /* -2: read env on first use */
    bool accepts(int v) const {
        for (int k = 0; k < n_accepted; k++)
            if (accepted[k] == v) return true;
        return false;
    }
};
static AggrlcSwitch g_aggrlc_sw[AGGRLC_SW_N] = {
    { "HBLS_AGG_VERIFY_MODE", -1, { 0, 1 }, 2, false, 0, -2 },
    { "HBLS_AGGRLC_FINAL", 16, { 0, 8, 16 }, 3, false, 0, -2 },
    { "HBLS_AGGRLC_SIGLEG", -1, { 0, 1 }, 2, false, AGGRLC_SIGLEG_MIN_BATCH, -2 },
    { "HBLS_AGGRLC_EARLY", -1, { 0, 1 }, 2, false, AGGRLC_EARLY_MIN_BATCH, -2 },
    { "HBLS_AGGRLC_MILLER", 2, { 0, 1, 2 }, 3, true, 0, -2 },
    { "HBLS_AGGRLC_CHUNKLEG", 16, { 0, 16 }, 2, false, 0, -2 },
};
/* the switch's value for a call over `batch` items */
static int aggrlc_switch(int which, size_t batch) {
    AggrlcSwitch &s = g_aggrlc_sw[which];
    if (s.value == -2) {
        const char *e = getenv(s.env);
        int v = s.dflt;
        if (e && s.one_digit) v = (e[0] >= '0' && e[0] <= '9' && e[1] == '\0') ? e[0] - '0' : -2;
        else if (e) v = atoi(e);
        s.value = s.accepts(v) ? v : s.dflt;
    }
    if (s.value >= 0 || !s.rule_min_batch) return s.value;
    return batch >= s.rule_min_batch ? 1 : 0;
}
static int aggrlc_switch_set(int which, int v) {
    AggrlcSwitch &s = g_aggrlc_sw[which];
    if (v == -1) v = s.dflt;
    else if (!s.accepts(v)) return HBLS_ERR_BADINPUT;
    s.value = v;
    return HBLS_OK;
}
extern "C" int hbls_set_agg_verify_mode(int v) { return aggrlc_switch_set(AGGRLC_SW_MODE, v); }
extern "C" int hbls_set_aggrlc_final(int v) { return aggrlc_switch_set(AGGRLC_SW_FINAL, v); }
extern "C" int hbls_set_aggrlc_sigleg(int v) { return aggrlc_switch_set(AGGRLC_SW_SIGLEG, v); }
extern "C" int hbls_set_aggrlc_early(int v) { return aggrlc_switch_set(AGGRLC_SW_EARLY, v); }
extern "C" int hbls_set_aggrlc_miller(int v) { return aggrlc_switch_set(AGGRLC_SW_MILLER, v); }
extern "C" int hbls_set_aggrlc_chunkleg(int v) { return aggrlc_switch_set(AGGRLC_SW_CHUNKLEG, v); }
/* test hook (not part of the ABI, kept out of include/hbls.h; needs no GPU):
 * what switch `which` resolves to for a call over `batch` items */
extern "C" int hbls_aggrlc_switch_value(int which, size_t batch) {
    if (which < 0 || which >= AGGRLC_SW_N) return HBLS_ERR_BADINPUT;
    return aggrlc_switch(which, batch);
}

/* the chunk legs' stream: non-blocking, created on first use and kept for
 * the life of the process, like the upload stream */
static hipStream_t g_aggrlc_side_stream = nullptr;
static std::once_flag g_aggrlc_side_flag;
static hipStream_t aggrlc_side_stream(void) {
    std::call_once(g_aggrlc_side_flag, [] {
        /* highest priority: where a chunk-leg block and a mask block compete
         * for a slot, the few long blocks go first */
        hipStream_t s = nullptr;
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
            (void)hipGetLastError();
            greatest = 0;
        }
        if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) == hipSuccess)
            g_aggrlc_side_stream = s;
        else
            (void)hipGetLastError();    /* no stream: nothing is hoisted */
    });
    return g_aggrlc_side_stream;
}

/* typed pieces of one device allocation, in the order they are taken; each
 * piece starts on a 256-byte boundary.  Over a null base it only adds up the
 * size, so one function lays a buffer out for both the allocation and the
 * pointers. */
struct Carve {
    uint8_t *base;
    size_t used = 0;
    explicit Carve(void *b) : base((uint8_t *)b) {}
    template <typename T> T *take(size_t n) {
        size_t at = used;
        used += (n * sizeof(T) + 255) & ~(size_t)255;
        return base ? (T *)(base + at) : nullptr;
    }
};

/* the device buffers of a combined call — one allocation, one shape for both
 * schedules: the hoisted one makes it ahead of the mask kernel (AggrlcEarly),
 * the other inside aggrlc_verify.  sc, elig: the items' scalars and classes.
 * The chunk-level leg's, none with the per-item leg: B = r_i*sig_i; S, sflag
 * the chunk sums; dirty the chunks to repair; FX the entries f(S_c; -G1).
 * F: the items' f, none at level 2.  FC: the chunk products.  ccnt | cforce |
 * verdict: one piece, which the host downloads. */
struct AggrlcBufs {
    uint64_t *sc;
    int32_t *elig, *sflag, *dirty, *ccnt, *cforce, *verdict;
    g2_t *B;
    g2aff_t *S;
    fp12_t *FX, *F, *FC;
    DevBuf buf;         /* after the pointers: its size comes from lay() */
    AggrlcBufs(size_t batch, size_t nc, const AggrlcPlan &plan) : buf(lay(nullptr, batch, nc, plan)) {
        if (!buf.err) lay(buf.p, batch, nc, plan);
    }
    size_t lay(void *base, size_t batch, size_t nc, const AggrlcPlan &plan) {
        const size_t nl = plan.leg ? nc : 0;
        Carve c(base);
        sc = c.take<uint64_t>(batch);
        elig = c.take<int32_t>(batch);
        B = c.take<g2_t>(nl ? batch : 0);
        S = c.take<g2aff_t>(nl);
        sflag = c.take<int32_t>(nl);
        dirty = c.take<int32_t>(nl);
        FX = c.take<fp12_t>(nl);
        F = c.take<fp12_t>(plan.level == 2 ? 0 : batch);
        FC = c.take<fp12_t>(nc);
        ccnt = c.take<int32_t>(3 * nc);
        cforce = ccnt + nc;
        verdict = cforce + nc;
        return c.used;
    }
};

/* ---- the hoisted schedule (DESIGN.md §4l).  The chunk entries depend on
 * the signature chain only (decompress, sigscale, sigsum), the item legs on
 * hash and mask only.  run_agg_verify_pipeline therefore runs the signature
 * chain ahead of the mask kernel and the chunk legs beside it:
 *   hash, decompress, sigscale, sigsum, { mask | chunk legs on the side
 *   stream }, Miller over the items, join, repair of dirty chunks, products,
 *   final.
 * This is everything the early part leaves behind for aggrlc_verify: device
 * buffers that outlive their work (the destructor waits for the side stream
 * before any of them is freed), the host scalars under the upload, and the
 * events.  ev: 0..1 around sigscale + sigsum on the null stream (slot 7),
 * 2..3 around the chunk-leg kernel on the side stream (slot 8), 4 the
 * scalars' upload. */
struct AggrlcEarly {
    std::vector<uint64_t> scalars;
    AggrlcBufs bufs;
    EventSet<5> ev;
    bool launched = false;
    AggrlcEarly(size_t b, size_t n, const AggrlcPlan &plan) : scalars(b), bufs(b, n, plan) {}
    bool ok() const { return !bufs.buf.err && ev.err == hipSuccess; }
    ~AggrlcEarly() {
        HostSpan sp(3);
        if (launched) (void)hipStreamSynchronize(g_aggrlc_side_stream);
    }
};
static void aggrlc_early_free(AggrlcEarly *e) { delete e; }

/* the signature chain of the chunk-level leg on the null stream: B_i, then
 * S_c and sflag[c].  hoisted: ahead of the mask kernel, d_agg not yet there */
static void launch_aggrlc_sig_chain(bool hoisted, const g1_t *d_agg, const g2aff_t *d_saff,
                                    const int32_t *d_sflags, const int32_t *d_hok,
                                    const AggrlcBufs &L, int32_t *d_res, size_t batch, size_t nc) {
    auto scale = hoisted ? k_aggrlc_sigscale<true> : k_aggrlc_sigscale<false>;
    hipLaunchKernelGGL(scale, dim3((uint32_t)((batch + 63) / 64)), dim3(64), 0, 0,
                       d_agg, d_saff, d_sflags, d_hok, (const uint64_t *)L.sc, L.B, L.elig,
                       d_res, (int)batch);
    hipLaunchKernelGGL(k_aggrlc_sigsum<false>, dim3((uint32_t)nc), dim3(AGGRLC_CHUNK), 0, 0,
                       L.B, (int)batch, (int)nc, L.S, L.sflag,
                       (const int32_t *)nullptr, (const int32_t *)nullptr);
}

/* the early part, called by the pipeline between the decompress and the
 * mask launches.  Returns null and takes the hoisting out of the plan —
 * nothing launched, nothing written — unless the plan asks for it and the
 * side stream, the scalars and the buffers are there.  When it returns the
 * state, d_res and elig carry k_aggrlc_sigscale<true>'s classification, S and
 * sflag the chunk sums, and the chunk legs are running on the side stream. */
static AggrlcEarly *aggrlc_early_begin(AggrlcPlan &plan, const g2aff_t *d_saff,
                                       const int32_t *d_sflags, const int32_t *d_hok,
                                       int32_t *d_res, size_t batch) {
    if (!plan.hoisted) return nullptr;
    plan.hoisted = false;               /* until everything below is in place */
    hipStream_t side = aggrlc_side_stream();
    if (!side) return nullptr;
    size_t nc = (batch + AGGRLC_CHUNK - 1) / AGGRLC_CHUNK;
    uint64_t t_alloc = host_now_ns();
    AggrlcEarly *st = new (std::nothrow) AggrlcEarly(batch, nc, plan);
    g_host_ns[0] += host_now_ns() - t_alloc;
    if (!st) return nullptr;
    if (!st->ok() || !rlc_draw_scalars(st->scalars.data(), batch)) {
        (void)hipGetLastError();
        delete st;
        return nullptr;
    }
    const AggrlcBufs &L = st->bufs;
    bool good = upload_then_wait(L.sc, st->scalars.data(), batch * 8, st->ev[4]) == hipSuccess;
    st->launched = true;    /* from here on the destructor waits for the side stream */
    good = good && hipMemsetAsync(L.dirty, 0, nc * 4, 0) == hipSuccess;
    if (!good) {
        /* the null stream may hold the upload wait and the memset, which
         * touch nothing the rest of the call reads */
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
        delete st;
        return nullptr;
    }
    (void)hipEventRecord(st->ev[0], 0);
    launch_aggrlc_sig_chain(true, nullptr, d_saff, d_sflags, d_hok, L, d_res, batch, nc);
    (void)hipEventRecord(st->ev[1], 0);
    /* the side stream starts behind the chunk sums; its end event is waited
     * for by aggrlc_verify, after the Miller launch */
    (void)hipStreamWaitEvent(side, st->ev[1], 0);
    (void)hipEventRecord(st->ev[2], side);
    /* the null stream — the mask kernel is its next launch — waits for the
     * side stream to have got as far as the chunk-leg launch: the legs' few
     * blocks are then next in their own queue while the mask kernel still sits
     * behind a cross-queue wait, and find the chip empty.  Launched at the
     * same moment, the mask kernel's 65536 short blocks refill every slot as
     * it frees and the legs' blocks, which need more registers and LDS than
     * one retiring mask wave leaves, start late or outlast it (§4l). */
    (void)hipStreamWaitEvent(0, st->ev[2], 0);
    if (plan.chunkleg_kernel == 16)
        hipLaunchKernelGGL(k_aggrlc_chunkleg_coop<16>, dim3((uint32_t)((nc + 15) / 16)),
                           dim3(16 * CV_LANES), 0, side, L.S, L.sflag, L.FX, (int)nc);
    else
        hipLaunchKernelGGL(k_aggrlc_chunkleg, dim3((uint32_t)((nc + 63) / 64)), dim3(64), 0, side,
                           L.S, L.sflag, (const int32_t *)nullptr, L.FX, (int)nc);
    (void)hipEventRecord(st->ev[3], side);
    plan.hoisted = true;
    return st;
}

static void launch_aggrlc_final(int kernel, const fp12_t *d_FC, const int32_t *d_ccnt,
                                const int32_t *d_cforce, int32_t *d_verdict, int nc) {
    if (kernel == 16)
        hipLaunchKernelGGL(k_aggrlc_final_coop<16>, dim3((uint32_t)((nc + 15) / 16)),
                           dim3(16 * CV_LANES), 0, 0, d_FC, d_ccnt, d_cforce, d_verdict, nc);
    else if (kernel == 8)
        hipLaunchKernelGGL(k_aggrlc_final_coop<8>, dim3((uint32_t)((nc + 7) / 8)),
                           dim3(8 * CV_LANES), 0, 0, d_FC, d_ccnt, d_cforce, d_verdict, nc);
    else
        hipLaunchKernelGGL(k_aggrlc_final, dim3((uint32_t)((nc + 63) / 64)), dim3(64), 0, 0,
                           d_FC, d_ccnt, d_cforce, d_verdict, nc);
}

/* selftest inputs, chunk c by c % 8:
 *   0, 6, 7  arbitrary nonzero element          -> computed, verdict 0
 *   1        element of the Fp6 subfield (c1=0) -> computed, verdict 1 (the
 *            easy part of the exponentiation sends the subfield to one)
 *   2        fp12 one                           -> computed, verdict 1
 *   3        arbitrary, ccnt == 0               -> verdict 1 without computing
 *   4        arbitrary, cforce set              -> verdict 0 without computing
 *   5        Fp6 subfield, cforce set           -> verdict 0 (cforce comes first)
 * The coefficients are small multiples of one pushed through two squarings,
 * so they are reduced field elements with no structure the chain could
 * exploit. */
__global__ void k_aggrlc_final_fill(fp12_t *FC, int32_t *ccnt, int32_t *cforce, int nchunks) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    int kind = c % 8;
    fp_t one;
    fp_one(one);
    fp_t co[12];
    for (int k = 0; k < 12; k++) {
        fp_t t;
        fp_zero(t);
        uint32_t m = (uint32_t)c * 12u + (uint32_t)k + 3u;
        for (int b = 31; b >= 0; b--) {
            fp_dbl(t, t);
            if ((m >> b) & 1u) fp_add(t, t, one);
        }
        fp_sqr(t, t);
        fp_add(t, t, one);
        fp_sqr(t, t);
        co[k] = t;
    }
    fp12_t f;
    fp2_t *s = &f.c0.c0;                /* six fp2 coefficients, c0 then c1 */
    for (int k = 0; k < 6; k++) { s[k].a = co[2 * k]; s[k].b = co[2 * k + 1]; }
    if (kind == 1 || kind == 5)
        for (int k = 3; k < 6; k++) { fp_zero(s[k].a); fp_zero(s[k].b); }
    if (kind == 2) fp12_one(f);
    FC[c] = f;
    ccnt[c] = kind == 3 ? 0 : 1 + c % 64;
    cforce[c] = (kind == 4 || kind == 5) ? 1 : 0;
}

/* both final kernels (the cooperative one at 16 and at 8 chunks per block)
 * on the inputs above: the number of chunk verdicts on which a cooperative
 * launch differs from the thread-per-chunk one (0 = parity), HBLS_ERR when
 * the thread-per-chunk verdicts are not what the input kinds dictate — in
 * particular when they are not a mix of 0 and 1 from two chunks up (a lone
 * chunk has a single verdict). */
extern "C" int hbls_aggrlc_final_selftest(int nchunks) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (nchunks < 1 || nchunks > (1 << 20)) return HBLS_ERR_BADINPUT;
    size_t nc = (size_t)nchunks;
    fp12_t *d_FC;
    int32_t *d_ccnt, *d_cforce, *d_v;               /* d_v: a verdict array per kernel */
    auto lay = [&](void *base) {
        Carve c(base);
        d_FC = c.take<fp12_t>(nc);
        d_ccnt = c.take<int32_t>(nc);
        d_cforce = c.take<int32_t>(nc);
        d_v = c.take<int32_t>(3 * nc);
        return c.used;
    };
    DevBuf buf(lay(nullptr));
    if (buf.err) return HBLS_ERR;
    lay(buf.p);
    HIP_OK(hipMemset(d_v, 0xff, 3 * nc * 4));       /* -1: verdict never stored */
    hipLaunchKernelGGL(k_aggrlc_final_fill, dim3((uint32_t)((nc + 63) / 64)), dim3(64), 0, 0,
                       d_FC, d_ccnt, d_cforce, nchunks);
    const int kernels[3] = { 0, 16, 8 };
    for (int k = 0; k < 3; k++)
        launch_aggrlc_final(kernels[k], d_FC, d_ccnt, d_cforce, d_v + k * nc, nchunks);
    HIP_OK(hipGetLastError());
    std::vector<int32_t> v(3 * nc);
    HIP_OK(hipMemcpy(v.data(), d_v, 3 * nc * 4, hipMemcpyDeviceToHost));
    int zeros = 0, ones = 0;
    for (size_t c = 0; c < nc; c++) {
        int kind = (int)(c % 8);
        int want = (kind == 1 || kind == 2 || kind == 3) ? 1 : 0;
        if (v[c] != want) return HBLS_ERR;
        if (v[c]) ones++; else zeros++;
    }
    if (nc >= 2 && (!zeros || !ones)) return HBLS_ERR;
    int diff = 0;
    for (size_t c = 0; c < nc; c++)
        if (v[nc + c] != v[c] || v[2 * nc + c] != v[c]) diff++;
    return diff;
}

/* fixed-base window table of -G1: gtab[w*255 + b-1] = b * 2^(8w) * (-G1) */
static g1aff_t *g_aggrlc_gtab = nullptr;
static int aggrlc_init_tables(void) {
    if (g_aggrlc_gtab) return HBLS_OK;
    const size_t m = AGGRLC_WINDOWS * 255;
    DevBuf dp2(64 * sizeof(g1aff_t)), dwj(m * sizeof(g1_t)), dwi(m);
    g1aff_t *d_gt = nullptr;
    if (dp2.err || dwj.err || dwi.err) return HBLS_ERR;
    HIP_OK(hipMalloc(&d_gt, m * sizeof(g1aff_t)));
    hipLaunchKernelGGL(k_aggrlc_pow2, dim3(1), dim3(64), 0, 0, dp2.as<g1aff_t>());
    hipLaunchKernelGGL(k_wtab_build_jac, dim3(1), dim3(64), 0, 0,
                       dp2.as<g1aff_t>(), 64, dwj.as<g1_t>(), AGGRLC_WINDOWS);
    hipLaunchKernelGGL(k_wtab_to_affine, dim3((int)((m + 255) / 256)), dim3(256), 0, 0,
                       dwj.as<g1_t>(), d_gt, dwi.as<uint8_t>(), m);
    std::vector<uint8_t> winf(m);
    bool ok = hipDeviceSynchronize() == hipSuccess &&
              hipMemcpy(winf.data(), dwi.p, m, hipMemcpyDeviceToHost) == hipSuccess;
    for (size_t k = 0; ok && k < m; k++)
        if (winf[k]) ok = false;         /* no multiple of G1 below 2^64 is the identity */
    if (!ok) { hipFree(d_gt); return HBLS_ERR; }
    g_aggrlc_gtab = d_gt;
    return HBLS_OK;
}

/* does a call over `batch` items take the combined path?  Mode 1 asks for it
 * from the threshold up; auto additionally stays off the latency (coop) sizes
 * and off the experiment switches, which select an exact kernel by name. */
static bool aggrlc_wanted(size_t batch) {
    int m = aggrlc_switch(AGGRLC_SW_MODE, batch);
    if (m == 0 || !g_aggrlc_gtab) return false;
    if (batch > RLC_MAX_ITEMS || (long long)batch < (long long)g_aggrlc_threshold) return false;
    if (m == 1) return true;
    return (int)batch > coop_threshold() && rf_mode() == 0 && !use_batch_affine();
}

/* the one place a call reads the switches.  Combined or exact is decided on
 * mode_batch (the size the caller was given), the leg and the hoisting on the
 * items that reach the pairing stage; may_hoist: the caller runs the early part */
static AggrlcPlan aggrlc_plan(size_t batch, size_t mode_batch, bool may_hoist) {
    AggrlcPlan p = { false, 0, false, 0, 0, 0 };
    p.combined = aggrlc_wanted(mode_batch);
    if (!p.combined) return p;
    p.leg = aggrlc_switch(AGGRLC_SW_SIGLEG, batch);
    p.hoisted = may_hoist && p.leg && aggrlc_switch(AGGRLC_SW_EARLY, batch);
    if (p.leg) p.level = aggrlc_switch(AGGRLC_SW_MILLER, batch);
    p.final_kernel = aggrlc_switch(AGGRLC_SW_FINAL, batch);
    if (p.hoisted) p.chunkleg_kernel = aggrlc_switch(AGGRLC_SW_CHUNKLEG, batch);
    return p;
}

/* one combined call, as its stages below see it */
struct AggrlcRun {
    const AggrlcPlan &plan;
    const g1_t *d_agg; const g2_t *d_hm; const g2aff_t *d_saff;
    const int32_t *d_sflags, *d_hok;
    int32_t *d_res;
    size_t batch, nc;
    const AggrlcBufs &L;
};

/* the Miller legs of the items — and, with the chunk-level leg not hoisted,
 * of the chunk entries behind them: one dispatch on the plan */
static void launch_aggrlc_items(const AggrlcRun &r) {
    const AggrlcBufs &L = r.L;
    if (!r.plan.leg) {
        hipLaunchKernelGGL(k_aggrlc_miller, dim3((uint32_t)((r.batch + 63) / 64)), dim3(64), 0, 0,
                           r.d_agg, r.d_hm, r.d_saff, r.d_sflags, r.d_hok,
                           (const uint64_t *)L.sc, g_aggrlc_gtab, r.L.F, L.elig, r.d_res,
                           (int)r.batch);
        return;
    }
    static const decltype(&k_aggrlc_item<false, 0>) kernels[2][3] = {
        { k_aggrlc_item<false, 0>, k_aggrlc_item<false, 1>, k_aggrlc_item<false, 2> },
        { k_aggrlc_item<true, 0>, k_aggrlc_item<true, 1>, k_aggrlc_item<true, 2> } };
    /* level 2: a block per chunk, then the entries, thread per chunk; below
     * it a thread per item and per entry */
    const size_t nx = r.plan.hoisted ? 0 : r.nc;
    const size_t blocks = r.plan.level == 2 ? r.nc + (nx + 63) / 64 : (r.batch + nx + 63) / 64;
    hipLaunchKernelGGL(kernels[r.plan.hoisted ? 1 : 0][r.plan.level], dim3((uint32_t)blocks),
                       dim3(64), 0, 0, r.d_agg, r.d_hm, (const uint64_t *)L.sc,
                       (const g2aff_t *)L.S, (const int32_t *)L.sflag, r.L.F, L.FX, L.elig,
                       r.d_res, (int)r.batch, (int)r.nc, L.dirty, r.L.FC, r.L.ccnt, r.L.cforce);
}

/* hoisted: the join with the side stream's chunk entries, then the repair,
 * over all chunks: blocks and threads of clean chunks return at once */
static void launch_aggrlc_join_repair(const AggrlcRun &r, hipEvent_t legs_done) {
    const AggrlcBufs &L = r.L;
    (void)hipStreamWaitEvent(0, legs_done, 0);
    hipLaunchKernelGGL(k_aggrlc_sigsum<true>, dim3((uint32_t)r.nc), dim3(AGGRLC_CHUNK), 0, 0,
                       L.B, (int)r.batch, (int)r.nc, L.S, L.sflag, L.elig, L.dirty);
    hipLaunchKernelGGL(k_aggrlc_chunkleg, dim3((uint32_t)((r.nc + 63) / 64)), dim3(64), 0, 0,
                       L.S, L.sflag, L.dirty, L.FX, (int)r.nc);
}

/* FC[c]: the chunk's product with its own entry — a tree over F, or at
 * level 2 the entry folded into what the item kernel left */
static void launch_aggrlc_products(const AggrlcRun &r) {
    if (r.plan.level == 2)
        hipLaunchKernelGGL(k_aggrlc_chunk_fold, dim3((uint32_t)((r.nc + 63) / 64)), dim3(64), 0, 0,
                           r.L.FC, r.L.FX, (int)r.nc);
    else
        hipLaunchKernelGGL(k_aggrlc_chunk_prod, dim3((uint32_t)r.nc), dim3(AGGRLC_CHUNK), 0, 0,
                           r.L.F, r.L.elig, (int)r.batch, (int)r.nc, r.L.FC, r.L.ccnt,
                           r.L.cforce, r.plan.leg ? r.L.FX : (const fp12_t *)nullptr);
}

/* ccnt | cforce | verdict to the host (the call's first wait for the device)
 * and the stage slots: ev[0..4] bound 7, 4, 5, 6; hoisted, 7 and 8 come from
 * the early part's own events */
static int aggrlc_download(const AggrlcRun &r, const EventSet<5> &ev, const AggrlcEarly *early,
                           std::vector<int32_t> &hc) {
    hipError_t e = hipMemcpy(hc.data(), r.L.ccnt, 3 * r.nc * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipGetLastError();
    auto ns = [e](hipEvent_t a, hipEvent_t b) {         /* zero after an error */
        float ms = 0;
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms, a, b);
        return (uint64_t)(ms * 1e6);
    };
    for (int i = 1; i < 4; i++) g_stage_ns[3 + i] = ns(ev[i], ev[i + 1]);
    g_stage_ns[7] = early ? ns(early->ev[0], early->ev[1]) : r.plan.leg ? ns(ev[0], ev[1]) : 0;
    if (early && e == hipSuccess) g_stage_ns[8] = ns(early->ev[2], early->ev[3]);
    HIP_OK(e);
    return HBLS_OK;
}

/* the statistics, and the refinement, one level: the eligible items of
 * failing chunks go through the exact per-item pairing */
static int aggrlc_refine(const AggrlcRun &r, const std::vector<int32_t> &hc) {
    std::vector<uint32_t> failed;
    for (size_t c = 0; c < r.nc; c++) {
        if (hc[c] <= 0) continue;
        g_aggrlc_stats[0]++;
        if (hc[2 * r.nc + c] == 1) continue;
        g_aggrlc_stats[1]++;
        failed.push_back((uint32_t)c);
    }
    if (failed.empty()) return HBLS_OK;
    std::vector<int32_t> helig(r.batch);
    HIP_OK(hipMemcpy(helig.data(), r.L.elig, r.batch * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> sel;
    for (uint32_t c : failed)
        for (size_t i = (size_t)c * AGGRLC_CHUNK;
             i < r.batch && i < ((size_t)c + 1) * AGGRLC_CHUNK; i++)
            if (helig[i]) sel.push_back((uint32_t)i);
    size_t ns = sel.size();
    g_aggrlc_stats[2] = (uint32_t)ns;
    if (!ns) return HBLS_OK;
    DevBuf dsel(ns * 4);
    if (dsel.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dsel.p, sel.data(), ns * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_verify_sel, dim3((uint32_t)((ns + 63) / 64)), dim3(64), 0, 0,
                       dsel.as<uint32_t>(), (int)ns, r.d_agg, r.d_hm, r.d_saff, r.d_sflags,
                       r.d_hok, r.d_res, (int)r.batch);
    HIP_OK(hipGetLastError());
    return HBLS_OK;
}

/* the verify stage of run_agg_verify_pipeline on the combined path; inputs
 * as k_verify's.  Returns HBLS_OK with d_res complete, AGGRLC_FALLBACK when
 * randomness or memory for the combination is unavailable, HBLS_ERR on a
 * device error.  g_stage_ns[4..6] = Miller, products, final exponentiation;
 * g_stage_ns[7] = the signature scaling and chunk sums of the chunk-level
 * leg (zero with the per-item leg).  Every launch lies between the caller's
 * verify-stage events.
 * With `early` (the hoisted schedule) the scalars, the signature chain and
 * the chunk legs are the pipeline's earlier work.  g_stage_ns[4] then covers
 * the item kernel, the join and the repair launches, g_stage_ns[7] the early
 * part's own interval and g_stage_ns[8] the chunk-leg kernel's on its stream. */
static int aggrlc_verify(const AggrlcPlan &plan, const g1_t *d_agg, const g2_t *d_hm,
                         const g2aff_t *d_saff, const int32_t *d_sflags, const int32_t *d_hok,
                         int32_t *d_res, size_t batch, AggrlcEarly *early) {
    const size_t nc = (batch + AGGRLC_CHUNK - 1) / AGGRLC_CHUNK;
    std::vector<uint64_t> scalars(early ? 0 : batch);
    if (!early && !rlc_draw_scalars(scalars.data(), batch)) return AGGRLC_FALLBACK;
    FreeClock fclk;
    uint64_t t_alloc = host_now_ns();
    std::unique_ptr<AggrlcBufs> own;    /* the hoisted schedule brings its own */
    if (!early) own.reset(new (std::nothrow) AggrlcBufs(batch, nc, plan));
    g_host_ns[0] += host_now_ns() - t_alloc;
    FreeClockArm farm(fclk);
    const AggrlcBufs *bufs = early ? &early->bufs : own.get();
    if (!bufs || bufs->buf.err) {
        (void)hipGetLastError();
        return AGGRLC_FALLBACK;
    }
    const AggrlcRun r = { plan, d_agg, d_hm, d_saff, d_sflags, d_hok, d_res, batch, nc, *bufs };
    /* the scalars go up beside the kernels already queued, not behind them;
     * `scalars` outlives the copy (the verdict download below waits for the
     * Miller kernel, which waits for the upload) */
    EventSet<1> up;
    if (up.err != hipSuccess) return HBLS_ERR;
    if (!early) HIP_OK(upload_then_wait(bufs->sc, scalars.data(), batch * 8, up[0]));
    /* ev[0..1] around the signature scaling and sums, then Miller (with the
     * join and repair), products, final */
    EventSet<5> ev;
    if (ev.err != hipSuccess) return HBLS_ERR;
    (void)hipEventRecord(ev[0], 0);
    if (plan.leg && !early)
        launch_aggrlc_sig_chain(false, d_agg, d_saff, d_sflags, d_hok, *bufs, d_res, batch, nc);
    (void)hipEventRecord(ev[1], 0);
    launch_aggrlc_items(r);
    if (early) launch_aggrlc_join_repair(r, early->ev[3]);
    (void)hipEventRecord(ev[2], 0);
    launch_aggrlc_products(r);
    (void)hipEventRecord(ev[3], 0);
    launch_aggrlc_final(plan.final_kernel, bufs->FC, bufs->ccnt, bufs->cforce, bufs->verdict,
                        (int)nc);
    (void)hipEventRecord(ev[4], 0);
    std::vector<int32_t> hc(3 * nc);
    int rc = aggrlc_download(r, ev, early, hc);
    if (rc != HBLS_OK) return rc;
    return aggrlc_refine(r, hc);
}

/* ---- test hook for the functions above (not part of the ABI, kept out of
 * include/hbls.h; raw device-domain limbs as hbls_arith_probe, DESIGN.md §4j,
 * whose operation table is pinned by its own test and stays as it is).
 * Item layouts, fp = 48 B:
 *   0 g1_mul64w   in Jacobian point (3 fp) | u64 scalar   out Jacobian (3 fp)
 *   1 g2_mul64w   in Jacobian point (6 fp) | u64 scalar   out Jacobian (6 fp)
 *   2 miller1_fe  in affine Q (4 fp) | affine P (2 fp)    out fp12 (12 fp):
 *                 final_exp(conj(miller_loop1_h(Q, P))), what the final
 *                 kernels apply to a chunk product
 *   3 miller1j_fe in Jacobian Q (6 fp) | Jacobian P (3 fp) out fp12 (12 fp):
 *                 final_exp(conj(miller_loop1_hj(Q, P)))
 *   4 wave_prod   in 64 fp12 (768 fp), one 64-lane block per item
 *                 out fp12_wave_prod as held by lane 0 | by lane 63 (24 fp) */
enum { AGGRLC_PROBE_G1_MUL64W = 0, AGGRLC_PROBE_G2_MUL64W = 1, AGGRLC_PROBE_MILLER1_FE = 2,
       AGGRLC_PROBE_MILLER1J_FE = 3, AGGRLC_PROBE_WAVE_PROD = 4, AGGRLC_PROBE_N_OPS = 5 };
#define AGGRLC_PROBE_MAX_GROUPS 64
#define AGGRLC_PROBE_MAX_ITEMS 4096
__global__ void k_aggrlc_probe(int op, const uint64_t *in, int in_w, uint64_t *out, int out_w,
                               int n) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t *src = in + (size_t)j * in_w;
    uint64_t *dst = out + (size_t)j * out_w;
    union { uint64_t w[72]; g1_t g1; g2_t g2; g2aff_t q; fp12_t f; } a, o;
    for (int i = 0; i < in_w && i < 72; i++) a.w[i] = src[i];
    if (op == AGGRLC_PROBE_G1_MUL64W) {
        g1_mul64w(o.g1, a.g1, src[18]);
    } else if (op == AGGRLC_PROBE_G2_MUL64W) {
        g2_mul64w(o.g2, a.g2, src[36]);
    } else if (op == AGGRLC_PROBE_MILLER1J_FE) {
        g1_t p;
        for (int k = 0; k < 6; k++) {
            p.x.l[k] = src[36 + k]; p.y.l[k] = src[42 + k]; p.z.l[k] = src[48 + k];
        }
        fp12_t f;
        miller_loop1_hj(f, a.g2, p);
        fp12_conj(f, f);
        final_exp(o.f, f);
    } else {
        g1aff_t p;
        for (int k = 0; k < 6; k++) { p.x.l[k] = src[24 + k]; p.y.l[k] = src[30 + k]; }
        fp12_t f;
        miller_loop1_h(f, a.q, p);
        fp12_conj(f, f);
        final_exp(o.f, f);
    }
    for (int i = 0; i < out_w; i++) dst[i] = o.w[i];
}
/* block per group of 64 elements, lane l holds element l */
__global__ void k_aggrlc_probe_wave_prod(const fp12_t *in, fp12_t *out, int n) {
    int g = blockIdx.x;
    if (g >= n) return;
    fp12_t f = in[(size_t)g * 64 + threadIdx.x];
    fp12_wave_prod(f);
    if (threadIdx.x == 0) out[2 * g] = f;
    if (threadIdx.x == 63) out[2 * g + 1] = f;
}
static bool probe_limbs_lt_p(const uint8_t *b);     /* hbls_probe.inc */
extern "C" int hbls_aggrlc_probe(int op, const uint8_t *in, size_t n_items, uint8_t *out) {
    if (op < 0 || op >= AGGRLC_PROBE_N_OPS) return HBLS_ERR_BADINPUT;
    if (!in || !out || n_items == 0 || n_items > AGGRLC_PROBE_MAX_ITEMS)
        return HBLS_ERR_BADINPUT;
    const bool wave = op == AGGRLC_PROBE_WAVE_PROD;
    if (wave && n_items > AGGRLC_PROBE_MAX_GROUPS) return HBLS_ERR_BADINPUT;
    const bool mul = op == AGGRLC_PROBE_G1_MUL64W || op == AGGRLC_PROBE_G2_MUL64W;
    const int n_fp = op == AGGRLC_PROBE_G1_MUL64W ? 3 : op == AGGRLC_PROBE_MILLER1J_FE ? 9
                     : wave ? 64 * 12 : 6;                      /* fp elements in */
    const int in_w = n_fp * 6 + (mul ? 1 : 0);
    const int out_w = op == AGGRLC_PROBE_G1_MUL64W ? 18 : op == AGGRLC_PROBE_G2_MUL64W ? 36
                      : wave ? 144 : 72;
    for (size_t j = 0; j < n_items; j++)
        for (int i = 0; i < n_fp; i++)
            if (!probe_limbs_lt_p(in + j * (size_t)in_w * 8 + 48 * i)) return HBLS_ERR_BADINPUT;
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf din(n_items * in_w * 8), dout(n_items * out_w * 8);
    if (din.err || dout.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(din.p, in, n_items * in_w * 8, hipMemcpyHostToDevice));
    if (wave)
        hipLaunchKernelGGL(k_aggrlc_probe_wave_prod, dim3((uint32_t)n_items), dim3(64), 0, 0,
                           din.as<fp12_t>(), dout.as<fp12_t>(), (int)n_items);
    else
        hipLaunchKernelGGL(k_aggrlc_probe, dim3((uint32_t)((n_items + 63) / 64)), dim3(64), 0, 0,
                           op, din.as<uint64_t>(), in_w, dout.as<uint64_t>(), out_w, (int)n_items);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, dout.p, n_items * out_w * 8, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
