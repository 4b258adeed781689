/* hbls_probe.inc — operation-level arithmetic probe (included by
 * hbls_dev.hip after the host layer's helpers).
 *
 * A TEST HOOK, not part of the ABI (kept out of include/hbls.h, like
 * hbls_coop_selftest and hbls_fpmul_asm_check).  One call runs one field,
 * tower or group operation on n_items independent operand sets and returns
 * the raw results, so tests/test_arith_probe_gpu.py can compare every
 * production function with plain big-integer arithmetic (oracle/pyref.py)
 * on operands chosen to hit the carry and boundary cases (DESIGN.md §4j).
 *
 * Wire format: RAW DEVICE-DOMAIN LIMBS.  An fp is 6 x u64 little-endian
 * (48 B), exactly the fp_t contents in Montgomery form; towers follow the
 * fp2_t / fp6_t / fp12_t memory order; points are Jacobian x|y|z or affine
 * x|y.  Nothing is converted on the way in or out, so fp_to_mont and
 * fp_from_mont are on the path of their own operations only.  Exceptions,
 * by the nature of the operation: fp_to_mont takes and fp_from_mont returns
 * a plain (non-Montgomery) integer, fp_from_le48 takes and fp_to_le48
 * returns 48 serialized bytes.
 *
 * The kernels CALL the production functions; no body is copied here.
 * k_arith_probe runs one thread per item.  k_arith_probe_coop has the
 * geometry of k_verify_coop (64 threads = 16 items x 4 lanes, the same LDS
 * arena type and stride): the cv_* primitives contain block barriers, so
 * the lanes of absent items in the last block run every round on a copy of
 * the last item's operands and skip only the final store.
 *
 * Operation table: X(name, fp elements in, fp elements out, class).
 * Classes: S scalar kernel, every input component < p; Z the same and the
 * first operand non-zero (inversions, final exponentiations); B scalar
 * kernel, input is 48 arbitrary bytes (fp_from_le48 rejects >= p itself);
 * C / CZ cooperative kernel, as S / Z.  The Python table in
 * tests/arith_cases.py lists the same names in the same order; the test
 * checks both against hbls_arith_probe_op_count / _op_name. */
#define PROBE_OPS(X) \
    X(fp_add, 2, 1, S) X(fp_sub, 2, 1, S) X(fp_neg, 1, 1, S) X(fp_dbl, 1, 1, S) \
    X(fp_half, 1, 1, S) \
    X(fp_mul, 2, 1, S) X(fp_mul_inl, 2, 1, S) X(fp_mul_c, 2, 1, S) \
    X(fp_mul_asm, 2, 1, S) X(fp_mul_rs, 2, 1, S) \
    X(fp_sqr, 1, 1, S) X(fp_inv, 1, 1, Z) X(fp_sqrt, 1, 1, S) \
    X(fp_legendre, 1, 0, S) X(fp_is_odd, 1, 0, S) \
    X(fp_to_mont, 1, 1, S) X(fp_from_mont, 1, 1, S) \
    X(fp_from_le48, 1, 1, B) X(fp_to_le48, 1, 1, S) \
    X(fp2_add, 4, 2, S) X(fp2_sub, 4, 2, S) X(fp2_neg, 2, 2, S) \
    X(fp2_conj, 2, 2, S) X(fp2_half, 2, 2, S) \
    X(fp2_mul, 4, 2, S) X(fp2_mul_ri, 4, 2, S) X(cvr_fp2_mul, 4, 2, S) \
    X(fp2_sqr, 2, 2, S) X(cvr_fp2_sqr, 2, 2, S) \
    X(fp2_mul_fp, 3, 2, S) X(fp2_mul_xi, 2, 2, S) X(fp2_inv, 2, 2, Z) \
    X(fp2_sqrt, 2, 2, S) X(fp2_sqrt_any, 2, 2, S) \
    X(fp6_mul, 12, 6, S) X(fp6_mul_rs6, 12, 6, S) X(fp6_mul_v, 6, 6, S) \
    X(fp6_inv, 6, 6, Z) \
    X(fp12_mul, 24, 12, S) X(fp12_mul_6, 24, 12, S) \
    X(fp12_sqr, 12, 12, S) X(fp12_sqr_6, 12, 12, S) \
    X(fp12_inv, 12, 12, Z) X(fp12_conj, 12, 12, S) \
    X(fp12_frob, 12, 12, S) X(fp12_frob2, 12, 12, S) \
    X(fp12_mul_line, 18, 12, S) X(fp12_mul_line_6, 18, 12, S) \
    X(fp12_mul_line2, 24, 12, S) \
    X(fp12_cyc_sqr, 12, 12, S) \
    X(fp12_pow_u, 12, 12, S) X(fp12_pow_u_6, 12, 12, S) \
    X(final_exp, 12, 12, Z) X(final_exp_6, 12, 12, Z) \
    X(g1_dbl, 3, 3, S) X(g1_add, 6, 3, S) X(g1_madd, 5, 3, S) \
    X(g2_dbl, 6, 6, S) X(g2_add, 12, 6, S) \
    X(cv_fp6_mul, 12, 6, C) \
    X(cv_fp12_mul, 24, 12, C) X(cv_fp12_sqr, 12, 12, C) \
    X(cv_fp12_inv_q0, 12, 12, CZ) \
    X(cv_fp12_frob_q0, 12, 12, C) X(cv_fp12_frob2_q0, 12, 12, C) \
    X(cv_fp12_mul_line, 18, 12, C) X(cv_fp12_cyc_sqr, 12, 12, C) \
    X(cv_pow_u, 12, 12, C) X(cv_final_exp, 12, 12, CZ) \
    X(cv_g2_dbl_plain, 6, 6, C) X(cv_g2_addj, 12, 6, C)

enum {
#define X(name, nin, nout, cls) PROBE_##name,
    PROBE_OPS(X)
#undef X
    PROBE_N_OPS
};
enum { PROBE_S = 0, PROBE_Z = 1, PROBE_B = 2, PROBE_C = 4, PROBE_CZ = 5 };
struct probe_op_t { const char *name; int n_in, n_out, cls; };
static const probe_op_t PROBE_TAB[PROBE_N_OPS] = {
#define X(name, nin, nout, cls) { #name, nin, nout, PROBE_##cls },
    PROBE_OPS(X)
#undef X
};
#define PROBE_MAX_IN 24
#define PROBE_MAX_OUT 12
#define PROBE_MAX_ITEMS 4096

/* one item's operands / results, viewed at every level of the tower */
union probe_in_t {
    uint64_t w[PROBE_MAX_IN * 6];
    fp_t f[PROBE_MAX_IN];
    fp2_t f2[PROBE_MAX_IN / 2];
    fp6_t f6[PROBE_MAX_IN / 6];
    fp12_t f12[PROBE_MAX_IN / 12];
    g1_t g1[2];
    g2_t g2[2];
};
union probe_out_t {
    uint64_t w[PROBE_MAX_OUT * 6];
    fp_t f[PROBE_MAX_OUT];
    fp2_t f2[PROBE_MAX_OUT / 2];
    fp6_t f6[PROBE_MAX_OUT / 6];
    fp12_t f12[1];
    g1_t g1[1];
    g2_t g2[1];
};

__global__ void k_arith_probe(int op, const uint64_t *in, int n_in, uint64_t *out,
                              int n_out, int32_t *flag, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    probe_in_t a;
    probe_out_t o;
    const uint64_t *src = in + (size_t)j * n_in * 6;
    for (int i = 0; i < n_in * 6; i++) a.w[i] = src[i];
    for (int i = 0; i < PROBE_MAX_OUT * 6; i++) o.w[i] = 0;
    int32_t fl = 0;
    switch (op) {
    case PROBE_fp_add: fp_add(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_sub: fp_sub(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_neg: fp_neg(o.f[0], a.f[0]); break;
    case PROBE_fp_dbl: fp_dbl(o.f[0], a.f[0]); break;
    case PROBE_fp_half: fp_half(o.f[0], a.f[0]); break;
    case PROBE_fp_mul: fp_mul(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_mul_inl: fp_mul_inl(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_mul_c: fp_mul_c(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_mul_asm: fp_mul_asm(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_mul_rs: RFM(o.f[0], a.f[0], a.f[1]); break;
    case PROBE_fp_sqr: fp_sqr(o.f[0], a.f[0]); break;
    case PROBE_fp_inv: fp_inv(o.f[0], a.f[0]); break;
    case PROBE_fp_sqrt: fl = fp_sqrt(o.f[0], a.f[0]) ? 1 : 0; break;
    case PROBE_fp_legendre: fl = fp_legendre(a.f[0]); break;
    case PROBE_fp_is_odd: fl = fp_is_odd(a.f[0]) ? 1 : 0; break;
    case PROBE_fp_to_mont: fp_to_mont(o.f[0], a.f[0].l); break;
    case PROBE_fp_from_mont: fp_from_mont(o.f[0].l, a.f[0]); break;
    case PROBE_fp_from_le48:
        fl = fp_from_le48(o.f[0], (const uint8_t *)a.w) ? 1 : 0;
        if (!fl) fp_zero(o.f[0]);
        break;
    case PROBE_fp_to_le48: fp_to_le48((uint8_t *)o.w, a.f[0]); break;
    case PROBE_fp2_add: fp2_add(o.f2[0], a.f2[0], a.f2[1]); break;
    case PROBE_fp2_sub: fp2_sub(o.f2[0], a.f2[0], a.f2[1]); break;
    case PROBE_fp2_neg: fp2_neg(o.f2[0], a.f2[0]); break;
    case PROBE_fp2_conj: fp2_conj(o.f2[0], a.f2[0]); break;
    case PROBE_fp2_half: fp2_half(o.f2[0], a.f2[0]); break;
    case PROBE_fp2_mul: fp2_mul(o.f2[0], a.f2[0], a.f2[1]); break;
    case PROBE_fp2_mul_ri: fp2_mul_ri(o.f2[0], a.f2[0], a.f2[1]); break;
    case PROBE_cvr_fp2_mul: cvr_fp2_mul(o.f2[0], a.f2[0], a.f2[1]); break;
    case PROBE_fp2_sqr: fp2_sqr(o.f2[0], a.f2[0]); break;
    case PROBE_cvr_fp2_sqr: cvr_fp2_sqr(o.f2[0], a.f2[0]); break;
    case PROBE_fp2_mul_fp: fp2_mul_fp(o.f2[0], a.f2[0], a.f[2]); break;
    case PROBE_fp2_mul_xi: fp2_mul_xi(o.f2[0], a.f2[0]); break;
    case PROBE_fp2_inv: fp2_inv(o.f2[0], a.f2[0]); break;
    case PROBE_fp2_sqrt:
        fl = fp2_sqrt(o.f2[0], a.f2[0]) ? 1 : 0;
        if (!fl) fp2_zero(o.f2[0]);
        break;
    case PROBE_fp2_sqrt_any:
        fl = fp2_sqrt_any(o.f2[0], a.f2[0]) ? 1 : 0;
        if (!fl) fp2_zero(o.f2[0]);
        break;
    case PROBE_fp6_mul: fp6_mul(o.f6[0], a.f6[0], a.f6[1]); break;
    case PROBE_fp6_mul_rs6: fp6_mul_rs6(o.f6[0], a.f6[0], a.f6[1]); break;
    case PROBE_fp6_mul_v: fp6_mul_v(o.f6[0], a.f6[0]); break;
    case PROBE_fp6_inv: fp6_inv(o.f6[0], a.f6[0]); break;
    case PROBE_fp12_mul: fp12_mul(o.f12[0], a.f12[0], a.f12[1]); break;
    case PROBE_fp12_mul_6: fp12_mul_6(o.f12[0], a.f12[0], a.f12[1]); break;
    case PROBE_fp12_sqr: fp12_sqr(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_sqr_6: fp12_sqr_6(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_inv: fp12_inv(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_conj: fp12_conj(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_frob: fp12_frob(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_frob2: fp12_frob2(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_mul_line:
        o.f12[0] = a.f12[0];
        fp12_mul_line(o.f12[0], a.f2[6], a.f2[7], a.f2[8]);
        break;
    case PROBE_fp12_mul_line_6:
        o.f12[0] = a.f12[0];
        fp12_mul_line_6(o.f12[0], a.f2[6], a.f2[7], a.f2[8]);
        break;
    case PROBE_fp12_mul_line2:
        o.f12[0] = a.f12[0];
        fp12_mul_line2(o.f12[0], a.f2[6], a.f2[7], a.f2[8], a.f2[9], a.f2[10], a.f2[11]);
        break;
    case PROBE_fp12_cyc_sqr: fp12_cyc_sqr(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_pow_u: fp12_pow_u(o.f12[0], a.f12[0]); break;
    case PROBE_fp12_pow_u_6: fp12_pow_u_6(o.f12[0], a.f12[0]); break;
    case PROBE_final_exp: final_exp(o.f12[0], a.f12[0]); break;
    case PROBE_final_exp_6: final_exp_6(o.f12[0], a.f12[0]); break;
    case PROBE_g1_dbl: g1_dbl(o.g1[0], a.g1[0]); break;
    case PROBE_g1_add: g1_add(o.g1[0], a.g1[0], a.g1[1]); break;
    case PROBE_g1_madd: {
        g1aff_t q;
        q.x = a.f[3]; q.y = a.f[4];
        g1_madd(o.g1[0], a.g1[0], q);
    } break;
    case PROBE_g2_dbl: g2_dbl(o.g2[0], a.g2[0]); break;
    case PROBE_g2_add: g2_add(o.g2[0], a.g2[0], a.g2[1]); break;
    default: break;                /* cooperative ops never reach this kernel */
    }
    uint64_t *dst = out + (size_t)j * n_out * 6;
    for (int i = 0; i < n_out * 6; i++) dst[i] = o.w[i];
    flag[j] = fl;
}

/* Cooperative twin.  Operands go to the arena regions the production
 * kernels use for the same primitive (k_coop_selftest / cv_final_exp /
 * k_hash_to_g2_coop): the first na fp2 to slot sa, the rest to slot sb; the
 * result is read from slot so. */
__global__ void __launch_bounds__(CV_ITEMS * CV_LANES) k_arith_probe_coop(
        int op, const uint64_t *in, int n_in, uint64_t *out, int n_out,
        int32_t *flag, int n) {
    __shared__ uint64_t arena[CV_ITEMS][CV_STRIDE64];
    __shared__ int edge[CV_ITEMS];
    const int sub = threadIdx.x / CV_LANES;
    const int q = threadIdx.x % CV_LANES;
    const int item = blockIdx.x * CV_ITEMS + sub;
    lds_fp2 *A = (lds_fp2 *)arena[sub];
    int sa = CV_X1, na = n_in / 2, sb = CV_Y1, so = CV_F0;
    switch (op) {
    case PROBE_cv_fp6_mul: na = 3; break;
    case PROBE_cv_fp12_mul: na = 6; break;
    case PROBE_cv_fp12_sqr: so = CV_F1; break;
    case PROBE_cv_fp12_inv_q0: sa = CV_F0; so = CV_Y1; break;
    case PROBE_cv_fp12_frob_q0:
    case PROBE_cv_fp12_frob2_q0: sa = CV_F1; so = CV_X1; break;
    case PROBE_cv_fp12_mul_line: na = 6; sb = CV_LC; break;
    case PROBE_cv_fp12_cyc_sqr: so = CV_F1; break;
    case PROBE_cv_pow_u: break;
    case PROBE_cv_final_exp: sa = CV_F0; break;
    case PROBE_cv_g2_dbl_plain: sa = CV_F0; break;
    case PROBE_cv_g2_addj: sa = CV_F0; na = 3; sb = CV_F0 + 3; break;
    default: break;
    }
    if (q == 0) {
        edge[sub] = 0;
        const int from = item < n ? item : n - 1;
        const uint64_t *src = in + (size_t)from * n_in * 6;
        for (int i = 0; i < n_in / 2; i++) {
            fp2_t v;
            for (int k = 0; k < 6; k++) {
                v.a.l[k] = src[i * 12 + k];
                v.b.l[k] = src[i * 12 + 6 + k];
            }
            lds_st(A + (i < na ? sa + i : sb + (i - na)), v);
        }
    }
    __syncthreads();
    switch (op) {                  /* uniform across the block */
    case PROBE_cv_fp6_mul: cv_fp6_mul(A, q, CV_F0, CV_X1, CV_Y1); break;
    case PROBE_cv_fp12_mul: cv_fp12_mul(A, q, CV_F0, CV_X1, CV_Y1); break;
    case PROBE_cv_fp12_sqr: cv_fp12_sqr(A, q, CV_F1, CV_X1); break;
    case PROBE_cv_fp12_inv_q0: cv_fp12_inv_q0(A, q, CV_Y1, CV_F0); break;
    case PROBE_cv_fp12_frob_q0: cv_fp12_frob_q0(A, q, CV_X1, CV_F1, 0); break;
    case PROBE_cv_fp12_frob2_q0: cv_fp12_frob_q0(A, q, CV_X1, CV_F1, 1); break;
    case PROBE_cv_fp12_mul_line: cv_fp12_mul_line(A, q, CV_F0, CV_X1); break;
    case PROBE_cv_fp12_cyc_sqr: cv_fp12_cyc_sqr(A, q, CV_F1, CV_X1); break;
    case PROBE_cv_pow_u: cv_pow_u(A, q, CV_F0, CV_X1, CV_F1); break;
    case PROBE_cv_final_exp: cv_final_exp(A, q); break;
    case PROBE_cv_g2_dbl_plain: cv_g2_dbl_plain(A, q, CV_F0); break;
    case PROBE_cv_g2_addj:
        cv_g2_addj(A, q, CV_F0, CV_F0, CV_F0 + 3, (lds_i32 *)&edge[sub]);
        break;
    default: break;
    }
    __syncthreads();
    if (q == 0 && item < n) {
        uint64_t *dst = out + (size_t)item * n_out * 6;
        for (int i = 0; i < n_out / 2; i++) {
            fp2_t v = lds_ld(A + (so + i));
            for (int k = 0; k < 6; k++) {
                dst[i * 12 + k] = v.a.l[k];
                dst[i * 12 + 6 + k] = v.b.l[k];
            }
        }
        flag[item] = edge[sub];
    }
}

static bool probe_limbs_lt_p(const uint8_t *b) {
    uint64_t v[6];
    memcpy(v, b, 48);
    for (int i = 5; i >= 0; i--) {
        if (v[i] < BLS_P[i]) return true;
        if (v[i] > BLS_P[i]) return false;
    }
    return false;
}

extern "C" int hbls_arith_probe_op_count(void) { return PROBE_N_OPS; }
extern "C" const char *hbls_arith_probe_op_name(int op) {
    return (op >= 0 && op < PROBE_N_OPS) ? PROBE_TAB[op].name : nullptr;
}
/* in: n_items x n_in x 48 B; out: n_items x n_out x 48 B; flag: n_items.
 * HBLS_ERR_BADINPUT for an unknown op, a bad count, or an operand outside
 * the operation's precondition (see the class letters above), so that a
 * test cannot run undefined behaviour unnoticed. */
extern "C" int hbls_arith_probe(int op, const uint8_t *in, size_t n_items, uint8_t *out,
                                int32_t *flag) {
    if (op < 0 || op >= PROBE_N_OPS) return HBLS_ERR_BADINPUT;
    if (!in || !out || !flag || n_items == 0 || n_items > PROBE_MAX_ITEMS)
        return HBLS_ERR_BADINPUT;
    const probe_op_t &t = PROBE_TAB[op];
    const size_t in_b = (size_t)t.n_in * 48, out_b = (size_t)t.n_out * 48;
    const int first = op == PROBE_fp_inv ? 1 : op == PROBE_fp2_inv ? 2
                    : op == PROBE_fp6_inv ? 6 : 12;     /* fp elements of operand 0 */
    for (size_t j = 0; j < n_items; j++) {
        const uint8_t *it = in + j * in_b;
        if (t.cls != PROBE_B)
            for (int i = 0; i < t.n_in; i++)
                if (!probe_limbs_lt_p(it + 48 * i)) return HBLS_ERR_BADINPUT;
        if (t.cls & PROBE_Z) {
            uint8_t acc = 0;
            for (int i = 0; i < first * 48; i++) acc |= it[i];
            if (!acc) return HBLS_ERR_BADINPUT;
        }
    }
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf din(n_items * in_b), dout(n_items * out_b), dflag(n_items * 4);
    if (din.err || dout.err || dflag.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(din.p, in, n_items * in_b, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dflag.p, 0, n_items * 4));
    if (t.cls & PROBE_C) {
        int nb = (int)((n_items + CV_ITEMS - 1) / CV_ITEMS);
        hipLaunchKernelGGL(k_arith_probe_coop, dim3(nb), dim3(CV_ITEMS * CV_LANES), 0, 0,
                           op, din.as<uint64_t>(), t.n_in, dout.as<uint64_t>(), t.n_out,
                           dflag.as<int32_t>(), (int)n_items);
    } else {
        int nb = (int)((n_items + 63) / 64);
        hipLaunchKernelGGL(k_arith_probe, dim3(nb), dim3(64), 0, 0,
                           op, din.as<uint64_t>(), t.n_in, dout.as<uint64_t>(), t.n_out,
                           dflag.as<int32_t>(), (int)n_items);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    if (out_b) HIP_OK(hipMemcpy(out, dout.p, n_items * out_b, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(flag, dflag.p, n_items * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* ---- stage probe: the two byte-to-point stages at the head of every verify
 * pipeline, per kernel variant (DESIGN.md §4j).  kernel 0 is the
 * thread-per-item kernel, kernel 1 the wave-cooperative one through the
 * production launch path, whatever coop_threshold() says.  Per-item results
 * come back uncollapsed, so tests/test_stage_probe_gpu.py can compare each
 * item with the reference. */

/* msgs: batch x msg_len bytes; out96: batch x 96 serialized hash points (zero
 * bytes where ok is 0); ok: batch flags.  Honours hbls_set_g2_cofactor_mode. */
extern "C" int hbls_hash_to_g2_probe(const uint8_t *msgs, size_t msg_len, size_t batch,
                                     int kernel, uint8_t *out96, int32_t *ok) {
    if (kernel < 0 || kernel > 1) return HBLS_ERR_BADINPUT;
    if (!msgs || !out96 || !ok || msg_len == 0 || batch == 0 || batch > PROBE_MAX_ITEMS)
        return HBLS_ERR_BADINPUT;
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dm(batch * msg_len), dhm(batch * sizeof(g2_t)), dok(batch * 4), dser(batch * 96);
    if (dm.err || dhm.err || dok.err || dser.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dm.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dok.p, 0xff, batch * 4));      /* an unwritten flag shows as -1 */
    if (kernel == 1)
        launch_hash_to_g2_coop(dm.as<uint8_t>(), msg_len, dhm.as<g2_t>(), dok.as<int32_t>(),
                               batch);
    else
        hipLaunchKernelGGL(k_hash_to_g2, dim3(scalar_blocks(batch)), dim3(64), 0, 0,
                           dm.as<uint8_t>(), (int)msg_len, dhm.as<g2_t>(), dok.as<int32_t>(),
                           (int)batch, g_fast_cofactor);
    hipLaunchKernelGGL(k_g2_serialize, dim3(scalar_blocks(batch)), dim3(64), 0, 0,
                       dhm.as<g2_t>(), dser.as<uint8_t>(), dok.as<int32_t>(), (int)batch);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out96, dser.p, batch * 96, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ok, dok.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* sigs96: batch x 96 bytes; aff_out: batch x 4 fp raw Montgomery limbs
 * (x.a, x.b, y.a, y.b), meaningful where the flag is 1 (the kernels may
 * leave the other entries unwritten, so the buffer is cleared first);
 * flags: 0 bad, 1 ok, 2 infinity. */
extern "C" int hbls_g2_decompress_probe(const uint8_t *sigs96, size_t batch, int kernel,
                                        uint8_t *aff_out, int32_t *flags) {
    if (kernel < 0 || kernel > 1) return HBLS_ERR_BADINPUT;
    if (!sigs96 || !aff_out || !flags || batch == 0 || batch > PROBE_MAX_ITEMS)
        return HBLS_ERR_BADINPUT;
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    DevBuf dsig(batch * 96), daff(batch * sizeof(g2aff_t)), dfl(batch * 4);
    if (dsig.err || daff.err || dfl.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(daff.p, 0, batch * sizeof(g2aff_t)));
    HIP_OK(hipMemset(dfl.p, 0xff, batch * 4));
    if (kernel == 1)
        LAUNCH_COOP(k_g2_decompress_coop, batch, dsig.as<uint8_t>(), daff.as<g2aff_t>(),
                    dfl.as<int32_t>(), (int)batch);
    else
        hipLaunchKernelGGL(k_g2_decompress, dim3(scalar_blocks(batch)), dim3(64), 0, 0,
                           dsig.as<uint8_t>(), daff.as<g2aff_t>(), dfl.as<int32_t>(),
                           (int)batch);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(aff_out, daff.p, batch * sizeof(g2aff_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(flags, dfl.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
