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

/* p2[k] = 2^k * (-G1), affine (thread k: k doublings, one inversion): the
 * 64 "keys" whose 8-key subset sums (k_wtab_build_jac) are the fixed-base
 * window table of -G1 */
__global__ void k_aggrlc_pow2(g1aff_t *p2) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 64) return;
    g1_t base, p;
    fp_load(base.x, BLS_G1_X); fp_load(base.y, BLS_G1_Y); fp_one(base.z);
    g1_neg(p, base);
    for (int j = 0; j < k; j++) g1_dbl(p, p);
    g1aff_t a;
    g1_to_affine(a, p);
    p2[k] = a;
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
    if (!hm_ok[i] || sig_flags[i] == 0) {
        results[i] = HBLS_ERR_BADINPUT; F[i] = f; return;
    }
    bool sig_inf = sig_flags[i] == 2;
    bool pub_inf = g1_is_inf(aggpubs[i]);
    if (pub_inf || sig_inf) {
        results[i] = (pub_inf && sig_inf) ? 1 : 0;   /* herumi edge */
        F[i] = f; return;
    }
    uint64_t r = scalars[i];
    if (r == 0) r = 1;
    g1_t A, C;
    g1_mul(A, aggpubs[i], &r, 1);
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
    results[i] = 1;      /* stands unless the chunk fails and is re-checked */
}

/* one block per chunk: LDS tree product of the chunk's eligible f values
 * (the ragged tail and the classified items contribute one).  ccnt[c] =
 * eligible items, cforce[c] = some item asked for the exact path. */
__global__ void __launch_bounds__(AGGRLC_CHUNK) k_aggrlc_chunk_prod(
        const fp12_t *F, const int32_t *elig, int batch, int nchunks,
        fp12_t *FC, int32_t *ccnt, int32_t *cforce) {
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
        FC[c] = red[0];
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
    if (!hm_ok[i] || sig_flags[i] == 0) { results[i] = HBLS_ERR_BADINPUT; return; }
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

static int g_agg_verify_mode = -2;      /* -2: read env on first use */
/* smallest batch the auto mode sends to the combined path: the smallest one
 * measured, with the cooperative tail (DESIGN.md §4h; 131072 with the
 * one-lane tail, §4e) */
#define AGGRLC_DEFAULT_THRESHOLD 16384
static int g_aggrlc_threshold = AGGRLC_DEFAULT_THRESHOLD;
static int agg_verify_mode(void) {
    if (g_agg_verify_mode == -2) {
        const char *e = getenv("HBLS_AGG_VERIFY_MODE");
        int m = e ? atoi(e) : -1;
        g_agg_verify_mode = (m == 0 || m == 1) ? m : -1;
    }
    return g_agg_verify_mode;
}
extern "C" int hbls_set_agg_verify_mode(int mode) {
    if (mode < -1 || mode > 1) return HBLS_ERR_BADINPUT;
    g_agg_verify_mode = mode;
    return HBLS_OK;
}
extern "C" void hbls_set_aggrlc_threshold(int n) {
    g_aggrlc_threshold = n < 0 ? AGGRLC_DEFAULT_THRESHOLD : n;
}

/* which kernel runs the chunks' final exponentiations: 16 or 8 = cooperative
 * with that many chunks per block, 0 = one lane per chunk (the measured
 * loser at 4096 chunks, DESIGN.md §4h, kept reproducible) */
#define AGGRLC_FINAL_DEFAULT 16
static int g_aggrlc_final = -2;         /* -2: read env on first use */
static int aggrlc_final_kernel(void) {
    if (g_aggrlc_final == -2) {
        const char *e = getenv("HBLS_AGGRLC_FINAL");
        int k = e ? atoi(e) : AGGRLC_FINAL_DEFAULT;
        g_aggrlc_final = (k == 0 || k == 8 || k == 16) ? k : AGGRLC_FINAL_DEFAULT;
    }
    return g_aggrlc_final;
}
extern "C" int hbls_set_aggrlc_final(int kernel) {
    if (kernel == -1) kernel = AGGRLC_FINAL_DEFAULT;
    if (kernel != 0 && kernel != 8 && kernel != 16) return HBLS_ERR_BADINPUT;
    g_aggrlc_final = kernel;
    return HBLS_OK;
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
    DevBuf dFC(nc * sizeof(fp12_t)), dcs(2 * nc * 4), dv(3 * nc * 4);
    if (dFC.err || dcs.err || dv.err) return HBLS_ERR;
    int32_t *d_ccnt = dcs.as<int32_t>(), *d_cforce = d_ccnt + nc;
    HIP_OK(hipMemset(dv.p, 0xff, 3 * nc * 4));      /* -1: verdict never stored */
    hipLaunchKernelGGL(k_aggrlc_final_fill, dim3((uint32_t)((nc + 63) / 64)), dim3(64), 0, 0,
                       dFC.as<fp12_t>(), d_ccnt, d_cforce, nchunks);
    const int kernels[3] = { 0, 16, 8 };
    for (int k = 0; k < 3; k++)
        launch_aggrlc_final(kernels[k], dFC.as<fp12_t>(), d_ccnt, d_cforce,
                            dv.as<int32_t>() + k * nc, nchunks);
    HIP_OK(hipGetLastError());
    std::vector<int32_t> v(3 * nc);
    HIP_OK(hipMemcpy(v.data(), dv.p, 3 * nc * 4, hipMemcpyDeviceToHost));
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

/* does this call take the combined path?  Mode 1 asks for it from the
 * threshold up; auto additionally stays off the latency (coop) sizes and
 * off the experiment switches, which select an exact kernel by name. */
static bool aggrlc_wanted(size_t batch) {
    int m = agg_verify_mode();
    if (m == 0 || !g_aggrlc_gtab) return false;
    if (batch > RLC_MAX_ITEMS || (long long)batch < (long long)g_aggrlc_threshold) return false;
    if (m == 1) return true;
    return (int)batch > coop_threshold() && rf_mode() == 0 && !use_batch_affine();
}

/* the verify stage of run_agg_verify_pipeline on the combined path; inputs
 * as k_verify's.  Returns HBLS_OK with d_res complete, AGGRLC_FALLBACK when
 * randomness or memory for the combination is unavailable, HBLS_ERR on a
 * device error.  g_stage_ns[4..6] = Miller, products, final exponentiation. */
static int aggrlc_verify(const g1_t *d_agg, const g2_t *d_hm, const g2aff_t *d_saff,
                         const int32_t *d_sflags, const int32_t *d_hok,
                         int32_t *d_res, size_t batch) {
    size_t nc = (batch + AGGRLC_CHUNK - 1) / AGGRLC_CHUNK;
    std::vector<uint64_t> scalars(batch);
    if (!rlc_draw_scalars(scalars.data(), batch)) return AGGRLC_FALLBACK;
    FreeClock fclk;
    uint64_t t_alloc = host_now_ns();
    DevBuf dsc(batch * 8), dF(batch * sizeof(fp12_t)), delig(batch * 4);
    DevBuf dFC(nc * sizeof(fp12_t)), dcs(3 * nc * 4);
    g_host_ns[0] += host_now_ns() - t_alloc;
    FreeClockArm farm(fclk);
    if (dsc.err || dF.err || delig.err || dFC.err || dcs.err) {
        (void)hipGetLastError();
        return AGGRLC_FALLBACK;
    }
    /* the scalars go up beside the kernels already queued, not behind them;
     * `scalars` outlives the copy (the verdict download below waits for the
     * Miller kernel, which waits for the upload) */
    EventSet<1> up;
    if (up.err != hipSuccess) return HBLS_ERR;
    HIP_OK(upload_then_wait(dsc.p, scalars.data(), batch * 8, up[0]));
    int32_t *d_ccnt = dcs.as<int32_t>(), *d_cforce = d_ccnt + nc, *d_verdict = d_cforce + nc;
    hipEvent_t ev[4];
    for (int i = 0; i < 4; i++) (void)hipEventCreate(&ev[i]);
    (void)hipEventRecord(ev[0], 0);
    hipLaunchKernelGGL(k_aggrlc_miller, dim3((uint32_t)((batch + 63) / 64)), dim3(64), 0, 0,
                       d_agg, d_hm, d_saff, d_sflags, d_hok, dsc.as<uint64_t>(),
                       g_aggrlc_gtab, dF.as<fp12_t>(), delig.as<int32_t>(), d_res, (int)batch);
    (void)hipEventRecord(ev[1], 0);
    hipLaunchKernelGGL(k_aggrlc_chunk_prod, dim3((uint32_t)nc), dim3(AGGRLC_CHUNK), 0, 0,
                       dF.as<fp12_t>(), delig.as<int32_t>(), (int)batch, (int)nc,
                       dFC.as<fp12_t>(), d_ccnt, d_cforce);
    (void)hipEventRecord(ev[2], 0);
    launch_aggrlc_final(aggrlc_final_kernel(), dFC.as<fp12_t>(), d_ccnt, d_cforce,
                        d_verdict, (int)nc);
    (void)hipEventRecord(ev[3], 0);
    std::vector<int32_t> hc(3 * nc);
    hipError_t e = hipMemcpy(hc.data(), dcs.p, 3 * nc * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipGetLastError();
    for (int i = 0; i < 3; i++) {
        float ms = 0;
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
        g_stage_ns[4 + i] = (uint64_t)(ms * 1e6);
    }
    for (int i = 0; i < 4; i++) (void)hipEventDestroy(ev[i]);
    HIP_OK(e);

    std::vector<uint32_t> failed;
    for (size_t c = 0; c < nc; c++) {
        if (hc[c] <= 0) continue;
        g_aggrlc_stats[0]++;
        if (hc[2 * nc + c] == 1) continue;
        g_aggrlc_stats[1]++;
        failed.push_back((uint32_t)c);
    }
    if (failed.empty()) return HBLS_OK;

    /* refinement, one level: the eligible items of failing chunks go through
     * the exact per-item pairing */
    std::vector<int32_t> helig(batch);
    HIP_OK(hipMemcpy(helig.data(), delig.p, batch * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> sel;
    for (uint32_t c : failed)
        for (size_t i = (size_t)c * AGGRLC_CHUNK;
             i < batch && i < ((size_t)c + 1) * AGGRLC_CHUNK; i++)
            if (helig[i]) sel.push_back((uint32_t)i);
    size_t ns = sel.size();
    g_aggrlc_stats[2] = (uint32_t)ns;
    if (!ns) return HBLS_OK;
    DevBuf dsel(ns * 4);
    if (dsel.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dsel.p, sel.data(), ns * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_verify_sel, dim3((uint32_t)((ns + 63) / 64)), dim3(64), 0, 0,
                       dsel.as<uint32_t>(), (int)ns, d_agg, d_hm, d_saff, d_sflags, d_hok,
                       d_res, (int)batch);
    HIP_OK(hipGetLastError());
    return HBLS_OK;
}
