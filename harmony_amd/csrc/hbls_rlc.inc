/* hbls_rlc.inc — random-combination batch verification of same-message votes
 * (included from hbls_dev.hip after the stream kernels).
 *
 * Votes (pk_i, sig_i) that sign one message with hash point H satisfy, for
 * secret scalars r_i,
 *       e(sum r_i*pk_i, H) == e(G1, sum r_i*sig_i)
 * whenever every vote is valid, and fail it except with probability ~2^-64
 * (64-bit r_i) when any is not — given all points lie in the prime-order
 * subgroups, which the committee build and the signature decompress check.
 * One pairing per GROUP (a round slot / a caller's message index) replaces
 * one pairing per vote; each vote pays a 64-bit G1 and a 64-bit G2 scalar
 * multiplication instead.
 *
 * Accept/reject parity with the per-item path is by construction: a group
 * whose combination fails is re-checked per CHUNK (a run of <= RLC_CHUNK of
 * its votes), and only the votes of failing chunks go to the per-item
 * pairing (k_verify_votes_sel).  Votes that the per-item kernel would
 * classify without a pairing (malformed, out-of-range, identity signature)
 * never enter a combination and get that classification directly.
 *
 * Bucketing is a host-side counting sort of the group indices the caller
 * already handed over: perm[] lists the vote indices group by group, a chunk
 * is (start, count) into perm[], a group is (first chunk, chunk count).
 * Every descriptor is built from the batch itself, so no device buffer is
 * indexed by an unchecked count; the kernels re-check the bounds anyway. */

#include <sys/random.h>
#include <errno.h>

#define RLC_CHUNK 64            /* votes per chunk == threads per sum block */

/* one thread per vote: classify with k_verify_votes' guard order, then
 * A_i = r_i*pk_i, B_i = r_i*sig_i for the eligible ones.  grp[] is the
 * CLAMPED group index (k_stream_clamp), grp_ok[] its in-range flag; an
 * out-of-range key or group index is never used as an address.  Eligible
 * votes are marked accepted here; refinement overwrites the ones it must. */
__global__ void k_rlc_scale(const g1aff_t *table, int n, const uint32_t *key_idx,
                            const uint32_t *grp, const int32_t *grp_ok,
                            const g2aff_t *sigs, const int32_t *sig_flags,
                            const int32_t *hm_ok, const uint64_t *scalars,
                            g1_t *A, g2_t *B, int32_t *elig, int32_t *results,
                            int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    elig[i] = 0;
    if (!grp_ok[i]) { results[i] = HBLS_ERR_BADINPUT; return; }
    if (!hm_ok[grp[i]] || sig_flags[i] == 0 || key_idx[i] >= (uint32_t)n) {
        results[i] = HBLS_ERR_BADINPUT; return;
    }
    /* identity sig never verifies a table key (keys != inf): verify_pairing's
     * pub_inf/sig_inf edge, without the pairing */
    if (sig_flags[i] == 2) { results[i] = 0; return; }
    uint64_t r = scalars[i];
    g1_t pk, a;
    pk.x = table[key_idx[i]].x;
    pk.y = table[key_idx[i]].y;
    fp_one(pk.z);
    g1_mul(a, pk, &r, 1);
    g2_t s, b;
    g2_from_affine(s, sigs[i]);
    g2_mul(b, s, &r, 1);
    A[i] = a;
    B[i] = b;
    elig[i] = 1;
    results[i] = 1;
}

/* k_rlc_scale for multi-key votes (hbls_multikey.inc): the public key of
 * vote i is its signer-set sum pks[i], pk_ok[i] != 1 marks a malformed signer
 * set.  Unlike a table key a sum can be the point at infinity; such a vote
 * never enters a combination (r*inf would hide its signature from the group
 * check) and gets verify_pairing's identity edge directly: accepted only
 * with an identity signature. */
__global__ void k_rlc_scale_pk(const g1_t *pks, const int32_t *pk_ok,
                               const uint32_t *grp, const int32_t *grp_ok,
                               const g2aff_t *sigs, const int32_t *sig_flags,
                               const int32_t *hm_ok, const uint64_t *scalars,
                               g1_t *A, g2_t *B, int32_t *elig, int32_t *results,
                               int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    elig[i] = 0;
    if (!grp_ok[i]) { results[i] = HBLS_ERR_BADINPUT; return; }
    if (!hm_ok[grp[i]] || sig_flags[i] == 0 || pk_ok[i] != 1) {
        results[i] = HBLS_ERR_BADINPUT; return;
    }
    g1_t pk = pks[i], a;
    bool pub_inf = g1_is_inf(pk), sig_inf = sig_flags[i] == 2;
    if (pub_inf || sig_inf) { results[i] = (pub_inf && sig_inf) ? 1 : 0; return; }
    uint64_t r = scalars[i];
    g1_mul(a, pk, &r, 1);
    g2_t s, b;
    g2_from_affine(s, sigs[i]);
    g2_mul(b, s, &r, 1);
    A[i] = a;
    B[i] = b;
    elig[i] = 1;
    results[i] = 1;
}

/* one RLC_CHUNK-thread block per chunk: LDS tree over the chunk's eligible
 * A_i / B_i (k_stream_accum shape).  pcnt[c] = eligible votes in the chunk. */
__global__ void __launch_bounds__(RLC_CHUNK) k_rlc_chunk_sum(
        const uint32_t *perm, int nperm, const uint32_t *chunk_start,
        const uint32_t *chunk_cnt, int nchunks, const g1_t *A, const g2_t *B,
        const int32_t *elig, int batch, g1_t *PA, g2_t *PB, int32_t *pcnt) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    __shared__ g2_t red2[RLC_CHUNK];
    __shared__ g1_t red1[RLC_CHUNK];
    uint32_t st = chunk_start[c], m = chunk_cnt[c];
    if (m > RLC_CHUNK) m = RLC_CHUNK;
    g1_t a;
    g2_t b;
    g1_set_inf(a);
    g2_set_inf(b);
    int e = 0;
    if (threadIdx.x < m && st + threadIdx.x < (uint32_t)nperm) {
        uint32_t v = perm[st + threadIdx.x];
        if (v < (uint32_t)batch && elig[v]) { a = A[v]; b = B[v]; e = 1; }
    }
    red1[threadIdx.x] = a;
    red2[threadIdx.x] = b;
    int cnt = __syncthreads_count(e);
    for (int s = RLC_CHUNK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            g2_t t2;
            g2_add(t2, red2[threadIdx.x], red2[threadIdx.x + s]);
            red2[threadIdx.x] = t2;
            g1_t t1;
            g1_add(t1, red1[threadIdx.x], red1[threadIdx.x + s]);
            red1[threadIdx.x] = t1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        PA[c] = red1[0];
        PB[c] = red2[0];
        pcnt[c] = cnt;
    }
}

/* verify-chain inputs for one combination (P, S) of group g: key sum as is,
 * the group's hash point, S as affine + flag — what k_stream_gather_check
 * prepares for sig_out / sflags_out */
DEV void rlc_emit_check(int j, const g1_t &P, const g2_t &S, uint32_t g, int n_groups,
                        const g2_t *hm, const int32_t *hm_ok,
                        g1_t *P_out, g2_t *hm_out, int32_t *hmok_out,
                        g2aff_t *sig_out, int32_t *sflags_out) {
    P_out[j] = P;
    if (g >= (uint32_t)n_groups) { hmok_out[j] = 0; sflags_out[j] = 0; return; }
    hm_out[j] = hm[g];
    hmok_out[j] = hm_ok[g];
    if (g2_is_inf(S)) {
        sflags_out[j] = 2;
    } else {
        sflags_out[j] = 1;
        g2_to_affine(sig_out[j], S);
    }
}

/* one block per non-empty group: fold its chunk partials into (P_g, S_g)
 * and emit the group's pairing-check inputs.  gcnt[j] = eligible votes. */
__global__ void __launch_bounds__(RLC_CHUNK) k_rlc_group_sum(
        const uint32_t *grp_id, const uint32_t *grp_cstart, const uint32_t *grp_ccnt,
        int ngroups, int nchunks, const g1_t *PA, const g2_t *PB, const int32_t *pcnt,
        const g2_t *hm, const int32_t *hm_ok, int n_groups,
        g1_t *P_out, g2_t *hm_out, int32_t *hmok_out, g2aff_t *sig_out,
        int32_t *sflags_out, int32_t *gcnt) {
    int j = blockIdx.x;
    if (j >= ngroups) return;
    __shared__ g2_t red2[RLC_CHUNK];
    __shared__ g1_t red1[RLC_CHUNK];
    __shared__ int32_t redc[RLC_CHUNK];
    uint32_t cs = grp_cstart[j], cn = grp_ccnt[j];
    g1_t a;
    g2_t b;
    g1_set_inf(a);
    g2_set_inf(b);
    int32_t e = 0;
    for (uint32_t k = threadIdx.x; k < cn; k += RLC_CHUNK) {
        uint32_t c = cs + k;
        if (c >= (uint32_t)nchunks) break;
        g1_add(a, a, PA[c]);
        g2_add(b, b, PB[c]);
        e += pcnt[c];
    }
    red1[threadIdx.x] = a;
    red2[threadIdx.x] = b;
    redc[threadIdx.x] = e;
    __syncthreads();
    for (int s = RLC_CHUNK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            g2_t t2;
            g2_add(t2, red2[threadIdx.x], red2[threadIdx.x + s]);
            red2[threadIdx.x] = t2;
            g1_t t1;
            g1_add(t1, red1[threadIdx.x], red1[threadIdx.x + s]);
            red1[threadIdx.x] = t1;
            redc[threadIdx.x] += redc[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        gcnt[j] = redc[0];
        rlc_emit_check(j, red1[0], red2[0], grp_id[j], n_groups, hm, hm_ok,
                       P_out, hm_out, hmok_out, sig_out, sflags_out);
    }
}

/* refinement: pairing-check inputs for the selected chunks' partials */
__global__ void k_rlc_chunk_prep(const uint32_t *sel, int nsel, int nchunks,
                                 const uint32_t *chunk_grp, const g1_t *PA, const g2_t *PB,
                                 const g2_t *hm, const int32_t *hm_ok, int n_groups,
                                 g1_t *P_out, g2_t *hm_out, int32_t *hmok_out,
                                 g2aff_t *sig_out, int32_t *sflags_out) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nsel) return;
    uint32_t c = sel[j];
    if (c >= (uint32_t)nchunks) { hmok_out[j] = 0; sflags_out[j] = 0; return; }
    rlc_emit_check(j, PA[c], PB[c], chunk_grp[c], n_groups, hm, hm_ok,
                   P_out, hm_out, hmok_out, sig_out, sflags_out);
}

/* k_verify_votes over a compacted index list (the votes of failing chunks) */
__global__ void k_verify_votes_sel(const uint32_t *sel, int nsel,
                                   const g1aff_t *table, int n, const uint32_t *key_idx,
                                   const g2_t *hms, const uint32_t *hm_idx,
                                   const g2aff_t *sigs,
                                   const int32_t *sig_flags, const int32_t *hm_ok,
                                   int32_t *results, int batch) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nsel) return;
    uint32_t i = sel[j];
    if (i >= (uint32_t)batch) return;
    int h = hm_idx ? (int)hm_idx[i] : (int)i;
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

/* k_verify_votes_sel for multi-key votes: public key from the signer-set
 * sums.  Only eligible votes are listed, so neither point is infinity. */
__global__ void k_verify_votes_sel_pk(const uint32_t *sel, int nsel,
                                      const g1_t *pks, const int32_t *pk_ok,
                                      const g2_t *hms, const uint32_t *hm_idx,
                                      const g2aff_t *sigs,
                                      const int32_t *sig_flags, const int32_t *hm_ok,
                                      int32_t *results, int batch) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nsel) return;
    uint32_t i = sel[j];
    if (i >= (uint32_t)batch) return;
    int h = hm_idx ? (int)hm_idx[i] : (int)i;
    if (!hm_ok[h] || sig_flags[i] == 0 || pk_ok[i] != 1) {
        results[i] = HBLS_ERR_BADINPUT; return;
    }
    g2aff_t dummy;
    bool sig_inf = sig_flags[i] == 2;
    results[i] = verify_pairing(pks[i], hms[h], sig_inf ? dummy : sigs[i], sig_inf);
}

/* ---------------------------------------------------------------- host side */

/* counters of the last batched call on this thread: groups pairing-checked,
 * groups failed, chunks pairing-checked in refinement, votes sent per-item */
static thread_local uint32_t g_rlc_stats[4] = {0, 0, 0, 0};

extern "C" int hbls_rlc_chunk_size(void) { return RLC_CHUNK; }
extern "C" void hbls_rlc_last_stats(uint32_t out[4]) {
    for (int i = 0; i < 4; i++) out[i] = g_rlc_stats[i];
}
static void rlc_stats_reset(void) {
    for (int i = 0; i < 4; i++) g_rlc_stats[i] = 0;
}

/* n fresh nonzero 64-bit scalars from the OS CSPRNG; false if it fails
 * (callers return HBLS_ERR — there is no weaker fallback) */
static bool rlc_draw_scalars(uint64_t *out, size_t n) {
    uint8_t *p = (uint8_t *)out;
    size_t left = n * 8;
    while (left) {
        ssize_t got = getrandom(p, left, 0);
        if (got < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        p += got;
        left -= (size_t)got;
    }
    for (size_t i = 0; i < n; i++)
        while (out[i] == 0) {
            ssize_t got = getrandom(&out[i], 8, 0);
            if (got < 0 && errno != EINTR) return false;
            if (got >= 0 && got != 8) out[i] = 0;
        }
    return true;
}

/* the batched verify chain.  Inputs are device-resident except h_grp, the
 * caller's raw group indices (host copy, for the counting sort):
 *   d_hm / d_hm_ok  n_groups hash points and their flags
 *   d_grp / d_grp_ok clamped group index per vote + in-range flag
 *   d_saff / d_sflags decompressed signatures
 * Writes d_res for every vote whose group index is in range with the codes
 * k_verify_votes gives; the others get HBLS_ERR_BADINPUT (and the caller's
 * k_merge_pok says the same).
 * d_pks != NULL (multi-key votes): vote i's public key is d_pks[i], valid
 * where d_pk_ok[i] == 1, instead of table[d_idx[i]]; d_idx is not read. */
static int rlc_verify_chain(const hbls_committee_t *c, const g2_t *d_hm,
                            const int32_t *d_hm_ok, size_t n_groups,
                            const uint32_t *h_grp, const uint32_t *d_idx,
                            const uint32_t *d_grp, const int32_t *d_grp_ok,
                            const g2aff_t *d_saff, const int32_t *d_sflags,
                            int32_t *d_res, size_t batch,
                            const g1_t *d_pks = nullptr, const int32_t *d_pk_ok = nullptr) {
    /* counting sort by group: perm, chunks, groups */
    std::vector<uint32_t> gcount(n_groups, 0);
    size_t nperm = 0;
    for (size_t i = 0; i < batch; i++)
        if (h_grp[i] < n_groups) { gcount[h_grp[i]]++; nperm++; }
    std::vector<uint32_t> goff(n_groups, 0);
    std::vector<uint32_t> grp_id, grp_cstart, grp_ccnt, chunk_start, chunk_cnt, chunk_grp;
    uint32_t off = 0;
    for (size_t g = 0; g < n_groups; g++) {
        goff[g] = off;
        if (!gcount[g]) continue;
        grp_id.push_back((uint32_t)g);
        grp_cstart.push_back((uint32_t)chunk_start.size());
        for (uint32_t o = 0; o < gcount[g]; o += RLC_CHUNK) {
            chunk_start.push_back(off + o);
            chunk_cnt.push_back(gcount[g] - o < RLC_CHUNK ? gcount[g] - o : RLC_CHUNK);
            chunk_grp.push_back((uint32_t)g);
        }
        grp_ccnt.push_back((uint32_t)chunk_start.size() - grp_cstart.back());
        off += gcount[g];
    }
    size_t ng = grp_id.size(), nc = chunk_start.size();
    /* one upload: perm | chunk_start | chunk_cnt | chunk_grp | grp_id |
     * grp_cstart | grp_ccnt */
    std::vector<uint32_t> desc(nperm + 3 * nc + 3 * ng);
    {
        std::vector<uint32_t> cur(goff);
        for (size_t i = 0; i < batch; i++)
            if (h_grp[i] < n_groups) desc[cur[h_grp[i]]++] = (uint32_t)i;
        uint32_t *q = desc.data() + nperm;
        for (size_t k = 0; k < nc; k++) {
            q[k] = chunk_start[k]; q[nc + k] = chunk_cnt[k]; q[2 * nc + k] = chunk_grp[k];
        }
        q += 3 * nc;
        for (size_t k = 0; k < ng; k++) {
            q[k] = grp_id[k]; q[ng + k] = grp_cstart[k]; q[2 * ng + k] = grp_ccnt[k];
        }
    }
    std::vector<uint64_t> scalars(batch);
    if (!rlc_draw_scalars(scalars.data(), batch)) return HBLS_ERR;

    DevBuf dsc(batch * 8), ddesc(desc.size() * 4);
    DevBuf dA(batch * sizeof(g1_t)), dB(batch * sizeof(g2_t)), delig(batch * 4);
    DevBuf dPA(nc * sizeof(g1_t)), dPB(nc * sizeof(g2_t)), dpcnt(nc * 4);
    DevBuf gP(ng * sizeof(g1_t)), ghm(ng * sizeof(g2_t)), ghok(ng * 4);
    DevBuf gsaff(ng * sizeof(g2aff_t)), gsflags(ng * 4), gout(2 * ng * 4);
    if (dsc.err || ddesc.err || dA.err || dB.err || delig.err || dPA.err || dPB.err ||
        dpcnt.err || gP.err || ghm.err || ghok.err || gsaff.err || gsflags.err ||
        gout.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dsc.p, scalars.data(), batch * 8, hipMemcpyHostToDevice));
    if (!desc.empty())
        HIP_OK(hipMemcpy(ddesc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice));
    const uint32_t *d_perm = ddesc.as<uint32_t>();
    const uint32_t *d_cstart = d_perm + nperm, *d_ccnt = d_cstart + nc;
    const uint32_t *d_cgrp = d_ccnt + nc, *d_gid = d_cgrp + nc;
    const uint32_t *d_gcs = d_gid + ng, *d_gcc = d_gcs + ng;

    int nb = (int)((batch + 63) / 64);
    if (d_pks)
        hipLaunchKernelGGL(k_rlc_scale_pk, dim3(nb), dim3(64), 0, 0,
                           d_pks, d_pk_ok, d_grp, d_grp_ok, d_saff, d_sflags,
                           d_hm_ok, dsc.as<uint64_t>(), dA.as<g1_t>(), dB.as<g2_t>(),
                           delig.as<int32_t>(), d_res, (int)batch);
    else
        hipLaunchKernelGGL(k_rlc_scale, dim3(nb), dim3(64), 0, 0,
                           c->d_table, (int)c->n, d_idx, d_grp, d_grp_ok, d_saff, d_sflags,
                           d_hm_ok, dsc.as<uint64_t>(), dA.as<g1_t>(), dB.as<g2_t>(),
                           delig.as<int32_t>(), d_res, (int)batch);
    if (!ng) { HIP_OK(hipGetLastError()); return HBLS_OK; }
    hipLaunchKernelGGL(k_rlc_chunk_sum, dim3((uint32_t)nc), dim3(RLC_CHUNK), 0, 0,
                       d_perm, (int)nperm, d_cstart, d_ccnt, (int)nc,
                       dA.as<g1_t>(), dB.as<g2_t>(), delig.as<int32_t>(), (int)batch,
                       dPA.as<g1_t>(), dPB.as<g2_t>(), dpcnt.as<int32_t>());
    int32_t *d_gres = gout.as<int32_t>(), *d_gcnt = d_gres + ng;
    hipLaunchKernelGGL(k_rlc_group_sum, dim3((uint32_t)ng), dim3(RLC_CHUNK), 0, 0,
                       d_gid, d_gcs, d_gcc, (int)ng, (int)nc,
                       dPA.as<g1_t>(), dPB.as<g2_t>(), dpcnt.as<int32_t>(),
                       d_hm, d_hm_ok, (int)n_groups,
                       gP.as<g1_t>(), ghm.as<g2_t>(), ghok.as<int32_t>(),
                       gsaff.as<g2aff_t>(), gsflags.as<int32_t>(), d_gcnt);
    launch_verify(gP.as<g1_t>(), ghm.as<g2_t>(), gsaff.as<g2aff_t>(),
                  gsflags.as<int32_t>(), ghok.as<int32_t>(), d_gres, ng);
    HIP_OK(hipGetLastError());
    std::vector<int32_t> hg(2 * ng);
    HIP_OK(hipMemcpy(hg.data(), gout.p, 2 * ng * 4, hipMemcpyDeviceToHost));

    /* groups without an eligible vote are identity-vs-identity (accepted
     * without a pairing); a checked group fails unless its verdict is 1.
     * A failing group of one chunk IS that chunk's combination: its votes go
     * per-item without a second pairing of the same sums. */
    std::vector<uint32_t> sel, failed;
    for (size_t j = 0; j < ng; j++) {
        if (hg[ng + j] <= 0) continue;
        g_rlc_stats[0]++;
        if (hg[j] == 1) continue;
        g_rlc_stats[1]++;
        if (grp_ccnt[j] == 1) { failed.push_back(grp_cstart[j]); continue; }
        for (uint32_t k = 0; k < grp_ccnt[j]; k++) sel.push_back(grp_cstart[j] + k);
    }
    if (sel.empty() && failed.empty()) return HBLS_OK;

    /* refinement level 1: every chunk of a failing multi-chunk group */
    size_t ns = sel.size();
    g_rlc_stats[2] = (uint32_t)ns;
    if (ns) {
        DevBuf dsel(ns * 4), cP(ns * sizeof(g1_t)), chm(ns * sizeof(g2_t)), chok(ns * 4);
        DevBuf csaff(ns * sizeof(g2aff_t)), csflags(ns * 4), cres(ns * 4);
        if (dsel.err || cP.err || chm.err || chok.err || csaff.err || csflags.err ||
            cres.err) return HBLS_ERR;
        HIP_OK(hipMemcpy(dsel.p, sel.data(), ns * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_rlc_chunk_prep, dim3((uint32_t)((ns + 63) / 64)), dim3(64), 0, 0,
                           dsel.as<uint32_t>(), (int)ns, (int)nc, d_cgrp,
                           dPA.as<g1_t>(), dPB.as<g2_t>(), d_hm, d_hm_ok, (int)n_groups,
                           cP.as<g1_t>(), chm.as<g2_t>(), chok.as<int32_t>(),
                           csaff.as<g2aff_t>(), csflags.as<int32_t>());
        launch_verify(cP.as<g1_t>(), chm.as<g2_t>(), csaff.as<g2aff_t>(),
                      csflags.as<int32_t>(), chok.as<int32_t>(), cres.as<int32_t>(), ns);
        HIP_OK(hipGetLastError());
        std::vector<int32_t> hc(ns);
        HIP_OK(hipMemcpy(hc.data(), cres.p, ns * 4, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < ns; j++)
            if (hc[j] != 1) failed.push_back(sel[j]);
    }

    /* refinement level 2: the eligible votes of failing chunks, per item */
    std::vector<int32_t> helig(batch);
    HIP_OK(hipMemcpy(helig.data(), delig.p, batch * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> vsel;
    for (uint32_t ck : failed)
        for (uint32_t t = 0; t < chunk_cnt[ck]; t++) {
            uint32_t v = desc[chunk_start[ck] + t];
            if (helig[v]) vsel.push_back(v);
        }
    if (vsel.empty()) return HBLS_OK;
    size_t nv = vsel.size();
    g_rlc_stats[3] = (uint32_t)nv;
    DevBuf dvsel(nv * 4);
    if (dvsel.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dvsel.p, vsel.data(), nv * 4, hipMemcpyHostToDevice));
    if (d_pks)
        hipLaunchKernelGGL(k_verify_votes_sel_pk, dim3((uint32_t)((nv + 63) / 64)), dim3(64), 0, 0,
                           dvsel.as<uint32_t>(), (int)nv, d_pks, d_pk_ok,
                           d_hm, d_grp, d_saff, d_sflags, d_hm_ok, d_res, (int)batch);
    else
        hipLaunchKernelGGL(k_verify_votes_sel, dim3((uint32_t)((nv + 63) / 64)), dim3(64), 0, 0,
                           dvsel.as<uint32_t>(), (int)nv, c->d_table, (int)c->n, d_idx,
                           d_hm, d_grp, d_saff, d_sflags, d_hm_ok, d_res, (int)batch);
    HIP_OK(hipGetLastError());
    return HBLS_OK;
}

/* largest batch / group count the int-indexed kernels take */
#define RLC_MAX_ITEMS ((size_t)1 << 30)

/* same-message batch verify against one committee: vote j is checked on
 * msgs[group_idx[j]].  Hashes n_groups messages (not batch), then runs the
 * batched chain; per-vote codes as hbls_batch_verify_votes. */
extern "C" int hbls_batch_verify_votes_grouped(const hbls_committee_t *c,
                                               const uint32_t *key_idx,
                                               const uint32_t *group_idx,
                                               const uint8_t *sigs96, const uint8_t *msgs,
                                               size_t msg_len, size_t n_groups,
                                               size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    rlc_stats_reset();
    if (!c || batch == 0 || n_groups == 0 || batch > RLC_MAX_ITEMS ||
        n_groups > RLC_MAX_ITEMS) return HBLS_ERR_BADINPUT;
    DevBuf didx(batch * 4), dgidx(batch * 4), dsig(batch * 96), dmsg(n_groups * msg_len);
    DevBuf dhm(n_groups * sizeof(g2_t)), dhok(n_groups * 4);
    DevBuf dclamp(batch * 4), dpok(batch * 4);
    DevBuf dsaff(batch * sizeof(g2aff_t)), dsflags(batch * 4), dres(batch * 4);
    if (didx.err || dgidx.err || dsig.err || dmsg.err || dhm.err || dhok.err ||
        dclamp.err || dpok.err || dsaff.err || dsflags.err || dres.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(didx.p, key_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dgidx.p, group_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmsg.p, msgs, n_groups * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    /* the hash dispatches on n_groups, the decompress on batch */
    launch_hash_to_g2(dmsg.as<uint8_t>(), msg_len, dhm.as<g2_t>(), dhok.as<int32_t>(), n_groups);
    hipLaunchKernelGGL(k_stream_clamp, dim3(nb), dim3(64), 0, 0,
                       dgidx.as<uint32_t>(), (int)n_groups,
                       dclamp.as<uint32_t>(), dpok.as<int32_t>(), (int)batch);
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    rc = rlc_verify_chain(c, dhm.as<g2_t>(), dhok.as<int32_t>(), n_groups, group_idx,
                          didx.as<uint32_t>(), dclamp.as<uint32_t>(), dpok.as<int32_t>(),
                          dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), dres.as<int32_t>(),
                          batch);
    tm.stop_and_store();
    if (rc != HBLS_OK) return rc;
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_stream_set_verify_mode(hbls_stream *s, int mode) {
    if (!s || (mode != 0 && mode != 1)) return HBLS_ERR_BADINPUT;
    s->verify_mode = mode;
    return HBLS_OK;
}
