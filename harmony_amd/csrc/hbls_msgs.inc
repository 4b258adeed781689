/* hbls_msgs.inc — signed-message windows: mixed contexts, mixed messages
 * (DESIGN.md §4p).
 *
 * The vote side of §4i.  A view change brings the new leader two single
 * verifies per VIEWCHANGE message (consensus/checks.go:186,
 * consensus/view_change_construct.go:266,339) over three distinct byte
 * strings; sender authentication (consensus/checks.go:20-39) verifies a
 * signature over the Keccak-256 digest of raw message bytes
 * (crypto/hash/hash.go:9-15); one device serves several shards.  Here every
 * item names its committee, its signer set and an entry of a message table;
 * a table entry is hashed to G2 once however many items sign it, and an entry
 * flagged as digested is Keccak'd on the device first.
 *
 * Included from hbls_dev.hip after hbls_ctxset.inc and hbls_multikey.inc: it
 * uses cx_ctx, CX_MSG_SLOT, cx_check_offsets, MK_SHORT_MAX, mk_check_offsets,
 * k_mk_gather_hm, keccak256_dev and the stage launchers.
 *
 * Barriers.  k_msgs_sum_long gives every listed item a block of one wave, so
 * a block never holds two items: the validation verdict goes through
 * __syncthreads_or before anyone leaves, and the levels of the reduction tree
 * are a constant.  The early returns ahead of the first barrier depend on
 * blockIdx alone.  k_msgs_stage and k_msgs_sum_short have no barrier.
 *
 * Alignment.  Message bytes stay where they were uploaded, at msg_off[i], and
 * are read by bytes; slots are 48 bytes apart and written by bytes.
 *
 * A launch never depends on the number of contexts or of distinct lengths:
 * stage, hash (n_msgs), key sums (short, long), decompress, gather, verify. */

#define MS_MAX_ENTRY 0x7fffffffu    /* bytes of one table entry (keccak256_dev's int length) */

/* Message staging: one thread per table entry.  An undigested entry gives its
 * first min(len, 48) bytes, zero-padded — k_ctx_prepare's slot rule, so hashing
 * the slot with mlen = 48 is hbls_hash_to_g2 of the original bytes.  A
 * digested entry gives keccak256 of all its bytes in 0..31 and zeros after.
 * digest NULL: no entry is digested. */
__global__ void k_msgs_stage(const uint8_t *msgs, const uint32_t *msg_off,
                             const uint8_t *digest, uint8_t *slots, int n_msgs) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_msgs) return;
    uint32_t b = msg_off[i], len = msg_off[i + 1] - b;
    const uint8_t *m = msgs + (size_t)b;
    uint8_t slot[CX_MSG_SLOT];
    for (int k = 0; k < CX_MSG_SLOT; k++) slot[k] = 0;
    if (digest && digest[i]) {
        keccak256_dev(m, (int)len, slot);
    } else {
        uint32_t nb = len < CX_MSG_SLOT ? len : CX_MSG_SLOT;
        for (uint32_t k = 0; k < nb; k++) slot[k] = m[k];
    }
    uint8_t *out = slots + (size_t)i * CX_MSG_SLOT;
    for (int k = 0; k < CX_MSG_SLOT; k++) out[k] = slot[k];
}

/* signer-set sum, short lists: k_mk_sum_short with table and n taken from the
 * item's context.  One thread per item.  The item is judged whole — context
 * index, message index, list non-empty, every key index < n of its own
 * context, strictly ascending — before the context's table pointer or any
 * key is read.  hm_idx[i] = the message index, 0 where out of range, for
 * k_mk_gather_hm (written for long lists too).  ok[i]: 1 /
 * HBLS_ERR_BADINPUT (sum = infinity).  Lists longer than MK_SHORT_MAX are
 * k_msgs_sum_long's. */
__global__ void k_msgs_sum_short(const cx_ctx *ctxs, uint32_t n_ctx, const uint32_t *ctx_idx,
                                 const uint32_t *key_off, const uint32_t *key_idx,
                                 const uint32_t *msg_idx, uint32_t n_msgs, g1_t *sums,
                                 int32_t *ok, uint32_t *hm_idx, int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    uint32_t ci = ctx_idx[i], mi = msg_idx[i];
    hm_idx[i] = mi < n_msgs ? mi : 0;
    uint32_t b = key_off[i], e = key_off[i + 1];
    if (e - b > MK_SHORT_MAX) return;
    g1_t acc;
    g1_set_inf(acc);
    bool good = ci < n_ctx && mi < n_msgs && e > b;
    uint32_t n = good ? ctxs[ci].n : 0;
    uint32_t prev = 0;
    for (uint32_t k = b; k < e; k++) {
        uint32_t v = key_idx[k];
        if (v >= n || (k > b && v <= prev)) good = false;
        prev = v;
    }
    if (!good) { sums[i] = acc; ok[i] = HBLS_ERR_BADINPUT; return; }
    const g1aff_t *table = ctxs[ci].table;
    acc.x = table[key_idx[b]].x;
    acc.y = table[key_idx[b]].y;
    fp_one(acc.z);
    /* g1_madd covers a key plus its negation (infinity, then restart) */
    for (uint32_t k = b + 1; k < e; k++) g1_madd(acc, acc, table[key_idx[k]]);
    sums[i] = acc;
    ok[i] = 1;
}

/* signer-set sum, long lists: k_mk_sum_long with table and n taken from the
 * item's context.  One 64-lane block (one wave) per listed item; same
 * judgement, complete and agreed on by the whole block before any table
 * read. */
__global__ void __launch_bounds__(64) k_msgs_sum_long(
        const cx_ctx *ctxs, uint32_t n_ctx, const uint32_t *ctx_idx, const uint32_t *key_off,
        const uint32_t *key_idx, const uint32_t *msg_idx, uint32_t n_msgs,
        const uint32_t *sel, int nsel, g1_t *sums, int32_t *ok, int batch) {
    int j = blockIdx.x;
    if (j >= nsel) return;
    uint32_t i = sel[j];
    if (i >= (uint32_t)batch) return;
    __shared__ g1_t red[64];
    uint32_t ci = ctx_idx[i], mi = msg_idx[i];
    uint32_t b = key_off[i], e = key_off[i + 1];
    int bad = ci >= n_ctx || mi >= n_msgs || e <= b;
    uint32_t n = bad ? 0 : ctxs[ci].n;
    for (uint32_t k = b + threadIdx.x; k < e; k += 64) {
        uint32_t v = key_idx[k];
        if (v >= n || (k > b && v <= key_idx[k - 1])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    g1_t acc;
    g1_set_inf(acc);
    if (bad) {
        if (threadIdx.x == 0) { sums[i] = acc; ok[i] = HBLS_ERR_BADINPUT; }
        return;
    }
    const g1aff_t *table = ctxs[ci].table;
    for (uint32_t k = b + threadIdx.x; k < e; k += 64)
        g1_madd(acc, acc, table[key_idx[k]]);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            g1_t t;
            g1_add(t, red[threadIdx.x], red[threadIdx.x + st]);
            red[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[i] = red[0]; ok[i] = 1; }
}

/* ---------------------------------------------------------------- host */

extern "C" int hbls_batch_verify_msgs_ctx(const hbls_ctxset_t *s, const uint32_t *ctx_idx,
                                          const uint32_t *key_off, const uint32_t *key_idx,
                                          const uint8_t *sigs96, const uint32_t *msg_idx,
                                          const uint8_t *msgs, const uint32_t *msg_off,
                                          size_t n_msgs, const uint8_t *msg_digest,
                                          size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!s || !ctx_idx || !sigs96 || !msg_idx || !results || batch == 0 || n_msgs == 0 ||
        batch > RLC_MAX_ITEMS || n_msgs > RLC_MAX_ITEMS) return HBLS_ERR_BADINPUT;
    size_t total = 0, nbytes = 0;
    rc = mk_check_offsets(key_off, batch, &total);
    if (rc != HBLS_OK) return rc;
    rc = cx_check_offsets(msg_off, n_msgs, &nbytes);
    if (rc != HBLS_OK) return rc;
    if ((total && !key_idx) || (nbytes && !msgs)) return HBLS_ERR_BADINPUT;
    for (size_t i = 0; i < n_msgs; i++)
        if (msg_off[i + 1] - msg_off[i] > MS_MAX_ENTRY) return HBLS_ERR_BADINPUT;
    /* the host partitions by list length, as mk_launch_sums does */
    std::vector<uint32_t> longv;
    for (size_t j = 0; j < batch; j++)
        if (key_off[j + 1] - key_off[j] > MK_SHORT_MAX) longv.push_back((uint32_t)j);

    DevBuf dci(batch * 4), doff((batch + 1) * 4), didx(total * 4), dsig(batch * 96);
    DevBuf dmi(batch * 4), dmsgs(nbytes), dmoff((n_msgs + 1) * 4);
    DevBuf ddig(n_msgs, msg_digest != nullptr), dsel(longv.size() * 4, !longv.empty());
    DevBuf dslots(n_msgs * CX_MSG_SLOT), dhm(n_msgs * sizeof(g2_t)), dhok(n_msgs * 4);
    DevBuf dsums(batch * sizeof(g1_t)), dvok(batch * 4), dhmi(batch * 4);
    DevBuf dsaff(batch * sizeof(g2aff_t)), dsflags(batch * 4);
    DevBuf ghm(batch * sizeof(g2_t)), ghok(batch * 4), dres(batch * 4);
    if (dci.err || doff.err || didx.err || dsig.err || dmi.err || dmsgs.err || dmoff.err ||
        ddig.err || dsel.err || dslots.err || dhm.err || dhok.err || dsums.err || dvok.err ||
        dhmi.err || dsaff.err || dsflags.err || ghm.err || ghok.err || dres.err)
        return HBLS_ERR;
    HIP_OK(hipMemcpy(dci.p, ctx_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(doff.p, key_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    if (total) HIP_OK(hipMemcpy(didx.p, key_idx, total * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmi.p, msg_idx, batch * 4, hipMemcpyHostToDevice));
    if (nbytes) HIP_OK(hipMemcpy(dmsgs.p, msgs, nbytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmoff.p, msg_off, (n_msgs + 1) * 4, hipMemcpyHostToDevice));
    if (msg_digest) HIP_OK(hipMemcpy(ddig.p, msg_digest, n_msgs, hipMemcpyHostToDevice));
    if (!longv.empty())
        HIP_OK(hipMemcpy(dsel.p, longv.data(), longv.size() * 4, hipMemcpyHostToDevice));

    Timer tm;
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_msgs_stage, dim3((uint32_t)((n_msgs + 63) / 64)), dim3(64), 0, 0,
                       dmsgs.as<uint8_t>(), dmoff.as<uint32_t>(), ddig.as<uint8_t>(),
                       dslots.as<uint8_t>(), (int)n_msgs);
    /* the table, not the batch: a shared message is hashed once */
    launch_hash_to_g2(dslots.as<uint8_t>(), CX_MSG_SLOT, dhm.as<g2_t>(), dhok.as<int32_t>(),
                      n_msgs);
    hipLaunchKernelGGL(k_msgs_sum_short, dim3(nb), dim3(64), 0, 0,
                       s->d_ctx, (uint32_t)s->n_ctx, dci.as<uint32_t>(), doff.as<uint32_t>(),
                       didx.as<uint32_t>(), dmi.as<uint32_t>(), (uint32_t)n_msgs,
                       dsums.as<g1_t>(), dvok.as<int32_t>(), dhmi.as<uint32_t>(), (int)batch);
    if (!longv.empty())
        hipLaunchKernelGGL(k_msgs_sum_long, dim3((uint32_t)longv.size()), dim3(64), 0, 0,
                           s->d_ctx, (uint32_t)s->n_ctx, dci.as<uint32_t>(),
                           doff.as<uint32_t>(), didx.as<uint32_t>(), dmi.as<uint32_t>(),
                           (uint32_t)n_msgs, dsel.as<uint32_t>(), (int)longv.size(),
                           dsums.as<g1_t>(), dvok.as<int32_t>(), (int)batch);
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    hipLaunchKernelGGL(k_mk_gather_hm, dim3(nb), dim3(64), 0, 0,
                       dhm.as<g2_t>(), dhmi.as<uint32_t>(), dhok.as<int32_t>(),
                       (const int32_t *)nullptr, dvok.as<int32_t>(), ghm.as<g2_t>(),
                       ghok.as<int32_t>(), (int)batch);
    launch_verify(dsums.as<g1_t>(), ghm.as<g2_t>(), dsaff.as<g2aff_t>(),
                  dsflags.as<int32_t>(), ghok.as<int32_t>(), dres.as<int32_t>(), batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
