/* hbls_multikey.inc — multi-key votes: signer sets in the vote stream
 * (DESIGN.md §4g).
 *
 * A node that runs several BLS keys sends one message per phase: one
 * signature, the sum of its keys' signatures (consensus/construct.go:99-114),
 * and a sender bitmap.  The leader sums the sender keys (leader.go:165-172,
 * :279-286), verifies once against the sum, drops the message if ANY of the
 * keys has voted (leader.go:127-135, :227-235) and otherwise sets all their
 * bits (SetKeysAtomic, crypto/bls/mask.go:226-242).
 *
 * Signer sets cross the ABI in CSR form: vote j is signed by
 * key_idx[key_off[j] .. key_off[j+1]), strictly ascending.  The host checks
 * only the offsets (they size the upload); every index is checked on the
 * device before it is used as an address.
 *
 * Included from hbls_dev.hip after hbls_quorum.inc: it uses the stream
 * kernels, rlc_verify_chain and the verify launch macros. */

#define MK_SHORT_MAX 8          /* keys summed by one thread; longer lists get a block */
#define MK_MAX_KEYS 0x7fffffffu /* total indices per call (uint32 loop counters) */
#define MK_LDS_ROW_MAX 49152    /* bytes of one bitmap row the claim kernel stages */

/* signer-set sum, short lists: one thread per vote.  Validates the whole list
 * (non-empty, every index < n, strictly ascending) before the first table
 * read; a single-key vote is then the plain gather k_verify_votes does.
 * ok[i]: 1 / HBLS_ERR_BADINPUT (sum = infinity).  Lists longer than
 * MK_SHORT_MAX are k_mk_sum_long's. */
__global__ void k_mk_sum_short(const g1aff_t *table, int n, const uint32_t *key_off,
                               const uint32_t *key_idx, g1_t *sums, int32_t *ok,
                               int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    uint32_t b = key_off[i], e = key_off[i + 1];
    if (e - b > MK_SHORT_MAX) return;
    g1_t acc;
    g1_set_inf(acc);
    bool good = e > b;
    uint32_t prev = 0;
    for (uint32_t k = b; k < e; k++) {
        uint32_t v = key_idx[k];
        if (v >= (uint32_t)n || (k > b && v <= prev)) good = false;
        prev = v;
    }
    if (!good) { sums[i] = acc; ok[i] = HBLS_ERR_BADINPUT; return; }
    acc.x = table[key_idx[b]].x;
    acc.y = table[key_idx[b]].y;
    fp_one(acc.z);
    /* g1_madd covers equal keys (doubling) and a key plus its negation
     * (infinity, then restart from the next key) */
    for (uint32_t k = b + 1; k < e; k++) g1_madd(acc, acc, table[key_idx[k]]);
    sums[i] = acc;
    ok[i] = 1;
}

/* signer-set sum, long lists: one 64-lane block per listed vote, the lanes
 * stride over the keys and reduce with an LDS tree (k_stream_accum shape).
 * Same validation, complete before any table read. */
__global__ void __launch_bounds__(64) k_mk_sum_long(
        const g1aff_t *table, int n, const uint32_t *key_off, const uint32_t *key_idx,
        const uint32_t *sel, int nsel, g1_t *sums, int32_t *ok, int batch) {
    int j = blockIdx.x;
    if (j >= nsel) return;
    uint32_t i = sel[j];
    if (i >= (uint32_t)batch) return;
    __shared__ g1_t red[64];
    uint32_t b = key_off[i], e = key_off[i + 1];
    int bad = e <= b;
    for (uint32_t k = b + threadIdx.x; k < e; k += 64) {
        uint32_t v = key_idx[k];
        if (v >= (uint32_t)n || (k > b && v <= key_idx[k - 1])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    g1_t acc;
    g1_set_inf(acc);
    if (bad) {
        if (threadIdx.x == 0) { sums[i] = acc; ok[i] = HBLS_ERR_BADINPUT; }
        return;
    }
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

/* per-vote inputs of the shared verify stage (k_verify_coop / the scalar
 * kernels take hms[i], hm_ok[i]): the vote's hash point, and every reason a
 * vote is malformed folded into its hm_ok flag so the verify kernel reports
 * HBLS_ERR_BADINPUT.  hm_idx NULL: hash points are per vote already, only
 * the flags are folded (hm_out NULL, hmok_out may be hm_ok_in). */
__global__ void k_mk_gather_hm(const g2_t *hms, const uint32_t *hm_idx,
                               const int32_t *hm_ok_in, const int32_t *idx_ok,
                               const int32_t *vote_ok, g2_t *hm_out, int32_t *hmok_out,
                               int batch) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    int h = hm_idx ? (int)hm_idx[i] : i;    /* pre-clamped (k_stream_clamp) */
    hmok_out[i] = (hm_ok_in[h] && (!idx_ok || idx_ok[i]) && vote_ok[i] == 1) ? 1 : 0;
    if (hm_out) hm_out[i] = hms[h];
}

/* ordered all-or-nothing claim (replaces k_stream_dedup for multi-key
 * ticks): one single-wave block per active round, its bitmap row staged in
 * LDS.  The wave scans the tick 64 votes at a time, ballots the valid votes
 * of its round and walks them in ascending batch index — the reference's
 * arrival order under its mutex.  Per vote the lanes stride over its keys:
 * any bit already set -> result 2 and nothing is set; otherwise all bits are
 * set (atomicOr: two keys can share a word).  A vote reaches here with result
 * 1 only after its indices were validated; the range test is kept anyway.
 * add[i] = 1 for the winners whose signature k_stream_accum is to add, for
 * every vote of the block's round: a winner with the identity signature (valid
 * only for a key sum of infinity) has no affine form and adds nothing. */
__global__ void __launch_bounds__(64) k_mk_claim(
        uint32_t *bitmap, int nwords, int n, const uint32_t *slots, int kslots,
        const uint32_t *key_off, const uint32_t *key_idx, const uint32_t *round_idx,
        const int32_t *sig_flags, int32_t *results, int32_t *add, int batch) {
    extern __shared__ uint32_t mk_row[];
    int s = blockIdx.x;
    if (s >= kslots) return;
    uint32_t r = slots[s];
    uint32_t *grow = bitmap + (size_t)r * nwords;
    for (int w = threadIdx.x; w < nwords; w += 64) mk_row[w] = grow[w];
    __syncthreads();
    for (int base = 0; base < batch; base += 64) {
        int i = base + (int)threadIdx.x;
        bool here = i < batch && round_idx[i] == r;
        bool mine = here && results[i] == 1;
        unsigned long long m = __ballot(mine);
        while (m) {
            int lane = __ffsll(m) - 1, v = base + lane;
            m &= m - 1;
            uint32_t b = key_off[v], e = key_off[v + 1];
            int hit = 0;
            for (uint32_t k = b + threadIdx.x; k < e; k += 64) {
                uint32_t id = key_idx[k];
                if (id < (uint32_t)n) hit |= (mk_row[id >> 5] >> (id & 31)) & 1;
            }
            hit = __syncthreads_or(hit);
            if (hit) {
                if ((int)threadIdx.x == lane) { results[v] = 2; mine = false; }
            } else {
                for (uint32_t k = b + threadIdx.x; k < e; k += 64) {
                    uint32_t id = key_idx[k];
                    if (id < (uint32_t)n) atomicOr(&mk_row[id >> 5], 1u << (id & 31));
                }
            }
            __syncthreads();
        }
        if (here) add[i] = (mine && sig_flags[i] == 1) ? 1 : 0;
    }
    for (int w = threadIdx.x; w < nwords; w += 64) grow[w] = mk_row[w];
}

/* ---------------------------------------------------------------- host */

/* offsets start at 0, never decrease, and stay within the loop counters;
 * *total = key_off[batch] */
static int mk_check_offsets(const uint32_t *key_off, size_t batch, size_t *total) {
    if (!key_off || key_off[0] != 0) return HBLS_ERR_BADINPUT;
    for (size_t j = 0; j < batch; j++)
        if (key_off[j + 1] < key_off[j]) return HBLS_ERR_BADINPUT;
    if (key_off[batch] > MK_MAX_KEYS) return HBLS_ERR_BADINPUT;
    *total = key_off[batch];
    return HBLS_OK;
}

/* enqueue the signer-set sums of a tick: the thread-per-vote kernel over the
 * whole batch, plus one block per vote longer than MK_SHORT_MAX (the host
 * partitions by list length; h_off is the caller's offset array). */
static int mk_launch_sums(const hbls_committee_t *c, const uint32_t *h_off,
                          const uint32_t *d_off, const uint32_t *d_idx, size_t batch,
                          g1_t *d_sums, int32_t *d_ok) {
    std::vector<uint32_t> longv;
    for (size_t j = 0; j < batch; j++)
        if (h_off[j + 1] - h_off[j] > MK_SHORT_MAX) longv.push_back((uint32_t)j);
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_mk_sum_short, dim3(nb), dim3(64), 0, 0,
                       c->d_table, (int)c->n, d_off, d_idx, d_sums, d_ok, (int)batch);
    if (!longv.empty()) {
        DevBuf dsel(longv.size() * 4);
        if (dsel.err) return HBLS_ERR;
        HIP_OK(hipMemcpy(dsel.p, longv.data(), longv.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_mk_sum_long, dim3((uint32_t)longv.size()), dim3(64), 0, 0,
                           c->d_table, (int)c->n, d_off, d_idx, dsel.as<uint32_t>(),
                           (int)longv.size(), d_sums, d_ok, (int)batch);
        HIP_OK(hipDeviceSynchronize());     /* dsel is freed at scope exit */
    }
    HIP_OK(hipGetLastError());
    return HBLS_OK;
}

extern "C" int hbls_vote_key_sums(const hbls_committee_t *c, const uint32_t *key_off,
                                  const uint32_t *key_idx, size_t batch,
                                  uint8_t *out48s, int32_t *ok) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!c || batch == 0 || batch > RLC_MAX_ITEMS || !out48s || !ok) return HBLS_ERR_BADINPUT;
    size_t total = 0;
    rc = mk_check_offsets(key_off, batch, &total);
    if (rc != HBLS_OK) return rc;
    if (total && !key_idx) return HBLS_ERR_BADINPUT;
    DevBuf doff((batch + 1) * 4), didx(total * 4), dsums(batch * sizeof(g1_t));
    DevBuf dok(batch * 4), dser(batch * 48);
    if (doff.err || didx.err || dsums.err || dok.err || dser.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(doff.p, key_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    if (total) HIP_OK(hipMemcpy(didx.p, key_idx, total * 4, hipMemcpyHostToDevice));
    Timer tm;
    rc = mk_launch_sums(c, key_off, doff.as<uint32_t>(), didx.as<uint32_t>(), batch,
                        dsums.as<g1_t>(), dok.as<int32_t>());
    if (rc == HBLS_OK)
        hipLaunchKernelGGL(k_g1_serialize, dim3((uint32_t)((batch + 63) / 64)), dim3(64), 0, 0,
                           dsums.as<g1_t>(), dser.as<uint8_t>(), (int)batch);
    tm.stop_and_store();
    if (rc != HBLS_OK) return rc;
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out48s, dser.p, batch * 48, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ok, dok.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_batch_verify_votes_multi(const hbls_committee_t *c,
                                             const uint32_t *key_off,
                                             const uint32_t *key_idx, const uint8_t *sigs96,
                                             const uint8_t *msgs, size_t msg_len,
                                             size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!c || batch == 0 || batch > RLC_MAX_ITEMS) return HBLS_ERR_BADINPUT;
    size_t total = 0;
    rc = mk_check_offsets(key_off, batch, &total);
    if (rc != HBLS_OK) return rc;
    if (total && !key_idx) return HBLS_ERR_BADINPUT;
    DevBuf doff((batch + 1) * 4), didx(total * 4), dsig(batch * 96), dmsg(batch * msg_len);
    DevBuf dsums(batch * sizeof(g1_t)), dvok(batch * 4);
    DevBuf dhm(batch * sizeof(g2_t)), dsaff(batch * sizeof(g2aff_t));
    DevBuf dsflags(batch * 4), dhok(batch * 4), dres(batch * 4);
    if (doff.err || didx.err || dsig.err || dmsg.err || dsums.err || dvok.err ||
        dhm.err || dsaff.err || dsflags.err || dhok.err || dres.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(doff.p, key_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    if (total) HIP_OK(hipMemcpy(didx.p, key_idx, total * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmsg.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    rc = mk_launch_sums(c, key_off, doff.as<uint32_t>(), didx.as<uint32_t>(), batch,
                        dsums.as<g1_t>(), dvok.as<int32_t>());
    if (rc != HBLS_OK) { tm.stop_and_store(); return rc; }
    launch_hash_to_g2(dmsg.as<uint8_t>(), msg_len, dhm.as<g2_t>(), dhok.as<int32_t>(), batch);
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    hipLaunchKernelGGL(k_mk_gather_hm, dim3(nb), dim3(64), 0, 0,
                       (const g2_t *)nullptr, (const uint32_t *)nullptr, dhok.as<int32_t>(),
                       (const int32_t *)nullptr, dvok.as<int32_t>(), (g2_t *)nullptr,
                       dhok.as<int32_t>(), (int)batch);
    /* the verify stage of run_agg_verify_pipeline, key sums for masked sums */
    launch_verify(dsums.as<g1_t>(), dhm.as<g2_t>(), dsaff.as<g2aff_t>(),
                  dsflags.as<int32_t>(), dhok.as<int32_t>(), dres.as<int32_t>(), batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* one tick of multi-key votes: signer-set sums -> verify against the sums ->
 * ordered all-or-nothing claim -> per-round accumulate.  results per vote:
 * 1 accepted (all bits set, signature added once), 2 valid but a key had
 * voted (nothing set, nothing added), 0 invalid, HBLS_ERR_BADINPUT
 * malformed.  Votes take effect as if applied in ascending batch index. */
extern "C" int hbls_stream_process_multi(hbls_stream *s, const uint32_t *key_off,
                                         const uint32_t *key_idx, const uint32_t *round_idx,
                                         const uint8_t *sigs96, const uint32_t *active_slots,
                                         int n_active, size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    rlc_stats_reset();
    if (!s || batch == 0 || n_active <= 0 || batch > RLC_MAX_ITEMS) return HBLS_ERR_BADINPUT;
    if ((size_t)s->nwords * 4 > MK_LDS_ROW_MAX) return HBLS_ERR_BADINPUT;
    /* one claim block per slot owns that round's row: slots must be distinct,
     * and must cover every in-range round of the tick (a valid vote of an
     * unlisted round would report 1 and take no effect) */
    std::vector<uint8_t> listed((size_t)s->max_rounds, 0);
    for (int i = 0; i < n_active; i++) {
        if (active_slots[i] >= (uint32_t)s->max_rounds || listed[active_slots[i]])
            return HBLS_ERR_BADINPUT;
        listed[active_slots[i]] = 1;
    }
    for (size_t j = 0; j < batch; j++)
        if (round_idx[j] < (uint32_t)s->max_rounds && !listed[round_idx[j]])
            return HBLS_ERR_BADINPUT;
    size_t total = 0;
    rc = mk_check_offsets(key_off, batch, &total);
    if (rc != HBLS_OK) return rc;
    if (total && !key_idx) return HBLS_ERR_BADINPUT;
    DevBuf doff((batch + 1) * 4), didx(total * 4), dridx(batch * 4), dsig(batch * 96);
    DevBuf dclamp(batch * 4), dpok(batch * 4), dsums(batch * sizeof(g1_t)), dvok(batch * 4);
    DevBuf dsaff(batch * sizeof(g2aff_t)), dsflags(batch * 4), dres(batch * 4);
    DevBuf dact(n_active * 4), dadd(batch * 4);
    size_t gsz = s->verify_mode == 1 ? 1 : batch;   /* per-vote hash points, mode 0 */
    DevBuf ghm(gsz * sizeof(g2_t)), ghok(gsz * 4);
    if (doff.err || didx.err || dridx.err || dsig.err || dclamp.err || dpok.err ||
        dsums.err || dvok.err || dsaff.err || dsflags.err || dres.err || dact.err ||
        dadd.err || ghm.err || ghok.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(doff.p, key_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    if (total) HIP_OK(hipMemcpy(didx.p, key_idx, total * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dridx.p, round_idx, batch * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dact.p, active_slots, n_active * 4, hipMemcpyHostToDevice));
    Timer tm;
    int nb = (int)((batch + 63) / 64);
    hipLaunchKernelGGL(k_stream_clamp, dim3(nb), dim3(64), 0, 0,
                       dridx.as<uint32_t>(), s->max_rounds,
                       dclamp.as<uint32_t>(), dpok.as<int32_t>(), (int)batch);
    rc = mk_launch_sums(s->c, key_off, doff.as<uint32_t>(), didx.as<uint32_t>(), batch,
                        dsums.as<g1_t>(), dvok.as<int32_t>());
    if (rc != HBLS_OK) { tm.stop_and_store(); return rc; }
    launch_g2_decompress(dsig.as<uint8_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), batch);
    if (s->verify_mode == 1) {
        rc = rlc_verify_chain(s->c, s->d_hm, s->d_hm_ok, (size_t)s->max_rounds, round_idx,
                              (const uint32_t *)nullptr, dclamp.as<uint32_t>(),
                              dpok.as<int32_t>(), dsaff.as<g2aff_t>(), dsflags.as<int32_t>(),
                              dres.as<int32_t>(), batch, dsums.as<g1_t>(), dvok.as<int32_t>());
        if (rc != HBLS_OK) { tm.stop_and_store(); return rc; }
    } else {
        hipLaunchKernelGGL(k_mk_gather_hm, dim3(nb), dim3(64), 0, 0,
                           s->d_hm, dclamp.as<uint32_t>(), s->d_hm_ok, dpok.as<int32_t>(),
                           dvok.as<int32_t>(), ghm.as<g2_t>(), ghok.as<int32_t>(), (int)batch);
        launch_verify(dsums.as<g1_t>(), ghm.as<g2_t>(), dsaff.as<g2aff_t>(),
                      dsflags.as<int32_t>(), ghok.as<int32_t>(), dres.as<int32_t>(), batch);
    }
    hipLaunchKernelGGL(k_merge_pok, dim3(nb), dim3(64), 0, 0,
                       dres.as<int32_t>(), dpok.as<int32_t>(), (int)batch);
    hipLaunchKernelGGL(k_mk_claim, dim3(n_active), dim3(64), (size_t)s->nwords * 4, 0,
                       s->d_bitmap, s->nwords, (int)s->c->n, dact.as<uint32_t>(), n_active,
                       doff.as<uint32_t>(), didx.as<uint32_t>(), dclamp.as<uint32_t>(),
                       dsflags.as<int32_t>(), dres.as<int32_t>(), dadd.as<int32_t>(),
                       (int)batch);
    /* k_stream_accum reads its flag only for votes of a listed round, all of
     * which the claim wrote */
    hipLaunchKernelGGL(k_stream_accum, dim3(n_active), dim3(64), 0, 0,
                       s->d_agg, dact.as<uint32_t>(), n_active, dclamp.as<uint32_t>(),
                       dsaff.as<g2aff_t>(), dadd.as<int32_t>(), (int)batch);
    tm.stop_and_store();
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(results, dres.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
