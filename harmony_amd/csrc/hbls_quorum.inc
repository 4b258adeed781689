/* hbls_quorum.inc — quorum by mask on device (DESIGN.md §4f).
 *
 * IsQuorumAchievedByMask (consensus/quorum/one-node-staked-vote.go:151-164,
 * one-node-one-vote.go:57-72) for a whole batch of bitmaps: per item the
 * masked voting-power sum and the in-range popcount, then
 *      quorum  <=>  sum > threshold          (strictly)
 * Power is uint64 in units of 1e-18 (the integer inside a numeric.Dec); the
 * uniform policy is weight 1 per key against floor(2n/3).
 *
 * Included from hbls_dev.hip after the stream kernels: it uses HIP_OK,
 * DevBuf, g_stage_ns, run_agg_verify_pipeline and struct hbls_stream.
 *
 * Kernel shape: L = 2^k lanes share one bitmap row, one 8-byte word per lane
 * and step (L = 64 for the 512-byte row of a 4096-key committee, 4 for a
 * 32-byte row), so the lanes of an item read consecutive words and a wave
 * reads 64/L consecutive rows.  Blocks are persistent (grid-stride over
 * groups of MP_THREADS/L items) so the power table is staged in LDS once per
 * block, not once per item. */

#define MP_THREADS 512
#define MP_MAX_BLOCKS 1024      /* 4 blocks of 512 threads per CU: every wave slot */
#define MP_LDS_KEYS 4096        /* table in LDS up to this many keys (32 KiB) */
#define MP_UNIFORM 0            /* popcount only */
#define MP_LDS 1                /* staked, table staged in LDS */
#define MP_GLOBAL 2             /* staked, table read through L2 */

/* up to 8 bytes of a row as a little-endian word.  align is what the host
 * established for every row start: 8, 4 or 1. */
__device__ __forceinline__ uint64_t mp_load_word(const uint8_t *p, int nb, int align) {
    if (align == 8 && nb == 8) return *(const uint64_t *)p;
    uint64_t v = 0;
    int b = 0;
    if (align >= 4)
        for (; b + 4 <= nb; b += 4) v |= (uint64_t)(*(const uint32_t *)(p + b)) << (8 * b);
    for (; b < nb; b++) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

/* one lane's share of one row: words sub, sub+L, ... of the row's
 * ceil(row_bytes/8); bits >= n are masked off.  Serves dense batch rows and
 * the stream's resident word rows alike (the word array is the LE byte
 * layout).  tab is the LDS copy (MP_LDS) or the global table (MP_GLOBAL). */
template <int MODE>
__device__ __forceinline__ void mp_row_partial(const uint8_t *row, int row_bytes, int n,
                                               int align, int sub, int L,
                                               const uint64_t *tab,
                                               uint64_t &sum, uint32_t &cnt) {
    int nw = (row_bytes + 7) >> 3;
    for (int w = sub; w < nw; w += L) {
        int nb = row_bytes - 8 * w;
        if (nb > 8) nb = 8;
        uint64_t v = mp_load_word(row + 8 * (size_t)w, nb, align);
        int valid = n - 64 * w;                 /* >= 1: w < ceil(n/64) */
        if (valid < 64) v &= (1ULL << valid) - 1;
        cnt += (uint32_t)__popcll(v);
        if (MODE != MP_UNIFORM && v) {
            /* all 64 bits, no branch on the data; lane `sub` starts at bit
             * `sub` so that the lanes of a wave, whose words lie 512 B apart
             * in the table, hit 64 different LDS banks */
            int base = 64 * w, last = n - 1;
#pragma unroll 8
            for (int b = 0; b < 64; b++) {
                int bit = (b + sub) & 63;
                int idx = base + bit;
                uint64_t p = tab[idx < last ? idx : last];
                sum += ((v >> bit) & 1) ? p : 0;
            }
        }
    }
}

/* rows: byte base of the bitmap rows, row_stride bytes apart, row_bytes valid
 * bytes each; slots (may be NULL) selects the row of item i, else row i.
 * Every output may be NULL.  live_count must be zeroed by the caller.
 * MP_LDS: the dynamic LDS holds the table, 8n bytes. */
template <int MODE>
__global__ void __launch_bounds__(MP_THREADS) k_mask_power(
        const uint8_t *rows, size_t row_stride, int row_bytes, int align,
        const uint32_t *slots, int n, const uint64_t *power, uint64_t threshold,
        int lanes_log2, uint64_t *power_out, uint32_t *count_out,
        int32_t *live_out, uint32_t *live_count, int items) {
    extern __shared__ uint64_t mp_tab[];
    __shared__ uint32_t block_live;
    const uint64_t *tab = power;
    if (threadIdx.x == 0) block_live = 0;
    uint32_t wave_live = 0;         /* live items this wave has seen (wave-uniform) */
    if (MODE == MP_LDS) {
        for (int i = threadIdx.x; i < n; i += MP_THREADS) mp_tab[i] = power[i];
        __syncthreads();
        tab = mp_tab;
    }
    int L = 1 << lanes_log2;
    int per_block = MP_THREADS >> lanes_log2;
    int sub = threadIdx.x & (L - 1);
    int ngroups = (items + per_block - 1) / per_block;
    /* the trip count is uniform over the block: the shuffles below need
     * every lane of the wave */
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        int item = g * per_block + (threadIdx.x >> lanes_log2);
        bool have = item < items;
        uint64_t sum = 0;
        uint32_t cnt = 0;
        if (have) {
            size_t r = slots ? slots[item] : (size_t)item;
            mp_row_partial<MODE>(rows + r * row_stride, row_bytes, n, align, sub, L,
                                 tab, sum, cnt);
        }
        for (int off = L >> 1; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            if (MODE != MP_UNIFORM) sum += __shfl_xor((unsigned long long)sum, off, 64);
        }
        if (MODE == MP_UNIFORM) sum = cnt;
        bool live = have && sub == 0 && sum > threshold;
        if (have && sub == 0) {
            if (power_out) power_out[item] = sum;
            if (count_out) count_out[item] = cnt;
            if (live_out) live_out[item] = live ? 1 : 0;
        }
        wave_live += (uint32_t)__popcll(__ballot(live));
    }
    /* one global atomic per block: a quarter of a million same-address
     * atomics (one per wave and step) cost more than the whole kernel */
    if (live_count) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && wave_live) atomicAdd(&block_live, wave_live);
        __syncthreads();
        if (threadIdx.x == 0 && block_live) atomicAdd(live_count, block_live);
    }
}

/* dense copies of the live items' bitmaps, signatures and messages: one
 * block per live item, idx[k] = its position in the full batch */
__global__ void __launch_bounds__(256) k_quorum_gather(
        const uint32_t *idx, int nlive, const uint8_t *bm, int bmlen,
        const uint8_t *sig, const uint8_t *msg, int msg_len,
        uint8_t *bm_out, uint8_t *sig_out, uint8_t *msg_out) {
    int k = blockIdx.x;
    if (k >= nlive) return;
    size_t j = idx[k];
    for (int i = threadIdx.x; i < bmlen; i += 256)
        bm_out[(size_t)k * bmlen + i] = bm[j * bmlen + i];
    for (int i = threadIdx.x; i < 96; i += 256)
        sig_out[(size_t)k * 96 + i] = sig[j * 96 + i];
    for (int i = threadIdx.x; i < msg_len; i += 256)
        msg_out[(size_t)k * msg_len + i] = msg[j * msg_len + i];
}

/* ---------------------------------------------------------------- host */

static int mp_lanes_log2(size_t row_bytes) {
    size_t nw = (row_bytes + 7) / 8;
    int l = 0;
    while (l < 6 && ((size_t)1 << l) < nw) l++;
    return l;
}

static int mp_align(const void *base, size_t stride) {
    uintptr_t a = (uintptr_t)base | (uintptr_t)stride;
    return (a & 7) == 0 ? 8 : (a & 3) == 0 ? 4 : 1;
}

/* enqueue k_mask_power on the default stream over `items` rows */
static int launch_mask_power(const hbls_committee_t *c, const uint8_t *d_rows,
                             size_t row_stride, const uint32_t *d_slots, size_t items,
                             uint64_t *d_power, uint32_t *d_count, int32_t *d_live,
                             uint32_t *d_nlive) {
    if (c->n == 0 || c->n > 0x7fffffc0u || items == 0 || items > 0x7fffffffu / 2)
        return HBLS_ERR_BADINPUT;
    size_t bm = (c->n + 7) / 8;
    int ll = mp_lanes_log2(bm);
    size_t per_block = MP_THREADS >> ll;
    size_t ngroups = (items + per_block - 1) / per_block;
    int nb = (int)(ngroups < MP_MAX_BLOCKS ? ngroups : MP_MAX_BLOCKS);
    int align = mp_align(d_rows, row_stride);
    if (d_nlive) HIP_OK(hipMemsetAsync(d_nlive, 0, 4, 0));
#define MP_LAUNCH(MODE, lds) hipLaunchKernelGGL(k_mask_power<MODE>, dim3(nb), dim3(MP_THREADS), \
        (lds), 0, d_rows, row_stride, (int)bm, align, d_slots, (int)c->n, c->d_power, \
        c->q_threshold, ll, d_power, d_count, d_live, d_nlive, (int)items)
    if (c->q_uniform) MP_LAUNCH(MP_UNIFORM, 0);
    else if (c->n <= MP_LDS_KEYS) MP_LAUNCH(MP_LDS, c->n * 8);
    else MP_LAUNCH(MP_GLOBAL, 0);
#undef MP_LAUNCH
    HIP_OK(hipGetLastError());
    return HBLS_OK;
}

extern "C" int hbls_committee_set_quorum(hbls_committee_t *c, const uint64_t *power,
                                         uint64_t threshold) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!c || c->n == 0) return HBLS_ERR_BADINPUT;
    std::vector<uint64_t> ones;
    if (!power) {
        ones.assign(c->n, 1);
        threshold = (uint64_t)(2 * c->n / 3);
    } else {
        const uint64_t cap = 1ULL << 63;
        uint64_t sum = 0;
        for (size_t i = 0; i < c->n; i++) {
            if (power[i] > cap - sum) return HBLS_ERR_BADINPUT;
            sum += power[i];
        }
    }
    HIP_OK(hipMemcpy(c->d_power, power ? power : ones.data(), c->n * 8,
                     hipMemcpyHostToDevice));
    c->q_threshold = threshold;
    c->q_uniform = power ? 0 : 1;
    c->q_set = 1;
    return HBLS_OK;
}

extern "C" int hbls_mask_power(const hbls_committee_t *c, const uint8_t *bitmaps,
                               size_t batch, uint64_t *power_out, uint32_t *count_out) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!c || !bitmaps || batch == 0) return HBLS_ERR_BADINPUT;
    size_t bm = (c->n + 7) / 8;
    DevBuf dbm(batch * bm), dpow(batch * 8), dcnt(batch * 4);
    if (dbm.err || dpow.err || dcnt.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dbm.p, bitmaps, batch * bm, hipMemcpyHostToDevice));
    Timer tm;
    rc = launch_mask_power(c, dbm.as<uint8_t>(), bm, nullptr, batch,
                           dpow.as<uint64_t>(), dcnt.as<uint32_t>(), nullptr, nullptr);
    tm.stop_and_store();
    if (rc != HBLS_OK) return rc;
    g_stage_ns[7] = g_last_ns;
    HIP_OK(hipGetLastError());
    if (power_out) HIP_OK(hipMemcpy(power_out, dpow.p, batch * 8, hipMemcpyDeviceToHost));
    if (count_out) HIP_OK(hipMemcpy(count_out, dcnt.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

/* measurement aid (tools/quorum_ab.py): device time of one device-to-device
 * copy of `bytes`, between the same HIP events the stage times use — the
 * memory-bound yardstick for k_mask_power.  0 on failure. */
extern "C" uint64_t hbls_copy_bench_ns(size_t bytes) {
    if (require_gpu() != HBLS_OK || bytes == 0) return 0;
    DevBuf src(bytes), dst(bytes);
    if (src.err || dst.err) return 0;
    if (hipMemset(src.p, 0x5a, bytes) != hipSuccess) return 0;
    if (hipMemcpy(dst.p, src.p, bytes, hipMemcpyDeviceToDevice) != hipSuccess) return 0;  /* warm */
    uint64_t keep = g_last_ns;
    Timer tm;
    hipError_t e = hipMemcpyAsync(dst.p, src.p, bytes, hipMemcpyDeviceToDevice, 0);
    tm.stop_and_store();
    uint64_t ns = g_last_ns;
    g_last_ns = keep;
    return e == hipSuccess ? ns : 0;
}

/* verifySignature (internal/chain/engine.go:619-642) over device-resident
 * inputs: k_mask_power decides which items are live; all live -> the
 * pipeline runs on the inputs as they are; otherwise on dense copies of the
 * live items, and the verdicts are scattered back around HBLS_NOQUORUM. */
static int run_agg_verify_quorum(const hbls_committee_t *c, const uint8_t *d_bm,
                                 const uint8_t *d_sig, const uint8_t *d_msg,
                                 size_t msg_len, size_t batch, int32_t *results) {
    if (!c->q_set || batch == 0) return HBLS_ERR_BADINPUT;
    size_t bm = (c->n + 7) / 8;
    DevBuf dlive(batch * 4), dnlive(4);
    if (dlive.err || dnlive.err) return HBLS_ERR;
    uint32_t nlive = 0;
    uint64_t mask_ns;
    {
        Timer tm;
        int rc = launch_mask_power(c, d_bm, bm, nullptr, batch, nullptr, nullptr,
                                   dlive.as<int32_t>(), dnlive.as<uint32_t>());
        tm.stop_and_store();
        if (rc != HBLS_OK) return rc;
        mask_ns = g_last_ns;
    }
    g_stage_ns[7] = mask_ns;
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(&nlive, dnlive.p, 4, hipMemcpyDeviceToHost));
    if (nlive == batch) {
        /* the pipeline resets slot 7 (the combined path's own use of it);
         * in this entry it stays k_mask_power's time */
        int prc = run_agg_verify_pipeline(c, d_bm, d_sig, d_msg, msg_len, batch, results);
        g_stage_ns[7] = mask_ns;
        return prc;
    }
    std::vector<int32_t> live(batch);
    HIP_OK(hipMemcpy(live.data(), dlive.p, batch * 4, hipMemcpyDeviceToHost));
    if (nlive == 0) {
        /* nothing to launch (a zero-block launch is an error) */
        aggrlc_stats_reset();
        for (int i = 0; i < 4; i++) g_stage_ns[i] = 0;
        for (size_t j = 0; j < batch; j++) results[j] = HBLS_NOQUORUM;
        return HBLS_OK;
    }
    std::vector<uint32_t> idx;
    idx.reserve(nlive);
    for (size_t j = 0; j < batch; j++)
        if (live[j]) idx.push_back((uint32_t)j);
    if (idx.size() != nlive) return HBLS_ERR;
    DevBuf didx((size_t)nlive * 4), gbm((size_t)nlive * bm), gsig((size_t)nlive * 96),
           gmsg((size_t)nlive * msg_len);
    if (didx.err || gbm.err || gsig.err || gmsg.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(didx.p, idx.data(), (size_t)nlive * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_quorum_gather, dim3(nlive), dim3(256), 0, 0,
                       didx.as<uint32_t>(), (int)nlive, d_bm, (int)bm, d_sig, d_msg,
                       (int)msg_len, gbm.as<uint8_t>(), gsig.as<uint8_t>(), gmsg.as<uint8_t>());
    HIP_OK(hipGetLastError());
    std::vector<int32_t> sub(nlive);
    int rc = run_agg_verify_pipeline(c, gbm.as<uint8_t>(), gsig.as<uint8_t>(),
                                     gmsg.as<uint8_t>(), msg_len, nlive, sub.data());
    g_stage_ns[7] = mask_ns;
    if (rc != HBLS_OK) return rc;
    size_t k = 0;
    for (size_t j = 0; j < batch; j++) results[j] = live[j] ? sub[k++] : HBLS_NOQUORUM;
    return HBLS_OK;
}

extern "C" int hbls_batch_agg_verify_quorum(const hbls_committee_t *c, const uint8_t *bitmaps,
                                            const uint8_t *sigs96, const uint8_t *msgs,
                                            size_t msg_len, size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!c || !c->q_set || batch == 0) return HBLS_ERR_BADINPUT;
    size_t bm = (c->n + 7) / 8;
    DevBuf dbm(batch * bm), dsig(batch * 96), dmsg(batch * msg_len);
    if (dbm.err || dsig.err || dmsg.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dbm.p, bitmaps, batch * bm, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dsig.p, sigs96, batch * 96, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmsg.p, msgs, batch * msg_len, hipMemcpyHostToDevice));
    return run_agg_verify_quorum(c, dbm.as<uint8_t>(), dsig.as<uint8_t>(),
                                 dmsg.as<uint8_t>(), msg_len, batch, results);
}

extern "C" int hbls_agg_verify_quorum(const hbls_committee_t *c, const uint8_t *bitmap,
                                      const uint8_t sig96[96], const uint8_t *msg,
                                      size_t msg_len) {
    int32_t r;
    int rc = hbls_batch_agg_verify_quorum(c, bitmap, sig96, msg, msg_len, 1, &r);
    if (rc != HBLS_OK) return rc;
    return r;
}

extern "C" int hbls_batch_seal_verify_quorum(const hbls_committee_t *c,
                                             const uint8_t *sig_bitmaps, size_t blob_len,
                                             const uint8_t *msgs, size_t msg_len,
                                             size_t batch, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!c || !c->q_set || batch == 0) return HBLS_ERR_BADINPUT;
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
    return run_agg_verify_quorum(c, dbm.as<uint8_t>(), dsig.as<uint8_t>(),
                                 dmsg.as<uint8_t>(), msg_len, batch, results);
}

extern "C" int hbls_stream_power(hbls_stream *s, const uint32_t *slots, int k,
                                 uint64_t *power_out, uint32_t *count_out,
                                 int32_t *quorum_out) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!s || !slots || k <= 0) return HBLS_ERR_BADINPUT;
    if (quorum_out && !s->c->q_set) return HBLS_ERR_BADINPUT;
    for (int i = 0; i < k; i++)
        if (slots[i] >= (uint32_t)s->max_rounds) return HBLS_ERR_BADINPUT;
    DevBuf dslots((size_t)k * 4), dpow((size_t)k * 8), dcnt((size_t)k * 4), dlive((size_t)k * 4);
    if (dslots.err || dpow.err || dcnt.err || dlive.err) return HBLS_ERR;
    HIP_OK(hipMemcpy(dslots.p, slots, (size_t)k * 4, hipMemcpyHostToDevice));
    Timer tm;
    rc = launch_mask_power(s->c, (const uint8_t *)s->d_bitmap, (size_t)s->nwords * 4,
                           dslots.as<uint32_t>(), (size_t)k, dpow.as<uint64_t>(),
                           dcnt.as<uint32_t>(), dlive.as<int32_t>(), nullptr);
    tm.stop_and_store();
    if (rc != HBLS_OK) return rc;
    g_stage_ns[7] = g_last_ns;
    HIP_OK(hipGetLastError());
    if (power_out) HIP_OK(hipMemcpy(power_out, dpow.p, (size_t)k * 8, hipMemcpyDeviceToHost));
    if (count_out) HIP_OK(hipMemcpy(count_out, dcnt.p, (size_t)k * 4, hipMemcpyDeviceToHost));
    if (quorum_out) HIP_OK(hipMemcpy(quorum_out, dlive.p, (size_t)k * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}
