/* hbls_ctxset.inc — epoch contexts: several committees in one batch
 * (DESIGN.md §4i).
 *
 * verifySignature (internal/chain/engine.go:619-642) looks up an epoch
 * context — key list and quorum verifier of one (shardID, epoch) — per item;
 * cross-link lists, the epoch chain and a sync window over an epoch boundary
 * mix contexts in one loop.  A context set is a device-resident table of
 * committee descriptors; every item names its context, and the front half of
 * the pipeline (validation, masked key sum, quorum by mask) takes table, n,
 * row length, full sum, window table, power table and threshold from the
 * item's context.  From the masked sums on, the single-committee code runs
 * unchanged over the whole mixed batch (run_agg_verify_pairing).
 *
 * Included from hbls_dev.hip after hbls_quorum.inc: it uses mp_load_word /
 * mp_row_partial, the hash and decompress kernels, HIP_OK, DevBuf, Timer and
 * run_agg_verify_pairing.
 *
 * Barriers.  The key-sum kernel gives every item a block of one wave, so a
 * block never holds two items: all trip counts that carry a __syncthreads()
 * (segments of the bitmap, levels of the reduction tree) depend on the item's
 * context alone and are uniform over the block.  k_mask_aggregate's four
 * items per block would put four different n behind one barrier.  The power
 * kernel gives every item a wave and has no block-wide barrier at all.
 *
 * Alignment.  A bitmap stays where it was uploaded, at blob_off[j] + 96, so
 * its address has no alignment to speak of.  The key-sum kernel reads it by
 * bytes; the power kernel derives mp_load_word's `align` from each item's own
 * row address.
 *
 * A launch never depends on the number of contexts: prepare, (power),
 * (gather), hash, decompress, key sums, pairing stage. */

#define CX_VALID 1u
#define CX_PREP_T 160           /* prepare/gather threads per item: 96 sig + 48 msg + 1 */
#define CX_MSG_SLOT 48          /* bytes of a message that hash_to_g2_point reads */

struct cx_ctx {
    const g1aff_t *table;
    const g1_t *full_sum;       /* may be null */
    const g1aff_t *wtab;        /* may be null, and then winf is too */
    const uint8_t *winf;
    const uint64_t *power;
    uint64_t threshold;
    uint32_t n;
    uint32_t uniform;
    uint32_t q_set;
    uint32_t pad;
};

struct cx_item {
    uint32_t ctx;               /* < n_ctx when CX_VALID */
    uint32_t bm_off;            /* byte offset of the bitmap in the uploaded buffer */
    uint32_t flags;
    uint32_t pad;
};

struct hbls_ctxset {
    cx_ctx *d_ctx;
    size_t n_ctx;
    int all_q_set;
};

/* Validates every item and stages its parts.  Item j is
 * bytes[off[j] .. off[j+1]) = hdr bytes of signature (96 or 0) || bitmap; it
 * is well formed when ctx_idx[j] < n_ctx and its length is
 * hdr + ceil(n/8) of that context — decided here, before the index or the
 * length is used as an address by any later kernel.  The signature goes to
 * a dense batch x 96 buffer and the message to a dense batch x 48 slot,
 * zero-padded: hash_to_g2_point reads only the first min(len, 48) bytes of a
 * message, zero-padded to 48, so hashing the slot with mlen = 48 gives
 * exactly hbls_hash_to_g2 of the original bytes, whatever their length.
 * The bitmap is not copied.  sig_out/msg_out may be NULL (hdr = 0). */
__global__ void __launch_bounds__(256) k_ctx_prepare(
        const cx_ctx *ctxs, uint32_t n_ctx, const uint32_t *ctx_idx,
        const uint8_t *bytes, const uint32_t *off, uint32_t hdr,
        const uint8_t *msgs, const uint32_t *msg_off, size_t batch,
        cx_item *items, int32_t *status, uint8_t *sig_out, uint8_t *msg_out) {
    size_t total = batch * CX_PREP_T;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        size_t j = t / CX_PREP_T;
        uint32_t k = (uint32_t)(t - j * CX_PREP_T);
        if (k > 144) continue;
        uint32_t ci = ctx_idx[j], b0 = off[j], b1 = off[j + 1];
        bool valid = ci < n_ctx;
        if (valid) {
            uint64_t want = (uint64_t)hdr + (((uint64_t)ctxs[ci].n + 7) >> 3);
            valid = (uint64_t)(b1 - b0) == want;
        }
        if (k < 96) {
            if (sig_out) sig_out[j * 96 + k] = valid ? bytes[(size_t)b0 + k] : 0;
        } else if (k < 144) {
            if (msg_out) {
                uint32_t m = k - 96, mo = msg_off[j], ml = msg_off[j + 1] - mo;
                msg_out[j * CX_MSG_SLOT + m] = (valid && m < ml) ? msgs[(size_t)mo + m] : 0;
            }
        } else {
            cx_item it;
            it.ctx = valid ? ci : 0;
            it.bm_off = valid ? b0 + hdr : 0;
            it.flags = valid ? CX_VALID : 0;
            it.pad = 0;
            items[j] = it;
            status[j] = valid ? HBLS_OK : HBLS_ERR_BADINPUT;
        }
    }
}

/* dense copies of the live items' descriptors, signatures and message
 * slots; idx[k] = position in the full batch.  Bitmaps stay in place: the
 * descriptor carries their offset. */
__global__ void __launch_bounds__(256) k_ctx_gather(
        const uint32_t *idx, size_t nlive, const cx_item *items, const uint8_t *sig,
        const uint8_t *msg, cx_item *items_out, uint8_t *sig_out, uint8_t *msg_out) {
    size_t total = nlive * CX_PREP_T;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        size_t k = t / CX_PREP_T;
        uint32_t b = (uint32_t)(t - k * CX_PREP_T);
        size_t j = idx[k];
        if (b < 96) sig_out[k * 96 + b] = sig[j * 96 + b];
        else if (b < 144) msg_out[k * CX_MSG_SLOT + (b - 96)] = msg[j * CX_MSG_SLOT + (b - 96)];
        else if (b == 144) items_out[k] = items[j];
    }
}

/* Masked key sum of one item per block (one wave): k_mask_aggregate and
 * k_mask_aggregate_w with table, n, row length, full sum and window table
 * taken from the item's context.  The complement side (participation above
 * one half, full sum present), the 8-bit window table (where the context has
 * one) and the clipping of padding bits past n are per-item decisions.  AL
 * lanes of the wave add points (16 where the item has little to add, so the
 * reduction tree stays short; 64 otherwise); the others idle but keep every
 * barrier.  Everything a barrier depends on is uniform over the block, which
 * holds one item.  An item that is not CX_VALID gets the point at infinity. */
__global__ void __launch_bounds__(64) k_ctx_mask_aggregate(
        const cx_ctx *ctxs, const cx_item *items, const uint8_t *bytes,
        g1_t *out, int count) {
    __shared__ g1_t red[64];
    __shared__ uint32_t idx[MASK_IDX_CAP];
    __shared__ int cnt;
    const int item = blockIdx.x;
    const int lane = threadIdx.x;
    if (item >= count) return;
    const cx_item it = items[item];
    if (!(it.flags & CX_VALID)) {
        if (lane == 0) {
            g1_t inf;
            g1_set_inf(inf);
            out[item] = inf;
        }
        return;
    }
    const cx_ctx cx = ctxs[it.ctx];
    const int n = (int)cx.n;
    const int bm_len = (n + 7) >> 3;
    const uint8_t *bm = bytes + it.bm_off;
    const bool windowed = cx.wtab != nullptr && cx.winf != nullptr;

    if (lane == 0) cnt = 0;
    __syncthreads();
    {
        int c = 0;
        for (int i = lane; i < bm_len; i += 64) c += __popc(bm[i]);
        if (c) atomicAdd(&cnt, c);
    }
    __syncthreads();
    const int set_count = cnt;
    const bool complement = cx.full_sum != nullptr && set_count > n / 2;
    int minority = complement ? n - set_count : set_count;
    const int AL = (windowed ? bm_len >= 256 : minority >= 256) ? 64 : 16;
    const bool worker = lane < AL;
    g1_t acc;
    g1_set_inf(acc);
    if (windowed) {
        if (worker) {
            for (int i = lane; i < bm_len; i += AL) {
                uint32_t v = bm[i];
                if (complement) v = ~v & 0xffu;
                const int tail = n - 8 * i;
                if (tail < 8) v &= (1u << tail) - 1;
                if (v) {
                    size_t e = (size_t)i * 255 + v - 1;
                    if (!cx.winf[e]) g1_madd_i(acc, acc, cx.wtab[e]);
                }
            }
        }
    } else {
        for (int base = 0; base < n; base += MASK_IDX_CAP) {
            __syncthreads();
            if (lane == 0) cnt = 0;
            __syncthreads();
            if (worker) {
                const int end = base + MASK_IDX_CAP < n ? base + MASK_IDX_CAP : n;
                for (int w = base / 32 + lane; w * 32 < end; w += AL) {
                    uint32_t word = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        int byte = w * 4 + k;
                        if (byte < bm_len) word |= (uint32_t)bm[byte] << (8 * k);
                    }
                    if (complement) word = ~word;
                    const int lo = w * 32;
                    /* clip past n: bitmap padding must not enter the complement */
                    if (n - lo < 32) word &= (1u << (n - lo)) - 1;
                    int c = __popc(word);
                    if (c) {
                        int pos = atomicAdd(&cnt, c);
                        while (word) {
                            int b = __ffs(word) - 1;
                            word &= word - 1;
                            idx[pos++] = (uint32_t)(lo + b);
                        }
                    }
                }
            }
            __syncthreads();
            if (worker) {
                const int m = cnt;
                for (int k = lane; k < m; k += AL)
                    g1_madd_i(acc, acc, cx.table[idx[k]]);
            }
        }
    }
    __syncthreads();
    red[lane] = acc;
    __syncthreads();
    for (int s = AL / 2; s > 0; s >>= 1) {
        if (lane < s) {
            g1_t t;
            g1_add(t, red[lane], red[lane + s]);
            red[lane] = t;
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (complement) {
            g1_t nsum, res;
            g1_neg(nsum, red[0]);
            g1_add(res, *cx.full_sum, nsum);
            out[item] = res;
        } else {
            out[item] = red[0];
        }
    }
}

/* Quorum by mask of one item per wave: k_mask_power with power table,
 * threshold and uniform flag of the item's context.  The tables are read
 * through L2 (a block's items need not share a context, so there is no LDS
 * copy); the wide loads of mp_load_word are taken only where this item's row
 * address allows them.  No block-wide barrier; the shuffles run over whole
 * waves, and a wave holds one item.  With quorum != 0 a valid item whose sum
 * does not exceed its context's threshold gets status HBLS_NOQUORUM.  An
 * item that is not CX_VALID reports power and count 0.  power_out and
 * count_out may be NULL. */
#define CX_MP_THREADS 256
__global__ void __launch_bounds__(CX_MP_THREADS) k_ctx_mask_power(
        const cx_ctx *ctxs, const cx_item *items, const uint8_t *bytes, int count,
        int quorum, uint64_t *power_out, uint32_t *count_out, int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * CX_MP_THREADS + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * CX_MP_THREADS) >> 6);
    for (int item = wave; item < count; item += nwaves) {
        const cx_item it = items[item];
        const bool valid = (it.flags & CX_VALID) != 0;
        uint64_t sum = 0, threshold = 0;
        uint32_t cnt = 0;
        bool uniform = true;
        if (valid) {
            const cx_ctx cx = ctxs[it.ctx];
            const uint8_t *row = bytes + it.bm_off;
            const int n = (int)cx.n;
            const int row_bytes = (n + 7) >> 3;
            const uintptr_t a = (uintptr_t)row;
            const int align = (a & 7) == 0 ? 8 : (a & 3) == 0 ? 4 : 1;
            uniform = cx.uniform != 0;
            threshold = cx.threshold;
            if (uniform)
                mp_row_partial<MP_UNIFORM>(row, row_bytes, n, align, lane, 64, nullptr, sum, cnt);
            else
                mp_row_partial<MP_GLOBAL>(row, row_bytes, n, align, lane, 64, cx.power, sum, cnt);
        }
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            sum += __shfl_xor((unsigned long long)sum, off, 64);
        }
        if (uniform) sum = cnt;
        if (lane == 0) {
            if (power_out) power_out[item] = sum;
            if (count_out) count_out[item] = cnt;
            if (quorum && valid && !(sum > threshold)) status[item] = HBLS_NOQUORUM;
        }
    }
}

/* ---------------------------------------------------------------- host */

static int cx_check_offsets(const uint32_t *off, size_t batch, size_t *total) {
    if (!off || off[0] != 0) return HBLS_ERR_BADINPUT;
    for (size_t j = 0; j < batch; j++)
        if (off[j + 1] < off[j]) return HBLS_ERR_BADINPUT;
    *total = off[batch];
    return HBLS_OK;
}

static int cx_blocks(size_t threads) {
    size_t nb = (threads + 255) / 256;
    return (int)(nb < 4096 ? (nb ? nb : 1) : 4096);
}

#define CX_MAX_BATCH ((size_t)0x3fffffff)

extern "C" hbls_ctxset_t *hbls_ctxset_create(const hbls_committee_t *const *cs, size_t n_ctx) {
    if (require_gpu() != HBLS_OK) return nullptr;
    if (!cs || n_ctx == 0 || n_ctx > 0xffffffffu) return nullptr;
    std::vector<cx_ctx> h(n_ctx);
    int all_q = 1;
    for (size_t i = 0; i < n_ctx; i++) {
        const hbls_committee_t *c = cs[i];
        if (!c || c->n == 0 || c->n > 0x7fffffc0u) return nullptr;
        h[i].table = c->d_table;
        h[i].full_sum = c->d_full_sum;
        h[i].wtab = c->d_winf ? c->d_wtab : nullptr;
        h[i].winf = c->d_wtab ? c->d_winf : nullptr;
        h[i].power = c->d_power;
        h[i].threshold = c->q_threshold;
        h[i].n = (uint32_t)c->n;
        h[i].uniform = c->q_uniform ? 1 : 0;
        h[i].q_set = c->q_set ? 1 : 0;
        h[i].pad = 0;
        if (!c->q_set) all_q = 0;
    }
    cx_ctx *d = nullptr;
    HIP_OKP(hipMalloc(&d, n_ctx * sizeof(cx_ctx)));
    if (hipMemcpy(d, h.data(), n_ctx * sizeof(cx_ctx), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return nullptr;
    }
    hbls_ctxset_t *s = new hbls_ctxset_t;
    s->d_ctx = d;
    s->n_ctx = n_ctx;
    s->all_q_set = all_q;
    return s;
}

extern "C" void hbls_ctxset_free(hbls_ctxset_t *s) {
    if (s) {
        hipFree(s->d_ctx);
        delete s;
    }
}

extern "C" size_t hbls_ctxset_size(const hbls_ctxset_t *s) { return s ? s->n_ctx : 0; }

extern "C" int hbls_ctx_mask_sums(const hbls_ctxset_t *s, const uint32_t *ctx_idx,
                                  const uint8_t *bitmaps, const uint32_t *bm_off, size_t batch,
                                  uint8_t *out48s, uint64_t *power_out, uint32_t *count_out,
                                  int32_t *ok) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!s || !ctx_idx || !ok || batch == 0 || batch > CX_MAX_BATCH) return HBLS_ERR_BADINPUT;
    size_t total = 0;
    rc = cx_check_offsets(bm_off, batch, &total);
    if (rc != HBLS_OK) return rc;
    if (total && !bitmaps) return HBLS_ERR_BADINPUT;
    DevBuf dbytes(total), doff((batch + 1) * 4), dci(batch * 4);
    DevBuf ditems(batch * sizeof(cx_item)), dst(batch * 4);
    DevBuf dsum(batch * sizeof(g1_t)), dser(batch * 48), dpow(batch * 8), dcnt(batch * 4);
    if (dbytes.err || doff.err || dci.err || ditems.err || dst.err || dsum.err || dser.err ||
        dpow.err || dcnt.err) return HBLS_ERR;
    if (total) HIP_OK(hipMemcpy(dbytes.p, bitmaps, total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(doff.p, bm_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dci.p, ctx_idx, batch * 4, hipMemcpyHostToDevice));
    Timer tm;
    hipLaunchKernelGGL(k_ctx_prepare, dim3(cx_blocks(batch * CX_PREP_T)), dim3(256), 0, 0,
                       s->d_ctx, (uint32_t)s->n_ctx, dci.as<uint32_t>(), dbytes.as<uint8_t>(),
                       doff.as<uint32_t>(), 0u, (const uint8_t *)nullptr,
                       (const uint32_t *)nullptr, batch, ditems.as<cx_item>(),
                       dst.as<int32_t>(), (uint8_t *)nullptr, (uint8_t *)nullptr);
    if (out48s) {
        hipLaunchKernelGGL(k_ctx_mask_aggregate, dim3((uint32_t)batch), dim3(64), 0, 0,
                           s->d_ctx, ditems.as<cx_item>(), dbytes.as<uint8_t>(),
                           dsum.as<g1_t>(), (int)batch);
        hipLaunchKernelGGL(k_g1_serialize, dim3((uint32_t)((batch + 63) / 64)), dim3(64), 0, 0,
                           dsum.as<g1_t>(), dser.as<uint8_t>(), (int)batch);
    }
    if (power_out || count_out)
        hipLaunchKernelGGL(k_ctx_mask_power, dim3(cx_blocks(batch * 64)), dim3(CX_MP_THREADS),
                           0, 0, s->d_ctx, ditems.as<cx_item>(), dbytes.as<uint8_t>(),
                           (int)batch, 0, dpow.as<uint64_t>(), dcnt.as<uint32_t>(),
                           dst.as<int32_t>());
    tm.stop_and_store();
    g_stage_ns[7] = g_last_ns;
    HIP_OK(hipGetLastError());
    if (out48s) HIP_OK(hipMemcpy(out48s, dser.p, batch * 48, hipMemcpyDeviceToHost));
    if (power_out) HIP_OK(hipMemcpy(power_out, dpow.p, batch * 8, hipMemcpyDeviceToHost));
    if (count_out) HIP_OK(hipMemcpy(count_out, dcnt.p, batch * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ok, dst.p, batch * 4, hipMemcpyDeviceToHost));
    return HBLS_OK;
}

extern "C" int hbls_batch_seal_verify_ctx(const hbls_ctxset_t *s, const uint32_t *ctx_idx,
                                          const uint8_t *blobs, const uint32_t *blob_off,
                                          const uint8_t *msgs, const uint32_t *msg_off,
                                          size_t batch, int quorum, int32_t *results) {
    int rc = require_gpu();
    if (rc != HBLS_OK) return rc;
    if (!s || !ctx_idx || !results || batch == 0 || batch > CX_MAX_BATCH)
        return HBLS_ERR_BADINPUT;
    if (quorum && !s->all_q_set) return HBLS_ERR_BADINPUT;
    size_t nblob = 0, nmsg = 0;
    rc = cx_check_offsets(blob_off, batch, &nblob);
    if (rc != HBLS_OK) return rc;
    rc = cx_check_offsets(msg_off, batch, &nmsg);
    if (rc != HBLS_OK) return rc;
    if ((nblob && !blobs) || (nmsg && !msgs)) return HBLS_ERR_BADINPUT;
    HostCall hcall;
    DevBuf dblob(nblob), dboff((batch + 1) * 4), dmsgs(nmsg), dmoff((batch + 1) * 4);
    DevBuf dci(batch * 4), ditems(batch * sizeof(cx_item)), dst(batch * 4);
    DevBuf dsig(batch * 96), dmsg(batch * CX_MSG_SLOT);
    if (dblob.err || dboff.err || dmsgs.err || dmoff.err || dci.err || ditems.err || dst.err ||
        dsig.err || dmsg.err) return HBLS_ERR;
    if (nblob) HIP_OK(hipMemcpy(dblob.p, blobs, nblob, hipMemcpyHostToDevice));
    if (nmsg) HIP_OK(hipMemcpy(dmsgs.p, msgs, nmsg, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dboff.p, blob_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dmoff.p, msg_off, (batch + 1) * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dci.p, ctx_idx, batch * 4, hipMemcpyHostToDevice));

    /* front: validate and stage, then the quorum gate */
    uint64_t front_ns;
    {
        Timer tm;
        hipLaunchKernelGGL(k_ctx_prepare, dim3(cx_blocks(batch * CX_PREP_T)), dim3(256), 0, 0,
                           s->d_ctx, (uint32_t)s->n_ctx, dci.as<uint32_t>(),
                           dblob.as<uint8_t>(), dboff.as<uint32_t>(), 96u, dmsgs.as<uint8_t>(),
                           dmoff.as<uint32_t>(), batch, ditems.as<cx_item>(), dst.as<int32_t>(),
                           dsig.as<uint8_t>(), dmsg.as<uint8_t>());
        if (quorum)
            hipLaunchKernelGGL(k_ctx_mask_power, dim3(cx_blocks(batch * 64)),
                               dim3(CX_MP_THREADS), 0, 0, s->d_ctx, ditems.as<cx_item>(),
                               dblob.as<uint8_t>(), (int)batch, 1, (uint64_t *)nullptr,
                               (uint32_t *)nullptr, dst.as<int32_t>());
        tm.stop_and_store();
        front_ns = g_last_ns;
    }
    HIP_OK(hipGetLastError());
    g_stage_ns[7] = front_ns;
    std::vector<int32_t> status(batch);
    HIP_OK(hipMemcpy(status.data(), dst.p, batch * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> idx;
    for (size_t j = 0; j < batch; j++)
        if (status[j] == HBLS_OK) idx.push_back((uint32_t)j);
    size_t nlive = idx.size();
    aggrlc_stats_reset();
    for (int i = 0; i < 7; i++) g_stage_ns[i] = 0;
    g_stage_ns[8] = 0;          /* nothing is hoisted here (DESIGN.md §4l) */
    if (nlive == 0) {
        /* nothing to launch (a zero-block launch is an error) */
        for (size_t j = 0; j < batch; j++) results[j] = status[j];
        return HBLS_OK;
    }

    /* malformed and quorumless items take no part in hash-to-G2,
     * decompression or pairing: the rest of the call sees the live ones only */
    DevBuf didx(nlive * 4), gitems(nlive * sizeof(cx_item)), gsig(nlive * 96),
           gmsg(nlive * CX_MSG_SLOT);
    DevBuf dagg(nlive * sizeof(g1_t)), dhm(nlive * sizeof(g2_t));
    DevBuf dsaff(nlive * sizeof(g2aff_t)), dsflags(nlive * 4), dhok(nlive * 4), dres(nlive * 4);
    if (didx.err || gitems.err || gsig.err || gmsg.err || dagg.err || dhm.err || dsaff.err ||
        dsflags.err || dhok.err || dres.err) return HBLS_ERR;
    EventSet<8> ev;
    if (ev.err != hipSuccess) return HBLS_ERR;
    uint64_t t_launch = host_now_ns();
    const cx_item *l_items = ditems.as<cx_item>();
    const uint8_t *l_sig = dsig.as<uint8_t>(), *l_msg = dmsg.as<uint8_t>();
    (void)hipEventRecord(ev[2], 0);
    if (nlive < batch) {
        HIP_OK(hipMemcpy(didx.p, idx.data(), nlive * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_ctx_gather, dim3(cx_blocks(nlive * CX_PREP_T)), dim3(256), 0, 0,
                           didx.as<uint32_t>(), nlive, l_items, l_sig, l_msg,
                           gitems.as<cx_item>(), gsig.as<uint8_t>(), gmsg.as<uint8_t>());
        l_items = gitems.as<cx_item>();
        l_sig = gsig.as<uint8_t>();
        l_msg = gmsg.as<uint8_t>();
    }
    /* every stage from here dispatches on nlive, not on batch */
    launch_hash_to_g2(l_msg, CX_MSG_SLOT, dhm.as<g2_t>(), dhok.as<int32_t>(), nlive);
    (void)hipEventRecord(ev[3], 0);
    (void)hipEventRecord(ev[4], 0);
    launch_g2_decompress(l_sig, dsaff.as<g2aff_t>(), dsflags.as<int32_t>(), nlive);
    (void)hipEventRecord(ev[5], 0);
    (void)hipEventRecord(ev[0], 0);
    hipLaunchKernelGGL(k_ctx_mask_aggregate, dim3((uint32_t)nlive), dim3(64), 0, 0,
                       s->d_ctx, l_items, dblob.as<uint8_t>(), dagg.as<g1_t>(), (int)nlive);
    (void)hipEventRecord(ev[1], 0);

    std::vector<int32_t> sub(nlive);
    rc = run_agg_verify_pairing(dagg.as<g1_t>(), dhm.as<g2_t>(), dsaff.as<g2aff_t>(),
                                dsflags.as<int32_t>(), dhok.as<int32_t>(), dres.as<int32_t>(),
                                nlive, aggrlc_plan(nlive, batch, false), ev, t_launch,
                                sub.data());
    if (rc != HBLS_OK) return rc;
    g_last_ns += front_ns;
    g_stage_ns[7] = front_ns;
    for (size_t j = 0; j < batch; j++) results[j] = status[j];
    for (size_t k = 0; k < nlive; k++) results[idx[k]] = sub[k];
    return HBLS_OK;
}
