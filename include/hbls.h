/* hbls.h — C-ABI of the MI355X-native BLS12-381 library (libhbls.so).
 *
 * This is the drop-in boundary for harmony-one/harmony's BLS FFI: the Go repo
 * reaches all curve/pairing arithmetic through the cgo package
 * `github.com/harmony-one/bls/ffi/go/bls` (imported as bls_core at e.g.
 * crypto/bls/bls.go:8, consensus/quorum/quorum.go:11, internal/chain/sig.go:6).
 * Each entry point below names the herumi bls C function (bls/bls.h /
 * src/bls_c_impl.hpp) the Go FFI binds and which this library replaces.
 * A maintainer wires this in with a cgo shim — see INTEGRATION.md.
 *
 * Conventions (match the herumi FFI the reference uses):
 *   - curve: BLS12-381 with BLS_SWAP_G=1 (reference Makefile:71-73):
 *     public keys in G1 (48 B compressed), signatures in G2 (96 B).
 *   - all points cross the ABI in herumi little-endian compressed form
 *     (or as opaque device-resident handles for committee tables).
 *   - secret keys: 32 B little-endian Fr, value < r.
 *   - return 0 = failure/reject, 1 = success/accept, negative = error,
 *     unless noted.  Thread-safe after hbls_init() (no mutable globals).
 *   - REQUIRES an AMD GPU (gfx950).  There is no CPU fallback: calls fail
 *     loudly (HBLS_ERR_NOGPU) when no device is present.
 */
#ifndef HBLS_H
#define HBLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    HBLS_OK = 1,
    HBLS_FALSE = 0,
    HBLS_ERR = -1,
    HBLS_ERR_NOGPU = -2,
    HBLS_ERR_BADINPUT = -3,
    HBLS_NOQUORUM = -4,     /* per-item result of the _quorum entries only */
};

/* numeric.NewDec(2).Quo(numeric.NewDec(3)) as the integer inside the Dec
 * (twoThird, one-node-staked-vote.go:23; Precision = 18, half-to-even) */
#define HBLS_TWO_THIRDS_DEC 666666666666666667ULL

/* blsInit(BLS12_381) (bls.h) — called once per process (crypto/bls/mask.go:18-20).
 * Initializes the HIP device context; device = HIP device index (normally
 * LOCAL_RANK; pass -1 for current device). */
int hbls_init(int device);

/* number of usable GPUs (0 -> every call returns HBLS_ERR_NOGPU) */
int hbls_device_count(void);

/* ---- scalar drop-ins (one call per object, like the cgo surface) ---- */

/* blsGetPublicKey: pk = sk * basePoint (SecretKey.GetPublicKey) */
int hbls_pk_from_sk(const uint8_t sk32[32], uint8_t pk48[48]);

/* blsSignHash: sig = sk * H2(msg)  (SecretKey.SignHash; construct.go:101,110) */
int hbls_sign_hash(const uint8_t sk32[32], const uint8_t *msg, size_t msg_len,
                   uint8_t sig96[96]);

/* blsVerifyHash: e(pub, H2(msg)) == e(base, sig)  (Sign.VerifyHash;
 * leader.go:173,287, validator.go:228, engine.go:638).
 * Returns HBLS_OK accept / HBLS_FALSE reject / HBLS_ERR_BADINPUT. */
int hbls_verify_hash(const uint8_t pk48[48], const uint8_t sig96[96],
                     const uint8_t *msg, size_t msg_len);

/* blsPublicKeyAdd / blsPublicKeySub (PublicKey.Add/Sub; mask.go:126-130).
 * Zero input (48 zero bytes) is the identity, matching zero-value structs. */
int hbls_g1_add(const uint8_t a48[48], const uint8_t b48[48], uint8_t out48[48]);
int hbls_g1_sub(const uint8_t a48[48], const uint8_t b48[48], uint8_t out48[48]);

/* blsSignatureAdd (Sign.Add; mask.go:57-64, construct.go:99-105) */
int hbls_g2_add(const uint8_t a96[96], const uint8_t b96[96], uint8_t out96[96]);

/* blsPublicKeyDeserialize / blsSignatureDeserialize validity check
 * (subgroup-checked, as herumi does on deserialize) */
int hbls_g1_check(const uint8_t p48[48]);
int hbls_g2_check(const uint8_t p96[96]);

/* blsHashToSignature equivalent: H2(msg) serialized (used by tests) */
int hbls_hash_to_g2(const uint8_t *msg, size_t msg_len, uint8_t out96[96]);

/* mcl G2 cofactor mode: 1 = Budroni-Pintore fast (default), 0 = full h2.
 * Mirrors mcl's useOriginalG2cofactor_ switch; see DESIGN.md parity notes. */
void hbls_set_g2_cofactor_mode(int fast);

/* ---- committee table (device-resident pubkey table) ----
 * Mirrors Decider.UpdateParticipants (consensus/quorum/quorum.go:326-334) +
 * the deserialized-pubkey cache (crypto/bls/bls.go:30-33, mask.go:13-15):
 * upload once per epoch, aggregate/verify against it many times. */
typedef struct hbls_committee hbls_committee_t;

/* build from n concatenated 48-B compressed keys; validates every key
 * (curve + subgroup) on the GPU; returns NULL on any invalid key */
hbls_committee_t *hbls_committee_build(const uint8_t *pks48, size_t n);
void hbls_committee_free(hbls_committee_t *c);
size_t hbls_committee_size(const hbls_committee_t *c);

/* Mask.SetMask / masked aggregate (crypto/bls/mask.go:113-134):
 * AggregatePublic = sum of pk_i with bit i set.  bitmap is ceil(n/8) bytes,
 * little-endian bit order (bit i of byte i/8 = cosigner i). */
int hbls_mask_aggregate_g1(const hbls_committee_t *c, const uint8_t *bitmap,
                           uint8_t out48[48]);

/* one aggregate verify: DecodeSigBitmap + IsQuorumAchievedByMask's cryptoleg +
 * VerifyHash (internal/chain/sig.go:37-49 -> engine.go:630-642) */
int hbls_agg_verify(const hbls_committee_t *c, const uint8_t *bitmap,
                    const uint8_t sig96[96], const uint8_t *msg, size_t msg_len);

/* ---- batch entry points (the GPU-native surface) ---- */

/* batch of independent aggregate-verifies against one committee:
 * bitmaps: batch * ceil(n/8) bytes; sigs: batch * 96; msgs: batch * msg_len.
 * results[j] = HBLS_OK / HBLS_FALSE / HBLS_ERR_BADINPUT. */
int hbls_batch_agg_verify(const hbls_committee_t *c, const uint8_t *bitmaps,
                          const uint8_t *sigs96, const uint8_t *msgs,
                          size_t msg_len, size_t batch, int32_t *results);

/* batch verify of per-signer votes (leader's onCommit loop, leader.go:221-301):
 * item j checks sig[j] by committee member key_idx[j] on msgs[j]. */
int hbls_batch_verify_votes(const hbls_committee_t *c, const uint32_t *key_idx,
                            const uint8_t *sigs96, const uint8_t *msgs,
                            size_t msg_len, size_t batch, int32_t *results);

/* same-message form of hbls_batch_verify_votes: vote j is checked on
 * msgs[group_idx[j]] (msgs: n_groups * msg_len; hashes n_groups messages, not
 * batch).  Votes of one group are verified by random linear combination —
 * one pairing per group, e(sum r_i*pk_i, H) == e(G1, sum r_i*sig_i) with
 * fresh secret 64-bit r_i from the OS CSPRNG (HBLS_ERR if that fails) — and a
 * failing group is re-checked per chunk, then per vote, so results[j] carries
 * exactly hbls_batch_verify_votes' codes; group_idx[j] >= n_groups gives that
 * vote HBLS_ERR_BADINPUT.  A false accept has probability ~2^-64 per call
 * (DESIGN.md "Random-combination batch verification"). */
int hbls_batch_verify_votes_grouped(const hbls_committee_t *c, const uint32_t *key_idx,
                                    const uint32_t *group_idx, const uint8_t *sigs96,
                                    const uint8_t *msgs, size_t msg_len, size_t n_groups,
                                    size_t batch, int32_t *results);
/* votes per refinement chunk of the batched path */
int hbls_rlc_chunk_size(void);
/* counters of the last batched call on this thread (zeroed by every
 * hbls_stream_process): out[0] groups pairing-checked, out[1] groups that
 * failed, out[2] chunks pairing-checked in refinement, out[3] votes sent to
 * the per-item kernel */
void hbls_rlc_last_stats(uint32_t out[4]);

/* batch hash-to-G2 (toG / mcl mapToG2 legacy) */
int hbls_batch_hash_to_g2(const uint8_t *msgs, size_t msg_len, size_t batch,
                          uint8_t *out96s);

/* batch sign: sigs[j] = sk[j] * H2(msgs[j]) */
int hbls_batch_sign(const uint8_t *sks32, const uint8_t *msgs, size_t msg_len,
                    size_t batch, uint8_t *sigs96);

/* batch sk->pk */
int hbls_batch_pk_from_sk(const uint8_t *sks32, size_t batch, uint8_t *pks48);

/* ---- config-4 (sharded 65536-key committee across GPUs) ----
 * Each rank holds one index-range slice of the committee as its table.
 * hbls_mask_partials computes this rank's per-item masked partial sums
 * (serialized, batch x 48 B) for the RCCL all-gather; the receiving rank
 * folds the other ranks' partials into its own slice's sums and finishes
 * the pairing check. */
int hbls_mask_partials(const hbls_committee_t *c, const uint8_t *bitmaps,
                       size_t batch, uint8_t *out48s);
int hbls_batch_agg_verify_partials(const hbls_committee_t *c, const uint8_t *bitmaps,
                                   const uint8_t *ext48s, size_t n_ext,
                                   const uint8_t *sigs96, const uint8_t *msgs,
                                   size_t msg_len, size_t batch, int32_t *results);

/* G1 MSM: out = sum_i scalar_i * P_i (scalars 32B LE each; Pippenger
 * bucket accumulation on device).  The serialized-points entry validates
 * every point (decompress + subgroup check); the committee entry runs the
 * MSM core against the resident, already-validated table — the production
 * shape (UpdateParticipants holds the table per epoch, quorum.go:326-334) */
int hbls_msm_g1(const uint8_t *points48, const uint8_t *scalars32, size_t n,
                uint8_t out48[48]);
int hbls_msm_g1_committee(const hbls_committee_t *c, const uint8_t *scalars32,
                          uint8_t out48[48]);

/* ConstructCommitPayload (consensus/signature/signature.go:12-24); returns 40/48 */
int hbls_construct_commit_payload(uint64_t block_num, const uint8_t hash32[32],
                                  uint64_t view_id, int staking, uint8_t out[48]);

/* ParseCommitSigAndBitmap (internal/chain/sig.go:22-35); returns bitmap length */
int hbls_parse_commit_sig_bitmap(const uint8_t *payload, size_t len,
                                 uint8_t sig96[96], uint8_t *bitmap, size_t bitmap_cap);

/* sync-path batch seal verification (stagedstreamsync/sig_verify.go:23-59):
 * items are raw commitSigAndBitmap blobs (96B sig || bitmap) + payloads */
int hbls_batch_seal_verify(const hbls_committee_t *c,
                           const uint8_t *sig_bitmaps, size_t blob_len,
                           const uint8_t *msgs, size_t msg_len,
                           size_t batch, int32_t *results);

/* ---- quorum by mask ----
 * Voting power crosses the ABI as uint64_t in units of 1e-18 — the integer
 * inside a numeric.Dec (Precision = 18, numeric/decimal.go:22); a committee's
 * powers sum to 1e18 < 2^60, so every masked sum is exact.  One rule covers
 * both policies: quorum <=> masked sum > threshold, strictly.  Only bits
 * i < n count (Mask.SetMask, crypto/bls/mask.go:121-132); padding bits of the
 * last byte are ignored.
 *
 * qrVerifier of an epoch context (internal/chain/engine.go:644-659,
 * quorum.go SetVoters).
 * power == NULL: uniform policy (one-node-one-vote.go:57-72), threshold
 * ignored and set to floor(2n/3) — popcount > floor(2n/3) is the reference's
 * popcount >= n*2/3 + 1.
 * power != NULL: n values (OverallPercent, one-node-staked-vote.go:151-164),
 * normally with threshold HBLS_TWO_THIRDS_DEC; HBLS_ERR_BADINPUT if the n
 * values sum above 2^63.
 * Call before the committee is shared between threads. */
int hbls_committee_set_quorum(hbls_committee_t *c, const uint64_t *power,
                              uint64_t threshold);

/* ComputeTotalPowerByMask (one-node-staked-vote.go:166-188) / CountOneBits
 * (one-node-one-vote.go:62), batch form; bitmaps: batch * ceil(n/8) bytes; either output
 * may be NULL.  Before hbls_committee_set_quorum every weight is 1, so power
 * equals count. */
int hbls_mask_power(const hbls_committee_t *c, const uint8_t *bitmaps, size_t batch,
                    uint64_t *power_out, uint32_t *count_out);

/* verifySignature (internal/chain/engine.go:619-642) complete:
 * IsQuorumAchievedByMask, then the pairing.  Arguments and per-item codes as
 * in hbls_batch_agg_verify / hbls_batch_seal_verify / hbls_agg_verify, plus
 * HBLS_NOQUORUM ("not enough signature collected") for an item whose mask
 * has no quorum.  Such an item is dropped on the device before hash-to-G2,
 * decompression and pairing, so it cannot fail a chunk of the combined mode.
 * One ordering difference to the reference: a quorumless item reports
 * HBLS_NOQUORUM even when its signature does not deserialise, where the
 * reference reports the deserialisation error first (DecodeSigBitmap runs
 * before the quorum check); both are errors there.
 * HBLS_ERR_BADINPUT until hbls_committee_set_quorum has been called: a
 * policy is never assumed. */
int hbls_batch_agg_verify_quorum(const hbls_committee_t *c, const uint8_t *bitmaps,
                                 const uint8_t *sigs96, const uint8_t *msgs,
                                 size_t msg_len, size_t batch, int32_t *results);
int hbls_batch_seal_verify_quorum(const hbls_committee_t *c,
                                  const uint8_t *sig_bitmaps, size_t blob_len,
                                  const uint8_t *msgs, size_t msg_len,
                                  size_t batch, int32_t *results);
int hbls_agg_verify_quorum(const hbls_committee_t *c, const uint8_t *bitmap,
                           const uint8_t sig96[96], const uint8_t *msg, size_t msg_len);

/* ---- epoch contexts: several committees in one batch ----
 * verifySignature looks up an epoch context — the key list and quorum
 * verifier of one (shardID, epoch), engine.go:644-659, :720-761 — per item, and
 * its callers mix contexts in one loop: cross-link lists
 * (core/blockchain_impl.go:403-424), the epoch chain (core/epochchain.go:125-138)
 * and a sync window that crosses an epoch boundary
 * (stagedstreamsync/sig_verify.go:51).  A context set makes that one call. */
typedef struct hbls_ctxset hbls_ctxset_t;

/* device-resident table of n_ctx committee descriptors.  The committees are
 * borrowed, not owned: they must outlive the set, and their quorum policy must
 * be set (if it is to be used) before the set is created.  Immutable after
 * creation, so it can be shared between threads.  NULL on n_ctx == 0, a NULL
 * member or allocation failure. */
hbls_ctxset_t *hbls_ctxset_create(const hbls_committee_t *const *cs, size_t n_ctx);
void   hbls_ctxset_free(hbls_ctxset_t *s);
size_t hbls_ctxset_size(const hbls_ctxset_t *s);

/* verifySignature (engine.go:619-642) for a window that mixes epoch contexts.
 * Item j is the raw commitSigAndBitmap blob  blobs[blob_off[j] .. blob_off[j+1])
 * checked against committee ctx_idx[j] on message msgs[msg_off[j] .. msg_off[j+1]).
 * blob_off and msg_off have batch+1 entries, start at 0 and never decrease
 * (else the call fails with HBLS_ERR_BADINPUT before any upload, as the CSR
 * arguments of the multi-key entries do).
 * results[j] is what hbls_batch_seal_verify (quorum != 0:
 * hbls_batch_seal_verify_quorum) returns for item j alone against
 * cs[ctx_idx[j]], in both verify modes; the exact/combined rule of
 * hbls_set_agg_verify_mode is applied to the size of the whole batch, and
 * chunks of the combined mode are formed over the mixed batch.
 * An item with ctx_idx[j] >= n_ctx, or whose blob is not 96 + ceil(n/8) bytes
 * of its context (ParseCommitSigAndBitmap, internal/chain/sig.go:23;
 * Mask.SetMask, crypto/bls/mask.go:114-120), gets HBLS_ERR_BADINPUT as its
 * own code, decided on the device before the index or the length is used as
 * an address; the other items keep their verdicts.
 * A message may have any length: the result is that of hbls_hash_to_g2 on
 * those bytes (which reads the first min(len, 48) bytes, zero-padded).
 * quorum != 0 runs IsQuorumAchievedByMask first, as the *_quorum entries do:
 * malformed -> HBLS_ERR_BADINPUT, then no quorum -> HBLS_NOQUORUM, then the
 * pairing, with the ordering difference noted at hbls_batch_agg_verify_quorum;
 * the call then fails with HBLS_ERR_BADINPUT if any committee of the set has
 * no policy set.  Malformed and quorumless items take no part in hash-to-G2,
 * decompression or pairing. */
int hbls_batch_seal_verify_ctx(const hbls_ctxset_t *s, const uint32_t *ctx_idx,
                               const uint8_t *blobs, const uint32_t *blob_off,
                               const uint8_t *msgs,  const uint32_t *msg_off,
                               size_t batch, int quorum, int32_t *results);

/* the front half alone, for parity tests and for callers that only need the
 * tally: per item the serialized masked key sum (48 zero bytes = infinity, as
 * hbls_mask_aggregate_g1), masked power and in-range popcount; ok[j] = 1 or
 * HBLS_ERR_BADINPUT (bad context index or a row that is not ceil(n/8) bytes:
 * zero block, power 0, count 0).  Items are bare bitmaps in CSR form.  Any
 * output but ok may be NULL. */
int hbls_ctx_mask_sums(const hbls_ctxset_t *s, const uint32_t *ctx_idx,
                       const uint8_t *bitmaps, const uint32_t *bm_off, size_t batch,
                       uint8_t *out48s, uint64_t *power_out, uint32_t *count_out,
                       int32_t *ok);

/* AggregateSig batch form (crypto/bls/mask.go:57-64): out = sum of n sigs */
int hbls_g2_aggregate(const uint8_t *sigs96, size_t n, uint8_t out96[96]);

/* ---- device-resident vote stream (config 5: the FBFT leader's per-message
 * hot loop, consensus/leader.go:221-309, re-shaped for the GPU) ----
 * A stream context holds, in HBM: per-round hash-to-G2 points
 * (ConstructCommitPayload outputs), participation bitmaps
 * (commitBitmap/Mask, crypto/bls/mask.go:226-242) and running aggregate
 * signatures (AddNewVote/Sign.Add, quorum.go:354-394).  One tick uploads
 * (key_idx, round_idx, sig) per vote and runs decompress -> verify ->
 * dedup -> per-round accumulate entirely on device. */
typedef struct hbls_stream hbls_stream_t;
hbls_stream_t *hbls_stream_create(const hbls_committee_t *c, int max_rounds);
void hbls_stream_free(hbls_stream_t *s);
/* (re)open round slots with their commit payloads (hashed on device) */
int hbls_stream_set_rounds(hbls_stream_t *s, const uint32_t *slots, int k,
                           const uint8_t *payloads, size_t payload_len);
/* one tick; results[j]: 1 accepted, 2 valid duplicate (quorum.go:354-394
 * double-vote rejection), 0 invalid, <0 malformed.  active_slots lists the
 * distinct round slots present in the batch. */
int hbls_stream_process(hbls_stream_t *s, const uint32_t *key_idx,
                        const uint32_t *round_idx, const uint8_t *sigs96,
                        const uint32_t *active_slots, int n_active,
                        size_t batch, int32_t *results);
/* how hbls_stream_process verifies a tick: 0 = one pairing per vote (default),
 * 1 = batched, one pairing per round slot present in the tick (see
 * hbls_batch_verify_votes_grouped; votes group by their round index).
 * Per-vote results, bitmaps and aggregates are the same in both modes.
 * Other values return HBLS_ERR_BADINPUT. */
int hbls_stream_set_verify_mode(hbls_stream_t *s, int mode);
/* pairing-check rounds' resident aggregates vs their masks
 * (validator.go:224-228); ok[i] = 1/0 */
int hbls_stream_check(hbls_stream_t *s, const uint32_t *slots, int k, int32_t *ok);
/* async form: snapshot the rounds' state (ordered after prior ticks) and run
 * the latency-bound check chain on a dedicated HIP stream, overlapping
 * subsequent ticks; one check in flight at a time.  poll waits and returns
 * the submitted k (0 if none pending). */
int hbls_stream_check_submit(hbls_stream_t *s, const uint32_t *slots, int k);
int hbls_stream_check_poll(hbls_stream_t *s, int32_t *ok);
/* export a round's bitmap + serialized aggregate
 * (consensus_service.go:305-322 commitSigAndBitmap shape) */
int hbls_stream_get(hbls_stream_t *s, uint32_t slot, uint8_t *bitmap_out,
                    uint8_t agg96_out[96]);

/* IsQuorumAchieved / the tally of resident rounds (quorum.go:409,
 * consensus/leader.go:240,319): masked power, in-range popcount and the
 * quorum verdict (1/0) of each listed round come back — 16 B per round
 * instead of the bitmap.  Any output may be NULL.  power_out and count_out
 * work before hbls_committee_set_quorum (uniform weights); quorum_out needs
 * it (HBLS_ERR_BADINPUT otherwise).  A slot >= max_rounds fails the call
 * with HBLS_ERR_BADINPUT, as in hbls_stream_get. */
int hbls_stream_power(hbls_stream_t *s, const uint32_t *slots, int k,
                      uint64_t *power_out, uint32_t *count_out, int32_t *quorum_out);

/* ---- multi-key votes ----
 * A node that runs several BLS keys sends one message per phase: one
 * signature, the sum of its keys' signatures (consensus/construct.go:99-114),
 * under a sender bitmap (SenderPubkeyBitmap, fbft_log.go:334-347).  Signer
 * sets cross the ABI in CSR form: vote j is signed by
 * key_idx[key_off[j] .. key_off[j+1]); key_off has batch + 1 entries, starts
 * at 0 and never decreases (else the call fails with HBLS_ERR_BADINPUT, before
 * any upload); the indices of one vote are strictly ascending, the order
 * GetSignedPubKeysFromBitmap yields (crypto/bls/mask.go:176-194).  A vote whose
 * list is empty, holds an index >= n or is not strictly ascending is malformed:
 * it gets HBLS_ERR_BADINPUT as its per-vote code, decided on the device before
 * any index is used as an address. */

/* signerPubKey.Add over each vote's keys (leader.go:165-172, :279-286):
 * out48s[j] = serialized key sum, ok[j] = 1; a sum that is the point at
 * infinity is 48 zero bytes, as in hbls_mask_aggregate_g1.  A malformed vote
 * has ok[j] = HBLS_ERR_BADINPUT and a zero block. */
int hbls_vote_key_sums(const hbls_committee_t *c, const uint32_t *key_off,
                       const uint32_t *key_idx, size_t batch,
                       uint8_t *out48s, int32_t *ok);

/* hbls_batch_verify_votes for signer sets: results[j] is what
 * hbls_verify_hash(sum of vote j's keys, sig_j, msg_j) returns, herumi's
 * identity edges included (an infinity key sum accepts the identity signature
 * and nothing else). */
int hbls_batch_verify_votes_multi(const hbls_committee_t *c, const uint32_t *key_off,
                                  const uint32_t *key_idx, const uint8_t *sigs96,
                                  const uint8_t *msgs, size_t msg_len, size_t batch,
                                  int32_t *results);

/* hbls_stream_process for signer sets; results[j]: 1 accepted — all of the
 * vote's bits are set (SetKeysAtomic, mask.go:226-242) and its signature is
 * added once to the round's aggregate; 2 valid, but at least one of its keys
 * had already voted in that round — no bit is set, nothing is added
 * (leader.go:127-135, :227-235); 0 invalid signature; <0 malformed.  Votes
 * of one tick take effect as if applied in ascending batch index (the
 * reference's arrival order under its mutex): {1,2}, {2,3}, {3,4} give 1, 2, 1.
 * active_slots lists the distinct round slots present in the batch; a repeated
 * slot, or an in-range round of the batch that is not listed, fails the call.
 * Honours hbls_stream_set_verify_mode, with equal results in both modes. */
int hbls_stream_process_multi(hbls_stream_t *s, const uint32_t *key_off,
                              const uint32_t *key_idx, const uint32_t *round_idx,
                              const uint8_t *sigs96, const uint32_t *active_slots,
                              int n_active, size_t batch, int32_t *results);

/* ---- signed-message windows: mixed contexts, mixed messages ----
 * hbls_batch_verify_votes_multi for a window whose items differ in committee
 * and in message: the view-ID and view-change signatures of VIEWCHANGE
 * messages (consensus/checks.go:186, view_change_construct.go:266,339), sender
 * authentication over raw message bytes (consensus/checks.go:20-39), votes of
 * several shards in one tick.
 * Item j is signed by the keys key_idx[key_off[j] .. key_off[j+1]) of
 * committee ctx_idx[j] (CSR form and rules of the multi-key entries) over
 * entry msg_idx[j] of a message table.  Table entry i is
 * msgs[msg_off[i] .. msg_off[i+1]), any length up to 2^31 - 1; when
 * msg_digest is not NULL and msg_digest[i] != 0 the message signed is the
 * Keccak-256 digest of those bytes (crypto/hash/hash.go:9-15), computed on the
 * device.  Each entry is hashed to G2 once, however many items name it.
 * results[j] is what hbls_verify_hash(K, sig_j, M) returns for the key sum K
 * and the message M (bytes or digest), with the codes of
 * hbls_batch_verify_votes_multi: herumi's identity edges included, an
 * undecodable signature and a message that does not hash (the all-zero slot,
 * which an empty undigested entry is) as that entry reports them.
 * An item with ctx_idx[j] >= n_ctx, msg_idx[j] >= n_msgs, an empty list, an
 * index >= n of its own committee or a list that is not strictly ascending is
 * malformed: HBLS_ERR_BADINPUT as its own code, decided on the device before
 * any of those values is used as an address; no key table is read for it and
 * the other items keep their verdicts.
 * The call fails with HBLS_ERR_BADINPUT before any upload on a NULL set or
 * array, batch == 0, n_msgs == 0, key_off or msg_off that does not start at 0
 * or decreases, more than 2^30 items or entries, more than 2^31 - 1 key
 * indices or entry bytes, or more than 2^32 - 1 message bytes. */
int hbls_batch_verify_msgs_ctx(const hbls_ctxset_t *s, const uint32_t *ctx_idx,
                               const uint32_t *key_off, const uint32_t *key_idx,
                               const uint8_t *sigs96, const uint32_t *msg_idx,
                               const uint8_t *msgs, const uint32_t *msg_off, size_t n_msgs,
                               const uint8_t *msg_digest, size_t batch, int32_t *results);

/* ---- combined aggregate verify ----
 * How hbls_batch_agg_verify / hbls_batch_seal_verify run their pairing stage:
 *   0  exact: one final exponentiation per item
 *   1  combined: items are weighted by fresh secret 64-bit scalars and share
 *      one final exponentiation per chunk of hbls_aggrlc_chunk_size() items,
 *      for batches >= the threshold; the items of a failing chunk are
 *      re-checked exactly, so per-item results equal mode 0 except that an
 *      invalid item is accepted with probability ~2^-64 per chunk
 *  -1  auto (default): combined for batches >= the threshold that are also
 *      above the cooperative-kernel threshold, exact otherwise
 * Other values return HBLS_ERR_BADINPUT.  The environment variable
 * HBLS_AGG_VERIFY_MODE (0/1) sets the initial mode.  When the OS random
 * source or the combination's device memory is unavailable the call takes
 * the exact path.  hbls_batch_agg_verify_partials always runs mode 0 (its
 * external partial sums are not subgroup-checked). */
int hbls_set_agg_verify_mode(int mode);
void hbls_set_aggrlc_threshold(int min_batch);   /* < 0 restores the default */
int hbls_aggrlc_chunk_size(void);
/* chunks checked, chunks failed, items re-checked per item — of the last
 * aggregate-verify call on this thread (zeros when it ran exact) */
void hbls_aggrlc_last_stats(uint32_t out[3]);
/* the kernel that runs the chunks' final exponentiations on the combined
 * path: 16 or 8 = four lanes per chunk with that many chunks
 * per block, 0 = one lane per chunk, -1 restores the default (16).  Verdicts
 * are the same for every choice.  Other values return HBLS_ERR_BADINPUT.
 * The environment variable HBLS_AGGRLC_FINAL (0/8/16) sets the initial one. */
int hbls_set_aggrlc_final(int kernel);
/* runs every final kernel on nchunks deterministic chunk products (arbitrary
 * elements, Fp6-subfield elements, one; empty and forced chunks) and returns
 * the number of chunks on which a cooperative launch and the one-lane kernel
 * disagree (0 = parity); HBLS_ERR if the one-lane verdicts are not the ones
 * the inputs dictate, a mix of 0 and 1 from two chunks up. */
int hbls_aggrlc_final_selftest(int nchunks);
/* where the combined path pairs the signatures: 0 = one
 * Miller leg per item, 1 = one per chunk, on the sum of the chunk's scaled
 * signatures, -1 = the default rule (1 from 16384 items).  Per-item results
 * and hbls_aggrlc_last_stats are the same for both.  Other values return
 * HBLS_ERR_BADINPUT and change nothing.  The environment variable
 * HBLS_AGGRLC_SIGLEG (0/1) sets the initial one.  With leg 1,
 * hbls_last_stage_ns(7) of the plain entries is the signature scaling and
 * chunk sums, inside hbls_last_stage_ns(3). */
int hbls_set_aggrlc_sigleg(int leg);
/* when leg 1's chunk entries are paired: 0 = inside the
 * Miller kernel, behind the items; 1 = hoisted: signature scaling and chunk
 * sums run ahead of the mask kernel and the chunk legs beside it on a side
 * stream (hbls_batch_agg_verify, the seal and the quorum entries; the
 * epoch-context entry keeps the sequence of 0); -1 = the default rule
 * (hoisted from 262144 items).  Per-item results and
 * hbls_aggrlc_last_stats are the same for both.  Other values return
 * HBLS_ERR_BADINPUT and change nothing.  The environment variable
 * HBLS_AGGRLC_EARLY (0/1) sets the initial one.  When hoisted,
 * hbls_last_stage_ns(7) lies ahead of the mask stage and is counted into
 * hbls_last_stage_ns(3); hbls_last_stage_ns(8) is the chunk-leg kernel's own
 * interval on its stream (zero when nothing was hoisted) and
 * hbls_last_stage_ns(4) includes the repair launches. */
int hbls_set_aggrlc_early(int early);
/* the kernel that runs the hoisted chunk legs: 16 = four lanes per chunk with
 * 16 chunks per block, 0 = one lane per chunk, -1 restores the default (16).
 * Verdicts are the same for both.  Other values return HBLS_ERR_BADINPUT.
 * The environment variable HBLS_AGGRLC_CHUNKLEG (0/16) sets the initial one. */
int hbls_set_aggrlc_chunkleg(int kernel);
/* the Miller kernel of leg 1's items: 0 = affine arguments
 * (two inversions per item), per-item values stored and multiplied by a
 * kernel of their own; 1 = Jacobian arguments, no inversion; 2 = that, and
 * the chunk product taken inside the Miller kernel, across the lanes of the
 * wave that is the chunk; -1 restores the default (2).  Honoured wherever
 * leg 1 runs, hoisted or not, the epoch-context entry included.  Per-item
 * results and hbls_aggrlc_last_stats are the same for every level.  Other
 * values return HBLS_ERR_BADINPUT and change nothing.  The environment
 * variable HBLS_AGGRLC_MILLER (0/1/2) sets the initial one.
 * hbls_last_stage_ns(5) is the chunk products' interval at every level: at 2
 * only the chunk entries' one multiplication per chunk is left in it. */
int hbls_set_aggrlc_miller(int level);

/* batch Keccak-256 (consensus message digests, crypto/hash/hash.go:9-15) */
int hbls_batch_keccak256(const uint8_t *msgs, size_t msg_len, size_t batch,
                         uint8_t *out32s);

/* ---- introspection ---- */
const char *hbls_version(void);
/* measured device 64x64->128 integer-mad throughput (ops/s) — the VALU
 * roofline peak for this integer-bound path (no datasheet figure exists) */
double hbls_mad_peak_ops(void);
/* elapsed device-time of the last batch call on this thread's stream, in ns
 * (HIP events); 0 if unavailable.  For bench.py's roofline leg. */
uint64_t hbls_last_kernel_ns(void);
/* host-side intervals (steady clock, ns) of the last aggregate-verify call on
 * this thread: 0 device allocations, 1 time spent inside upload calls,
 * 2 first launch to results on the host, 3 frees, 4 the whole call.  Other
 * indices return 0. */
uint64_t hbls_last_host_ns(int i);

#ifdef __cplusplus
}
#endif
#endif /* HBLS_H */
