"""harmony_amd.stream — config-5 streaming FBFT round harness
(BASELINE.json configs[4]): a stream of Prepare/Commit vote messages,
each a protobuf-like blob -> Keccak-256 digest -> per-message signature
verify against the sender's committee key -> incremental aggregate
(mask bit + G2 sum), with pairing checks of the running aggregates.

Mirrors the leader's per-message hot loop (consensus/leader.go:221-309:
parse -> ConstructCommitPayload -> Sign.Deserialize -> VerifyHash ->
AddNewVote -> commitBitmap.SetKeysAtomic) over the DEVICE-RESIDENT stream
context (core.Stream / hbls_stream_*): per-round hash points, bitmaps and
running G2 aggregates live in HBM; each tick is one upload + a fixed kernel
chain (decompress -> verify -> dedup -> per-round accumulate) + one
4B-per-vote download.  Round-1's shape (host bookkeeping + per-round
aggregation launches) capped at ~3.4k msgs/s; this is the round-2 redesign.
"""
from . import core


def ordered_claim_model(bitmaps, tick):
    """Pure-Python model of the multi-key tick's ordered all-or-nothing rule
    (hbls_stream_process_multi; the reference's
    drop-if-any-key-voted check, leader.go:127-135, followed by SetKeysAtomic).

    bitmaps: the rounds' current bitmaps, a list of bytes indexed by round.
    tick: (round, keys, valid) per vote in batch order; valid is the verify
    stage's verdict — True/1 for a valid signature, False/0 for an invalid
    one, or a negative code for a malformed vote.
    Returns (results, new_bitmaps): a valid vote gets 1 and sets all its bits
    when none of them is set at its turn, else 2 and sets nothing; any other
    vote keeps its verdict as its result."""
    new = [bytearray(b) for b in bitmaps]
    results = []
    for r, keys, valid in tick:
        if int(valid) != 1:
            results.append(int(valid))
            continue
        bm = new[r]
        if any(bm[k >> 3] & (1 << (k & 7)) for k in keys):
            results.append(2)
            continue
        for k in keys:
            bm[k >> 3] |= 1 << (k & 7)
        results.append(1)
    return results, [bytes(b) for b in new]


class StreamVerifier:
    """Single-round stream (window-checked).  External API kept from round 1:
    process_batch / final_check / accepted / rejected / bitmap / agg_sig."""

    def __init__(self, pks_cat: bytes, n: int, payload: bytes, window: int = 100,
                 batched: bool = False):
        """pks_cat: committee table; payload: the commit payload all votes of
        this round sign (leader.go:250); window: aggregate-check period;
        batched: verify each tick by random combination (one pairing per
        round) instead of one pairing per vote — same results."""
        self.committee = core.Committee(pks_cat, n)
        self.n = n
        self.payload = payload
        self.window = window
        self.stream = core.Stream(self.committee, 1)
        if batched:
            self.stream.set_verify_mode(1)
        self.stream.set_rounds([0], payload, len(payload))
        self.accepted = 0
        self.rejected = 0
        self.window_checks = 0
        self._since_check = 0

    @property
    def bitmap(self) -> bytes:
        return self.stream.get(0)[0]

    @property
    def agg_sig(self) -> bytes:
        return self.stream.get(0)[1]

    def process_batch(self, key_idx, sigs_cat: bytes, blobs_cat: bytes, blob_len: int,
                      expected_digests: bytes = None):
        """One micro-batch of votes: blobs are hashed on-GPU (sender-auth
        digest path, checks.go:20-39 analog), then one device tick
        (verify + dedup + accumulate).

        expected_digests: batch*32 bytes of Keccak-256 digests the senders
        committed to (the hash the message signature covers in
        consensus_service.go:115-119); a vote whose blob hashes differently
        is rejected before the signature check."""
        batch = len(key_idx)
        # keccak digests of the raw message blobs (crypto/hash/hash.go:9-15)
        digests = core.batch_keccak256(blobs_cat, blob_len, batch)
        digest_ok = [True] * batch
        if expected_digests is not None:
            if len(expected_digests) != 32 * batch:
                raise ValueError("expected_digests must be batch*32 bytes")
            digest_ok = [digests[32 * j:32 * (j + 1)] ==
                         expected_digests[32 * j:32 * (j + 1)] for j in range(batch)]
        live = [j for j in range(batch) if digest_ok[j]]
        res = [0] * batch
        if live:
            sigs = b"".join(sigs_cat[96 * j:96 * (j + 1)] for j in live) \
                if len(live) != batch else sigs_cat
            dev = self.stream.process([key_idx[j] for j in live],
                                      [0] * len(live), sigs)
            for j, r in zip(live, dev):
                res[j] = r
        for r in res:
            if r == 1:
                self.accepted += 1
            else:
                self.rejected += 1
        self._since_check += batch
        if self._since_check >= self.window:
            self._since_check = 0
            self.window_checks += 1
            if not self.stream.check([0])[0]:
                raise RuntimeError("streaming aggregate diverged from mask")
        # report duplicates/invalid alike as non-1 (round-1 API shape)
        return [r if r == 1 else 0 for r in res]

    def final_check(self) -> bool:
        return self.stream.check([0])[0]


class _RoundView:
    """per-round state accessor (bitmap/aggregate fetched from the device)"""

    def __init__(self, msv, slot):
        self._msv = msv
        self._slot = slot
        self.payload = msv.payloads[slot]
        self.accepted = 0
        self.rejected = 0

    @property
    def bitmap(self) -> bytes:
        return self._msv.stream.get(self._slot)[0]

    @property
    def agg_sig(self) -> bytes:
        return self._msv.stream.get(self._slot)[1]


class MultiStreamVerifier:
    """R concurrent FBFT rounds (consecutive blocks / multiple shards) sharing
    one committee: pending votes from ALL rounds are verified, deduped and
    folded into their rounds' resident aggregates in ONE device tick.
    This is the production shape of the vote pipeline — per-item latency is
    amortized across rounds in flight, so throughput tracks the batch rate
    instead of the single-pairing latency."""

    def __init__(self, pks_cat: bytes, n: int, payloads, window: int = 100,
                 batched: bool = False):
        if len(set(len(p) for p in payloads)) > 1:
            raise ValueError("payloads must share a length for the batched launch")
        self.committee = core.Committee(pks_cat, n)
        self.n = n
        self.payloads = list(payloads)
        self.mlen = len(payloads[0])
        self.stream = core.Stream(self.committee, len(payloads))
        if batched:
            self.stream.set_verify_mode(1)
        self.stream.set_rounds(list(range(len(payloads))),
                               b"".join(payloads), self.mlen)
        self.rounds = [_RoundView(self, r) for r in range(len(payloads))]
        self.window = window
        self._since_check = [0] * len(payloads)
        self.window_checks = 0

    def process(self, votes):
        """votes: list of (round_idx, key_idx, sig96 bytes).  One device
        tick; per-round bookkeeping from the downloaded results.  Rounds
        whose message count crosses the window get ONE batched pairing
        check (the 'periodic batch pairing' of BASELINE configs[4]).

        key_idx may be a tuple of ascending indices for a multi-key sender
        (one summed signature, consensus/construct.go:99-114); a tick that
        holds any tuple goes through the multi-key entry, where votes take
        effect in list order and a vote with an already-voted key sets
        nothing."""
        key_idx = [v[1] for v in votes]
        round_idx = [v[0] for v in votes]
        sigs = b"".join(v[2] for v in votes)
        if any(isinstance(k, tuple) for k in key_idx):
            res = self.stream.process_multi(
                [k if isinstance(k, tuple) else (k,) for k in key_idx], round_idx, sigs)
        else:
            res = self.stream.process(key_idx, round_idx, sigs)
        for (r, _i, _s), ok in zip(votes, res):
            if ok == 1:
                self.rounds[r].accepted += 1
            else:
                self.rounds[r].rejected += 1
            self._since_check[r] += 1
        due = [r for r, c in enumerate(self._since_check) if c >= self.window]
        if due:
            self.window_checks += len(due)
            for r in due:
                self._since_check[r] = 0
            # async: collect the PREVIOUS window check's verdicts, then
            # submit this one on the side stream so the pairing chain
            # overlaps the next ticks (divergence detection trails by one
            # window, like the reference's eventually-checked aggregates)
            self._collect_window_check()
            self.stream.check_submit(due)
        return [r if r == 1 else 0 for r in res]

    def _collect_window_check(self):
        verdicts = self.stream.check_poll()
        if verdicts and not all(verdicts.values()):
            raise RuntimeError("streaming aggregate diverged from mask")

    def reset_rounds(self, payloads):
        """open a fresh set of rounds in place (new block heights): hashes
        the payloads on device and clears bitmaps + aggregates, one call."""
        self._collect_window_check()   # verdicts belong to the old rounds
        if len(payloads) != len(self.payloads) or \
                any(len(p) != self.mlen for p in payloads):
            raise ValueError("reset_rounds: shape mismatch")
        self.payloads = list(payloads)
        self.stream.set_rounds(list(range(len(payloads))),
                               b"".join(payloads), self.mlen)
        for r, rv in enumerate(self.rounds):
            rv.payload = payloads[r]
            rv.accepted = rv.rejected = 0
        self._since_check = [0] * len(payloads)

    def final_check_all(self) -> bool:
        """one batched aggregate-verify across every round in flight"""
        self._collect_window_check()
        return all(self.stream.check(list(range(len(self.rounds)))))

    def final_check_submit(self):
        """async form of final_check_all: snapshots every round's state now
        (safe across a following reset_rounds — the snapshot is taken on
        the tick stream before the reset) and verifies on the side stream;
        collect the verdict with final_check_collect.  The pipelined shape:
        submit at the end of one block batch, collect at the start of the
        next — every aggregate still gets checked, one batch later."""
        self._collect_window_check()
        self.stream.check_submit(list(range(len(self.rounds))))

    def final_check_collect(self) -> bool:
        verdicts = self.stream.check_poll()
        return all(verdicts.values()) if verdicts else True
