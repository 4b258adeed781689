"""harmony_amd.engine — host mirror of engineImpl's signature leg
(internal/chain/engine.go:581-718), re-built around one device call per
window.

The reference verifies one seal at a time: verifySignatureCached looks the
seal up in a cache of accepted seals, verifySignature fetches the epoch
context of the item's (shardID, epoch) from an LRU of 20, decodes signature
and bitmap, asks the context's quorum verifier and runs the pairing.  Here a
whole window — headers of a sync batch, the epoch chain, a list of
cross-links — is resolved on the host (cache hits, epoch contexts, commit
payloads) and every miss goes to the device in a single
ContextSet.seal_verify call, whatever mix of committees and
payload lengths the window holds.

This is bookkeeping only.  The verifier is injectable, so everything in this
module can be exercised without a GPU; the default one runs on the device.

One deliberate difference to the reference: the verified-seal cache keys on
the WHOLE bitmap.  The reference copies the bitmap into a fixed 64-byte array
(newVerifiedSigKey, engine.go:661-680, "Support 512 at most validator
nodes"), so two bitmaps of a committee above 512 keys that agree in their
first 64 bytes share a cache entry there — the second would be accepted
unverified.  This library serves committees of 4096 keys and more, so the key
is (block hash, signature, full bitmap).
"""
from collections import OrderedDict, namedtuple

HBLS_OK = 1
HBLS_ERR_BADINPUT = -3

EPOCH_CTX_CACHE = 20        # epochCtxCache (engine.go:39)
VERIFIED_SIG_CACHE = 100    # verifiedSigCache (engine.go:38)

# payloadArgs + sigArgs (engine.go:682-718) of one header or cross-link
SealItem = namedtuple("SealItem", "shard_id epoch block_hash number view_id sig bitmap")

VerifyResult = namedtuple("VerifyResult", "codes first_failure")


def construct_commit_payload(number: int, block_hash: bytes, view_id: int,
                             is_staking: bool) -> bytes:
    """ConstructCommitPayload (consensus/signature/signature.go:12-24):
    LE64(number) || hash, and from the staking epoch on || LE64(viewID):
    40 or 48 bytes"""
    out = number.to_bytes(8, "little") + block_hash
    if is_staking:
        out += view_id.to_bytes(8, "little")
    return out


class EpochContext:
    """epochCtx (engine.go:727-733) of one (shardID, epoch): the key list and
    what the quorum verifier needs.  power None is the uniform policy, else n
    voting powers in 1e-18 units (votepower.compute).  `committee` is filled
    by the device verifier on first use."""

    def __init__(self, key, pks: bytes, n: int, power, is_staking: bool):
        if len(pks) != 48 * n:
            raise ValueError(f"epoch context {key}: expected {48 * n} key bytes got {len(pks)}")
        if power is not None and len(power) != n:
            raise ValueError(f"epoch context {key}: expected {n} powers got {len(power)}")
        self.key = key
        self.pks = pks
        self.n = n
        self.power = None if power is None else list(power)
        self.is_staking = bool(is_staking)
        self.committee = None


class DeviceVerifier:
    """the default verifier: device committees per context and one ContextSet,
    rebuilt when the list of contexts it is handed changes"""

    def __init__(self):
        self._set = None
        self._set_ids = None

    def __call__(self, contexts, ctx_idx, blobs, msgs, quorum):
        from . import core
        ids = tuple(id(c) for c in contexts)
        if self._set is None or ids != self._set_ids:
            for c in contexts:
                if c.committee is None:
                    committee = core.Committee(c.pks, c.n)
                    committee.set_quorum(c.power)
                    c.committee = committee
            self._set = core.ContextSet([c.committee for c in contexts])
            self._set_ids = ids
            self._contexts = list(contexts)     # keeps the ids valid
        return self._set.seal_verify(ctx_idx, blobs, msgs, quorum=quorum)


class Engine:
    """loader(shard_id, epoch) -> (pks, n, power or None, is_staking) reads an
    epoch context from the chain (readEpochCtxFromChain, engine.go:735-761).
    verifier(contexts, ctx_idx, blobs, msgs, quorum) -> per-item codes; the
    default runs ContextSet.seal_verify on the device."""

    def __init__(self, loader, verifier=None, quorum=True,
                 ctx_cache=EPOCH_CTX_CACHE, sig_cache=VERIFIED_SIG_CACHE):
        self._loader = loader
        self._verifier = DeviceVerifier() if verifier is None else verifier
        self._quorum = bool(quorum)
        self._ctx_cap = ctx_cache
        self._sig_cap = sig_cache
        self._ctx = OrderedDict()       # (shard_id, epoch) -> EpochContext, LRU
        self._verified = OrderedDict()  # (hash, sig, whole bitmap) -> None, LRU

    # -- getEpochCtxCached (engine.go:644-659)
    def epoch_context(self, shard_id: int, epoch: int) -> EpochContext:
        key = (shard_id, epoch)
        ctx = self._ctx.get(key)
        if ctx is not None:
            self._ctx.move_to_end(key)
            return ctx
        pks, n, power, is_staking = self._loader(shard_id, epoch)
        ctx = EpochContext(key, pks, n, power, is_staking)
        self._ctx[key] = ctx
        while len(self._ctx) > self._ctx_cap:
            self._ctx.popitem(last=False)
        return ctx

    def resident_contexts(self):
        """keys of the cached epoch contexts, least recently used first"""
        return list(self._ctx)

    @staticmethod
    def _verified_key(item):
        return (bytes(item.block_hash), bytes(item.sig), bytes(item.bitmap))

    def _verify(self, items):
        items = list(items)
        codes = [None] * len(items)
        miss, used, order = [], {}, []
        for j, it in enumerate(items):
            key = self._verified_key(it)
            if key in self._verified:
                self._verified.move_to_end(key)
                codes[j] = HBLS_OK
                continue
            ctx = self.epoch_context(it.shard_id, it.epoch)
            if ctx.key not in used:
                used[ctx.key] = ctx
                order.append(ctx)
            miss.append((j, ctx, key))
        if miss:
            # the resident list is stable from call to call, so the device set
            # is reused; a window that touches more contexts than the cache
            # holds brings its own list
            if all(k in self._ctx for k in used):
                contexts = list(self._ctx.values())
            else:
                contexts = order
            pos = {c.key: i for i, c in enumerate(contexts)}
            ctx_idx = [pos[c.key] for _, c, _ in miss]
            blobs = [bytes(items[j].sig) + bytes(items[j].bitmap) for j, _, _ in miss]
            msgs = [construct_commit_payload(items[j].number, items[j].block_hash,
                                             items[j].view_id, c.is_staking)
                    for j, c, _ in miss]
            res = self._verifier(contexts, ctx_idx, blobs, msgs, self._quorum)
            if len(res) != len(miss):
                raise RuntimeError("verifier returned a wrong number of codes")
            for (j, _, key), r in zip(miss, res):
                codes[j] = r
                if r == HBLS_OK:        # accepted items only (engine.go:612-615)
                    self._verified[key] = None
                    self._verified.move_to_end(key)
                    while len(self._verified) > self._sig_cap:
                        self._verified.popitem(last=False)
        first = next((j for j, r in enumerate(codes) if r != HBLS_OK), None)
        return VerifyResult(codes, first)

    def verify_headers(self, items) -> VerifyResult:
        """VerifyHeaderSignature (engine.go:581-589) over a window of
        SealItems: per-item codes (1 accept, 0 reject, HBLS_ERR_BADINPUT,
        NOQUORUM) and the index of the first item that is not accepted (None
        if all are) — what the reference's loop stops at."""
        return self._verify(items)

    def verify_crosslinks(self, items) -> VerifyResult:
        """VerifyCrossLink (engine.go:591-604) over a list: a cross-link of
        block number <= 1 is refused before anything else ("crossLink
        BlockNumber should greater than 1") with HBLS_ERR_BADINPUT and is not
        sent to the verifier."""
        items = list(items)
        keep = [j for j, it in enumerate(items) if it.number > 1]
        sub = self._verify([items[j] for j in keep])
        codes = [HBLS_ERR_BADINPUT] * len(items)
        for j, r in zip(keep, sub.codes):
            codes[j] = r
        first = next((j for j, r in enumerate(codes) if r != HBLS_OK), None)
        return VerifyResult(codes, first)
