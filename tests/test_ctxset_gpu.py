"""Epoch contexts: seal batches that span several committees
in one device call.  The front half (per-item masked key sum, power, count)
is checked against the CPU oracle and Python integer sums; the verdicts of
ContextSet.seal_verify against Committee.batch_seal_verify(_quorum) of each
item alone against its own committee and against the oracle's
Committee.batch_agg_verify, in both pairing modes."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from oracle import pyref as pr  # noqa: E402
from harmony_amd import votepower as vp  # noqa: E402


def _gpu_available():
    try:
        from harmony_amd import core
        return core.device_count() > 0
    except Exception:
        return False


if not os.environ.get("HBLS_FORCE_GPU_TESTS"):
    pytestmark = [pytest.mark.gpu,
                  pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]

# 1, 7, 8, 9: byte boundaries; 250 twice: right size, wrong committee; 1025
# crosses the 1024-bit compaction segment; 2053 takes the window table with a
# ragged last group
SIZES = [1, 7, 8, 9, 64, 250, 250, 1025, 2053]
NCTX = len(SIZES)
SMALL, BIG = (0, 1), (7, 8)         # contexts of 1 | 7 and of 1025 | 2053 keys
TOTAL = 130
E18 = 10 ** 18
HP, EP = 49 * E18 // 100, 51 * E18 // 100
BADINPUT = -3
NOQUORUM = -4


def _mask_of(n, signers):
    bm = bytearray((n + 7) // 8)
    for i in signers:
        bm[i >> 3] |= 1 << (i & 7)
    return bytes(bm)


def _staked_weights(n, seed):
    rng = random.Random(seed)
    stakes = [None if rng.random() < 0.2 else rng.randrange(1, 10 ** 6) * 10 ** 15
              for _ in range(n)]
    if n > 1:
        stakes[0] = None
    stakes[-1] = 3 * E18
    w = vp.compute(stakes, HP, EP)
    assert sum(w) == E18
    return w


def _one_big_weights(n, big):
    """key `big` holds 0.7: it alone decides"""
    if n == 1:
        return [E18]
    rest = 3 * E18 // 10
    w = [rest // (n - 1)] * n
    w[big] = 7 * E18 // 10
    last = n - 1 if big != n - 1 else n - 2
    w[last] += E18 - sum(w)
    assert sum(w) == E18
    return w


def _expect_power(row, n, w):
    x = int.from_bytes(row, "little") & ((1 << n) - 1)
    bits = [i for i in range(n) if (x >> i) & 1]
    return (len(bits) if w is None else sum(w[i] for i in bits)), len(bits)


class _Env:
    """nine committees of disjoint keys with their quorum policies (uniform on
    even positions, one key holding 0.7 on odd ones), the oracle's twins, 130
    valid seal items over all of them, and caches of the per-item reference
    verdicts — built once, never modified."""

    def __init__(self, capi):
        from harmony_amd import core
        self.core = core
        self.capi = capi
        self.sk = [[pr.synth_sk(20000 + 4096 * c + i) for i in range(n)]
                   for c, n in enumerate(SIZES)]
        flat = [k for ks in self.sk for k in ks]
        cat = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in flat), len(flat))
        self.pks, at = [], 0
        for n in SIZES:
            self.pks.append(cat[48 * at:48 * (at + n)])
            at += n
        self.big = [n // 2 for n in SIZES]
        self.weights = [None if c % 2 == 0 else _one_big_weights(n, self.big[c])
                        for c, n in enumerate(SIZES)]
        self.committees = self.fresh_committees()
        for c, committee in enumerate(self.committees):
            committee.set_quorum(self.weights[c])
        self.ctxset = core.ContextSet(self.committees)
        self.oracles = [capi.Committee(self.pks[c], n) for c, n in enumerate(SIZES)]
        self._alone, self._oracle, self._valid = {}, {}, None

        rng = random.Random(11)
        spec = []
        for j in range(TOTAL):
            c = j % NCTX
            n = SIZES[c]
            signers = rng.sample(range(n), rng.randrange(1, n + 1))
            mlen = (32, 40, 48)[rng.randrange(3)]
            msg = pr.construct_commit_payload(j, pr.synth_msg(900 + j), j + 1)[:mlen]
            spec.append((c, signers, msg))
        self.ctx_idx = [c for c, _, _ in spec]
        self.msgs = [m for _, _, m in spec]
        self.blobs = self.sign(spec)
        assert {len(m) for m in self.msgs} == {32, 40, 48}
        # a valid signature that belongs to no item
        self.D = capi.sign_hash(pr.fr_serialize(pr.synth_sk(999)), self.msgs[0])
        assert core.aggrlc_chunk_size() == 64

    def valid_verdicts(self):
        if self._valid is None:
            self._valid = self.ctxset.seal_verify(self.ctx_idx, self.blobs, self.msgs)
        return self._valid

    def fresh_committees(self):
        return [self.core.Committee(self.pks[c], n) for c, n in enumerate(SIZES)]

    def sign(self, spec):
        """blobs (signature || mask) of (context, signers, message) items: one
        signature under the sum of the signers' secret keys (BLS is linear in
        the key), signed on the device per message length"""
        sigs = [None] * len(spec)
        for mlen in sorted({len(m) for _, _, m in spec}):
            pick = [j for j, s in enumerate(spec) if len(s[2]) == mlen]
            sks = b"".join(pr.fr_serialize(sum(self.sk[spec[j][0]][i] for i in spec[j][1]) % pr.R)
                           for j in pick)
            cat = self.core.batch_sign(sks, b"".join(spec[j][2] for j in pick), mlen, len(pick))
            for k, j in enumerate(pick):
                sigs[j] = cat[96 * k:96 * (k + 1)]
        return [sigs[j] + _mask_of(SIZES[c], signers) for j, (c, signers, _) in enumerate(spec)]

    def alone(self, c, blob, msg, quorum=False):
        """the item alone through the single-committee entry; a call that
        fails with bad input is that item's HBLS_ERR_BADINPUT"""
        key = (c, blob, msg, quorum)
        if key not in self._alone:
            committee = self.committees[c]
            fn = committee.batch_seal_verify_quorum if quorum else committee.batch_seal_verify
            try:
                self._alone[key] = fn(blob, len(blob), msg, len(msg), 1)[0]
            except self.core.BadInputError:
                self._alone[key] = BADINPUT
        return self._alone[key]

    def oracle(self, c, blob, msg):
        """the CPU oracle's verdict of a well-formed item (1/0, negative on a
        signature that does not deserialise)"""
        key = (c, blob, msg)
        if key not in self._oracle:
            r = self.oracles[c].batch_agg_verify(blob[96:], blob[:96], msg, len(msg), 1)[0]
            self._oracle[key] = r
        return self._oracle[key]

    def check_refs(self, ctx_idx, blobs, msgs, res, quorum=False):
        """res against the single-committee entry and the oracle, per item"""
        for j, (c, blob, msg) in enumerate(zip(ctx_idx, blobs, msgs)):
            if c >= NCTX:
                assert res[j] == BADINPUT, j
                continue
            assert res[j] == self.alone(c, blob, msg, quorum), (j, c)
            if res[j] in (0, 1):
                assert self.oracle(c, blob, msg) == res[j], (j, c)


@pytest.fixture(scope="module")
def env(oracle_lib):
    return _Env(oracle_lib)


# ------------------------------------------------------------ 1. mask sums

def _density_row(n, p, rng):
    bm = (n + 7) // 8
    x = 0
    for i in range(8 * bm):             # padding bits too
        if rng.random() < p:
            x |= 1 << i
    return x.to_bytes(bm, "little")


def _mask_items():
    """(context, row) items: per context all-zero, all-ones with the padding
    bits set, one bit, ~10 % and ~90 % density; the smallest and the largest
    contexts get a ~50 % row too, so that there are enough of them to put one
    of each into every run of four.  Returned in the mixed order."""
    rng = random.Random(5)
    per_ctx = []
    for c, n in enumerate(SIZES):
        bm = (n + 7) // 8
        rows = [bytes(bm), b"\xff" * bm, _mask_of(n, [n // 2]),
                _density_row(n, 0.1, rng), _density_row(n, 0.9, rng)]
        if c in SMALL or c in BIG:
            rows.append(_density_row(n, 0.5, rng))
        per_ctx.append(rows)

    def interleave(ctxs):
        out = []
        for k in range(max(len(per_ctx[c]) for c in ctxs)):
            out += [(c, per_ctx[c][k]) for c in ctxs if k < len(per_ctx[c])]
        return out
    small, big = interleave(SMALL), interleave(BIG)
    other = interleave([c for c in range(NCTX) if c not in SMALL and c not in BIG])
    assert len(small) == len(big) == 12 and len(other) == 25
    mixed = [other.pop()]
    for k in range(12):
        mixed += [small[k], big[k], other.pop(), other.pop()]
    assert not other
    for a, b in zip(mixed, mixed[1:]):
        assert a[0] != b[0]
    for k in range(len(mixed) - 3):
        run = {c for c, _ in mixed[k:k + 4]}
        assert run & set(SMALL) and run & set(BIG)
    return mixed


def test_mask_sums(env):
    core = env.core
    mixed = _mask_items()
    by_ctx = sorted(mixed, key=lambda it: it[0])
    want_sum = {}
    for c, row in mixed:
        want_sum[(c, row)] = env.oracles[c].mask_aggregate(row)
        if not any(row):
            assert want_sum[(c, row)] == bytes(48)
    committees = env.fresh_committees()
    staked = [_staked_weights(n, 40 + c) for c, n in enumerate(SIZES)]
    for policy in ("unset", "uniform", "staked"):
        if policy != "unset":
            for c, committee in enumerate(committees):
                committee.set_quorum(staked[c] if policy == "staked" else None)
        cs = core.ContextSet(committees)
        assert len(cs) == NCTX
        for items in (mixed, by_ctx):
            idx = [c for c, _ in items]
            rows = [r for _, r in items]
            sums, pw, cn, ok = cs.mask_sums(idx, rows)
            assert ok == [1] * len(items), policy
            for j, (c, row) in enumerate(items):
                w = staked[c] if policy == "staked" else None
                p, k = _expect_power(row, SIZES[c], w)
                assert cn[j] == k, (policy, j, c)
                assert pw[j] == p, (policy, j, c)
                assert sums[j] == want_sum[(c, row)], (policy, j, c)
                if not any(row):
                    assert sums[j] == bytes(48)
    # a bad context index and a wrong row length cost that item alone
    idx = [c for c, _ in mixed]
    rows = [r for _, r in mixed]
    idx[3], idx[17] = NCTX, 0xffffffff
    rows[8] = rows[8] + b"\x01"
    rows[20] = rows[20][:-1]
    rows[30] = b""
    bad = {3, 17, 8, 20, 30}
    sums, pw, cn, ok = cs.mask_sums(idx, rows)
    for j, (c, row) in enumerate(mixed):
        if j in bad:
            assert (ok[j], sums[j], pw[j], cn[j]) == (BADINPUT, bytes(48), 0, 0), j
        else:
            assert ok[j] == 1 and sums[j] == want_sum[(c, row)], j
            assert (pw[j], cn[j]) == _expect_power(row, SIZES[c], staked[c]), j


# ------------------------------------------------------------ 2./3. verdicts

def _cases(env):
    """(name, ctx_idx, blobs, expected verdicts, failing chunks of the
    combined mode); the messages are env.msgs throughout"""
    ok = [1] * TOTAL
    yield "valid", env.ctx_idx, env.blobs, ok, 0
    for at in (0, 64, 129):
        blobs = list(env.blobs)
        blobs[at] = env.D + blobs[at][96:]
        yield f"wrong{at}", env.ctx_idx, blobs, [0 if j == at else 1 for j in range(TOTAL)], 1
    # an item of one 250-key committee submitted under the other
    idx = list(env.ctx_idx)
    at = idx.index(5)
    idx[at] = 6
    yield "other250", idx, env.blobs, [0 if j == at else 1 for j in range(TOTAL)], 1
    idx, blobs, want = list(env.ctx_idx), list(env.blobs), list(ok)
    idx[3], idx[10] = NCTX, 0xffffffff
    blobs[20] = blobs[20][:-1]
    blobs[30] = blobs[30] + b"\x00"
    blobs[40] = blobs[40][:95]
    for j in (3, 10, 20, 30, 40):
        want[j] = BADINPUT
    yield "malformed", idx, blobs, want, 0


@pytest.mark.parametrize("part", range(5))
def test_valid_items_alone(env, part):
    """the 130 valid items, a fifth at a time (a single-item call costs tens of
    milliseconds): the mixed call's verdicts against each item alone and the
    oracle.  Fills the reference caches test_verdicts reads."""
    res = env.valid_verdicts()
    assert res == [1] * TOTAL
    for j in range(part, TOTAL, 5):
        c, blob, msg = env.ctx_idx[j], env.blobs[j], env.msgs[j]
        assert env.alone(c, blob, msg) == res[j], (j, c)
        assert env.oracle(c, blob, msg) == res[j], (j, c)


def test_verdicts(env):
    for name, idx, blobs, want, _ in _cases(env):
        res = env.ctxset.seal_verify(idx, blobs, env.msgs)
        assert res == want, name
        env.check_refs(idx, blobs, env.msgs, res)


def test_offsets_must_not_decrease(env):
    core = env.core
    _, boff = core.pack_blobs(env.blobs)
    _, moff = core.pack_blobs(env.msgs)
    for which in (0, 1):
        offs = [list(boff), list(moff)]
        offs[which][5], offs[which][6] = offs[which][6], offs[which][5]
        with pytest.raises(core.BadInputError):
            env.ctxset.seal_verify(env.ctx_idx, env.blobs, env.msgs, offsets=tuple(offs))
        offs = [list(boff), list(moff)]
        offs[which][0] = 1
        with pytest.raises(core.BadInputError):
            env.ctxset.seal_verify(env.ctx_idx, env.blobs, env.msgs, offsets=tuple(offs))


def test_both_pairing_modes(env):
    core = env.core
    for name, idx, blobs, want, failing in _cases(env):
        eligible = sum(1 for r in want if r != BADINPUT)
        with core.aggrlc_switches(mode=0):
            r0 = env.ctxset.seal_verify(idx, blobs, env.msgs)
            s0 = core.aggrlc_last_stats()
        with core.aggrlc_switches(mode=1, threshold=1):
            r1 = env.ctxset.seal_verify(idx, blobs, env.msgs)
            s1 = core.aggrlc_last_stats()
        assert r0 == want and r1 == want, name
        assert s0 == [0, 0, 0], name
        # chunks are formed over the mixed batch, malformed items left out
        assert s1[0] == (eligible + 63) // 64, (name, s1)
        assert s1[1] == failing, (name, s1)


# ------------------------------------------------------------ 4. quorum gate

def _quorum_items(env):
    """(context, signers, expected code) with valid signatures: uniform
    contexts at exactly floor(2n/3) bits and one more; one-big-key contexts
    without the big key (every other key signs) and with it alone"""
    spec, want = [], []
    for c, n in enumerate(SIZES):
        msg = pr.construct_commit_payload(c, pr.synth_msg(1200 + c), c + 1)
        if env.weights[c] is None:
            k = 2 * n // 3
            if k:
                spec.append((c, list(range(k)), msg))
                want.append(NOQUORUM)
            spec.append((c, list(range(k + 1)), msg))
            want.append(1)
        else:
            big = env.big[c]
            spec.append((c, [i for i in range(n) if i != big], msg))
            want.append(NOQUORUM)
            spec.append((c, [big], msg))
            want.append(1)
    return spec, want


def test_quorum_gate(env):
    core = env.core
    spec, want = _quorum_items(env)
    idx = [c for c, _, _ in spec]
    msgs = [m for _, _, m in spec]
    blobs = env.sign(spec)
    # the empty mask of the one-key committee: nothing signed
    idx.append(0)
    msgs.append(msgs[0])
    blobs.append(bytes(96) + b"\x00")
    want.append(NOQUORUM)
    res = env.ctxset.seal_verify(idx, blobs, msgs, quorum=True)
    assert res == want
    env.check_refs(idx, blobs, msgs, res, quorum=True)
    # without the gate the quorumless items with valid signatures verify
    assert env.ctxset.seal_verify(idx, blobs, msgs)[:-1] == [1] * (len(want) - 1)

    # garbage signature without quorum: NOQUORUM; malformed stays BADINPUT
    at = want.index(NOQUORUM)
    blobs2, idx2, want2 = list(blobs), list(idx), list(want)
    blobs2[at] = b"\xff" * 96 + blobs[at][96:]
    live = want.index(1)
    blobs2[live] = blobs2[live][:-1]
    want2[live] = BADINPUT
    idx2[-2] = NCTX
    want2[-2] = BADINPUT
    for mode in (0, 1):
        with core.aggrlc_switches(mode=mode, threshold=1):
            res = env.ctxset.seal_verify(idx2, blobs2, msgs, quorum=True)
            stats = core.aggrlc_last_stats()
        assert res == want2, mode
        if mode == 1:
            # quorumless and malformed items never reach a chunk
            assert stats[:2] == [(want2.count(1) + 63) // 64, 0]
    env.check_refs(idx2, blobs2, msgs, res, quorum=True)

    # nothing live: no launch error
    dead = [j for j, r in enumerate(want2) if r != 1]
    res = env.ctxset.seal_verify([idx2[j] for j in dead], [blobs2[j] for j in dead],
                                 [msgs[j] for j in dead], quorum=True)
    assert res == [want2[j] for j in dead]
    res = env.ctxset.seal_verify([NCTX], [blobs[0]], [msgs[0]])
    assert res == [BADINPUT]

    # a committee without a policy fails the call, with the gate only
    bare = core.Committee(env.pks[2], SIZES[2])
    cs = core.ContextSet(env.committees[:2] + [bare])
    with pytest.raises(core.BadInputError):
        cs.seal_verify(idx[:1], blobs[:1], msgs[:1], quorum=True)
    assert idx[0] == 0 and want[0] == 1
    assert cs.seal_verify(idx[:1], blobs[:1], msgs[:1]) == [1]


# ------------------------------------------------------------ 5. message lengths

def test_message_lengths(env):
    core, capi = env.core, env.capi
    c, n = 4, SIZES[4]
    lens = [1, 32, 47, 48, 49, 64]
    rng = random.Random(21)
    msgs = [bytes(rng.randrange(1, 256) for _ in range(k)) for k in lens]
    signers = list(range(0, n, 3))
    sk = pr.fr_serialize(sum(env.sk[c][i] for i in signers) % pr.R)
    mask = _mask_of(n, signers)
    sigs = [capi.sign_hash(sk, m) for m in msgs]
    idx = [c] * len(lens)
    assert env.ctxset.seal_verify(idx, [s + mask for s in sigs], msgs) == [1] * len(lens)
    # every other item's signature: over other bytes
    rot = sigs[1:] + sigs[:1]
    assert env.ctxset.seal_verify(idx, [s + mask for s in rot], msgs) == [0] * len(lens)
    # only the first 48 bytes count: a signature over them serves the long
    # message, and a change past them changes nothing; a change inside does
    long_msg = msgs[-1]
    variants = [long_msg[:48], long_msg[:48] + bytes(16),
                long_msg[:10] + bytes([long_msg[10] ^ 1]) + long_msg[11:]]
    res = env.ctxset.seal_verify([c] * 3, [sigs[-1] + mask] * 3, variants)
    assert res == [1, 1, 0]
    # the hash point is hbls_hash_to_g2 of the bytes = the padded 48-byte slot's
    slots = b"".join(m[:48].ljust(48, b"\x00") for m in msgs)
    cat = core.batch_hash_to_g2(slots, 48, len(msgs))
    for j, m in enumerate(msgs):
        assert core.hash_to_g2(m) == cat[96 * j:96 * (j + 1)], lens[j]
        assert capi.hash_to_g2(m) == cat[96 * j:96 * (j + 1)], lens[j]


# ------------------------------------------------------------ 6. degenerate shapes

def test_degenerate_shapes(env):
    core = env.core
    # batch = 1, each context in turn
    for j in range(NCTX):
        assert env.ctxset.seal_verify([env.ctx_idx[j]], [env.blobs[j]], [env.msgs[j]]) == [1]
    # n_ctx = 1 against the single-committee entry on the same window
    c = 4
    pick = [j for j in range(TOTAL) if env.ctx_idx[j] == c and len(env.msgs[j]) == 48]
    assert len(pick) >= 3
    blobs = [env.blobs[j] for j in pick]
    blobs[1] = env.D + blobs[1][96:]
    msgs = [env.msgs[j] for j in pick]
    one = core.ContextSet([env.committees[c]])
    assert len(one) == 1
    res = one.seal_verify([0] * len(pick), blobs, msgs)
    want = env.committees[c].batch_seal_verify(b"".join(blobs), len(blobs[0]), b"".join(msgs),
                                               48, len(pick))
    assert res == want
    assert res == [0 if k == 1 else 1 for k in range(len(pick))]
    # many contexts of one item each (the epoch-chain shape)
    many = core.ContextSet([env.committees[k % NCTX] for k in range(45)])
    assert len(many) == 45
    pos, blobs, msgs = [], [], []
    for k in range(45):
        j = next(j for j in range(k, TOTAL) if env.ctx_idx[j] == k % NCTX)
        pos.append(k)
        blobs.append(env.blobs[j])
        msgs.append(env.msgs[j])
    assert many.seal_verify(pos, blobs, msgs) == [1] * 45
    shifted = [(k + 1) % 45 for k in pos]          # every item under a wrong context
    res = many.seal_verify(shifted, blobs, msgs)
    assert all(r in (0, BADINPUT) for r in res)
    with pytest.raises(core.BadInputError):
        core.ContextSet([])


# ------------------------------------------------------------ engine, end to end

def test_engine_end_to_end(env):
    from harmony_amd import engine as eng
    # four contexts: shard 0 and shard 1, epoch 1 (pre-staking, 40-byte
    # payloads) and epoch 2 (staking, 48 bytes, staked policy)
    ctx_of = {(0, 1): 1, (1, 1): 2, (0, 2): 3, (1, 2): 4}
    loads = []

    def loader(shard_id, epoch):
        c = ctx_of[(shard_id, epoch)]
        loads.append((shard_id, epoch))
        staking = epoch >= 2
        return env.pks[c], SIZES[c], (env.weights[c] if staking else None), staking

    calls = []
    device = eng.DeviceVerifier()

    def verifier(contexts, ctx_idx, blobs, msgs, quorum):
        calls.append(len(ctx_idx))
        return device(contexts, ctx_idx, blobs, msgs, quorum)

    e = eng.Engine(loader, verifier=verifier)
    keys = [(0, 1), (1, 1), (0, 2), (1, 2)]
    spec, meta = [], []
    for j in range(8):
        shard, epoch = keys[j % 4]
        c = ctx_of[(shard, epoch)]
        h = pr.synth_msg(1500 + j)
        msg = pr.construct_commit_payload(10 + j, h, 20 + j, staking=epoch >= 2)
        assert len(msg) == (48 if epoch >= 2 else 40)
        spec.append((c, list(range(SIZES[c])), msg))
        meta.append((shard, epoch, h, 10 + j, 20 + j))
    blobs = env.sign(spec)
    items = [eng.SealItem(s, ep, h, num, view, blobs[j][:96], blobs[j][96:])
             for j, (s, ep, h, num, view) in enumerate(meta)]
    res = e.verify_headers(items)
    assert res.codes == [1] * 8 and res.first_failure is None
    assert calls == [8] and sorted(loads) == sorted(keys)
    # all cached now: no device call
    assert e.verify_headers(items).codes == [1] * 8
    assert calls == [8]
    # a forged seal and a quorumless one in a cross-link list
    forged = items[2]._replace(sig=env.D)
    c5 = ctx_of[(1, 1)]
    few = env.sign([(c5, [0], spec[1][2])])[0]
    quorumless = items[1]._replace(sig=few[:96], bitmap=few[96:])
    res = e.verify_crosslinks([items[0], forged, quorumless, items[3]])
    assert res.codes == [1, 0, NOQUORUM, 1] and res.first_failure == 1
    assert calls == [8, 2]
    # rejected seals are not cached
    res = e.verify_crosslinks([forged])
    assert res.codes == [0] and calls == [8, 2, 1]
