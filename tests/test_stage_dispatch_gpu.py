"""Every verify entry point on both sides of the cooperative / thread-per-item
threshold: a committee of 16, batches of 8, the threshold
forced to 0 (thread-per-item kernels) and to 10**9 (cooperative kernels), and,
where one call dispatches on two sizes, to a value between them.  Each batch
mixes accepted items, wrong-signer or wrong-message rejects and an undecodable
signature; the expected codes come from the CPU oracle alone.

batch_agg_verify and batch_verify_votes_multi have the same pair of cases in
test_verify_scalar_gpu.py and test_multikey_gpu.py."""
import contextlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from oracle import pyref as pr  # noqa: E402


def _gpu_available():
    try:
        from harmony_amd import core
        return core.device_count() > 0
    except Exception:
        return False


if not os.environ.get("HBLS_FORCE_GPU_TESTS"):
    pytestmark = [pytest.mark.gpu,
                  pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]

N = 16
BATCH = 8
BAD = -3                # HBLS_ERR_BADINPUT
NOQUORUM = -4
UNDECODABLE = b"\xff" * 96
BOTH_SIDES = pytest.mark.parametrize("threshold", [0, 10 ** 9], ids=["scalar", "coop"])


def _bitmap(n, keys):
    bm = bytearray((n + 7) // 8)
    for k in keys:
        bm[k >> 3] |= 1 << (k & 7)
    return bytes(bm)


class _Env:
    """16 keys, 8 payloads and an oracle for every expected code; built once,
    never modified"""

    def __init__(self, core, capi):
        self.core, self.capi = core, capi
        self.sks = [pr.fr_serialize(pr.synth_sk(i)) for i in range(N)]
        self.pk = [capi.pk_from_sk(sk) for sk in self.sks]
        self.pks = b"".join(self.pk)
        self.committee = core.Committee(self.pks, N)
        self.oracle = capi.Committee(self.pks, N)
        self.msgs = [pr.construct_commit_payload(j, pr.synth_msg(900 + j), j + 1)
                     for j in range(BATCH)]
        self.mlen = len(self.msgs[0])
        self._sigs = {}

    def sign(self, keys, msg):
        """the sum of the keys' signatures on msg"""
        keys = tuple(keys)
        if (keys, msg) not in self._sigs:
            self._sigs[(keys, msg)] = self.capi.aggregate_sigs(
                [self.capi.sign_hash(self.sks[i], msg) for i in keys])
        return self._sigs[(keys, msg)]

    def vote_code(self, keys, sig, msg):
        """oracle.verify_hash(sum of keys, sig, msg) as a result code"""
        pk = self.capi.mask_aggregate(self.pk, _bitmap(N, keys))
        try:
            return 1 if self.capi.verify_hash(pk, sig, msg) else 0
        except ValueError:
            return BAD

    @staticmethod
    def seal_code(oracle, bitmap, sig, msg):
        try:
            return 1 if oracle.agg_verify(bitmap, sig, msg) else 0
        except ValueError:
            return BAD

    @contextlib.contextmanager
    def threshold(self, value):
        self.core.set_coop_threshold(value)
        try:
            yield
        finally:
            self.core.set_coop_threshold(-1)

    @contextlib.contextmanager
    def exact_pairing(self):
        """pin the aggregate entries to the exact pairing stage, so that the
        stage launcher and no combined kernel judges the items"""
        with self.core.aggrlc_switches(mode=0):
            yield
            assert self.core.aggrlc_last_stats() == [0, 0, 0]


@pytest.fixture(scope="module")
def env(oracle_lib):
    from harmony_amd import core
    core.init(-1 if core.device_count() == 0 else 0)
    return _Env(core, oracle_lib)


# ---------------------------------------------------------------- vote entries

@pytest.fixture(scope="module")
def votes(env):
    """8 single-key votes, one message each: (keys, sigs, want)"""
    keys = [0, 3, 5, 15, 2, 7, 9, 11]
    sigs = [env.sign([k], env.msgs[j]) for j, k in enumerate(keys)]
    sigs[4] = env.sign([6], env.msgs[4])            # wrong signer
    sigs[5] = env.sign([7], env.msgs[0])            # wrong message
    sigs[6] = UNDECODABLE
    want = [env.vote_code([k], sigs[j], env.msgs[j]) for j, k in enumerate(keys)]
    assert want == [1, 1, 1, 1, 0, 0, BAD, 1]
    return keys, sigs, want


@BOTH_SIDES
def test_batch_verify_votes(env, votes, threshold):
    keys, sigs, want = votes
    with env.threshold(threshold):
        got = env.committee.batch_verify_votes(keys, b"".join(sigs), b"".join(env.msgs),
                                               env.mlen)
    assert got == want


@pytest.fixture(scope="module")
def grouped(env):
    """8 votes over 2 messages: (keys, groups, sigs, want)"""
    keys = [0, 1, 2, 3, 4, 5, 6, 7]
    grps = [0, 1, 0, 1, 0, 1, 0, 1]
    sigs = [env.sign([k], env.msgs[g]) for k, g in zip(keys, grps)]
    sigs[2] = env.sign([9], env.msgs[0])            # wrong signer
    sigs[5] = env.sign([5], env.msgs[0])            # the other group's message
    sigs[6] = UNDECODABLE
    want = [env.vote_code([k], sigs[j], env.msgs[g])
            for j, (k, g) in enumerate(zip(keys, grps))]
    assert want == [1, 1, 0, 1, 1, 0, BAD, 1]
    return keys, grps, sigs, want


@pytest.mark.parametrize("threshold", [0, 10 ** 9, 4], ids=["scalar", "coop", "between"])
def test_batch_verify_votes_grouped(env, grouped, threshold):
    """between: the hash of the 2 messages is cooperative, the decompress of
    the 8 signatures thread-per-item"""
    keys, grps, sigs, want = grouped
    with env.threshold(threshold):
        got = env.committee.batch_verify_votes_grouped(
            keys, grps, b"".join(sigs), env.msgs[0] + env.msgs[1], env.mlen)
    assert got == want


# ----------------------------------------------------------- aggregate entries

@pytest.fixture(scope="module")
def seals(env):
    """8 (bitmap, aggregate signature) items: (bitmaps, sigs, want)"""
    sets = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], [1, 3, 5, 7, 9, 11, 13, 15], [15],
            list(range(N)), [2, 4, 6, 8, 10, 12]]
    bms = [_bitmap(N, s) for s in sets]
    sigs = [env.sign(s, env.msgs[j]) for j, s in enumerate(sets)]
    s = [2, 4, 6, 8, 10, 12]
    bms.append(_bitmap(N, s[:-1] + [13]))           # wrong signer set
    sigs.append(env.sign(s, env.msgs[5]))
    bms.append(_bitmap(N, s))                       # wrong message
    sigs.append(env.sign(s, env.msgs[0]))
    bms.append(_bitmap(N, s))
    sigs.append(UNDECODABLE)
    want = [env.seal_code(env.oracle, bms[j], sigs[j], env.msgs[j]) for j in range(BATCH)]
    assert want == [1, 1, 1, 1, 1, 0, 0, BAD]
    return bms, sigs, want


@BOTH_SIDES
def test_batch_seal_verify(env, seals, threshold):
    bms, sigs, want = seals
    blobs = b"".join(s + b for s, b in zip(sigs, bms))
    with env.threshold(threshold), env.exact_pairing():
        got = env.committee.batch_seal_verify(blobs, 96 + len(bms[0]), b"".join(env.msgs),
                                              env.mlen, BATCH)
    assert got == want


@BOTH_SIDES
def test_batch_agg_verify_partials(env, seals, threshold):
    """the committee in two slices of 8: the high slice's masked key sums
    arrive serialized (n_ext = 1) and the low slice's call must give the
    whole committee's verdicts"""
    bms, sigs, want = seals
    low = env.core.Committee(env.pks[:48 * 8], 8)
    assert all(bm[1] for bm in bms)                 # a key of the high slice signs each
    ext = b"".join(env.capi.mask_aggregate(env.pk[8:], bm[1:]) for bm in bms)
    with env.threshold(threshold):
        got = low.batch_agg_verify_partials(b"".join(bm[:1] for bm in bms), ext, 1,
                                            b"".join(sigs), b"".join(env.msgs), env.mlen,
                                            BATCH)
    assert got == want


# ------------------------------------------------------------------ vote stream

R = 3


def _stream(env, mode):
    st = env.core.Stream(env.committee, R)
    st.set_rounds(list(range(R)), b"".join(env.msgs[:R]), env.mlen)
    if mode:
        st.set_verify_mode(mode)
    return st


def _round_state(env, accepted):
    """per round: the bitmap and aggregate the accepted votes leave, and the
    oracle's verdict on them"""
    out = []
    for r in range(R):
        sets = [keys for rr, keys in accepted if rr == r]
        bm = _bitmap(N, [k for keys in sets for k in keys])
        agg = env.capi.aggregate_sigs([env.sign(keys, env.msgs[r]) for keys in sets]) \
            if sets else bytes(96)
        out.append((bm, agg, env.oracle.agg_verify(bm, agg, env.msgs[r])))
    return out


@pytest.fixture(scope="module")
def ticks(env):
    """one tick of 8 single-key votes over rounds 0 and 1; round 2 stays empty:
    (votes, sigs, want, state)"""
    votes = [(0, 0), (1, 1), (0, 2), (1, 3), (0, 4), (1, 5), (0, 6), (1, 7)]
    sigs = [env.sign([k], env.msgs[r]) for r, k in votes]
    sigs[2] = env.sign([12], env.msgs[0])           # wrong signer
    sigs[5] = env.sign([5], env.msgs[0])            # the other round's message
    sigs[6] = UNDECODABLE
    want = [env.vote_code([k], sigs[j], env.msgs[r]) for j, (r, k) in enumerate(votes)]
    assert want == [1, 1, 0, 1, 1, 0, BAD, 1]
    state = _round_state(env, [(r, [k]) for (r, k), w in zip(votes, want) if w == 1])
    assert [ok for _bm, _agg, ok in state] == [True] * R
    return votes, sigs, want, state


@pytest.mark.parametrize("mode", [0, 1], ids=["per_vote", "batched"])
@BOTH_SIDES
def test_stream_process_and_check(env, ticks, threshold, mode):
    """set_rounds always hashes cooperatively, so at threshold 0 this is also
    the always-cooperative hash feeding thread-per-item kernels"""
    votes, sigs, want, state = ticks
    with env.threshold(threshold):
        st = _stream(env, mode)
        got = st.process([k for _r, k in votes], [r for r, _k in votes], b"".join(sigs))
        checks = st.check(list(range(R)))
        exported = [st.get(r) for r in range(R)]
    assert got == want
    assert checks == [ok for _bm, _agg, ok in state]
    assert exported == [(bm, agg) for bm, agg, _ok in state]


@BOTH_SIDES
def test_stream_process_multi(env, threshold):
    lists = [[0, 1], [2], [3, 4, 5], [6, 7], [8], [9, 10], [11], [12, 13, 14]]
    rounds = [0, 1, 0, 1, 0, 1, 0, 1]
    sigs = [env.sign(keys, env.msgs[r]) for keys, r in zip(lists, rounds)]
    sigs[1] = env.sign([15], env.msgs[1])           # wrong signer
    sigs[3] = env.sign([6], env.msgs[1])            # one key signed for two
    sigs[4] = env.sign([8], env.msgs[1])            # the other round's message
    sigs[6] = UNDECODABLE
    want = [env.vote_code(keys, sigs[j], env.msgs[r])
            for j, (keys, r) in enumerate(zip(lists, rounds))]
    assert want == [1, 0, 1, 0, 0, 1, BAD, 1]
    state = _round_state(env, [(r, keys) for keys, r, w in zip(lists, rounds, want) if w == 1])
    with env.threshold(threshold):
        st = _stream(env, 0)
        got = st.process_multi(lists, rounds, b"".join(sigs))
        checks = st.check(list(range(R)))
        exported = [st.get(r) for r in range(R)]
    assert got == want
    assert checks == [ok for _bm, _agg, ok in state]
    assert exported == [(bm, agg) for bm, agg, _ok in state]


def test_stream_async_check_below_threshold(env, ticks):
    """check_submit always takes the cooperative kernel: at threshold 0 its
    verdicts are those of the thread-per-item check and of the oracle"""
    votes, sigs, _want, state = ticks
    with env.threshold(0):
        st = _stream(env, 0)
        st.process([k for _r, k in votes], [r for r, _k in votes], b"".join(sigs))
        st.check_submit(list(range(R)))
        polled = st.check_poll()
        checks = st.check(list(range(R)))
    assert checks == [ok for _bm, _agg, ok in state]
    assert polled == dict(enumerate(checks))


# ---------------------------------------------------------------- context sets

class _Contexts:
    """two committees over the same keys (16 and 9 of them), uniform quorum
    policy set, behind one context set"""

    SIZES = (16, 9)

    def __init__(self, env):
        self.env = env
        self.committees, self.oracles = [], []
        for n in self.SIZES:
            c = env.core.Committee(env.pks[:48 * n], n)
            c.set_quorum()
            self.committees.append(c)
            self.oracles.append(env.capi.Committee(env.pks[:48 * n], n))
        self.ctxset = env.core.ContextSet(self.committees)

    def blob(self, ctx, mask_keys, sig):
        return sig + _bitmap(self.SIZES[ctx], mask_keys)

    def code(self, ctx, blob, msg, quorum):
        """the oracle's code for one item; the uniform quorum rule is
        popcount > floor(2n/3)"""
        if ctx >= len(self.SIZES):
            return BAD
        n = self.SIZES[ctx]
        if quorum and sum(bin(b).count("1") for b in blob[96:]) <= 2 * n // 3:
            return NOQUORUM
        return self.env.seal_code(self.oracles[ctx], blob[96:], blob[:96], msg)


@pytest.fixture(scope="module")
def contexts(env):
    return _Contexts(env)


@BOTH_SIDES
def test_ctxset_seal_verify(env, contexts, threshold):
    big, small = list(range(12)), list(range(7))
    idx = [0, 1, 0, 1, 0, 1, 0, 1]
    blobs = [contexts.blob(c, big if c == 0 else small,
                           env.sign(big if c == 0 else small, env.msgs[j]))
             for j, c in enumerate(idx)]
    blobs[2] = contexts.blob(0, big[:-1] + [13], env.sign(big, env.msgs[2]))   # wrong signers
    blobs[3] = contexts.blob(1, small, env.sign(small, env.msgs[0]))           # wrong message
    blobs[4] = contexts.blob(0, big, env.sign(small, env.msgs[4]))             # other committee's
    blobs[5] = contexts.blob(1, small, UNDECODABLE)
    want = [contexts.code(c, blobs[j], env.msgs[j], False) for j, c in enumerate(idx)]
    assert want == [1, 1, 0, 0, 0, BAD, 1, 1]
    with env.threshold(threshold), env.exact_pairing():
        got = contexts.ctxset.seal_verify(idx, blobs, env.msgs)
    assert got == want


def test_ctxset_live_items_below_threshold(env, contexts):
    """6 items at threshold 4: two die ahead of the pairing (a context index
    out of range, a mask without quorum), so the 4 live ones go through the
    cooperative kernels although the batch is above the threshold; every
    code lands at its item's own index"""
    big, small = list(range(12)), list(range(7))
    idx = [0, len(contexts.SIZES), 1, 0, 0, 1]
    blobs = [contexts.blob(0, big, env.sign(big, env.msgs[0])),
             contexts.blob(0, big, env.sign(big, env.msgs[1])),     # context out of range
             contexts.blob(1, small, env.sign(small, env.msgs[2])),
             contexts.blob(0, big[:5], env.sign(big[:5], env.msgs[3])),   # valid, no quorum
             contexts.blob(0, big, env.sign(big, env.msgs[0])),     # wrong message
             contexts.blob(1, small, UNDECODABLE)]
    msgs = env.msgs[:6]
    want = [contexts.code(c, blobs[j], msgs[j], True) for j, c in enumerate(idx)]
    assert want == [1, BAD, 1, NOQUORUM, 0, BAD]
    with env.threshold(4), env.exact_pairing():
        got = contexts.ctxset.seal_verify(idx, blobs, msgs, quorum=True)
    assert got == want
