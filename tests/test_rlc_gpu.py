"""Random-combination batch verification of same-message votes (stream
verify mode 1 and Committee.batch_verify_votes_grouped): per-vote results,
bitmaps and aggregates must equal the per-item path's, with the pairing
count shown by core.rlc_last_stats()."""
import ctypes
import os
import random
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

R = 4            # round slots; slot 3 stays open but empty


class _Env:
    """committee of 3*C+2 keys, 4 round payloads and every (round, key)
    signature the tests use — built once, never modified"""

    def __init__(self):
        from harmony_amd import core
        self.core = core
        self.C = core.rlc_chunk_size()
        self.n = 3 * self.C + 2
        self.sks = [pr.fr_serialize(pr.synth_sk(i)) for i in range(self.n)]
        self.pks = core.batch_pk_from_sk(b"".join(self.sks), self.n)
        self.committee = core.Committee(self.pks, self.n)
        self.payloads = [pr.construct_commit_payload(r, pr.synth_msg(700 + r), r + 1)
                         for r in range(R)]
        self.mlen = len(self.payloads[0])
        # round sizes 3*C+2, C and 1
        self.votes = [(0, i) for i in range(self.n)] + \
                     [(1, i) for i in range(self.C)] + [(2, 7)]
        sigs = core.batch_sign(b"".join(self.sks[i] for _r, i in self.votes),
                               b"".join(self.payloads[r] for r, _i in self.votes),
                               self.mlen, len(self.votes))
        self.sig = {v: sigs[96 * j:96 * (j + 1)] for j, v in enumerate(self.votes)}

    def stream(self, mode):
        st = self.core.Stream(self.committee, R)
        st.set_rounds(list(range(R)), b"".join(self.payloads), self.mlen)
        if mode:
            st.set_verify_mode(mode)
        return st

    def tick(self, st, votes, sigs=None, active=None):
        """one hbls_stream_process call; `active` overrides the slot list
        (Stream.process derives it from round_idx, which refuses a tick that
        carries an out-of-range round index)"""
        sigs = sigs if sigs is not None else [self.sig[v] for v in votes]
        if active is None:
            return st.process([v[1] for v in votes], [v[0] for v in votes],
                              b"".join(sigs))
        b = len(votes)
        ki = (ctypes.c_uint32 * b)(*[v[1] for v in votes])
        ri = (ctypes.c_uint32 * b)(*[v[0] for v in votes])
        act = (ctypes.c_uint32 * len(active))(*active)
        res = (ctypes.c_int32 * b)()
        rc = self.core._lib.hbls_stream_process(st._h, ki, ri, b"".join(sigs), act,
                                                len(active), b, res)
        assert rc == self.core.HBLS_OK
        return list(res)

    def both(self, ticks, active=None):
        """feed the same ticks (lists of (votes, sigs)) to a per-item and a
        batched stream; returns (results0, results1, stats per batched tick,
        stream0, stream1)"""
        st0, st1 = self.stream(0), self.stream(1)
        res0, res1, stats = [], [], []
        for votes, sigs in ticks:
            res0.append(self.tick(st0, votes, sigs, active))
            res1.append(self.tick(st1, votes, sigs, active))
            stats.append(self.core.rlc_last_stats())
        return res0, res1, stats, st0, st1

    def bitmap_of(self, keys):
        bm = bytearray((self.n + 7) // 8)
        for i in keys:
            bm[i >> 3] |= 1 << (i & 7)
        return bytes(bm)


@pytest.fixture(scope="module")
def env(oracle_lib):
    return _Env()


def _same_state(env, st0, st1):
    for r in range(R):
        assert st0.get(r) == st1.get(r), r


def test_all_valid_differential(env, oracle_lib):
    order = list(env.votes)
    random.Random(11).shuffle(order)
    res0, res1, stats, st0, st1 = env.both([(order, None)])
    assert res0[0] == res1[0] == [1] * len(order)
    assert stats[0] == [3, 0, 0, 0]
    _same_state(env, st0, st1)
    assert st1.check(list(range(R))) == [True] * R
    oc = oracle_lib.Committee(env.pks, env.n)
    for r in range(3):
        bm, agg = st1.get(r)
        assert bm == env.bitmap_of(i for rr, i in env.votes if rr == r)
        assert oc.agg_verify(bm, agg, env.payloads[r]) is True


def test_one_bad_vote(env, oracle_lib):
    order = list(env.votes)
    random.Random(12).shuffle(order)
    bad = (0, 2 * env.C + 1)
    sigs = [env.sig[v] for v in order]
    # a valid subgroup point, but the same key's signature on another payload
    sigs[order.index(bad)] = oracle_lib.sign_hash(env.sks[bad[1]], env.payloads[3])
    res0, res1, stats, st0, st1 = env.both([(order, sigs)])
    want = [0 if v == bad else 1 for v in order]
    assert res0[0] == want
    assert res1[0] == want
    s = stats[0]
    assert s[0] == 3 and s[1] == 1
    assert s[2] == (env.n + env.C - 1) // env.C      # every chunk of that group
    assert 0 < s[3] <= env.C
    _same_state(env, st0, st1)
    bm, agg = st1.get(0)
    assert bm == env.bitmap_of(i for i in range(env.n) if i != bad[1])
    assert st1.check([0]) == [True]
    assert oracle_lib.Committee(env.pks, env.n).agg_verify(bm, agg, env.payloads[0])


@pytest.mark.parametrize("kind,pa,pb", [
    ("swap", 3, 10),
    ("delta", 3, 10),           # both forged votes in one chunk
    ("delta", 3, None),         # in different chunks (pb = C + 5)
])
def test_cancelling_forgeries(env, oracle_lib, kind, pa, pb):
    """forgeries whose errors cancel in an UNWEIGHTED sum of the signatures"""
    pb = env.C + 5 if pb is None else pb
    votes = [(0, i) for i in range(env.n)]      # one group; chunk = position // C
    sigs = [env.sig[v] for v in votes]
    if kind == "swap":
        sigs[pa], sigs[pb] = sigs[pb], sigs[pa]
    else:
        d = oracle_lib.hash_to_g2(b"delta")
        sigs[pa] = oracle_lib.g2_add(sigs[pa], d)
        sigs[pb] = oracle_lib.g2_add(sigs[pb], d, sub=True)
    assert (pa // env.C == pb // env.C) == (pb == 10)
    # the forgery is real: the plain sum verifies against the all-ones mask
    oc = oracle_lib.Committee(env.pks, env.n)
    assert oc.agg_verify(env.bitmap_of(range(env.n)), oracle_lib.aggregate_sigs(sigs),
                         env.payloads[0]) is True
    res0, res1, stats, st0, st1 = env.both([(votes, sigs)])
    want = [0 if j in (pa, pb) else 1 for j in range(env.n)]
    assert res0[0] == want
    assert res1[0] == want
    assert stats[0][0] == 1 and stats[0][1] == 1
    _same_state(env, st0, st1)


def test_malformed_votes(env):
    core = env.core
    # x = (c, 1): first c with no y on E'(Fp2), first c with y but [r]Q != O
    off_curve = off_subgroup = None
    c = 1
    while off_curve is None or off_subgroup is None:
        x = (c, 1)
        y = pr.f2_sqrt(pr.f2_add(pr.f2_mul(pr.f2_sqr(x), x), pr.B2))
        if y is None:
            off_curve = off_curve or pr.fp_to_le48(c) + pr.fp_to_le48(1)
        elif pr.g2_mul((x, y), pr.R) is not None:
            off_subgroup = off_subgroup or pr.g2_serialize((x, y))
        c += 1
    with pytest.raises(ValueError):
        pr.g2_deserialize(off_curve, check_subgroup=False)
    assert not core.g2_check(off_curve) and not core.g2_check(off_subgroup)

    good = [(1, i) for i in range(env.C)] + [(2, 7)] + [(0, i) for i in range(5)]
    malformed = [
        ((0, env.n), env.sig[(0, 0)]),          # key_idx == n
        ((R, 1), env.sig[(0, 1)]),              # round index == max_rounds
        ((0, 10), off_curve),
        ((0, 11), off_subgroup),
        ((0, 12), bytes(96)),                   # identity signature
    ]
    votes = list(good)
    sigs = [env.sig[v] for v in good]
    for pos, (v, s) in zip((2, 9, 17, 40, 66), malformed):
        votes.insert(pos, v)
        sigs.insert(pos, s)
    res0, res1, stats, st0, st1 = env.both([(votes, sigs)], active=[0, 1, 2])
    bad_code = {v: core.HBLS_ERR_BADINPUT for v, _s in malformed[:4]}
    bad_code[malformed[4][0]] = 0
    want = [bad_code.get(v, 1) for v in votes]
    assert res0[0] == want
    assert res1[0] == want
    # malformed votes alone cause no re-check
    assert stats[0] == [3, 0, 0, 0]
    _same_state(env, st0, st1)
    assert st1.check([0, 1, 2]) == [True] * 3


def test_duplicates(env):
    t1 = [(1, i) for i in range(10)] + [(1, 4)]            # in-tick duplicate
    t2 = [(1, i) for i in range(10, 20)] + [(1, 2)]        # cross-tick duplicate
    res0, res1, stats, st0, st1 = env.both([(t1, None), (t2, None)])
    for res in (res0, res1):
        assert sorted([res[0][4], res[0][10]]) == [1, 2]   # one of the pair wins
        assert all(r == 1 for j, r in enumerate(res[0]) if j not in (4, 10))
        assert res[1] == [1] * 10 + [2]
    assert stats == [[1, 0, 0, 0], [1, 0, 0, 0]]
    _same_state(env, st0, st1)
    assert st1.get(1)[0] == env.bitmap_of(range(20))
    assert st1.check([1]) == [True]


def test_grouped_committee_entry(env, oracle_lib):
    core = env.core
    msgs = env.payloads[0] + env.payloads[1]
    votes = [(0, i) for i in range(env.C + 6)] + [(1, i) for i in range(10)]
    random.Random(13).shuffle(votes)
    bad = votes.index((0, 20))
    oor = 33 if bad != 33 else 34           # this vote gets group_idx == n_groups
    keys = [i for _g, i in votes]
    grps = [g for g, _i in votes]
    grps[oor] = 2

    def run():
        sigs = core.batch_sign(b"".join(env.sks[i] for i in keys),
                               b"".join(env.payloads[g] for g, _i in votes),
                               env.mlen, len(votes))
        sigs = sigs[:96 * bad] + core.sign_hash(env.sks[20], env.payloads[3]) + \
            sigs[96 * (bad + 1):]
        want = env.committee.batch_verify_votes(
            keys, sigs, b"".join(env.payloads[g] for g, _i in votes), env.mlen)
        assert want == [0 if j == bad else 1 for j in range(len(votes))]
        want[oor] = core.HBLS_ERR_BADINPUT
        got = env.committee.batch_verify_votes_grouped(keys, grps, sigs, msgs, env.mlen)
        assert got == want
        s = core.rlc_last_stats()
        assert s[0] == 2 and s[1] == 1 and s[2] == 2 and 0 < s[3] <= env.C

    run()
    core.set_g2_cofactor_mode(False)
    try:
        run()
    finally:
        core.set_g2_cofactor_mode(True)


def test_mode_validation(env):
    st = env.stream(0)
    with pytest.raises(ValueError):
        st.set_verify_mode(2)
    votes = [(1, i) for i in range(4)]
    assert env.tick(env.stream(1), votes) == [1] * 4
    assert env.core.rlc_last_stats() == [1, 0, 0, 0]
    # a stream left at its default runs the per-item path: counters stay zero
    assert env.tick(st, votes) == [1] * 4
    assert env.core.rlc_last_stats() == [0, 0, 0, 0]
