"""Quorum by mask on the device: k_mask_power against plain
Python integer sums, the strict > threshold rule, the quorum gate in front of
the aggregate-verify pipeline (exact and combined mode) and the stream's
per-round tally.  Expected quorum comes from Python ints here; expected
pairing verdicts from the CPU oracle's Committee.batch_agg_verify."""
import ctypes
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

E18 = 10 ** 18
TWO_THIRDS = 666666666666666667
HP, EP = 49 * E18 // 100, 51 * E18 // 100

# 8..4096 are the issue's sizes; the pairs around 64, 128, ..., 2048 are the
# steps of the lanes-per-item choice (1, 2, 4, ..., 64 lanes for rows of up to
# 8, 16, ..., 512 bytes), 4096 | 4097 is the LDS | global power-table switch
SIZES = [8, 64, 65, 70, 128, 129, 256, 257, 512, 513, 520, 1024, 1025,
         2048, 2049, 4096, 4097]
BATCHES = [1, 63, 65]
MAXN = max(SIZES)


@pytest.fixture(scope="module")
def core():
    from harmony_amd import core
    return core


@pytest.fixture(scope="module")
def keys(core):
    """secret keys (ints) and serialized public keys of the largest committee;
    smaller committees are prefixes"""
    sk = [pr.synth_sk(7000 + i) for i in range(MAXN)]
    pks = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in sk), MAXN)
    return sk, pks


def _staked_weights(n, seed):
    rng = random.Random(seed)
    stakes = [None if rng.random() < 0.2 else rng.randrange(1, 10 ** 6) * 10 ** 15
              for _ in range(n)]
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


def _rows(n, count, seed):
    """all-zero, all-one (padding bits set too) and seeded random rows of
    mixed density; random rows carry random padding bits"""
    rng = random.Random(seed)
    bm = (n + 7) // 8
    rows = []
    for j in range(count):
        a, b = rng.getrandbits(8 * bm), rng.getrandbits(8 * bm)
        x = (a, a & b, a | b)[j % 3]
        rows.append(x.to_bytes(bm, "little"))
    if count > 2:
        rows[1] = bytes(bm)
        rows[2] = b"\xff" * bm
    return rows


def _expect(row, n, w):
    x = int.from_bytes(row, "little") & ((1 << n) - 1)
    bits = [i for i in range(n) if (x >> i) & 1]
    return (len(bits) if w is None else sum(w[i] for i in bits)), len(bits)


def _has_quorum(core, committee, masks):
    """the gate's verdict per mask, read off the gated entry: an identity
    signature never verifies, so an item is NOQUORUM or 0"""
    k = len(masks)
    msgs = b"".join(pr.construct_commit_payload(j, pr.synth_msg(j), j + 1) for j in range(k))
    res = committee.batch_agg_verify_quorum(b"".join(masks), bytes(96 * k),
                                            msgs, len(msgs) // k, k)
    assert all(r in (0, core.NOQUORUM) for r in res), res
    return [r != core.NOQUORUM for r in res]


def _mask_of(n, signers):
    bm = bytearray((n + 7) // 8)
    for i in signers:
        bm[i >> 3] |= 1 << (i & 7)
    return bytes(bm)


@pytest.mark.parametrize("n", SIZES)
def test_mask_power(core, keys, n):
    committee = core.Committee(keys[1][:48 * n], n)
    rows = _rows(n, max(BATCHES), 100 + n)
    big = n // 2
    policies = [("unset", None), ("uniform", None),
                ("staked", _staked_weights(n, n)), ("one_big", _one_big_weights(n, big))]
    for name, w in policies:
        if name == "uniform":
            committee.set_quorum()
        elif w is not None:
            committee.set_quorum(w)
        want = [_expect(r, n, w) for r in rows]
        for batch in BATCHES:
            pw, cn = committee.mask_power(b"".join(rows[:batch]), batch)
            assert cn == [c for _, c in want[:batch]], (n, name, batch)
            assert pw == [p for p, _ in want[:batch]], (n, name, batch)
        if name == "one_big" and n > 1:
            only_big = _mask_of(n, [big])
            all_but_big = _mask_of(n, [i for i in range(n) if i != big])
            assert _has_quorum(core, committee, [only_big, all_but_big]) == [True, False]


def test_padding_bits_ignored(core, keys):
    """n = 70: a 9-byte row whose last byte has two padding bits"""
    n = 70
    committee = core.Committee(keys[1][:48 * n], n)
    rows = _rows(n, 16, 5)
    clean = [r[:8] + bytes([r[8] & 0x3F]) for r in rows]
    dirty = [r[:8] + bytes([r[8] | 0xC0]) for r in clean]
    for w in (None, _staked_weights(n, 9)):
        committee.set_quorum(w)
        a = committee.mask_power(b"".join(clean), 16)
        b = committee.mask_power(b"".join(dirty), 16)
        assert a == b
        assert a[1] == [_expect(r, n, w)[1] for r in clean]
        assert a[0] == [_expect(r, n, w)[0] for r in clean]
    # 46 signers plus the two padding bits is still 46: no quorum
    committee.set_quorum()
    m46 = bytearray(_mask_of(n, range(46)))
    m46[8] |= 0xC0
    assert _has_quorum(core, committee, [bytes(m46)]) == [False]


@pytest.mark.parametrize("n,below", [(64, 42), (70, 46)])
def test_uniform_is_strict(core, keys, n, below):
    assert below == 2 * n // 3 and below + 1 == n * 2 // 3 + 1
    committee = core.Committee(keys[1][:48 * n], n)
    committee.set_quorum()
    rng = random.Random(n)
    masks = [_mask_of(n, rng.sample(range(n), k)) for k in (below, below + 1, below - 1, n)]
    assert _has_quorum(core, committee, masks) == [False, True, False, True]


def test_staked_is_strict(core, keys):
    n = 8
    committee = core.Committee(keys[1][:48 * n], n)
    w = [TWO_THIRDS - 5, 5, 1, 0, E18 - TWO_THIRDS - 1 - 10, 4, 3, 3]
    assert sum(w) == E18
    committee.set_quorum(w)
    at, above = _mask_of(n, [0, 1, 3]), _mask_of(n, [0, 1, 2])
    pw, _ = committee.mask_power(at + above, 2)
    assert pw == [TWO_THIRDS, TWO_THIRDS + 1]
    assert _has_quorum(core, committee, [at, above]) == [False, True]
    # the threshold is the caller's: one unit lower and the first mask passes
    committee.set_quorum(w, TWO_THIRDS - 1)
    assert _has_quorum(core, committee, [at, above]) == [True, True]


def test_policy_must_be_set(core, keys):
    n = 8
    committee = core.Committee(keys[1][:48 * n], n)
    mask, sig, msg = _mask_of(n, range(n)), bytes(96), pr.construct_commit_payload(1, pr.synth_msg(1), 2)
    with pytest.raises(core.HblsError):
        committee.batch_agg_verify_quorum(mask, sig, msg, len(msg), 1)
    with pytest.raises(core.HblsError):
        committee.batch_seal_verify_quorum(sig + mask, 97, msg, len(msg), 1)
    with pytest.raises(core.HblsError):
        committee.agg_verify_quorum(mask, sig, msg)
    res = (ctypes.c_int32 * 1)()
    assert core._lib.hbls_batch_agg_verify_quorum(
        committee._h, mask, sig, msg, len(msg), 1, res) == core.HBLS_ERR_BADINPUT
    # mask_power needs no policy: uniform weights
    assert committee.mask_power(mask, 1) == ([n], [n])
    st = core.Stream(committee, 1)
    slots = (ctypes.c_uint32 * 1)(0)
    qr = (ctypes.c_int32 * 1)()
    assert core._lib.hbls_stream_power(st._h, slots, 1, None, None, qr) == core.HBLS_ERR_BADINPUT
    committee.set_quorum()
    assert committee.agg_verify_quorum(_mask_of(n, [0]), sig, msg) == core.NOQUORUM
    assert committee.agg_verify_quorum(mask, sig, msg) == 0


def test_power_sum_too_large(core, keys):
    n = 8
    committee = core.Committee(keys[1][:48 * n], n)
    with pytest.raises(core.HblsError):
        committee.set_quorum([2 ** 63, 1] + [0] * 6)
    with pytest.raises(core.HblsError):
        committee.set_quorum([2 ** 64 - 1] * 8)
    arr = (ctypes.c_uint64 * n)(2 ** 62, 2 ** 62, 1, 0, 0, 0, 0, 0)
    assert core._lib.hbls_committee_set_quorum(committee._h, arr, 5) == core.HBLS_ERR_BADINPUT
    # a rejected call leaves the committee without a policy
    with pytest.raises(core.HblsError):
        committee.agg_verify_quorum(_mask_of(n, range(n)), bytes(96), bytes(48))
    committee.set_quorum([2 ** 62, 2 ** 62] + [0] * 6, 2 ** 62)     # exactly 2^63 is allowed
    assert committee.mask_power(_mask_of(n, [0, 1]), 1) == ([2 ** 63], [2])


# ------------------------------------------------------------------ the gate

N = 64
TOTAL = 130
QLESS = (0, 64, 129)
BAD = -1


class _Env:
    """64 keys and 130 valid items as in test_aggrlc_gpu.py, every mask with
    at least 43 signers (uniform quorum), plus 1-signer variants of items 0,
    64 and 129 with a valid signature for that mask.  Built once, never
    modified."""

    def __init__(self, core, capi):
        self.core, self.capi = core, capi
        rng = random.Random(4)
        sk = [pr.synth_sk(300 + i) for i in range(N)]
        self.pks = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in sk), N)
        self.committee = core.Committee(self.pks, N)
        self.committee.set_quorum()
        self.oracle = capi.Committee(self.pks, N)
        self.bmlen = N // 8
        self.masks, self.msgs, agg_sk = [], [], []
        for j in range(TOTAL):
            signers = rng.sample(range(N), rng.randrange(43, N + 1))
            self.masks.append(_mask_of(N, signers))
            self.msgs.append(pr.construct_commit_payload(j, pr.synth_msg(500 + j), j + 1))
            agg_sk.append(sum(sk[i] for i in signers) % pr.R)
        self.mlen = len(self.msgs[0])
        self.lone = {j: rng.randrange(N) for j in QLESS}
        cat = core.batch_sign(
            b"".join(pr.fr_serialize(k) for k in agg_sk + [sk[self.lone[j]] for j in QLESS]),
            b"".join(self.msgs + [self.msgs[j] for j in QLESS]), self.mlen, TOTAL + 3)
        self.sigs = [cat[96 * j:96 * (j + 1)] for j in range(TOTAL)]
        self.q_masks, self.q_sigs = list(self.masks), list(self.sigs)
        for k, j in enumerate(QLESS):
            self.q_masks[j] = _mask_of(N, [self.lone[j]])
            self.q_sigs[j] = cat[96 * (TOTAL + k):96 * (TOTAL + k + 1)]

    def run(self, mode, fn, batch, sigs, masks):
        """(results, stats) of committee.<fn> over the first `batch` items"""
        core = self.core
        with core.aggrlc_switches(mode=mode, threshold=1):
            res = getattr(self.committee, fn)(
                b"".join(masks[:batch]), b"".join(sigs[:batch]),
                b"".join(self.msgs[:batch]), self.mlen, batch)
            stats = core.aggrlc_last_stats()
        return res, stats

    def seal(self, mode, batch, sigs, masks):
        core = self.core
        blobs = b"".join(sigs[j] + masks[j] for j in range(batch))
        with core.aggrlc_switches(mode=mode, threshold=1):
            return self.committee.batch_seal_verify_quorum(
                blobs, 96 + self.bmlen, b"".join(self.msgs[:batch]), self.mlen, batch)

    def oracle_run(self, batch, sigs, masks):
        return self.oracle.batch_agg_verify(
            b"".join(masks[:batch]), b"".join(sigs[:batch]),
            b"".join(self.msgs[:batch]), self.mlen, batch)


@pytest.fixture(scope="module")
def env(core, oracle_lib):
    return _Env(core, oracle_lib)


MODES = [0, 1]


@pytest.mark.parametrize("mode", MODES)
def test_gate_all_quorum(env, mode):
    sigs = list(env.sigs)
    sigs[7] = env.sigs[8]                      # one honest reject among them
    want = env.oracle_run(TOTAL, sigs, env.masks)
    assert want == [0 if j == 7 else 1 for j in range(TOTAL)]
    plain, _ = env.run(mode, "batch_agg_verify", TOTAL, sigs, env.masks)
    gated, stats = env.run(mode, "batch_agg_verify_quorum", TOTAL, sigs, env.masks)
    assert plain == want
    assert gated == want
    assert stats[0] == (3 if mode else 0)
    assert env.seal(mode, TOTAL, sigs, env.masks) == want


@pytest.mark.parametrize("mode", MODES)
def test_gate_quorumless_valid_signature(env, mode):
    """the case the ungated entries accept: one committee member, that
    member's valid signature"""
    assert env.oracle_run(TOTAL, env.q_sigs, env.q_masks) == [1] * TOTAL
    plain, _ = env.run(mode, "batch_agg_verify", TOTAL, env.q_sigs, env.q_masks)
    assert plain == [1] * TOTAL
    want = [env.core.NOQUORUM if j in QLESS else 1 for j in range(TOTAL)]
    gated, stats = env.run(mode, "batch_agg_verify_quorum", TOTAL, env.q_sigs, env.q_masks)
    assert gated == want
    assert stats == ([2, 0, 0] if mode else [0, 0, 0])
    assert env.seal(mode, TOTAL, env.q_sigs, env.q_masks) == want
    j = QLESS[1]
    assert env.committee.agg_verify_quorum(
        env.q_masks[j], env.q_sigs[j], env.msgs[j]) == env.core.NOQUORUM
    assert env.committee.agg_verify_quorum(env.masks[j], env.sigs[j], env.msgs[j]) == 1


@pytest.mark.parametrize("mode", MODES)
def test_gate_quorumless_wrong_signature(env, mode):
    """a quorumless item never reaches the pairing: in combined mode no chunk
    fails and nothing is re-checked"""
    sigs = list(env.q_sigs)
    for j in QLESS:
        sigs[j] = env.sigs[(j + 1) % TOTAL]
    want = [env.core.NOQUORUM if j in QLESS else 1 for j in range(TOTAL)]
    gated, stats = env.run(mode, "batch_agg_verify_quorum", TOTAL, sigs, env.q_masks)
    assert gated == want
    assert stats == ([(127 + 63) // 64, 0, 0] if mode else [0, 0, 0])


@pytest.mark.parametrize("mode", MODES)
def test_gate_undecodable_and_bad_signatures(env, mode):
    core = env.core
    sigs = list(env.q_sigs)
    sigs[0] = b"\xff" * 96                     # quorumless and undecodable
    sigs[5] = env.sigs[6]                      # quorum, wrong signature
    sigs[70] = b"\xff" * 96                    # quorum, undecodable
    oracle = env.oracle_run(TOTAL, sigs, env.q_masks)
    assert oracle[5] == 0 and oracle[70] < 0
    gated, _ = env.run(mode, "batch_agg_verify_quorum", TOTAL, sigs, env.q_masks)
    for j in range(TOTAL):
        if j in QLESS:
            assert gated[j] == core.NOQUORUM
        elif j == 70:
            assert gated[j] < 0 and gated[j] != core.NOQUORUM
        else:
            assert gated[j] == oracle[j] == (0 if j == 5 else 1)
    plain, _ = env.run(mode, "batch_agg_verify", TOTAL, sigs, env.q_masks)
    assert [gated[j] for j in range(TOTAL) if j not in QLESS] == \
        [plain[j] for j in range(TOTAL) if j not in QLESS]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", [1, 65])
def test_gate_nobody_has_quorum(env, mode, batch):
    rng = random.Random(batch)
    masks = [_mask_of(N, rng.sample(range(N), rng.randrange(0, 43))) for _ in range(batch)]
    gated, stats = env.run(mode, "batch_agg_verify_quorum", batch, env.sigs, masks)
    assert gated == [env.core.NOQUORUM] * batch
    assert stats == [0, 0, 0]
    assert env.seal(mode, batch, env.sigs, masks) == [env.core.NOQUORUM] * batch


def test_decider_batch_verify_seals_quorum(env):
    from harmony_amd import quorum

    class _W:
        def __init__(self, b):
            self.Bytes = b

    d = quorum.Decider([_W(env.pks[48 * i:48 * (i + 1)]) for i in range(N)])
    res = d.batch_verify_seals_quorum(b"".join(env.q_masks[:65]), b"".join(env.q_sigs[:65]),
                                      b"".join(env.msgs[:65]), env.mlen, 65)
    assert res == [env.core.NOQUORUM if j in QLESS else 1 for j in range(65)]
    assert d.batch_verify_seals(b"".join(env.q_masks[:65]), b"".join(env.q_sigs[:65]),
                                b"".join(env.msgs[:65]), env.mlen, 65) == [1] * 65


# ---------------------------------------------------------------- the stream

def _count(bitmap, n):
    return bin(int.from_bytes(bitmap, "little") & ((1 << n) - 1)).count("1")


class _StreamEnv:
    def __init__(self, core):
        n = self.n = 64
        self.sk = [pr.synth_sk(i) for i in range(n)]
        sks = [pr.fr_serialize(k) for k in self.sk]
        self.pks = core.batch_pk_from_sk(b"".join(sks), n)
        self.payloads = [pr.construct_commit_payload(r, pr.synth_msg(100 + r), r + 1)
                         for r in range(2)]
        mlen = len(self.payloads[0])
        cat = core.batch_sign(b"".join(sks) * 2,
                              b"".join(self.payloads[r] for r in range(2) for _ in range(n)),
                              mlen, 2 * n)
        self.sig = {(r, i): cat[96 * (r * n + i):96 * (r * n + i + 1)]
                    for r in range(2) for i in range(n)}

    def open(self, core, committee):
        st = core.Stream(committee, 2)
        st.set_rounds([0, 1], b"".join(self.payloads), len(self.payloads[0]))
        return st

    def tick(self, st, votes):
        return st.process([i for _, i in votes], [r for r, _ in votes],
                          b"".join(self.sig[v] for v in votes))


@pytest.fixture(scope="module")
def senv(core):
    return _StreamEnv(core)


def _agrees_with_get(st, n, w=None):
    pw, cn, qr = st.power([0, 1])
    for slot in (0, 1):
        bm = st.get(slot)[0]
        assert cn[slot] == _count(bm, n)
        assert pw[slot] == _expect(bm, n, w)[0]
    return pw, cn, qr


def test_stream_power_uniform(core, senv):
    n = senv.n
    committee = core.Committee(senv.pks, n)
    st = senv.open(core, committee)
    assert st.power([0, 1]) == ([0, 0], [0, 0], None)      # no policy yet: no verdict
    committee.set_quorum()
    assert st.power([1, 0, 1]) == ([0, 0, 0], [0, 0, 0], [0, 0, 0])
    res = senv.tick(st, [(0, i) for i in range(42)] + [(1, i) for i in range(10)])
    assert res == [1] * 52
    assert _agrees_with_get(st, n) == ([42, 10], [42, 10], [0, 0])
    assert senv.tick(st, [(0, 50)]) == [1]                  # the 43rd vote
    assert _agrees_with_get(st, n) == ([43, 10], [43, 10], [1, 0])
    assert senv.tick(st, [(0, i) for i in range(5)]) == [2] * 5   # valid duplicates
    assert _agrees_with_get(st, n) == ([43, 10], [43, 10], [1, 0])
    assert st.power([1]) == ([10], [10], [0])
    with pytest.raises(ValueError):
        st.power([2])
    with pytest.raises(ValueError):
        st.power([0, 7])


def test_stream_power_staked(core, senv):
    n = senv.n
    w = _staked_weights(n, 64)
    acc, flip = 0, None
    for i in range(n):
        acc += w[i]
        if acc > TWO_THIRDS:
            flip = i
            break
    assert flip is not None and 0 < flip < n - 1
    committee = core.Committee(senv.pks, n)
    committee.set_quorum(w)
    st = senv.open(core, committee)
    assert senv.tick(st, [(0, i) for i in range(flip)] + [(1, n - 1)]) == [1] * (flip + 1)
    pw, cn, qr = _agrees_with_get(st, n, w)
    assert pw == [sum(w[:flip]), w[n - 1]] and cn == [flip, 1] and qr == [0, 0]
    assert senv.tick(st, [(0, flip)]) == [1]
    pw, cn, qr = _agrees_with_get(st, n, w)
    assert pw == [sum(w[:flip + 1]), w[n - 1]] and cn == [flip + 1, 1] and qr == [1, 0]
