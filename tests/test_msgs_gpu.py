"""Signed-message windows on the device:
ContextSet.verify_msgs over items that mix committees, signer sets and
entries of a message table, some of them Keccak'd on the device — each code
checked against the CPU oracle, and against the single-committee entry where
the two overlap."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from oracle import pyref as pr  # noqa: E402
from test_multikey_gpu import _Keys, _gpu_available  # noqa: E402

if not os.environ.get("HBLS_FORCE_GPU_TESTS"):
    pytestmark = [pytest.mark.gpu,
                  pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]

BAD = -3            # HBLS_ERR_BADINPUT
ZERO_SIG = bytes(96)
NINE = {0: [0, 1, 2, 3, 4, 5, 6, 7, 10], 1: [3, 5, 8, 13, 21, 30, 34, 38, 39],
        2: list(range(9))}                      # above MK_SHORT_MAX: the wave kernel


class _OtherKeys(_Keys):
    """_Keys over its own secret keys (synthetic keys base .. base + n - 1), so
    that an index names different keys in different committees"""

    def __init__(self, core, capi, n, base):
        self.capi, self.n, self.negate_9 = capi, n, False
        self.sks = [pr.fr_serialize(pr.synth_sk(base + i)) for i in range(n)]
        self.pks = core.batch_pk_from_sk(b"".join(self.sks), n)
        self.committee = core.Committee(self.pks, n)
        self.oracle = capi.Committee(self.pks, n)
        self._sigs = {}


class _Env:
    def __init__(self, core, capi):
        self.core, self.capi = core, capi
        self.keys = [_Keys(core, capi, 33, True), _OtherKeys(core, capi, 40, 1000),
                     _OtherKeys(core, capi, 9, 2000)]
        self.set = core.ContextSet([k.committee for k in self.keys])

    def signed(self, msg, digest):
        """the bytes a signer of table entry `msg` signs"""
        return self.capi.keccak256(msg) if digest else msg

    def sign(self, ctx, keys, msg, digest=False):
        return self.keys[ctx].sign(keys, self.signed(msg, digest))

    def expected(self, ctx, keys, sig, msg, digest=False):
        return self.keys[ctx].expected(keys, sig, self.signed(msg, digest))


@pytest.fixture(scope="module")
def env(oracle_lib):
    from harmony_amd import core
    return _Env(core, oracle_lib)


def _blob(n, seed):
    return bytes((seed + 7 * i) & 0xff for i in range(n))


@pytest.fixture(scope="module")
def window(env):
    """37 interleaved items over three committees and a 13-entry table; built
    and judged by the oracle once"""
    m48 = pr.synth_msg(1) + pr.synth_msg(2)[:16]
    table = [b"\x01", (77).to_bytes(8, "little"), pr.synth_msg(3),
             pr.construct_commit_payload(5, pr.synth_msg(4), 9, staking=False),
             m48, m48 + b"\x07"]
    assert [len(m) for m in table] == [1, 8, 32, 40, 48, 49]
    digest = [False] * len(table)
    for k, n in enumerate((0, 135, 136, 137, 300, 5000)):
        table.append(_blob(n, 11 + k))
        digest.append(True)
    flipped = bytearray(table[11])
    flipped[-1] ^= 1
    table.append(bytes(flipped))                # 12: the 5000-byte blob, last byte flipped
    digest.append(True)

    items = []                                  # (ctx, keys, msg_idx, sig)

    def good(ctx, keys, mi, signs=None):
        signs = mi if signs is None else signs
        items.append((ctx, keys, mi, env.sign(ctx, keys, table[signs], digest[signs])))

    shapes = [lambda c: [c + 1], lambda c: [2, 6 + c], lambda c: NINE[c]]
    for mi in range(12):                        # every entry, contexts and shapes rotating
        ctx = mi % 3
        good(ctx, shapes[(mi // 3 + mi) % 3](ctx), mi)
    good(0, [4], 5, signs=4)                    # signed the 48-byte string, item names the 49-byte one
    good(1, [4, 7], 4, signs=5)                 # and the other way round: the slot rule
    good(1, [11], 12, signs=11)                 # digest of the flipped blob: reject
    items.append((0, [8, 9], 0, ZERO_SIG))      # infinity key sum, identity signature: accept
    items.append((0, [8, 9], 0, env.sign(0, [0], table[0])))    # ... real signature: reject
    items.append((0, [1], 1, env.sign(0, [2], table[1])))       # wrong signer
    good(2, [3, 4], 3, signs=2)                 # wrong message
    items.append((1, [5], 2, env.sign(0, [5], table[2])))       # right index, wrong committee
    items.append((2, [0], 0, b"\xff" * 96))     # undecodable
    for s in range(5):                          # a view change: shared NIL and view-ID entries
        for ctx in range(3):
            if len(items) < 36:
                good(ctx, [s + 12 if ctx < 2 else s + 4], s & 1)
    good(1, NINE[1], 8)                         # a long list on a digested entry
    # interleave: deal the items out in a fixed scrambled order
    order = sorted(range(len(items)), key=lambda j: (j * 7) % len(items))
    items = [items[j] for j in order]
    want = [env.expected(c, k, s, table[mi], digest[mi]) for c, k, mi, s in items]
    by_item = {j: w for j, w in zip(order, want)}
    assert [by_item[j] for j in range(12)] == [1] * 12
    assert [by_item[j] for j in range(12, 21)] == [1, 1, 0, 1, 0, 0, 0, 0, BAD]
    assert len(items) == 37 and want.count(1) == len(items) - 6
    return table, digest, items, want


def _run(env, table, digest, items, **kw):
    return env.set.verify_msgs([c for c, _, _, _ in items], [k for _, k, _, _ in items],
                               b"".join(s for _, _, _, s in items),
                               [mi for _, _, mi, _ in items], table, digest, **kw)


@pytest.mark.parametrize("threshold", [10 ** 9, 0])
def test_mixed_window(env, window, threshold):
    """cooperative kernels (threshold above the batch) and thread-per-item
    kernels (threshold 0): the oracle's codes from both"""
    table, digest, items, want = window
    env.core.set_coop_threshold(threshold)
    try:
        got = _run(env, table, digest, items)
    finally:
        env.core.set_coop_threshold(-1)
    assert got == want


def test_malformed_items_alone_are_refused(env, window):
    table, digest, items, want = window
    keep = items[:8]
    n_ctx, n_msgs = 3, len(table)
    sig = keep[0][3]
    s35 = env.sign(1, [35], table[0])
    long0 = NINE[0][:-1] + [35]                 # index 35 in the 33-key committee, wave kernel
    malformed = [
        (n_ctx, [1], 0, sig), (0xffffffff, [1], 0, sig), (0, [1], n_msgs, sig),
        (0, [], 0, sig), (0, [35], 0, s35), (0, [5, 3], 0, sig), (0, [4, 4], 0, sig),
        (0, long0, 0, sig), (n_ctx, NINE[1], 0, sig), (1, NINE[1], 0xffffffff, sig),
        (2, NINE[2][::-1], 0, sig),
    ]
    fine35 = (1, [35], 0, s35)                  # the same index in the 40-key one
    mixed, expect = [], []
    for j, bad in enumerate(malformed):
        mixed += [bad, keep[j % len(keep)]]
        expect += [BAD, want[j % len(keep)]]
    mixed.append(fine35)
    expect.append(env.expected(1, [35], s35, table[0]))
    assert expect[-1] == 1
    assert _run(env, table, digest, mixed) == expect


def test_call_level_refusals(env, window):
    table, digest, items, _ = window
    core, one = env.core, items[:1]
    two = items[:2]
    with pytest.raises(core.BadInputError):     # key_off does not start at 0
        _run(env, table, digest, one, csr=([1, 2], [0, 1]))
    with pytest.raises(core.BadInputError):     # key_off decreases
        _run(env, table, digest, two, csr=([0, 2, 1], [0, 1]))
    small = [(c, k, 0, s) for c, k, _, s in two]
    with pytest.raises(core.BadInputError):     # msg_off does not start at 0
        _run(env, [b"ab", b"c"], None, small, csr=(None, None, [1, 2, 3]))
    with pytest.raises(core.BadInputError):     # msg_off decreases
        _run(env, [b"ab", b"c"], None, small, csr=(None, None, [0, 2, 1]))
    with pytest.raises(core.BadInputError):     # no messages
        _run(env, [], None, small)
    with pytest.raises(core.BadInputError):     # an empty batch
        _run(env, table, digest, [])


def test_agrees_with_the_single_committee_entry(env):
    core, K = env.core, env.keys[1]
    batch = 10
    lists = [[j, j + 20] if j & 1 else [j] for j in range(batch)]
    msgs = [pr.construct_commit_payload(j, pr.synth_msg(600 + j), j + 1, staking=False)
            for j in range(batch)]
    sigs = [K.sign(lists[j], msgs[j]) for j in range(batch)]
    sigs[4] = K.sign(lists[4], msgs[5])
    want = K.committee.batch_verify_votes_multi(lists, b"".join(sigs), b"".join(msgs), 40)
    assert want.count(1) == batch - 1 and want[4] == 0
    one_ctx = core.ContextSet([K.committee])
    got = one_ctx.verify_msgs([0] * batch, lists, b"".join(sigs), list(range(batch)), msgs)
    assert got == want

    # digests: the device's own Keccak in front of the existing entry
    blobs = [_blob(100, 50 + j) for j in range(batch)]
    digests = core.batch_keccak256(b"".join(blobs), 100, batch)
    dsigs = [K.sign(lists[j], digests[32 * j:32 * (j + 1)]) for j in range(batch)]
    dsigs[7] = dsigs[6]
    want = K.committee.batch_verify_votes_multi(lists, b"".join(dsigs), digests, 32)
    assert want.count(1) == batch - 1 and want[7] == 0
    got = one_ctx.verify_msgs([0] * batch, lists, b"".join(dsigs), list(range(batch)), blobs,
                              digest=[True] * batch)
    assert got == want

    # the all-zero slot: 48 zero bytes, and an empty undigested message
    zero = K.committee.batch_verify_votes_multi([[1]], sigs[1], bytes(48), 48)
    got = one_ctx.verify_msgs([0, 0], [[1], [1]], sigs[1] * 2, [0, 1], [bytes(48), b""])
    assert got == zero * 2


def test_sizes(env, window):
    table, digest, items, want = window
    assert _run(env, table, digest, items[5:6]) == want[5:6]         # a batch of 1
    msg = table[1]
    twenty = [(j % 3, [j % 9], 0, env.sign(j % 3, [j % 9], msg)) for j in range(19)]
    twenty.append((1, [2], 0, twenty[0][3]))
    expect = [env.expected(c, k, s, msg) for c, k, _, s in twenty]
    assert expect == [1] * 19 + [0]
    assert _run(env, [msg], None, twenty) == expect                  # one table entry
