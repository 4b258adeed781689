"""Multi-key votes on the device: signer-set key sums, batch
verify against the sums, and the stream tick with the ordered all-or-nothing
claim — each checked against the CPU oracle and the pure-Python model."""
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

BAD = -3            # HBLS_ERR_BADINPUT
ZERO_SIG = bytes(96)


def _bitmap(n, keys):
    bm = bytearray((n + 7) // 8)
    for k in keys:
        bm[k >> 3] |= 1 << (k & 7)
    return bytes(bm)


class _Keys:
    """n synthetic keys; with negate_9, key 9 is the negation of key 8 (the
    y-parity flip of test_mask_windowed_edges), so {8, 9} sums to infinity and
    key 9's signature is the negated signature of key 8."""

    def __init__(self, core, capi, n, negate_9):
        self.capi, self.n, self.negate_9 = capi, n, negate_9
        self.sks = [pr.fr_serialize(pr.synth_sk(i)) for i in range(n)]
        pks = bytearray(core.batch_pk_from_sk(b"".join(self.sks), n))
        if negate_9:
            pks[9 * 48:10 * 48] = pks[8 * 48:9 * 48]
            pks[10 * 48 - 1] ^= 0x80
        self.pks = bytes(pks)
        self.committee = core.Committee(self.pks, n)
        self.oracle = capi.Committee(self.pks, n)
        self._sigs = {}

    def sign1(self, i, msg):
        if (i, msg) not in self._sigs:
            if self.negate_9 and i == 9:
                s = self.capi.g2_add(ZERO_SIG, self.sign1(8, msg), sub=True)
            else:
                s = self.capi.sign_hash(self.sks[i], msg)
            self._sigs[(i, msg)] = s
        return self._sigs[(i, msg)]

    def sign(self, keys, msg):
        """the multi-key sender's signature: the sum of its keys' signatures"""
        return self.capi.aggregate_sigs([self.sign1(i, msg) for i in keys])

    def expected(self, keys, sig, msg):
        """oracle.verify_hash(mask_aggregate(keys), sig, msg) as a result code"""
        pk = self.oracle.mask_aggregate(_bitmap(self.n, keys))
        try:
            return 1 if self.capi.verify_hash(pk, sig, msg) else 0
        except ValueError:
            return BAD


@pytest.fixture(scope="module")
def keys33(oracle_lib):
    from harmony_amd import core
    return _Keys(core, oracle_lib, 33, True)


@pytest.fixture(scope="module")
def keys40(oracle_lib):
    from harmony_amd import core
    return _Keys(core, oracle_lib, 40, False)


@pytest.fixture(scope="module")
def keys130(oracle_lib):
    from harmony_amd import core
    return _Keys(core, oracle_lib, 130, False)


def test_key_sums(keys33):
    from harmony_amd import core
    n, c = 33, keys33.committee
    good = [[0], [31, 32], [1, 2, 3, 5, 7], list(range(33)), [8, 9]]
    bad = [[], [5, 5], [7, 3], [2, 40]]
    sums, ok = c.vote_key_sums(good + bad)
    for j, keys in enumerate(good):
        assert ok[j] == 1, (keys, ok[j])
        assert sums[j] == keys33.oracle.mask_aggregate(_bitmap(n, keys)), keys
    assert sums[4] == bytes(48)                       # {8, 9}: infinity
    for j in range(len(good), len(good) + len(bad)):
        assert ok[j] == BAD and sums[j] == bytes(48), (j, ok[j])
    # whole-call errors: offsets that do not start at 0, or that decrease
    with pytest.raises(core.BadInputError):
        c.vote_key_sums(None, csr=([1, 2], [0, 1]))
    with pytest.raises(core.BadInputError):
        c.vote_key_sums(None, csr=([0, 2, 1], [0, 1]))


@pytest.fixture(scope="module")
def verify_cases(keys33):
    """70 votes (two 64-thread blocks on the scalar path), 1 to 4 keys each,
    one message per vote; built and judged by the oracle once"""
    rng = random.Random(41)
    n, batch = 33, 70
    msgs = [pr.construct_commit_payload(j, pr.synth_msg(700 + j), j + 1) for j in range(batch)]
    lists, sigs = [], []
    for j in range(batch):
        keys = sorted(rng.sample(range(n), rng.randint(1, 4)))
        lists.append(keys)
        sigs.append(keys33.sign(keys, msgs[j]))
    lists[3], sigs[3] = [1, 2], keys33.sign([1], msgs[3])       # one key signed for two
    sigs[10] = keys33.sign(lists[10], msgs[11])                 # wrong message
    lists[20], sigs[20] = [8, 9], ZERO_SIG                      # inf sum, identity sig
    lists[30], sigs[30] = [8, 9], keys33.sign([0], msgs[30])    # inf sum, real sig
    lists[40] = [5, 5]                                          # malformed list
    sigs[65] = b"\xff" * 96                                     # undecodable
    want = [BAD if j == 40 else keys33.expected(lists[j], sigs[j], msgs[j])
            for j in range(batch)]
    assert want[3] == 0 and want[10] == 0 and want[30] == 0 and want[65] == BAD
    assert want[20] == 1                                        # herumi identity edge
    assert sum(1 for w in want if w == 1) == batch - 5
    return lists, b"".join(sigs), b"".join(msgs), len(msgs[0]), want


@pytest.mark.parametrize("threshold", [10 ** 9, 0])
def test_batch_verify_votes_multi(keys33, verify_cases, threshold):
    """cooperative kernel (threshold above the batch) and thread-per-item
    kernel (threshold 0): the same codes as the oracle"""
    from harmony_amd import core
    lists, sigs, msgs, mlen, want = verify_cases
    core.set_coop_threshold(threshold)
    try:
        got = keys33.committee.batch_verify_votes_multi(lists, sigs, msgs, mlen)
    finally:
        core.set_coop_threshold(-1)
    assert got == want


def test_stream_ordered_rule(keys33):
    from harmony_amd import core
    n = 33
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(800 + r), r + 1) for r in range(2)]
    st = core.Stream(keys33.committee, 2)
    st.set_rounds([0, 1], b"".join(payloads), len(payloads[0]))

    tick1 = [(0, [1, 2]), (0, [2, 3]), (0, [3, 4]), (0, [31, 32])]
    sigs1 = b"".join(keys33.sign(k, payloads[r]) for r, k in tick1)
    res1 = st.process_multi([k for _, k in tick1], [r for r, _ in tick1], sigs1)
    assert res1 == [1, 2, 1, 1]

    tick2 = [(0, [4, 5]), (0, [6, 7]), (0, [6]), (1, [0])]
    sigs2 = [keys33.sign(k, payloads[r]) for r, k in tick2]
    sigs2[1] = keys33.sign([6, 7], payloads[1])                 # signed the other round
    res2 = st.process_multi([k for _, k in tick2], [r for r, _ in tick2], b"".join(sigs2))
    assert res2 == [2, 0, 1, 1]

    want = [_bitmap(n, [1, 2, 3, 4, 6, 31, 32]), _bitmap(n, [0])]   # 5 and 7 stay clear
    assert want[0] == bytes([0x5E, 0x00, 0x00, 0x80, 0x01])
    power, count, _ = st.power([0, 1])
    assert count == [7, 1] and power == [7, 1]
    assert st.check([0, 1]) == [True, True]
    for r in range(2):
        bm, agg = st.get(r)
        assert bm == want[r]
        # each accepted signature was added exactly once
        assert keys33.oracle.agg_verify(bm, agg, payloads[r]) is True


@pytest.mark.parametrize("mode", [0, 1])
def test_stream_infinity_sum(keys33, mode):
    """{8, 9} sums to infinity: valid only with the identity signature, which
    sets both bits and adds nothing to the aggregate — in both verify modes"""
    from harmony_amd import core
    n = 33
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(850 + r), r + 1) for r in range(2)]
    st = core.Stream(keys33.committee, 2)
    st.set_verify_mode(mode)
    st.set_rounds([0, 1], b"".join(payloads), len(payloads[0]))
    tick = [(0, [1]), (0, [8, 9]), (1, [8, 9]), (1, [2, 9]), (0, [9, 10])]
    sigs = [keys33.sign(k, payloads[r]) for r, k in tick]
    assert sigs[1] == ZERO_SIG
    sigs[2] = keys33.sign([0], payloads[1])          # a real signature: invalid
    res = st.process_multi([k for _, k in tick], [r for r, _ in tick], b"".join(sigs))
    assert res == [1, 1, 0, 1, 2]
    want = [_bitmap(n, [1, 8, 9]), _bitmap(n, [2, 9])]
    assert st.check([0, 1]) == [True, True]
    for r in range(2):
        bm, agg = st.get(r)
        assert bm == want[r]
        assert keys33.oracle.agg_verify(bm, agg, payloads[r]) is True
    assert st.get(0)[1] == keys33.sign([1], payloads[0])


@pytest.fixture(scope="module")
def model_ticks(keys40):
    """60 votes over three ticks, 2 rounds, 1 to 4 keys each drawn from 40 keys
    (about 75 key slots per round: overlaps within and across ticks are the
    rule), one vote in ten signed over the other round's payload"""
    rng = random.Random(43)
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(900 + r), r + 1) for r in range(2)]
    ticks = []
    for _ in range(3):
        tick = []
        for _ in range(20):
            r = rng.randrange(2)
            keys = sorted(rng.sample(range(40), rng.randint(1, 4)))
            valid = rng.random() >= 0.1
            sig = keys40.sign(keys, payloads[r if valid else 1 - r])
            tick.append((r, keys, valid, sig))
        ticks.append(tick)
    ticks[0][1] = ticks[0][0]              # an exact repeat inside a tick
    return payloads, ticks


def _run_ticks(keys40, payloads, ticks, mode):
    from harmony_amd import core
    st = core.Stream(keys40.committee, 2)
    st.set_verify_mode(mode)
    st.set_rounds([0, 1], b"".join(payloads), len(payloads[0]))
    out = []
    for tick in ticks:
        res = st.process_multi([t[1] for t in tick], [t[0] for t in tick],
                               b"".join(t[3] for t in tick))
        out.append((res, [st.get(r) for r in range(2)]))
    return out


def test_stream_against_model(keys40, model_ticks):
    from harmony_amd.stream import ordered_claim_model
    payloads, ticks = model_ticks
    runs = [_run_ticks(keys40, payloads, ticks, mode) for mode in (0, 1)]
    bitmaps = [bytes(5), bytes(5)]
    seen = set()
    for t, tick in enumerate(ticks):
        want, bitmaps = ordered_claim_model(bitmaps, [(r, k, v) for r, k, v, _ in tick])
        seen.update(want)
        for mode in (0, 1):
            res, state = runs[mode][t]
            assert res == want, (mode, t)
            assert [bm for bm, _ in state] == bitmaps, (mode, t)
        # mode 1: identical aggregates too
        assert runs[0][t][1] == runs[1][t][1], t
    assert seen == {0, 1, 2}               # the data exercises every outcome
    for r in range(2):
        bm, agg = runs[0][-1][1][r]
        assert keys40.oracle.agg_verify(bm, agg, payloads[r]) is True


def test_single_key_equivalence(keys40):
    """a single-key tick without duplicates: process and process_multi agree
    on results, bitmaps and serialized aggregates"""
    from harmony_amd import core
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(950 + r), r + 1) for r in range(2)]
    votes = [(i % 2, i) for i in range(0, 40, 3)] + [(1, 38), (0, 31), (0, 32)]
    assert len(set(votes)) == len(votes)
    sigs = [keys40.sign([i], payloads[r]) for r, i in votes]
    sigs[4] = keys40.sign([votes[4][1]], payloads[1 - votes[4][0]])    # one invalid
    sigs = b"".join(sigs)
    states = []
    for multi in (False, True):
        st = core.Stream(keys40.committee, 2)
        st.set_rounds([0, 1], b"".join(payloads), len(payloads[0]))
        if multi:
            res = st.process_multi([[i] for _, i in votes], [r for r, _ in votes], sigs)
        else:
            res = st.process([i for _, i in votes], [r for r, _ in votes], sigs)
        states.append((res, st.get(0), st.get(1)))
    assert states[0] == states[1]
    assert states[0][0] == [0 if j == 4 else 1 for j in range(len(votes))]


@pytest.mark.parametrize("mode", [0, 1])
def test_stream_long_signer_sets(keys130, mode):
    """signer sets longer than a wave (the 64-lane block sum and the strided
    claim), up to the whole committee; n = 130 spans five bitmap words"""
    from harmony_amd import core
    keys, n = keys130, 130
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(990 + r), r + 1) for r in range(2)]
    st = core.Stream(keys.committee, 2)
    st.set_verify_mode(mode)
    st.set_rounds([0, 1], b"".join(payloads), len(payloads[0]))
    tick = [(0, list(range(n))), (0, [129]), (1, list(range(70))),
            (1, list(range(64, 101))), (1, list(range(70, 130)))]
    sigs = b"".join(keys.sign(k, payloads[r]) for r, k in tick)
    sums, ok = keys.committee.vote_key_sums([k for _, k in tick])
    assert ok == [1] * 5
    assert sums == [keys.oracle.mask_aggregate(_bitmap(n, k)) for _, k in tick]
    res = st.process_multi([k for _, k in tick], [r for r, _ in tick], sigs)
    assert res == [1, 2, 1, 2, 1]
    assert st.power([0, 1])[1] == [n, n]
    for r in range(2):
        bm, agg = st.get(r)
        assert bm == _bitmap(n, range(n))
        assert keys.oracle.agg_verify(bm, agg, payloads[r]) is True


def test_multistream_verifier_takes_tuples(keys40):
    """MultiStreamVerifier.process: an int or a tuple of ints per vote"""
    from harmony_amd.stream import MultiStreamVerifier
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(970 + r), r + 1) for r in range(2)]
    msv = MultiStreamVerifier(keys40.pks, 40, payloads, window=10 ** 9)
    votes = [(0, (1, 2), keys40.sign([1, 2], payloads[0])),
             (0, 2, keys40.sign([2], payloads[0])),
             (1, 2, keys40.sign([2], payloads[1]))]
    assert msv.process(votes) == [1, 0, 1]      # the verifier reports non-1 as 0
    assert msv.rounds[0].bitmap == _bitmap(40, [1, 2])
    assert msv.process(votes[2:]) == [0]        # single-key ticks keep the old entry
    assert msv.final_check_all() is True
