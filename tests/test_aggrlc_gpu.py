"""Combined aggregate verify (agg-verify mode 1): per-item
verdicts of Committee.batch_agg_verify must equal the exact per-item path's
(mode 0) and the CPU oracle's, with the shared final exponentiations and the
refinement shown by core.aggrlc_last_stats()."""
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

N = 64                      # committee
BATCHES = [1, 63, 64, 65, 130]
TOTAL = max(BATCHES)
BAD = -1                    # any negative code (the oracle and the library number them apart)


def _norm(res):
    return [BAD if v < 0 else v for v in res]


class _Env:
    """64 keys and 130 valid (mask, message, aggregate signature) items plus
    the forged signatures the tests swap in — built once, never modified.
    An item's aggregate signature is one signature under the sum of its
    signers' secret keys (BLS is linear in the key)."""

    def __init__(self, capi):
        from harmony_amd import core
        self.core = core
        self.capi = capi
        rng = random.Random(4)
        sk = [pr.synth_sk(300 + i) for i in range(N)]
        self.pks = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in sk), N)
        self.committee = core.Committee(self.pks, N)
        self.oracle = capi.Committee(self.pks, N)
        self.bmlen = (N + 7) // 8
        self.masks, self.msgs, agg_sk = [], [], []
        for j in range(TOTAL):
            signers = rng.sample(range(N), rng.randrange(1, N + 1))
            bm = bytearray(self.bmlen)
            for i in signers:
                bm[i >> 3] |= 1 << (i & 7)
            self.masks.append(bytes(bm))
            self.msgs.append(pr.construct_commit_payload(j, pr.synth_msg(500 + j), j + 1))
            agg_sk.append(sum(sk[i] for i in signers) % pr.R)
        self.mlen = len(self.msgs[0])
        cat = core.batch_sign(b"".join(pr.fr_serialize(k) for k in agg_sk),
                              b"".join(self.msgs), self.mlen, TOTAL)
        self.sigs = [cat[96 * j:96 * (j + 1)] for j in range(TOTAL)]
        self.D = capi.sign_hash(pr.fr_serialize(pr.synth_sk(999)), self.msgs[0])
        assert core.aggrlc_chunk_size() == 64

    def run(self, mode, batch, sigs=None, masks=None):
        """(normalised verdicts, stats) of one batch_agg_verify call over the
        first `batch` items in the given mode"""
        core = self.core
        sigs = self.sigs if sigs is None else sigs
        masks = self.masks if masks is None else masks
        core.set_agg_verify_mode(mode)
        core.set_aggrlc_threshold(1)
        try:
            res = self.committee.batch_agg_verify(
                b"".join(masks[:batch]), b"".join(sigs[:batch]),
                b"".join(self.msgs[:batch]), self.mlen, batch)
            stats = core.aggrlc_last_stats()
        finally:
            core.set_agg_verify_mode(-1)
            core.set_aggrlc_threshold(-1)
        return _norm(res), stats

    def oracle_run(self, batch, sigs=None, masks=None):
        sigs = self.sigs if sigs is None else sigs
        masks = self.masks if masks is None else masks
        return _norm(self.oracle.batch_agg_verify(
            b"".join(masks[:batch]), b"".join(sigs[:batch]),
            b"".join(self.msgs[:batch]), self.mlen, batch))

    def check(self, batch, expect, sigs=None, masks=None):
        """mode 1 == mode 0 == oracle == expect; returns mode 1's stats"""
        r1, stats = self.run(1, batch, sigs, masks)
        r0, stats0 = self.run(0, batch, sigs, masks)
        assert stats0 == [0, 0, 0]
        assert r1 == expect
        assert r0 == expect
        assert self.oracle_run(batch, sigs, masks) == expect
        return stats


@pytest.fixture(scope="module")
def env(oracle_lib):
    return _Env(oracle_lib)


def _chunks(batch):
    return (batch + 63) // 64


@pytest.mark.parametrize("batch", BATCHES)
def test_all_valid(env, batch):
    stats = env.check(batch, [1] * batch)
    assert stats == [_chunks(batch), 0, 0]


@pytest.mark.parametrize("bad", [0, 64, 129])
def test_one_wrong_signature(env, bad):
    sigs = list(env.sigs)
    sigs[bad] = env.sigs[(bad + 1) % TOTAL]          # a valid point, the wrong one
    expect = [1] * TOTAL
    expect[bad] = 0
    stats = env.check(TOTAL, expect, sigs=sigs)
    assert stats[0] == _chunks(TOTAL) and stats[1] == 1
    assert 1 <= stats[2] <= 64


def test_cancelling_pair_in_one_chunk(env):
    """sig_a + D and sig_b - D: the unweighted product of the two items
    passes, the weighted one must not"""
    a, b = 3, 41
    sigs = list(env.sigs)
    sigs[a] = env.capi.g2_add(env.sigs[a], env.D)
    sigs[b] = env.capi.g2_add(env.sigs[b], env.D, sub=True)
    expect = [1] * 65
    expect[a] = expect[b] = 0
    stats = env.check(65, expect, sigs=sigs)
    assert stats == [2, 1, 64]


def test_undecodable_signature(env):
    sigs = list(env.sigs)
    sigs[5] = b"\xff" * 96
    expect = [1] * 65
    expect[5] = BAD
    stats = env.check(65, expect, sigs=sigs)
    assert stats == [2, 0, 0]


def test_identity_signature_nonempty_mask(env):
    sigs = list(env.sigs)
    sigs[64] = b"\x00" * 96
    expect = [1] * 65
    expect[64] = 0
    stats = env.check(65, expect, sigs=sigs)
    assert stats == [1, 0, 0]        # chunk 1 holds no eligible item


def test_empty_mask_identity_signature(env):
    """the herumi edge: identity key sum and identity signature accept;
    an empty mask with a real signature does not"""
    sigs, masks = list(env.sigs), list(env.masks)
    sigs[7] = b"\x00" * 96
    masks[7] = bytes(env.bmlen)
    masks[9] = bytes(env.bmlen)
    expect = [1] * 63
    expect[9] = 0
    stats = env.check(63, expect, sigs=sigs, masks=masks)
    assert stats == [1, 0, 0]


def test_two_calls_agree(env):
    sigs = list(env.sigs)
    sigs[100] = env.sigs[101]
    first = env.run(1, TOTAL, sigs=sigs)
    second = env.run(1, TOTAL, sigs=sigs)
    assert first == second
    assert first[0].count(0) == 1 and first[0][100] == 0


def test_seal_verify_takes_the_combined_path(env):
    blobs = b"".join(env.sigs[j] + env.masks[j] for j in range(65))
    core = env.core
    core.set_agg_verify_mode(1)
    core.set_aggrlc_threshold(1)
    try:
        res = env.committee.batch_seal_verify(blobs, 96 + env.bmlen,
                                              b"".join(env.msgs[:65]), env.mlen, 65)
        stats = core.aggrlc_last_stats()
    finally:
        core.set_agg_verify_mode(-1)
        core.set_aggrlc_threshold(-1)
    assert res == [1] * 65
    assert stats == [2, 0, 0]


@pytest.mark.parametrize("mode", [2, -2])
def test_mode_setter_rejects(env, mode):
    with pytest.raises(ValueError):
        env.core.set_agg_verify_mode(mode)
    # the rejected call changed nothing: a small batch still runs exact
    res, stats = env.run(-1, 1)
    assert res == [1] and stats == [0, 0, 0]
