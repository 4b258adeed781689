"""Hoisted schedule of the combined aggregate verify: the
signature chain ahead of the mask kernel, the chunk legs beside it on a side
stream, the key-sum part of the classification inside the Miller kernel and
a repair of the chunks it marks dirty.

Every case runs through batch_agg_verify four ways — hoisted (early 1), chunk
entries inside the Miller kernel (early 0), the per-item leg (leg 0) and the
exact path (mode 0) — and is compared with the CPU oracle item for item; the
three combined runs must report equal core.aggrlc_last_stats().  The hoisted
run uses the default chunk-leg kernel (four lanes per chunk); the all-valid
and wrong-signature cases repeat it with the one-lane kernel."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

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


@pytest.fixture(scope="module")
def core():
    from harmony_amd import core as c
    c.init(-1 if c.device_count() == 0 else 0)
    return c


N = 64                      # committee
BATCHES = [1, 63, 64, 65, 129, 130]
TOTAL = max(BATCHES)
BAD = -1                    # any negative code (the oracle and the library number them apart)


def _norm(res):
    return [BAD if v < 0 else v for v in res]


class _Env:
    """64 keys and 130 valid (mask, message, aggregate signature) items plus
    the forged signature the tests swap in — built once, never modified"""

    def __init__(self, capi, core):
        self.core = core
        self.capi = capi
        rng = random.Random(7)
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

    def configured(self, mode, leg, early, call, kernel=-1):
        """(results, stats, stage slots 7 and 8) of one call under the setting"""
        core = self.core
        core.set_agg_verify_mode(mode)
        core.set_aggrlc_threshold(1)
        core.set_aggrlc_sigleg(leg)
        core.set_aggrlc_early(early)
        core.set_aggrlc_chunkleg(kernel)
        try:
            res = call()
            stats = core.aggrlc_last_stats()
            slots = (core.last_stage_ns(7), core.last_stage_ns(8))
        finally:
            core.set_agg_verify_mode(-1)
            core.set_aggrlc_threshold(-1)
            core.set_aggrlc_sigleg(-1)
            core.set_aggrlc_early(-1)
            core.set_aggrlc_chunkleg(-1)
        return _norm(res), stats, slots

    def run(self, mode, leg, early, batch, sigs=None, masks=None, kernel=-1):
        sigs = self.sigs if sigs is None else sigs
        masks = self.masks if masks is None else masks
        return self.configured(mode, leg, early, lambda: self.committee.batch_agg_verify(
            b"".join(masks[:batch]), b"".join(sigs[:batch]),
            b"".join(self.msgs[:batch]), self.mlen, batch), kernel)

    def check(self, batch, expect, sigs=None, masks=None, onelane=False):
        """early 1 == early 0 == leg 0 == mode 0 == oracle == expect, the three
        combined runs' stats are equal, and slot 8 tells the hoisted call from
        the others; returns the stats"""
        r1, s1, t1 = self.run(1, 1, 1, batch, sigs, masks)
        if onelane:
            rk, sk, tk = self.run(1, 1, 1, batch, sigs, masks, kernel=0)
            assert rk == r1 and sk == s1
            assert tk[0] > 0 and tk[1] > 0
        r0, s0, t0 = self.run(1, 1, 0, batch, sigs, masks)
        rl, sl, tl = self.run(1, 0, 1, batch, sigs, masks)      # leg 0: nothing to hoist
        rx, sx, tx = self.run(0, -1, 1, batch, sigs, masks)
        assert sx == [0, 0, 0]
        assert r1 == expect
        assert r0 == expect
        assert rl == expect
        assert rx == expect
        sigs = self.sigs if sigs is None else sigs
        masks = self.masks if masks is None else masks
        assert _norm(self.oracle.batch_agg_verify(
            b"".join(masks[:batch]), b"".join(sigs[:batch]),
            b"".join(self.msgs[:batch]), self.mlen, batch)) == expect
        assert s1 == s0 == sl
        assert t1[0] > 0 and t1[1] > 0          # hoisted: sigscale + sigsum, chunk legs
        assert t0[0] > 0 and t0[1] == 0
        assert tl == (0, 0) and tx == (0, 0)
        return s1


@pytest.fixture(scope="module")
def env(oracle_lib, core):
    return _Env(oracle_lib, core)


def _chunks(batch):
    return (batch + 63) // 64


@pytest.mark.parametrize("batch", BATCHES)
def test_all_valid(env, batch):
    assert env.check(batch, [1] * batch, onelane=True) == [_chunks(batch), 0, 0]


@pytest.mark.parametrize("batch,bad", [(b, i) for b in BATCHES for i in (0, 64, 129) if i < b])
def test_one_wrong_signature(env, batch, bad):
    sigs = list(env.sigs)
    sigs[bad] = env.sigs[(bad + 1) % TOTAL]          # a valid point, the wrong one
    expect = [1] * batch
    expect[bad] = 0
    stats = env.check(batch, expect, sigs=sigs, onelane=True)
    first = 64 * (bad // 64)
    assert stats == [_chunks(batch), 1, min(batch, first + 64) - first]


# ------------------------------------------------------------------ dirty chunks
def test_dirty_chunk(env):
    """an empty mask under a real signature: the signature is scaled and
    summed before the key sum is known, the Miller kernel rejects the item and
    marks its chunk, and the repaired chunk verifies without it"""
    masks = list(env.masks)
    masks[9] = bytes(env.bmlen)
    expect = [1] * 63
    expect[9] = 0
    assert env.check(63, expect, masks=masks) == [1, 0, 0]


def test_dirty_chunk_next_to_wrong_signature(env):
    """the dirty chunk 0 is repaired and passes; chunk 1 fails on its own"""
    masks, sigs = list(env.masks), list(env.sigs)
    masks[9] = bytes(env.bmlen)
    sigs[70] = env.sigs[71]
    expect = [1] * TOTAL
    expect[9] = expect[70] = 0
    assert env.check(TOTAL, expect, sigs=sigs, masks=masks) == [3, 1, 64]


def test_two_dirty_items_in_one_chunk(env):
    masks = list(env.masks)
    masks[66] = bytes(env.bmlen)
    masks[127] = bytes(env.bmlen)
    expect = [1] * TOTAL
    expect[66] = expect[127] = 0
    assert env.check(TOTAL, expect, masks=masks) == [3, 0, 0]


def test_empty_mask_with_identity_signature(env):
    """the herumi edge: identity key sum and identity signature accept; the
    hoisted sigscale leaves the verdict open and the Miller kernel gives it"""
    sigs, masks = list(env.sigs), list(env.masks)
    sigs[7] = b"\x00" * 96
    masks[7] = bytes(env.bmlen)
    assert env.check(63, [1] * 63, sigs=sigs, masks=masks) == [1, 0, 0]


def test_identity_signature_alone_in_last_chunk(env):
    """chunk 1 holds no eligible item: it is not counted, and its chunk
    entry (an identity sum) contributes one"""
    sigs = list(env.sigs)
    sigs[64] = b"\x00" * 96
    expect = [1] * 65
    expect[64] = 0
    assert env.check(65, expect, sigs=sigs) == [1, 0, 0]


def test_undecodable_signature(env):
    sigs = list(env.sigs)
    sigs[5] = b"\xff" * 96
    expect = [1] * 65
    expect[5] = BAD
    assert env.check(65, expect, sigs=sigs) == [2, 0, 0]


def _cancelling(env, a, b):
    sigs = list(env.sigs)
    sigs[a] = env.capi.g2_add(env.sigs[a], env.D)
    sigs[b] = env.capi.g2_add(env.sigs[b], env.D, sub=True)
    return sigs


def test_cancelling_pair_in_one_chunk(env):
    a, b = 3, 41
    expect = [1] * 65
    expect[a] = expect[b] = 0
    assert env.check(65, expect, sigs=_cancelling(env, a, b)) == [2, 1, 64]


def test_cancelling_pair_across_chunks(env):
    a, b = 10, 70
    expect = [1] * TOTAL
    expect[a] = expect[b] = 0
    assert env.check(TOTAL, expect, sigs=_cancelling(env, a, b)) == [3, 2, 128]


# ------------------------------------------------------------------ other entries
def test_seal_verify(env):
    blobs = b"".join(env.sigs[j] + env.masks[j] for j in range(65))
    call = lambda: env.committee.batch_seal_verify(  # noqa: E731
        blobs, 96 + env.bmlen, b"".join(env.msgs[:65]), env.mlen, 65)
    r1, s1, t1 = env.configured(1, 1, 1, call)
    r0, s0, t0 = env.configured(1, 1, 0, call)
    assert r1 == r0 == [1] * 65
    assert s1 == s0 == [2, 0, 0]
    assert t1[1] > 0 and t0[1] == 0


def test_ctxset_seal_verify_keeps_its_sequence(env):
    """the epoch-context entry hoists nothing: equal results and stats at
    early 0 and early 1, and no chunk-leg interval at either"""
    core = env.core
    cs = core.ContextSet([env.committee])
    n = 66
    sigs = list(env.sigs[:n])
    sigs[65] = env.sigs[0]
    blobs = [sigs[j] + env.masks[j] for j in range(n)]
    call = lambda: cs.seal_verify([0] * n, blobs, env.msgs[:n])  # noqa: E731
    want = [1] * n
    want[65] = 0
    r1, s1, t1 = env.configured(1, 1, 1, call)
    r0, s0, t0 = env.configured(1, 1, 0, call)
    assert r1 == want and r0 == want
    assert s1 == s0 == [2, 1, 2]
    assert t1[1] == 0 and t0[1] == 0


@pytest.mark.parametrize("early", [2, -2])
def test_setter_rejects(env, early):
    core = env.core
    core.set_agg_verify_mode(1)
    core.set_aggrlc_threshold(1)
    core.set_aggrlc_sigleg(1)
    core.set_aggrlc_early(1)
    try:
        with pytest.raises(ValueError):
            core.set_aggrlc_early(early)
        # the rejected call changed nothing: the next call is still hoisted
        res = env.committee.batch_agg_verify(
            b"".join(env.masks[:3]), b"".join(env.sigs[:3]), b"".join(env.msgs[:3]), env.mlen, 3)
        assert res == [1, 1, 1]
        assert core.last_stage_ns(7) > 0
        assert core.last_stage_ns(8) > 0
        core.set_aggrlc_early(0)
        with pytest.raises(ValueError):
            core.set_aggrlc_early(early)
        res = env.committee.batch_agg_verify(
            b"".join(env.masks[:3]), b"".join(env.sigs[:3]), b"".join(env.msgs[:3]), env.mlen, 3)
        assert res == [1, 1, 1]
        assert core.last_stage_ns(7) > 0
        assert core.last_stage_ns(8) == 0
    finally:
        core.set_agg_verify_mode(-1)
        core.set_aggrlc_threshold(-1)
        core.set_aggrlc_sigleg(-1)
        core.set_aggrlc_early(-1)
