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
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aggrlc_env import BAD, Env, _chunks, gpu_marks, init_core  # noqa: E402

pytestmark = gpu_marks()


@pytest.fixture(scope="module")
def core():
    return init_core()


BATCHES = [1, 63, 64, 65, 129, 130]
TOTAL = max(BATCHES)


class _Env(Env):
    def configured(self, mode, leg, early, call, kernel=-1):
        """(results, stats, stage slots 7 and 8) of one call under the setting"""
        res, stats, slots = super().configured(call, mode=mode, sigleg=leg, early=early,
                                               chunkleg=kernel)
        return res, stats, (slots[7], slots[8])

    def run(self, mode, leg, early, batch, sigs=None, masks=None, kernel=-1):
        a = self.args(batch, sigs, masks)
        return self.configured(mode, leg, early,
                               lambda: self.committee.batch_agg_verify(*a), kernel)

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
        assert self.oracle_run(batch, sigs, masks) == expect
        assert s1 == s0 == sl
        assert t1[0] > 0 and t1[1] > 0          # hoisted: sigscale + sigsum, chunk legs
        assert t0[0] > 0 and t0[1] == 0
        assert tl == (0, 0) and tx == (0, 0)
        return s1


@pytest.fixture(scope="module")
def env(oracle_lib, core):
    return _Env(oracle_lib, core, seed=7)


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


def test_cancelling_pair_in_one_chunk(env):
    a, b = 3, 41
    expect = [1] * 65
    expect[a] = expect[b] = 0
    assert env.check(65, expect, sigs=env.cancelling(a, b)) == [2, 1, 64]


def test_cancelling_pair_across_chunks(env):
    a, b = 10, 70
    expect = [1] * TOTAL
    expect[a] = expect[b] = 0
    assert env.check(TOTAL, expect, sigs=env.cancelling(a, b)) == [3, 2, 128]


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
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=1, early=1):
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
