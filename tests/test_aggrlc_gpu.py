"""Combined aggregate verify (agg-verify mode 1): per-item
verdicts of Committee.batch_agg_verify must equal the exact per-item path's
(mode 0) and the CPU oracle's, with the shared final exponentiations and the
refinement shown by core.aggrlc_last_stats()."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aggrlc_env import BAD, Env, _chunks, gpu_marks  # noqa: E402

pytestmark = gpu_marks()

BATCHES = [1, 63, 64, 65, 130]
TOTAL = max(BATCHES)


class _Env(Env):
    def run(self, mode, batch, sigs=None, masks=None):
        """(normalised verdicts, stats) of one batch_agg_verify call over the
        first `batch` items in the given mode"""
        return super().run(batch, sigs, masks, mode=mode)[:2]

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
    from harmony_amd import core
    return _Env(oracle_lib, core, seed=4)


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
    sigs = env.cancelling(a, b)
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


def test_every_class_in_one_chunk(env):
    """the one classification routine under every kernel that
    calls it: chunk 0 holds a wrong signature, an undecodable one, the herumi
    accept (empty mask, identity signature), an empty mask under a real
    signature and an identity signature under a real mask; item 64 is valid
    and alone in chunk 1.  Chunk 0 fails on the wrong signature, and four of
    its items are classified without a pairing: 60 go to the per-item path."""
    sigs, masks = list(env.sigs), list(env.masks)
    sigs[3] = env.sigs[4]                   # a valid point, the wrong one
    sigs[5] = b"\xff" * 96
    sigs[7], masks[7] = b"\x00" * 96, bytes(env.bmlen)
    masks[9] = bytes(env.bmlen)
    sigs[11] = b"\x00" * 96
    expect = [1] * 65
    expect[3], expect[5], expect[9], expect[11] = 0, BAD, 0, 0
    assert env.oracle_run(65, sigs, masks) == expect
    assert env.run(0, 65, sigs, masks) == (expect, [0, 0, 0])
    combined = [dict(sigleg=0)] + [dict(sigleg=1, early=early, miller=level)
                                   for early in (0, 1) for level in (0, 1, 2)]
    for switches in combined:
        res, stats, slots = Env.run(env, 65, sigs, masks, mode=1, **switches)
        assert res == expect, switches
        assert stats == [2, 1, 60], switches
        # slot 8, the hoisted chunk legs' own interval, tells the schedules apart
        assert (slots[8] > 0) == bool(switches.get("early")), switches


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
    with core.aggrlc_switches(mode=1, threshold=1):
        res = env.committee.batch_seal_verify(blobs, 96 + env.bmlen,
                                              b"".join(env.msgs[:65]), env.mlen, 65)
        stats = core.aggrlc_last_stats()
    assert res == [1] * 65
    assert stats == [2, 0, 0]


@pytest.mark.parametrize("mode", [2, -2])
def test_mode_setter_rejects(env, mode):
    with pytest.raises(ValueError):
        env.core.set_agg_verify_mode(mode)
    # the rejected call changed nothing: a small batch still runs exact
    res, stats = env.run(-1, 1)
    assert res == [1] and stats == [0, 0, 0]
