"""The tail and the uploads of batch aggregate verify.

The combined path's final exponentiations run on the cooperative kernel
(k_aggrlc_final_coop, 16 chunks per block); the thread-per-chunk kernel stays
selectable.  Both must give the same chunk verdicts, and so the same per-item
results and refinement statistics, as each other, as the exact path (mode 0)
and as the CPU oracle.  hbls_batch_agg_verify uploads each input just ahead
of the kernel that reads it; a kernel that ran before its bytes arrived would
put verdicts at the wrong indices.

Shapes: 64 items = one chunk and 15 dummy sub-items in its block; 1089 items
= 18 chunks, two blocks, the last chunk holding one item."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aggrlc_env import BAD, CHUNK, N, Env, _chunks, _norm, gpu_marks  # noqa: E402

pytestmark = gpu_marks()

TOTAL = 1089                # 17 * 64 + 1


class _Env(Env):
    """1089 valid items.  The oracle's verdicts on them are computed once; an
    altered input set costs one oracle run over the altered items only (every
    item is its own check, so the others keep their verdicts)."""

    def __init__(self, capi, core):
        super().__init__(capi, core, seed=11, total=TOTAL, sk_base=700, msg_base=900)
        self.base = self._oracle(self.masks, self.sigs, self.msgs)
        assert self.base == [1] * TOTAL

    def _oracle(self, masks, sigs, msgs):
        n = len(masks)
        return _norm(self.oracle.batch_agg_verify(
            b"".join(masks), b"".join(sigs), b"".join(msgs), self.mlen, n))

    def oracle_run(self, batch, sigs=None, msgs=None, changed=()):
        """the oracle's verdicts on the first `batch` items, of which only
        the indices in `changed` differ from the valid set"""
        sigs = self.sigs if sigs is None else sigs
        msgs = self.msgs if msgs is None else msgs
        out = list(self.base[:batch])
        idx = [i for i in changed if i < batch]
        if idx:
            got = self._oracle([self.masks[i] for i in idx], [sigs[i] for i in idx],
                               [msgs[i] for i in idx])
            for i, v in zip(idx, got):
                out[i] = v
        return out

    def run(self, mode, batch, sigs=None, msgs=None, final=-1):
        """(normalised verdicts, stats) of one batch_agg_verify call over the
        first `batch` items in the given mode and final kernel"""
        return super().run(batch, sigs, None, msgs, mode=mode, final=final)[:2]

    def check(self, batch, expect, sigs=None, msgs=None, changed=()):
        """mode 1 == mode 0 == oracle == expect, item for item; returns mode
        1's stats"""
        r1, stats = self.run(1, batch, sigs, msgs)
        r0, stats0 = self.run(0, batch, sigs, msgs)
        assert stats0 == [0, 0, 0]
        assert r1 == expect
        assert r0 == expect
        assert self.oracle_run(batch, sigs, msgs, changed) == expect
        return stats


@pytest.fixture(scope="module")
def env(oracle_lib):
    from harmony_amd import core
    return _Env(oracle_lib, core)


# ---- the final kernels alone

@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_final_selftest(env, n):
    """cooperative (16 and 8 chunks per block) against thread-per-chunk on
    arbitrary, Fp6-subfield and unit products, empty and forced chunks, at
    the chunk counts around the 16-chunk block boundary"""
    assert env.core.aggrlc_final_selftest(n) == 0


# ---- end to end with the cooperative tail

@pytest.mark.parametrize("batch", [64, TOTAL])
def test_all_valid(env, batch):
    stats = env.check(batch, [1] * batch)
    assert stats == [_chunks(batch), 0, 0]


def test_one_wrong_signature_single_chunk(env):
    """one chunk, 15 dummy sub-items beside it in the block"""
    sigs = list(env.sigs)
    sigs[9] = env.sigs[10]
    expect = [1] * 64
    expect[9] = 0
    stats = env.check(64, expect, sigs=sigs, changed=[9])
    assert stats == [1, 1, 64]


@pytest.mark.parametrize("chunk", [0, 15, 16, 17])
def test_one_wrong_signature(env, chunk):
    """first and last chunk of the first block, first chunk of the second,
    and the one-item chunk: exactly that chunk fails and its eligible items
    are re-checked"""
    bad = min(chunk * CHUNK + 5, TOTAL - 1)
    sigs = list(env.sigs)
    sigs[bad] = env.sigs[bad - 1]                    # a valid point, the wrong one
    expect = [1] * TOTAL
    expect[bad] = 0
    stats = env.check(TOTAL, expect, sigs=sigs, changed=[bad])
    live = min(CHUNK, TOTAL - chunk * CHUNK)
    assert stats == [_chunks(TOTAL), 1, live]


def test_empty_chunk_beside_failing_and_passing_chunks(env):
    """chunk 5 holds only undecodable signatures (ccnt == 0) and shares its
    block with a failing chunk (3) and passing ones: no verdict moves"""
    sigs = list(env.sigs)
    dead = list(range(5 * CHUNK, 6 * CHUNK))
    for i in dead:
        sigs[i] = b"\xff" * 96
    wrong = 3 * CHUNK + 8
    sigs[wrong] = env.sigs[wrong + 1]
    expect = [1] * TOTAL
    for i in dead:
        expect[i] = BAD
    expect[wrong] = 0
    stats = env.check(TOTAL, expect, sigs=sigs, changed=dead + [wrong])
    assert stats == [_chunks(TOTAL) - 1, 1, CHUNK]


@pytest.mark.parametrize("final", [0, 8])
def test_final_kernel_switch(env, final):
    """the thread-per-chunk kernel (0) and the 8-chunk cooperative blocks
    give the default kernel's results and stats"""
    sigs = list(env.sigs)
    sigs[70] = env.sigs[71]
    sigs[TOTAL - 1] = env.sigs[0]
    sigs[400] = b"\xff" * 96
    want = env.run(1, TOTAL, sigs=sigs)
    got = env.run(1, TOTAL, sigs=sigs, final=final)
    assert got == want
    assert want[1] == [_chunks(TOTAL), 2, CHUNK + 1]
    assert [i for i, v in enumerate(want[0]) if v != 1] == [70, 400, TOTAL - 1]


def test_final_setter_rejects(env):
    with pytest.raises(ValueError):
        env.core.set_aggrlc_final(4)


# ---- uploads behind the first kernels

@pytest.mark.parametrize("batch", [1, 63, 65, TOTAL])
@pytest.mark.parametrize("mode", [0, 1])
def test_upload_order_matches_oracle(env, mode, batch):
    """item 0 carries a wrong signature at every batch, so a uniform answer
    cannot pass"""
    sigs = list(env.sigs)
    sigs[0] = env.sigs[1]
    expect = env.oracle_run(batch, sigs=sigs, changed=[0])
    assert expect[0] == 0 and expect[1:] == [1] * (batch - 1)
    res, _ = env.run(mode, batch, sigs=sigs)
    assert res == expect


@pytest.mark.parametrize("mode", [0, 1])
def test_bad_inputs_keep_their_indices(env, mode):
    """an undecodable signature and a wrong message are reported where they
    are: each verdict depends on its own signature, message and mask"""
    sigs, msgs = list(env.sigs), list(env.msgs)
    sigs[130] = b"\xff" * 96
    msgs[1000] = env.msgs[3]
    expect = env.oracle_run(TOTAL, sigs=sigs, msgs=msgs, changed=[130, 1000])
    assert expect[130] == BAD and expect[1000] == 0 and expect.count(1) == TOTAL - 2
    res, _ = env.run(mode, TOTAL, sigs=sigs, msgs=msgs)
    assert res == expect


def test_seal_and_quorum_entries_unchanged(env):
    """the device-resident entries run the same kernel order: mode 1 equals
    mode 0 on the 1089 items, with one wrong signature among them"""
    core = env.core
    sigs = list(env.sigs)
    sigs[640] = env.sigs[641]
    blobs = b"".join(sigs[j] + env.masks[j] for j in range(TOTAL))
    msgs = b"".join(env.msgs)
    qc = core.Committee(env.pks, N)
    qc.set_quorum()
    out = {}
    for mode in (0, 1):
        with core.aggrlc_switches(mode=mode, threshold=1):
            seal = env.committee.batch_seal_verify(blobs, 96 + env.bmlen, msgs,
                                                   env.mlen, TOTAL)
            quorum = qc.batch_agg_verify_quorum(b"".join(env.masks), b"".join(sigs),
                                                msgs, env.mlen, TOTAL)
        out[mode] = (seal, quorum)
    assert out[1] == out[0]
    seal, quorum = out[1]
    expect = [1] * TOTAL
    expect[640] = 0
    assert seal == expect
    # quorum: popcount > floor(2 * 64 / 3); items below it never reach the pairing
    live = [sum(bin(b).count("1") for b in m) > 2 * N // 3 for m in env.masks]
    assert any(live) and not all(live)
    for j in range(TOTAL):
        if live[j]:
            assert quorum[j] == expect[j]
        else:
            assert quorum[j] < 0


def test_host_intervals(env):
    core = env.core
    env.run(1, TOTAL)
    whole, launch_to_results = core.last_host_ns(4), core.last_host_ns(2)
    assert whole >= launch_to_results > 0
    assert core.last_host_ns(5) == 0
