"""Item Miller kernel of the combined aggregate verify without its two
inversions and without the product pass.

Probe cases (hbls_aggrlc_probe, raw limbs as §4j): the one-leg loop on
Jacobian arguments through the final exponentiation against the affine loop,
limb for limb, and against pyref's pairing (cubed, §4j); the product across
the 64 lanes of a wave against a chain of pyref multiplications.

End to end: levels 0 (affine arguments, product kernel), 1 (Jacobian
arguments) and 2 (Jacobian arguments, product inside the Miller kernel), each
hoisted and not, agree with the CPU oracle item for item and report the same
core.aggrlc_last_stats()."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arith_cases as ac  # noqa: E402
from aggrlc_env import BAD, Env, _chunks, gpu_marks, init_core  # noqa: E402
from oracle import pyref as pr  # noqa: E402

pytestmark = gpu_marks()

P = ac.P
LEVELS = (0, 1, 2)


@pytest.fixture(scope="module")
def core():
    return init_core()


# ------------------------------------------------------------------ the probe
def test_miller1j_fe(core):
    """(H, pk) of two items and (S, -G1), each with Z = 1 and with a random Z
    on either side and on both: every Jacobian form gives the affine loop's
    value after the final exponentiation, which is pyref's pairing cubed"""
    r = ac.rng("miller1j")
    sk = [pr.synth_sk(720 + i) for i in range(2)]
    hm = [pr.hash_to_g2(pr.synth_msg(920 + i)) for i in range(2)]
    pk = [pr.get_public_key(k) for k in sk]
    S = pr.g2_add(pr.g2_mul(hm[0], sk[0]), pr.g2_mul(hm[1], sk[1]))
    pairs = [(hm[0], pk[0]), (hm[1], pk[1]), (S, pr.g1_neg(pr.HERUMI_G1))]
    aff = [tuple(ac.tm(c) for c in q[0] + q[1]) + (ac.tm(p[0]), ac.tm(p[1])) for q, p in pairs]
    want = ac.unpack(core.aggrlc_probe("miller1_fe", ac.pack(aff), len(aff)), 12)
    for (q, p), w in zip(pairs, want):
        assert ac.f12_of(w) == pr.f12_pow(pr.pairing(q, p), 3)
    items, which = [], []
    for n, (q, p) in enumerate(pairs):
        for zq_rand, zp_rand in ((False, False), (True, False), (False, True), (True, True)):
            zq = (r.randrange(1, P), r.randrange(P)) if zq_rand else (1, 0)
            zp = r.randrange(1, P) if zp_rand else 1
            items.append(ac._jac(True, q, zq) + ac._jac(False, p, zp))
            which.append(n)
    assert len(items) == 12
    outs = ac.unpack(core.aggrlc_probe("miller1j_fe", ac.pack(items), len(items)), 12)
    assert len(outs) == 12
    for n, o in zip(which, outs):
        assert o == want[n]


def _wave_groups():
    """64 seeded reduced elements; all ones; one non-one element at lane 0, 1,
    31, 32 and 63 in turn: a lane per butterfly level's edge and both sides of
    the crossing between the wave's halves; lanes 2 and 3 with them, so that
    every role of a quad (the rounds that split one multiplication over four
    lanes) has held the odd element"""
    r = ac.rng("wave-prod")
    rnd = lambda: tuple(r.randrange(P) for _ in range(12))  # noqa: E731
    one = tuple(ac.f12_raw(pr.F12_ONE))
    groups = [[rnd() for _ in range(64)], [one] * 64]
    for lane in (0, 1, 2, 3, 31, 32, 63):
        g = [one] * 64
        g[lane] = rnd()
        groups.append(g)
    return groups


def test_wave_prod(core):
    groups = _wave_groups()
    data = b"".join(ac.pack(g) for g in groups)
    outs = ac.unpack(core.aggrlc_probe("wave_prod", data, len(groups)), 24)
    assert len(outs) == len(groups)
    for g, o in zip(groups, outs):
        want = pr.F12_ONE
        for el in g:
            want = pr.f12_mul(want, ac.f12_of(el))
        assert o[:12] == o[12:]                     # lane 0 and lane 63
        assert all(v < P for v in o)
        assert o[:12] == ac.f12_raw(want)
    assert outs[1][:12] == ac.f12_raw(pr.F12_ONE)


# ------------------------------------------------------------------ end to end
BATCHES = [1, 63, 64, 65, 129, 130]
TOTAL = max(BATCHES)


class _Env(Env):
    def configured(self, level, early, call):
        """(results, stats, stage slots 5 and 8) of one call on the combined
        path with the chunk-level leg under the setting"""
        res, stats, slots = super().configured(call, mode=1, sigleg=1, early=early,
                                               miller=level)
        return res, stats, (slots[5], slots[8])

    def check_call(self, call, expect, hoists=True):
        """every level, hoisted and not: results == expect, equal stats, the
        product slot positive, and at level 2 short enough to tell that
        k_aggrlc_chunk_prod was not launched; returns the stats.

        Slot 5 at levels 0 and 1 is k_aggrlc_chunk_prod: lone waves here, a
        load, six tree levels of one fp12_mul each behind a barrier, and the
        chunk entry's, seven dependent multiplications.  At level 2 it is
        k_aggrlc_chunk_fold: a load and one.  The ratio expected from that is
        about seven (the per-call sweep of DESIGN.md §4m has 2.10 against 0.28
        ms at 256 chunks); the assertion asks for two, which leaves the launch
        overhead inside both intervals a factor of three."""
        stats = None
        for early in (0, 1):
            prod = {}
            for level in LEVELS:
                r, s, t = self.configured(level, early, call)
                assert r == expect, (level, early)
                assert stats is None or s == stats, (level, early)
                stats = s
                assert t[0] > 0, (level, early)         # chunk_prod, or the chunk fold
                assert (t[1] > 0) == bool(early and hoists), (level, early)
                prod[level] = t[0]
            print("slot 5 ns, early %d: %s" % (early, prod))
            assert 2 * prod[2] < min(prod[0], prod[1]), (early, prod)
        return stats

    def check(self, batch, expect, sigs=None, masks=None):
        args = self.args(batch, sigs, masks)
        assert self.oracle_run(batch, sigs, masks) == expect
        return self.check_call(lambda: self.committee.batch_agg_verify(*args), expect)


@pytest.fixture(scope="module")
def env(oracle_lib, core):
    return _Env(oracle_lib, core, seed=8)


@pytest.mark.parametrize("batch", BATCHES)
def test_all_valid(env, batch):
    assert env.check(batch, [1] * batch) == [_chunks(batch), 0, 0]


@pytest.mark.parametrize("batch,bad", [(b, i) for b in BATCHES for i in (0, 64, 129) if i < b])
def test_one_wrong_signature(env, batch, bad):
    sigs = list(env.sigs)
    sigs[bad] = env.sigs[(bad + 1) % TOTAL]          # a valid point, the wrong one
    expect = [1] * batch
    expect[bad] = 0
    stats = env.check(batch, expect, sigs=sigs)
    first = 64 * (bad // 64)
    assert stats == [_chunks(batch), 1, min(batch, first + 64) - first]


def test_dirty_chunk(env):
    """§4l's dirty chunk: an empty mask under a real signature.  Hoisted, the
    Miller kernel demotes the item itself, and at level 2 the item must drop
    out of that block's product"""
    masks = list(env.masks)
    masks[9] = bytes(env.bmlen)
    expect = [1] * 63
    expect[9] = 0
    assert env.check(63, expect, masks=masks) == [1, 0, 0]


def test_dirty_chunk_next_to_wrong_signature(env):
    masks, sigs = list(env.masks), list(env.sigs)
    masks[9] = bytes(env.bmlen)
    sigs[70] = env.sigs[71]
    expect = [1] * TOTAL
    expect[9] = expect[70] = 0
    assert env.check(TOTAL, expect, sigs=sigs, masks=masks) == [3, 1, 64]


def test_empty_mask_with_identity_signature(env):
    """the herumi edge: identity key sum and identity signature accept"""
    sigs, masks = list(env.sigs), list(env.masks)
    sigs[7] = b"\x00" * 96
    masks[7] = bytes(env.bmlen)
    assert env.check(63, [1] * 63, sigs=sigs, masks=masks) == [1, 0, 0]


def test_identity_signature_alone_in_last_chunk(env):
    """chunk 1 holds no eligible item: its block's product is one and it is
    not counted"""
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


def test_cancelling_pair_across_chunks(env):
    a, b = 10, 70
    sigs = env.cancelling(a, b)
    expect = [1] * TOTAL
    expect[a] = expect[b] = 0
    assert env.check(TOTAL, expect, sigs=sigs) == [3, 2, 128]


# ------------------------------------------------------------------ other entries
def test_seal_verify(env):
    blobs = b"".join(env.sigs[j] + env.masks[j] for j in range(65))
    call = lambda: env.committee.batch_seal_verify(  # noqa: E731
        blobs, 96 + env.bmlen, b"".join(env.msgs[:65]), env.mlen, 65)
    assert env.check_call(call, [1] * 65) == [2, 0, 0]


def test_ctxset_seal_verify_two_committees(env):
    """one call over two committees (the second lists the same keys in reverse
    order, so its items carry the mirrored mask); this entry hoists nothing"""
    cs, idx, blobs, msgs, want = env.two_committees()
    call = lambda: cs.seal_verify(idx, blobs, msgs)  # noqa: E731
    assert env.check_call(call, want, hoists=False) == [2, 1, 2]


@pytest.mark.parametrize("level", [3, -2])
def test_setter_rejects(env, level):
    """a rejected value changes nothing: the call after it runs and agrees"""
    core = env.core
    args = (b"".join(env.masks[:3]), b"".join(env.sigs[:3]), b"".join(env.msgs[:3]), env.mlen, 3)
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=1, miller=-1):
        for keep in LEVELS:
            core.set_aggrlc_miller(keep)
            with pytest.raises(ValueError):
                core.set_aggrlc_miller(level)
            assert env.committee.batch_agg_verify(*args) == [1, 1, 1]
            assert core.aggrlc_last_stats() == [1, 0, 0]
            assert core.last_stage_ns(5) > 0
