"""Chunk-level signature leg of the combined aggregate verify.

Probe cases (hbls_aggrlc_probe, raw limbs as §4j): the windowed 64-bit scalar
multiplications against pyref's double-and-add, compared as affine points,
and the one-leg Miller loop through the final exponentiation against pyref's
pairing (cubed, §4j).

End to end: combined path with the signature leg per chunk (leg 1), per item
(leg 0), the exact path (mode 0) and the CPU oracle agree item for item, and
the two legs report the same core.aggrlc_last_stats()."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arith_cases as ac  # noqa: E402
from aggrlc_env import BAD, Env, _chunks, gpu_marks, init_core  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from test_aggrlc_sigleg_formulas import ALL_DIGITS, PROBE_SCALARS, recode64  # noqa: E402

pytestmark = gpu_marks()

P = ac.P


@pytest.fixture(scope="module")
def core():
    return init_core()


# ------------------------------------------------------------------ the probe
def _points(F2):
    """(name, affine point or None, Jacobian raw limbs): the generator with
    Z = 1, three seeded subgroup points under a random Z, the identity"""
    r = ac.rng("sigleg-g2" if F2 else "sigleg-g1")
    gen = pr.G2_GEN if F2 else pr.G1_GEN
    mul = pr.g2_mul if F2 else pr.g1_mul
    one = (1, 0) if F2 else 1
    rz = (lambda: (r.randrange(1, P), r.randrange(P))) if F2 else (lambda: r.randrange(1, P))
    out = [("gen", gen, ac._jac(F2, gen, one))]
    for k in range(3):
        pt = mul(gen, r.randrange(1, pr.R))
        out.append(("pt%d" % k, pt, ac._jac(F2, pt, rz())))
    n = 6 if F2 else 3
    inf = tuple(ac.tm(1) for _ in range(n - (2 if F2 else 1))) + ((0, 0) if F2 else (0,))
    out.append(("inf", None, inf))
    return out


@pytest.mark.parametrize("F2", [False, True], ids=["g1_mul64w", "g2_mul64w"])
def test_mul64w(core, F2):
    assert set(recode64(ALL_DIGITS)) == set(range(-8, 9))
    assert ALL_DIGITS in PROBE_SCALARS and len(PROBE_SCALARS) == 13 + 16
    name = "g2_mul64w" if F2 else "g1_mul64w"
    n_fp = 6 if F2 else 3
    mul = pr.g2_mul if F2 else pr.g1_mul
    cases = [(pn, pt, raw, k) for pn, pt, raw in _points(F2) for k in PROBE_SCALARS]
    data = b"".join(ac.pack([raw]) + k.to_bytes(8, "little") for _, _, raw, k in cases)
    out = core.aggrlc_probe(name, data, len(cases))
    outs = ac.unpack(out, n_fp)
    assert len(outs) == len(cases)
    for (pn, pt, _, k), o in zip(cases, outs):
        assert all(v < P for v in o), (pn, hex(k))
        want = mul(pt, k) if pt is not None else None
        assert ac.jac_to_affine(F2, o) == want, (pn, hex(k))


def test_miller1_fe(core):
    """final_exp(conj(miller_loop1_h(Q, P))) is pyref's pairing, cubed (§4j):
    (H, pk) of two items and (S, -G1) for the sum of their signatures"""
    sk = [pr.synth_sk(710 + i) for i in range(2)]
    hm = [pr.hash_to_g2(pr.synth_msg(910 + i)) for i in range(2)]
    pk = [pr.get_public_key(k) for k in sk]
    S = pr.g2_add(pr.g2_mul(hm[0], sk[0]), pr.g2_mul(hm[1], sk[1]))
    pairs = [(hm[0], pk[0]), (hm[1], pk[1]), (S, pr.g1_neg(pr.HERUMI_G1))]
    items = [tuple(ac.tm(c) for c in q[0] + q[1]) + (ac.tm(p[0]), ac.tm(p[1])) for q, p in pairs]
    out = core.aggrlc_probe("miller1_fe", ac.pack(items), len(items))
    outs = ac.unpack(out, 12)
    got = [ac.f12_of(o) for o in outs]
    for (q, p), g, o in zip(pairs, got, outs):
        assert all(v < P for v in o)
        assert g == pr.f12_pow(pr.pairing(q, p), 3)
    # the three values are the two sides of the two items' verification
    assert pr.f12_mul(pr.f12_mul(got[0], got[1]), got[2]) == pr.F12_ONE


# ------------------------------------------------------------------ end to end
BATCHES = [1, 63, 64, 65, 129, 130]
TOTAL = max(BATCHES)


class _Env(Env):
    def configured(self, mode, leg, call):
        return super().configured(call, mode=mode, sigleg=leg)[:2]

    def run(self, mode, leg, batch, sigs=None, masks=None):
        return super().run(batch, sigs, masks, mode=mode, sigleg=leg)[:2]

    def check(self, batch, expect, sigs=None, masks=None):
        """leg 1 == leg 0 == mode 0 == oracle == expect, and the two legs'
        stats are equal; returns them"""
        r1, s1 = self.run(1, 1, batch, sigs, masks)
        r0, s0 = self.run(1, 0, batch, sigs, masks)
        rx, sx = self.run(0, -1, batch, sigs, masks)
        assert sx == [0, 0, 0]
        assert r1 == expect
        assert r0 == expect
        assert rx == expect
        assert self.oracle_run(batch, sigs, masks) == expect
        assert s1 == s0
        return s1


@pytest.fixture(scope="module")
def env(oracle_lib, core):
    return _Env(oracle_lib, core, seed=6)


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


def test_cancelling_pair_in_one_chunk(env):
    """sig_a + D and sig_b - D: the unweighted sum of the two signatures is
    that of the valid ones, the weighted one must not be"""
    a, b = 3, 41
    expect = [1] * 65
    expect[a] = expect[b] = 0
    assert env.check(65, expect, sigs=env.cancelling(a, b)) == [2, 1, 64]


def test_cancelling_pair_across_chunks(env):
    a, b = 10, 70
    expect = [1] * TOTAL
    expect[a] = expect[b] = 0
    assert env.check(TOTAL, expect, sigs=env.cancelling(a, b)) == [3, 2, 128]


def test_undecodable_signature(env):
    sigs = list(env.sigs)
    sigs[5] = b"\xff" * 96
    expect = [1] * 65
    expect[5] = BAD
    assert env.check(65, expect, sigs=sigs) == [2, 0, 0]


def test_identity_signature_alone_in_last_chunk(env):
    """chunk 1 holds no eligible item: it is not counted, and its chunk
    entry (an identity sum) contributes one"""
    sigs = list(env.sigs)
    sigs[64] = b"\x00" * 96
    expect = [1] * 65
    expect[64] = 0
    assert env.check(65, expect, sigs=sigs) == [1, 0, 0]


def test_empty_mask(env):
    """the herumi edge: identity key sum and identity signature accept; an
    empty mask with a real signature does not, and neither enters a sum"""
    sigs, masks = list(env.sigs), list(env.masks)
    sigs[7] = b"\x00" * 96
    masks[7] = bytes(env.bmlen)
    masks[9] = bytes(env.bmlen)
    expect = [1] * 63
    expect[9] = 0
    assert env.check(63, expect, sigs=sigs, masks=masks) == [1, 0, 0]


def test_seal_verify(env):
    blobs = b"".join(env.sigs[j] + env.masks[j] for j in range(65))
    call = lambda: env.committee.batch_seal_verify(  # noqa: E731
        blobs, 96 + env.bmlen, b"".join(env.msgs[:65]), env.mlen, 65)
    r1, s1 = env.configured(1, 1, call)
    r0, s0 = env.configured(1, 0, call)
    assert r1 == r0 == [1] * 65
    assert s1 == s0 == [2, 0, 0]


def test_ctxset_seal_verify_two_committees(env):
    """one call over two committees: the second lists the same keys in
    reverse order, so its items carry the mirrored mask"""
    cs, idx, blobs, msgs, want = env.two_committees()
    call = lambda: cs.seal_verify(idx, blobs, msgs)  # noqa: E731
    r1, s1 = env.configured(1, 1, call)
    r0, s0 = env.configured(1, 0, call)
    rx, _ = env.configured(0, -1, call)
    assert r1 == want and r0 == want and rx == want
    assert s1 == s0 == [2, 1, 2]


@pytest.mark.parametrize("leg", [2, -2])
def test_setter_rejects(env, leg):
    core = env.core
    sigs = list(env.sigs)
    sigs[1] = env.sigs[2]
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=1):
        with pytest.raises(ValueError):
            core.set_aggrlc_sigleg(leg)
        # the rejected call changed nothing: leg 1 still runs, so a failing
        # chunk is found through its chunk entry
        res = env.committee.batch_agg_verify(
            b"".join(env.masks[:3]), b"".join(sigs[:3]), b"".join(env.msgs[:3]), env.mlen, 3)
        assert res == [1, 0, 1]
        assert core.last_stage_ns(7) > 0          # the signature scaling ran
        core.set_aggrlc_sigleg(-1)                # the default rule: per item at 3 items
        res = env.committee.batch_agg_verify(
            b"".join(env.masks[:3]), b"".join(sigs[:3]), b"".join(env.msgs[:3]), env.mlen, 3)
        assert res == [1, 0, 1]
        assert core.last_stage_ns(7) == 0
