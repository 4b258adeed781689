"""Executable spec of the chunk-level signature leg of the combined aggregate
verify, in plain big-integer arithmetic (oracle/pyref.py):

  * the chunk check  prod_i f(H_i; r_i*pk_i) * f(sum_i r_i*sig_i; -G1)  passes
    the final exponentiation for valid items, fails with a wrong signature and
    fails for a pair of signatures that cancels in the unweighted product;
  * the signed 4-bit recoding that g1_mul64w / g2_mul64w walk (recode64 below
    is aggrlc_recode64 of csrc/hbls_aggrlc.inc, line for line).

PROBE_SCALARS and recode64 are shared with tests/test_aggrlc_sigleg_gpu.py."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402

M64 = (1 << 64) - 1
# recodes to every digit value from -8 to 8 (asserted below)
ALL_DIGITS = 0xC648A83CF28369FE
_rng = random.Random("hbls-aggrlc-sigleg-1")
PROBE_SCALARS = ([1, 2, 7, 8, 9, 15, 16, 1 << 63, M64,
                  0x8888888888888888, 0x7777777777777777, 0xFFFFFFFF00000000, ALL_DIGITS]
                 + [_rng.randrange(1, 1 << 64) for _ in range(16)])


def recode64(k):
    """the 17 signed digits d_0..d_16 of a 64-bit k: a window value above 8
    becomes value-16 with a carry; exactly 8 goes to -8 with a carry when the
    next window's nibble is 8 or more (it carries anyway), else stays +8"""
    assert 0 <= k <= M64
    c, out = 0, []
    for j in range(16):
        v = ((k >> (4 * j)) & 15) + c
        nx = (k >> (4 * j + 4)) & 15 if j < 15 else 0
        c = 1 if v > 8 or (v == 8 and nx >= 8) else 0
        out.append(v - 16 if c else v)
    out.append(c)
    return out


def test_recoding():
    for k in PROBE_SCALARS:
        d = recode64(k)
        assert len(d) == 17
        assert all(-8 <= x <= 8 for x in d)
        assert d[16] in (0, 1)
        assert sum(x << (4 * j) if x >= 0 else -((-x) << (4 * j)) for j, x in enumerate(d)) == k


def test_recoding_coverage():
    assert set(recode64(ALL_DIGITS)) == set(range(-8, 9))
    # every window of 0x88..88 carries; 2^64-1 is 16^16 - 1
    assert recode64(0x8888888888888888) == [-8] + [-7] * 15 + [1]
    assert recode64(M64) == [-1] + [0] * 15 + [1]
    assert recode64(8) == [8] + [0] * 16
    assert recode64(0x7777777777777777)[16] == 0


# ------------------------------------------------------------ the chunk check
SCALARS = [0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9]
NEG_G1 = pr.g1_neg(pr.HERUMI_G1)


class _Items:
    def __init__(self):
        self.sk = [pr.synth_sk(700 + i) for i in range(3)]
        self.msg = [pr.synth_msg(900 + i) for i in range(3)]
        self.pk = [pr.get_public_key(k) for k in self.sk]
        self.hm = [pr.hash_to_g2(m) for m in self.msg]
        self.sig = [pr.g2_mul(h, k) for h, k in zip(self.hm, self.sk)]
        # the items' own factors f(H_i; r_i*pk_i) do not depend on the signatures
        self.own = pr.F12_ONE
        for h, p, r in zip(self.hm, self.pk, SCALARS):
            self.own = pr.f12_mul(self.own, pr.miller_loop(h, pr.g1_mul(p, r)))

    def passes(self, sigs, scalars=SCALARS, own=None):
        s = None
        for sg, r in zip(sigs, scalars):
            s = pr.g2_add(s, pr.g2_mul(sg, r))
        f = pr.f12_mul(self.own if own is None else own, pr.miller_loop(s, NEG_G1))
        return pr.f12_pow(pr.f12_conj(f), pr.FINAL_EXP) == pr.F12_ONE


_items = None


def items():
    global _items
    if _items is None:
        _items = _Items()
    return _items


def test_chunk_check_accepts_valid_items():
    it = items()
    assert it.passes(it.sig)


def test_chunk_check_rejects_one_wrong_signature():
    it = items()
    other = pr.sign_hash(pr.synth_sk(999), it.msg[0])
    for i in range(3):
        sigs = list(it.sig)
        sigs[i] = other
        assert not it.passes(sigs)


def test_chunk_check_rejects_cancelling_pair():
    """sig_a + D and sig_b - D.  With every r_i = 1 the D terms cancel in the
    sum and the check passes (asserted), which is why the scalars are random
    and secret; with distinct r_i the sum keeps (r_a - r_b)*D and it fails."""
    it = items()
    D = pr.sign_hash(pr.synth_sk(998), it.msg[1])
    sigs = list(it.sig)
    sigs[0] = pr.g2_add(sigs[0], D)
    sigs[1] = pr.g2_add(sigs[1], pr.g2_neg(D))
    assert not it.passes(sigs)
    own1 = pr.F12_ONE
    for h, p in zip(it.hm, it.pk):
        own1 = pr.f12_mul(own1, pr.miller_loop(h, p))
    assert it.passes(sigs, scalars=[1, 1, 1], own=own1)
