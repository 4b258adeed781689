"""Executable spec for the combined aggregate verify (DESIGN.md §4e,
harmony_amd/csrc/hbls_aggrlc.inc).  CPU only, over the oracle's field ops:
the product over the items of the two-leg Miller values with SCALED G1
arguments,
    prod_i f(H_i, r_i*pk_i) * f(sig_i, r_i*(-G1)),
passes the final-exponentiation check exactly when every item verifies."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402

NEG_G1 = pr.g1_neg(pr.HERUMI_G1)
SCALARS = [0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x0000000100000001]


@pytest.fixture(scope="module")
def items():
    """three valid (pk, H, sig) items on distinct messages, one spare G2
    point D, and a cache of Miller values keyed by their arguments"""
    out = []
    for i in range(3):
        sk = pr.synth_sk(40 + i)
        msg = pr.synth_msg(900 + i)
        out.append((pr.get_public_key(sk), pr.hash_to_g2(msg), pr.sign_hash(sk, msg)))
    D = pr.sign_hash(pr.synth_sk(77), pr.synth_msg(977))
    return out, D, {}


def _miller(cache, q, p):
    key = (q, p)
    if key not in cache:
        cache[key] = pr.miller_loop(q, p)
    return cache[key]


def _combined_passes(cache, triples, scalars):
    f = pr.F12_ONE
    for (pk, hm, sig), r in zip(triples, scalars):
        f = pr.f12_mul(f, _miller(cache, hm, pr.g1_mul(pk, r)))
        f = pr.f12_mul(f, _miller(cache, sig, pr.g1_mul(NEG_G1, r)))
    return pr.f12_pow(pr.f12_conj(f), pr.FINAL_EXP) == pr.F12_ONE


def test_every_item_valid_passes(items):
    triples, _D, cache = items
    for pk, hm, sig in triples:
        assert pr.verify_pairing_eq(pk, hm, sig)
    assert _combined_passes(cache, triples, SCALARS)


@pytest.mark.parametrize("bad", [0, 1, 2])
def test_one_invalid_item_fails(items, bad):
    triples, D, cache = items
    forged = list(triples)
    pk, hm, _sig = triples[bad]
    forged[bad] = (pk, hm, D)
    assert not pr.verify_pairing_eq(pk, hm, D)
    assert not _combined_passes(cache, forged, SCALARS)


def test_cancelling_pair_needs_the_weights(items):
    """sig_a + D and sig_b - D: both items are invalid, their UNWEIGHTED
    product passes, the weighted one does not"""
    triples, D, cache = items
    (pa, ha, sa), (pb, hb, sb), c = triples
    forged = [(pa, ha, pr.g2_add(sa, D)), (pb, hb, pr.g2_add(sb, pr.g2_neg(D))), c]
    assert not pr.verify_pairing_eq(*forged[0])
    assert not pr.verify_pairing_eq(*forged[1])
    assert _combined_passes(cache, forged, [1, 1, 1])
    assert not _combined_passes(cache, forged, SCALARS)
