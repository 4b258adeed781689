"""harmony_amd.votepower: the integer mirror of numeric.Dec and
votepower.Compute (CPU only).  Expected values are worked out here with plain
ints from the reference's rules: Quo = trunc(a * 10^36 / b) chopped by 10^18,
Mul = a * b chopped by 10^18, the chop rounding half-to-even."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harmony_amd import votepower as vp  # noqa: E402

E18 = 10 ** 18


def test_two_thirds():
    assert vp.dec_quo(2 * E18, 3 * E18) == 666666666666666667
    assert vp.TWO_THIRDS == 666666666666666667
    # the dropped digits are .666...: above one half, so it rounds up
    assert (2 * E18 * E18 * E18 // (3 * E18)) % E18 > E18 // 2


def test_core_constant_matches():
    # core needs libhbls.so to import; the constant is checked textually
    src = open(os.path.join(os.path.dirname(vp.__file__), "core.py")).read()
    assert "TWO_THIRDS_DEC = 666666666666666667" in src
    hdr = open(os.path.join(os.path.dirname(vp.__file__), "..", "include", "hbls.h")).read()
    assert "#define HBLS_TWO_THIRDS_DEC 666666666666666667ULL" in hdr


def test_mul_half_to_even_both_ways():
    # 1e-18 * 0.5 = 0.5e-18 exactly: quotient 0 is even -> stays 0 (down)
    assert vp.dec_mul(1, E18 // 2) == 0
    # 3e-18 * 0.5 = 1.5e-18: quotient 1 is odd -> 2 (up)
    assert vp.dec_mul(3, E18 // 2) == 2
    # 5e-18 * 0.5 = 2.5e-18: quotient 2 is even -> 2 (down)
    assert vp.dec_mul(5, E18 // 2) == 2
    # not a tie: plain rounding either side
    assert vp.dec_mul(3, E18 // 2 + 1) == 2
    assert vp.dec_mul(3, E18 // 2 - 1) == 1
    assert vp.dec_mul(-3, E18 // 2) == -2


def test_quo_half_to_even_both_ways():
    # 1e-18 / 2 = 0.5e-18 -> 0 (even, down); 3e-18 / 2 = 1.5e-18 -> 2 (up)
    assert vp.dec_quo(1, 2 * E18) == 0
    assert vp.dec_quo(3, 2 * E18) == 2
    assert vp.dec_quo(5, 2 * E18) == 2
    assert vp.dec_quo(7, 2 * E18) == 4
    # exact quotients are untouched
    assert vp.dec_quo(E18, 4 * E18) == E18 // 4
    # big.Int.Quo truncates towards zero before the chop
    assert vp.dec_quo(-3, 2 * E18) == -2


def test_worked_vector():
    """three Harmony slots, stakes 1 and 2, 49% / 51%"""
    hp, ep = 49 * E18 // 100, 51 * E18 // 100

    def chop(d):
        q, r = divmod(d, E18)
        if r * 2 > E18 or (r * 2 == E18 and q % 2):
            q += 1
        return q

    hmy = chop(hp * E18 * E18 // (3 * E18))
    assert hmy == 163333333333333333
    g1 = chop(1 * E18 * E18 * E18 // (3 * E18))
    g2 = chop(2 * E18 * E18 * E18 // (3 * E18))
    assert (g1, g2) == (333333333333333333, 666666666666666667)
    s1, s2 = chop(g1 * ep), chop(g2 * ep)
    assert (s1, s2) == (170000000000000000, 340000000000000000)
    assert 3 * hmy + s1 + s2 == E18 - 1            # the last staker takes the 1

    want = [hmy, hmy, hmy, s1, s2 + 1]
    assert want == [163333333333333333] * 3 + [170000000000000000, 340000000000000001]
    assert vp.compute([None, None, None, 1 * E18, 2 * E18], hp, ep) == want
    # slot order is kept, and the last *staked* voter takes the difference
    assert vp.compute([1 * E18, None, 2 * E18, None, None], hp, ep) == \
        [s1, hmy, s2 + 1, hmy, hmy]


@pytest.mark.parametrize("seed", range(8))
def test_sums_to_one(seed):
    rng = random.Random(seed)
    n = rng.randrange(2, 400)
    stakes = [None if rng.random() < 0.3 else rng.randrange(1, 10 ** 9) * 10 ** rng.randrange(10, 19)
              for _ in range(n)]
    if all(e is None for e in stakes):
        stakes[-1] = E18
    if all(e is not None for e in stakes):
        stakes[0] = None
    pct = rng.randrange(1, 100)
    out = vp.compute(stakes, pct * E18 // 100, (100 - pct) * E18 // 100)
    assert len(out) == n and all(p >= 0 for p in out)
    assert sum(out) == E18


def test_all_staked_committee():
    # no Harmony slot and external percent one: still exactly one
    out = vp.compute([E18, E18, E18], 0, E18)
    assert out == [333333333333333333, 333333333333333333, 333333333333333334]
