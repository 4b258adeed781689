"""CPU checks of tests/arith_cases.py: the operand sets of the device
arithmetic probe must hit the edges they were built for.  Everything here
follows from the big-integer reference alone, so a weak case set cannot hide
a device fault behind a passing GPU test."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arith_cases as ac  # noqa: E402
from oracle import pyref as pr  # noqa: E402

P, R = ac.P, ac.R


def test_table_is_well_formed():
    names = [o.name for o in ac.OPS]
    assert len(set(names)) == len(names)
    for o in ac.OPS:
        items = ac.items_of(o)
        assert items, o.name
        assert all(len(it) == o.n_in for it in items), o.name
        if o.base is not None:
            b = ac.OPS[ac.OP_INDEX[o.base]]
            assert b.base is None, o.name
            assert (b.n_in, b.n_out) == (o.n_in, o.n_out), o.name
            assert ac.items_of(b) == items, o.name      # same cases, same expected bytes
        if o.name != "fp_from_le48":
            assert all(0 <= v < P for it in items for v in it), o.name


def test_sizes():
    """a few hundred items for cheap operations, 64 for inv / sqrt / pow_u,
    8 for the final exponentiation"""
    for o in ac.OPS:
        n = len(ac.items_of(o))
        if "final_exp" in o.name:
            assert n == 8, o.name
        elif any(s in o.name for s in ("inv", "sqrt", "pow_u", "legendre")):
            assert n <= 64, (o.name, n)
        else:
            assert n <= 600, (o.name, n)


def test_fp_pool():
    pool = set(ac.fp_pool())
    for v in [0, 1, R % P, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 380]:
        assert v in pool
    for k in range(32, 353, 32):
        assert (1 << k) - 1 in pool and P - (1 << k) in pool
    limbs = lambda v: [(v >> (32 * i)) & 0xffffffff for i in range(12)]
    assert limbs(ac.ALL_ONES) == [0xffffffff] * 11 + [0x1a0111e9]
    assert limbs(ac.ALT_EVEN) == [0xffffffff, 0] * 6
    assert limbs(ac.ALT_ODD)[:11] == [0, 0xffffffff] * 5 + [0]
    assert {ac.ALL_ONES, ac.ALT_EVEN, ac.ALT_ODD} <= pool
    assert len(ac.fp_pool()) == len(ac.FP_EDGES) + 64


def test_fp_addsub_hits_the_boundaries():
    sums = [x + y for x, y in ac.fp_addsub()]
    assert sums.count(P) >= 64 and sums.count(P - 1) >= 64 and sums.count(P + 1) >= 64
    assert sum(1 for x, y in ac.fp_addsub() if x == y) >= 64          # difference 0
    assert any(x < y for x, y in ac.fp_addsub()) and any(x > y for x, y in ac.fp_addsub())
    assert any(s >= 1 << 381 for s in sums)                            # carry past p's top bit
    assert (0,) in ac.fp_unary()                                       # neg(0), dbl(0), half(0)


def test_fp_mul_covers_both_sides_of_the_final_subtraction():
    cases = ac.fp_mul()
    t = [ac.premont(x, y) for x, y in cases]
    assert all(v < 2 * P for v in t)
    assert sum(v >= P for v in t) >= 32
    assert sum(v < P for v in t) >= 32
    res = {x * y * ac.RINV % P for x, y in cases}
    assert set(ac.MUL_TARGETS) <= res
    for r_ in ac.MUL_TARGETS:
        assert sum(1 for x, y in cases if x * y * ac.RINV % P == r_) >= len(ac.fp_pool()) - 1
    assert (P - 1, P - 1) in cases


def test_cvr_fp2_mul_third_product():
    """the interleaved CIOS multiplies the unreduced sums a+b, c+d (< 2p):
    the pre-subtraction value must stay below 2p for ONE conditional
    subtraction to suffice, and the worst case must be in the set"""
    cases = ac.f2_mul()
    assert ac.CVR_WORST in cases
    both = sum(1 for a, b, c, d in cases if a + b >= P and c + d >= P)
    one = sum(1 for a, b, c, d in cases if (a + b >= P) != (c + d >= P))
    assert both >= 16 and one >= 16
    t = [ac.premont(a + b, c + d) for a, b, c, d in cases]
    assert sum(v >= P for v in t) >= 32 and sum(v < P for v in t) >= 32
    # largest operands with the largest m = R-1: no pair of sums can exceed it
    bound = ((2 * (P - 1)) ** 2 + (R - 1) * P) // R
    assert 1.40 * P < bound < 1.41 * P                           # the header's "< 1.5p"
    assert max(t) <= bound
    assert max(t) > 1.25 * P                                     # and the set gets close


def test_fp2_pool_and_sqrt_classes():
    pool = ac.f2_pool()
    for a in ac.F2_EDGE_COMP:
        for b in ac.F2_EDGE_COMP:
            assert (a, b) in pool
    assert len(pool) == 16 + 32
    xs = [(ac.fm(a), ac.fm(b)) for a, b in ac.f2_sqrt()]
    assert (0, 0) in xs and (P - 1, 0) in xs
    cls = [ac.f2_sqrt_class(x) for x in xs]
    for c in ("qr", "nqr", "sq", "nsq"):
        assert cls.count(c) >= 8, c
    # both attempts of the b != 0 tail occur: t = (a+w)/2 a square, or not
    first = 0
    for (a, b), c in zip(xs, cls):
        if c == "sq":
            w = pr.fp_sqrt((a * a + b * b) % P)
            first += pr.fp_sqrt((a + w) * ac.INV2 % P) is not None
    assert 0 < first < cls.count("sq")
    fs = [pr.fp_sqrt(ac.fm(v[0])) is not None for v in ac.fp_sqrt()]
    assert fs.count(True) >= 16 and fs.count(False) >= 16


def _tower_checks(elems, n):
    z, one, mx = ac.Z2, ac.ONE2, ac.MAX2
    assert (z,) * n in elems and (one,) + (z,) * (n - 1) in elems and (mx,) * n in elems
    for i in range(n):
        assert any(e[i] != z and all(e[j] == z for j in range(n) if j != i) for e in elems), i
    dense = [e for e in elems if all(c != z for c in e)]
    assert len(dense) >= 17


def test_fp6_fp12_elements():
    e6, e12 = ac.f6_elems(), ac.f12_elems()
    _tower_checks(e6, 3)
    _tower_checks(e12, 6)
    assert any(e[1] == ac.Z2 and e[0] != ac.Z2 and e[2] != ac.Z2 for e in e6)
    # the Fp6 subfield of Fp12: c1 = 0 with a dense c0
    assert any(all(c != ac.Z2 for c in e[:3]) and all(c == ac.Z2 for c in e[3:]) for e in e12)
    zero6, zero12 = (0,) * 6, (0,) * 12
    assert zero6 in ac.f6_unary() and zero6 not in ac.f6_inv()
    assert zero12 in ac.f12_unary() and zero12 not in ac.f12_inv()
    assert len(ac.f6_inv()) == len(e6) - 1 and len(ac.f12_inv()) == len(e12) - 1


def test_cyclotomic_inputs():
    cyc = ac.f12_cyclotomic()
    assert len(cyc) == 9 and tuple(ac.f12_raw(pr.F12_ONE)) in cyc
    for v in cyc:
        x = ac.f12_of(v)
        # order divides p^4 - p^2 + 1: x^(p^4) * x == x^(p^2)
        p2 = ac.f12_frob2(x)
        assert pr.f12_mul(ac.f12_frob2(p2), x) == p2
        # so conjugation is inversion there
        assert pr.f12_mul(x, pr.f12_conj(x)) == pr.F12_ONE


def test_final_exp_inputs():
    ins = ac.final_exp_in()
    assert len(ins) == 8 and len(set(ins)) == 8
    assert tuple(ac.f12_raw(pr.F12_ONE)) == ins[0]
    assert all(any(v) for v in ins)
    nz = lambda v: [i for i in range(6) if (v[2 * i], v[2 * i + 1]) != (0, 0)]
    assert nz(ins[1]) == [0]                    # Fp2 subfield
    assert nz(ins[2]) == [0, 1, 2]              # Fp6 subfield
    assert nz(ins[3]) == [0, 4, 5]              # sparse, line shaped
    assert all(nz(v) == list(range(6)) for v in ins[4:])


def test_final_exp_exponent():
    """Walk the device's final_exp chain (hbls_dev.hip) as integer exponents.
    After the easy part the element is cyclotomic, where conjugation is
    multiplication by -1; pow_u multiplies by u = |z|, frob by p, frob2 by
    p^2.  The hard part comes out as 3 (p^4 - p^2 + 1) / r, so the device
    computes the CUBE of the reference's (p^12 - 1) / r power."""
    p, r, u = P, pr.R, ac.U
    assert u == 0xd201000000010000
    easy = (p ** 6 - 1) * (p ** 2 + 1)
    f = 1
    a = -(u * f + f)
    b = -(u * a + a)
    c = -(u * b) + p * b
    d = u * u * c + p * p * c - c
    hard = d + 3 * f                              # cyc_sqr(f) * f = f^3
    assert hard == (u + 1) ** 2 * (p - u) * (u * u + p * p - 1) + 3
    assert (p ** 4 - p ** 2 + 1) % r == 0
    assert hard == 3 * (p ** 4 - p ** 2 + 1) // r
    assert easy * hard == 3 * (p ** 12 - 1) // r == 3 * pr.FINAL_EXP
    # and the expected values really are that power, not the plain one
    one = ac.final_exp_expected()[0]
    assert tuple(one) == tuple(ac.f12_raw(pr.F12_ONE))
    x = ac.f12_of(ac.final_exp_in()[4])
    plain = pr.f12_pow(x, pr.FINAL_EXP)
    assert plain != pr.F12_ONE
    assert tuple(ac.f12_raw(pr.f12_mul(pr.f12_sqr(plain), plain))) == ac.final_exp_expected()[4]


def _group_checks(F2, cases):
    adds, dbls, madds = cases
    by = {c.name: c for c in adds}
    n = 6 if F2 else 3
    aff = lambda item, k: ac.jac_to_affine(F2, item[k * n:(k + 1) * n])
    zraw = lambda item, k: item[k * n + 2 * n // 3:(k + 1) * n]
    for c in adds:
        p1, p2 = aff(c.item, 0), aff(c.item, 1)
        want = pr.g2_add(p1, p2) if F2 else pr.g1_add(p1, p2)
        assert want == c.expect, c.name
        on = pr.g2_on_curve if F2 else pr.g1_on_curve
        assert all(q is None or on(q) for q in (p1, p2)), c.name
    one = (ac.RP, 0) if F2 else (ac.RP,)
    nontrivial = lambda z: tuple(z) != tuple(one) and any(z)
    for name in ("generic", "same_point_z_differs", "negation_z_differs"):
        c = by[name]
        assert nontrivial(zraw(c.item, 0)) and nontrivial(zraw(c.item, 1)), name
        assert zraw(c.item, 0) != zraw(c.item, 1), name
    for name in ("same_point_z_differs", "same_point_z_one"):
        c = by[name]
        assert aff(c.item, 0) == aff(c.item, 1) and c.item[:n] != c.item[n:]
        assert c.expect is not None and c.degenerate
    for name in ("negation_z_differs", "negation_z_one"):
        c = by[name]
        neg = pr.g2_neg if F2 else pr.g1_neg
        assert aff(c.item, 0) == neg(aff(c.item, 1)) and c.expect is None
    assert aff(by["inf_plus_p"].item, 0) is None and aff(by["inf_plus_p"].item, 1) is not None
    assert aff(by["p_plus_inf"].item, 1) is None and aff(by["p_plus_inf"].item, 0) is not None
    assert aff(by["inf_plus_inf"].item, 0) is None and aff(by["inf_plus_inf"].item, 1) is None
    # degenerate exactly when an operand is at infinity or the x coordinates agree
    for c in adds:
        p1, p2 = aff(c.item, 0), aff(c.item, 1)
        assert c.degenerate == (p1 is None or p2 is None or p1[0] == p2[0]), c.name
    assert sum(not c.degenerate for c in adds) >= 4
    assert any(aff(c.item, 0) is None and c.expect is None for c in dbls)
    assert sum(c.expect is not None for c in dbls) >= 4
    for c in dbls:
        p1 = aff(c.item, 0)
        assert c.expect == (pr.g2_add(p1, p1) if F2 else pr.g1_add(p1, p1)), c.name
    if not F2:
        m = {c.name: c for c in madds}
        q = lambda c: (ac.fm(c.item[3]), ac.fm(c.item[4]))
        for c in madds:
            assert pr.g1_add(aff(c.item, 0), q(c)) == c.expect, c.name
        c = m["acc_equals_table_point"]
        assert aff(c.item, 0) == q(c) and nontrivial(zraw(c.item, 0)) and c.expect is not None
        c = m["acc_is_negated_table_point"]
        assert aff(c.item, 0) == pr.g1_neg(q(c)) and c.expect is None
        assert aff(m["acc_inf"].item, 0) is None


def test_group_cases_g1():
    _group_checks(False, ac.g1_cases())


def test_group_cases_g2():
    _group_checks(True, ac.g2_cases())


def test_references_on_known_values():
    """spot checks of the reference plumbing (Montgomery conversion, tower
    order) against values that need no device"""
    one = ac.RP
    assert ac.OPS[ac.OP_INDEX["fp_mul"]].ref((one, one)) == ([one], None)
    assert ac.OPS[ac.OP_INDEX["fp_neg"]].ref((0,)) == ([0], None)
    assert ac.OPS[ac.OP_INDEX["fp_add"]].ref((5, P - 5)) == ([0], None)
    assert ac.OPS[ac.OP_INDEX["fp_from_le48"]].ref((P,)) == ([0], 0)
    assert ac.OPS[ac.OP_INDEX["fp_from_le48"]].ref((1,)) == ([one], 1)
    assert ac.OPS[ac.OP_INDEX["fp_to_mont"]].ref((1,)) == ([one], None)
    assert ac.OPS[ac.OP_INDEX["fp_from_mont"]].ref((one,)) == ([1], None)
    one12 = tuple(ac.f12_raw(pr.F12_ONE))
    assert one12 == (one,) + (0,) * 11
    x = ac.f12_unary()[-1]
    assert ac.OPS[ac.OP_INDEX["fp12_mul"]].ref(x + one12) == (list(x), None)
    # a line with only c0 = 1 is the identity; pack / unpack round trip
    line_one = (one, 0, 0, 0, 0, 0)
    assert ac.OPS[ac.OP_INDEX["fp12_mul_line"]].ref(x + line_one) == (list(x), None)
    assert ac.unpack(ac.pack([x]), 12) == [list(x)]
