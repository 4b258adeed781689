"""Executable spec for the homogeneous-projective Miller steps and the
two-line fold used by miller_loop2 in harmony_amd/csrc/hbls_dev.hip
(DESIGN.md §4c).  CPU only: the device formulas are transcribed one to one
over the oracle's field ops and checked against the oracle's generic Fp12
arithmetic and its textbook pairing."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402

P = pr.P
INV2 = (P + 1) // 2


def f2_half(x):
    return (x[0] * INV2 % P, x[1] * INV2 % P)


def f2_dbl(x):
    return pr.f2_add(x, x)


def f2_tpl(x):
    return pr.f2_add(f2_dbl(x), x)


def dbl_step(T, Pa):
    """ml_dbl_step_h: 3 mul + 6 sqr + 2 mul_fp.  Returns (T', (c0, c3, c5))."""
    X, Y, Z = T
    xP, yP = Pa
    A = f2_half(pr.f2_mul(X, Y))
    B = pr.f2_sqr(Y)
    C = pr.f2_sqr(Z)
    E = f2_tpl(f2_dbl(f2_dbl(pr.f2_mul_xi(C))))      # 3 b' C, b' = 4 xi
    F = f2_tpl(E)
    G = f2_half(pr.f2_add(B, F))
    H = pr.f2_sub(pr.f2_sqr(pr.f2_add(Y, Z)), pr.f2_add(B, C))
    XX = pr.f2_sqr(X)
    c0 = pr.f2_mul_xi(pr.f2_muls(H, yP))
    c3 = pr.f2_sub(B, E)
    c5 = pr.f2_neg(pr.f2_muls(f2_tpl(XX), xP))
    X3 = pr.f2_mul(A, pr.f2_sub(B, F))
    Y3 = pr.f2_sub(pr.f2_sqr(G), f2_tpl(pr.f2_sqr(E)))
    Z3 = pr.f2_mul(B, H)
    return (X3, Y3, Z3), (c0, c3, c5)


def add_step(T, Q, Pa):
    """ml_add_step_h: mixed addition with affine Q."""
    X, Y, Z = T
    x2, y2 = Q
    xP, yP = Pa
    th = pr.f2_sub(Y, pr.f2_mul(y2, Z))
    la = pr.f2_sub(X, pr.f2_mul(x2, Z))
    c0 = pr.f2_mul_xi(pr.f2_muls(la, yP))
    c3 = pr.f2_sub(pr.f2_mul(x2, th), pr.f2_mul(y2, la))
    c5 = pr.f2_neg(pr.f2_muls(th, xP))
    C = pr.f2_sqr(th)
    D = pr.f2_sqr(la)
    E = pr.f2_mul(la, D)
    F = pr.f2_mul(Z, C)
    G = pr.f2_mul(X, D)
    H = pr.f2_sub(pr.f2_add(E, F), f2_dbl(G))
    X3 = pr.f2_mul(la, H)
    Y3 = pr.f2_sub(pr.f2_mul(th, pr.f2_sub(G, H)), pr.f2_mul(E, Y))
    Z3 = pr.f2_mul(Z, E)
    return (X3, Y3, Z3), (c0, c3, c5)


class Counter:
    """counts fp2 multiplies so the 6 + 17 structure is asserted, not assumed"""

    def __init__(self):
        self.n = 0

    def mul(self, x, y):
        self.n += 1
        return pr.f2_mul(x, y)


def f6_mul_counted(k, a, b):
    a0, a1, a2 = a
    b0, b1, b2 = b
    t0 = k.mul(a0, b0)
    t1 = k.mul(a1, b1)
    t2 = k.mul(a2, b2)
    c0 = pr.f2_add(t0, pr.f2_mul_xi(pr.f2_sub(pr.f2_sub(
        k.mul(pr.f2_add(a1, a2), pr.f2_add(b1, b2)), t1), t2)))
    c1 = pr.f2_add(pr.f2_sub(pr.f2_sub(
        k.mul(pr.f2_add(a0, a1), pr.f2_add(b0, b1)), t0), t1), pr.f2_mul_xi(t2))
    c2 = pr.f2_add(pr.f2_sub(pr.f2_sub(
        k.mul(pr.f2_add(a0, a2), pr.f2_add(b0, b2)), t0), t2), t1)
    return (c0, c1, c2)


def mul_line2(f, l1, l2, k=None):
    """fp12_mul_line2: f * l1 * l2 for lines c0 + (c3 v + c5 v^2) w.
    6 fp2-mul for the line product m = m0 + m1 w with m1 = (0, x, y), then
    f0*m0 (6), f1*m1 (5, Karatsuba on the 2-sparse operand) and
    (f0+f1)(m0+m1) (6)."""
    k = k or Counter()
    a0, a3, a5 = l1
    b0, b3, b5 = l2
    p00 = k.mul(a0, b0)
    p33 = k.mul(a3, b3)
    p55 = k.mul(a5, b5)
    cross = pr.f2_sub(pr.f2_sub(k.mul(pr.f2_add(a3, a5), pr.f2_add(b3, b5)), p33), p55)
    m0 = (pr.f2_add(p00, pr.f2_mul_xi(p33)), pr.f2_mul_xi(cross), pr.f2_mul_xi(p55))
    x = pr.f2_sub(pr.f2_sub(k.mul(pr.f2_add(a0, a3), pr.f2_add(b0, b3)), p00), p33)
    y = pr.f2_sub(pr.f2_sub(k.mul(pr.f2_add(a0, a5), pr.f2_add(b0, b5)), p00), p55)
    f0, f1 = f
    t0 = f6_mul_counted(k, f0, m0)
    g0, g1, g2 = f1
    q1 = k.mul(g1, x)
    q2 = k.mul(g2, y)
    q3 = pr.f2_sub(pr.f2_sub(k.mul(pr.f2_add(g1, g2), pr.f2_add(x, y)), q1), q2)
    t1 = (pr.f2_mul_xi(q3),
          pr.f2_add(k.mul(g0, x), pr.f2_mul_xi(q2)),
          pr.f2_add(k.mul(g0, y), q1))
    m01 = (m0[0], pr.f2_add(m0[1], x), pr.f2_add(m0[2], y))
    tt = f6_mul_counted(k, pr.f6_add(f0, f1), m01)
    c1 = pr.f6_sub(pr.f6_sub(tt, t0), t1)
    c0 = pr.f6_add(t0, pr.f6_mul_v(t1))
    return (c0, c1)


def line_f12(l):
    c0, c3, c5 = l
    z = (0, 0)
    return ((c0, z, z), (z, c3, c5))


def miller_loop2(Q1, P1, Q2, P2):
    T1 = (Q1[0], Q1[1], (1, 0))
    T2 = (Q2[0], Q2[1], (1, 0))
    f = pr.F12_ONE
    for bit in bin(-pr.Z)[3:]:
        f = pr.f12_sqr(f)
        T1, l1 = dbl_step(T1, P1)
        T2, l2 = dbl_step(T2, P2)
        f = mul_line2(f, l1, l2)
        if bit == "1":
            T1, l1 = add_step(T1, Q1, P1)
            T2, l2 = add_step(T2, Q2, P2)
            f = mul_line2(f, l1, l2)
    return T1, T2, f


def verdict(pub, hm, sig):
    """verify_pairing: e(pub, hm) * e(-base, sig) == 1"""
    _, _, f = miller_loop2(hm, pub, sig, pr.g1_neg(pr.HERUMI_G1))
    f = pr.f12_conj(f)
    return pr.f12_pow(f, pr.FINAL_EXP) == pr.F12_ONE


def _rand_f2(seed):
    import hashlib
    h = lambda t: int.from_bytes(hashlib.sha512(b"%s%d" % (t, seed)).digest(), "big") % P
    return (h(b"a"), h(b"b"))


@pytest.fixture(scope="module")
def signed():
    msg = pr.construct_commit_payload(5, pr.synth_msg(5), 6)
    sk = pr.synth_sk(3)
    hm = pr.hash_to_g2(msg)
    return pr.get_public_key(sk), pr.get_public_key(pr.synth_sk(4)), hm, pr.g2_mul(hm, sk)


def test_fold_equals_generic_product():
    for seed in range(4):
        f = (tuple(_rand_f2(100 * seed + i) for i in range(3)),
             tuple(_rand_f2(100 * seed + 3 + i) for i in range(3)))
        l1 = tuple(_rand_f2(100 * seed + 10 + i) for i in range(3))
        l2 = tuple(_rand_f2(100 * seed + 20 + i) for i in range(3))
        k = Counter()
        got = mul_line2(f, l1, l2, k)
        assert k.n == 6 + 17
        assert got == pr.f12_mul(pr.f12_mul(f, line_f12(l1)), line_f12(l2))


def test_fold_from_one():
    l1 = tuple(_rand_f2(i) for i in range(3))
    l2 = tuple(_rand_f2(7 + i) for i in range(3))
    assert mul_line2(pr.F12_ONE, l1, l2) == pr.f12_mul(line_f12(l1), line_f12(l2))


def test_steps_track_the_group_law(signed):
    """T stays [k]Q in homogeneous coordinates through doublings and additions"""
    pub, _, hm, _ = signed
    T = (hm[0], hm[1], (1, 0))
    T, _ = dbl_step(T, pub)
    T, _ = add_step(T, hm, pub)
    T, _ = dbl_step(T, pub)
    zi = pr.f2_inv(T[2])
    assert (pr.f2_mul(T[0], zi), pr.f2_mul(T[1], zi)) == pr.g2_mul(hm, 6)


def test_loop_end_point(signed):
    pub, _, hm, sig = signed
    T1, T2, _ = miller_loop2(hm, pub, sig, pr.g1_neg(pr.HERUMI_G1))
    for T, q in ((T1, hm), (T2, sig)):
        zi = pr.f2_inv(T[2])
        assert (pr.f2_mul(T[0], zi), pr.f2_mul(T[1], zi)) == pr.g2_mul(q, -pr.Z)


def test_verdicts_match_reference(signed):
    pub, other, hm, sig = signed
    assert pr.verify_pairing_eq(pub, hm, sig) is True
    assert verdict(pub, hm, sig) is True
    assert pr.verify_pairing_eq(other, hm, sig) is False
    assert verdict(other, hm, sig) is False
