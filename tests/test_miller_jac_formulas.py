"""Executable spec for the one-leg Miller loop on arguments that were never
made affine: miller_loop1_hj and ml_add_step_hj in
harmony_amd/csrc/hbls_dev.hip.  CPU only: the device formulas
are transcribed one to one over the oracle's field ops, next to the affine
loop of test_miller_formulas.py (§4c), and checked against it step by step
and against the oracle's textbook pairing.

G1, P = (x, y, z) Jacobian: xP = x/z^2, yP = y/z^3.  Every line is multiplied
by k = z^3, an element of Fp: the steps get (x z, y) = (xP k, yP k) in the
slots of (xP, yP), and c3, the one coefficient without a coordinate of P, is
multiplied by k.

G2, Q = (X, Y, Z) Jacobian: its homogeneous form is (X Z, Y, Z^3).  The loop
starts T there and the addition step adds that triple (X2, Y2, Z2) with
  theta' = Y Z2 - Y2 Z = Z2 theta,   lambda' = X Z2 - X2 Z = Z2 lambda,
where theta, lambda are ml_add_step_h's on the affine point (X2/Z2, Y2/Z2).
Its line is ml_add_step_h's scaled by Z2^2, its point the same scaled by Z2^4.
All scale factors lie in Fp2, which the final exponentiation sends to one."""
import hashlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import pyref as pr  # noqa: E402
from test_miller_formulas import add_step, dbl_step, f2_dbl, line_f12  # noqa: E402

P = pr.P
ONE2 = (1, 0)


class Count:
    """fp2 multiplications and squarings of a step, so that the five extra
    multiplications of the full addition are asserted, not assumed"""

    def __init__(self):
        self.mul = self.sqr = self.muls = 0

    def m(self, x, y):
        self.mul += 1
        return pr.f2_mul(x, y)

    def s(self, x):
        self.sqr += 1
        return pr.f2_sqr(x)

    def ms(self, x, k):
        self.muls += 1
        return pr.f2_muls(x, k)


def add_step_hj(T, Q2, Pp, k, n=None):
    """ml_add_step_hj: full addition with homogeneous Q2; Pp = (xP k, yP k)"""
    n = n or Count()
    X, Y, Z = T
    X2, Y2, Z2 = Q2
    xk, yk = Pp
    yz = n.m(Y, Z2)
    th = pr.f2_sub(yz, n.m(Y2, Z))
    xz = n.m(X, Z2)
    la = pr.f2_sub(xz, n.m(X2, Z))
    zz = n.m(Z, Z2)
    c0 = pr.f2_mul_xi(n.ms(n.m(la, Z2), yk))
    c3 = n.ms(pr.f2_sub(n.m(X2, th), n.m(Y2, la)), k)
    c5 = pr.f2_neg(n.ms(n.m(th, Z2), xk))
    C = n.s(th)
    D = n.s(la)
    E = n.m(la, D)
    F = n.m(zz, C)
    G = n.m(xz, D)
    H = pr.f2_sub(pr.f2_add(E, F), f2_dbl(G))
    X3 = n.m(la, H)
    Y3 = pr.f2_sub(n.m(th, pr.f2_sub(G, H)), n.m(E, yz))
    Z3 = n.m(zz, E)
    return (X3, Y3, Z3), (c0, c3, c5)


def loop_hj(Qj, Pj):
    """miller_loop1_hj; returns (f, [T after every step])"""
    x, y, z = Pj
    k = z * z % P * z % P
    Pp = (x * z % P, y)
    X, Y, Z = Qj
    Q2 = (pr.f2_mul(X, Z), Y, pr.f2_mul(pr.f2_sqr(Z), Z))
    T = Q2
    f = pr.F12_ONE
    trail = []
    for bit in bin(-pr.Z)[3:]:
        f = pr.f12_sqr(f)
        T, (c0, c3, c5) = dbl_step(T, Pp)
        f = pr.f12_mul(f, line_f12((c0, pr.f2_muls(c3, k), c5)))
        trail.append(T)
        if bit == "1":
            T, l = add_step_hj(T, Q2, Pp, k)
            f = pr.f12_mul(f, line_f12(l))
            trail.append(T)
    return f, trail


def loop_h(Q, Pa):
    """miller_loop1_h (hbls_aggrlc.inc): one leg of test_miller_formulas'
    miller_loop2, line by line"""
    T = (Q[0], Q[1], ONE2)
    f = pr.F12_ONE
    trail = []
    for bit in bin(-pr.Z)[3:]:
        f = pr.f12_sqr(f)
        T, l = dbl_step(T, Pa)
        f = pr.f12_mul(f, line_f12(l))
        trail.append(T)
        if bit == "1":
            T, l = add_step(T, Q, Pa)
            f = pr.f12_mul(f, line_f12(l))
            trail.append(T)
    return f, trail


def _h(tag, seed):
    return int.from_bytes(hashlib.sha512(b"%s%d" % (tag, seed)).digest(), "big") % P


def jac1(p, z):
    return (p[0] * z * z % P, p[1] * z * z % P * z % P, z)


def jac2(q, z):
    z2 = pr.f2_sqr(z)
    return (pr.f2_mul(q[0], z2), pr.f2_mul(q[1], pr.f2_mul(z2, z)), z)


def same_point(T, U):
    """equal as homogeneous projective points"""
    return (pr.f2_mul(T[0], U[2]) == pr.f2_mul(U[0], T[2])
            and pr.f2_mul(T[1], U[2]) == pr.f2_mul(U[1], T[2])
            and T[2] != (0, 0) and U[2] != (0, 0))


@pytest.fixture(scope="module")
def pairs():
    """two (H, pk) pairs with the affine loop's trail and the pairing, cubed"""
    out = []
    for i in range(2):
        hm = pr.hash_to_g2(pr.synth_msg(40 + i))
        pk = pr.get_public_key(pr.synth_sk(60 + i))
        f, trail = loop_h(hm, pk)
        e = pr.pairing(hm, pk)
        out.append((hm, pk, f, trail, e, pr.f12_pow(e, 3)))
    return out


def test_affine_loop_is_the_pairing(pairs):
    for hm, pk, f, trail, e, e3 in pairs:
        assert pr.f12_pow(pr.f12_conj(f), pr.FINAL_EXP) == e
        assert len(trail) == 63 + 5


# (Z of Q, Z of P): one on both sides, random on either side, on both
ZS = [("one", "one"), ("rand", "one"), ("one", "rand"), ("rand", "rand")]


@pytest.mark.parametrize("item", [0, 1])
@pytest.mark.parametrize("zq,zp", ZS, ids=["%s-%s" % z for z in ZS])
def test_jacobian_loop(pairs, item, zq, zp):
    hm, pk, f_h, trail_h, e, e3 = pairs[item]
    z2 = ONE2 if zq == "one" else (_h(b"zq-a", item), _h(b"zq-b", item))
    z1 = 1 if zp == "one" else _h(b"zp", item)
    assert z2 != (0, 0) and z1 != 0
    f, trail = loop_hj(jac2(hm, z2), jac1(pk, z1))
    assert len(trail) == len(trail_h)
    for T, U in zip(trail, trail_h):
        assert same_point(T, U)
    g = pr.f12_pow(pr.f12_conj(f), pr.FINAL_EXP)
    assert g == e
    assert pr.f12_pow(g, 3) == e3           # what the device's chain computes (§4j)
    if (zq, zp) == ("one", "one"):
        assert f == f_h                     # no scale at all: the same lines


def test_addition_costs_five_more_multiplications(pairs):
    """ml_add_step_h is 11 mul + 2 sqr + 2 mul_fp; the full addition is 16 mul
    + 2 sqr + 3 mul_fp (the third scales c3 by k)"""
    hm, pk = pairs[0][0], pairs[0][1]
    z2 = (_h(b"c-a", 0), _h(b"c-b", 0))
    Q2 = (pr.f2_mul(hm[0], z2), pr.f2_mul(hm[1], z2), z2)
    T, _ = dbl_step(Q2, pk)
    n = Count()
    T1, l1 = add_step_hj(T, Q2, pk, 1, n)
    assert (n.mul, n.sqr, n.muls) == (11 + 5, 2, 3)
    T0, l0 = add_step(T, hm, pk)
    assert same_point(T1, T0)
    # line and point scales: Z2^2 and Z2^4
    s2 = pr.f2_sqr(z2)
    s4 = pr.f2_sqr(s2)
    assert l1 == tuple(pr.f2_mul(c, s2) for c in l0)
    assert T1 == tuple(pr.f2_mul(c, s4) for c in T0)


def test_end_point(pairs):
    hm, pk = pairs[1][0], pairs[1][1]
    _, trail = loop_hj(jac2(hm, (_h(b"e-a", 1), _h(b"e-b", 1))), jac1(pk, _h(b"e", 1)))
    X, Y, Z = trail[-1]
    zi = pr.f2_inv(Z)
    assert (pr.f2_mul(X, zi), pr.f2_mul(Y, zi)) == pr.g2_mul(hm, -pr.Z)
