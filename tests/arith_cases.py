"""Operand sets and big-integer references for the device arithmetic probe
(harmony_amd/csrc/hbls_probe.inc).  Plain Python, no GPU
import; everything is generated from a fixed seed.

Operands cross to the device as RAW device-domain limbs: an Fp value v < p
stands for the field element v / R mod p (R = 2^384, Montgomery form), so
the case sets below choose LIMB PATTERNS directly.  A reference takes one
item (a tuple of raw integers), converts with x = v R^-1, computes in
oracle/pyref.py's plain integers and converts back with v = x R.

tests/test_arith_cases.py asserts from the reference alone that the sets
hit the edges they are meant to hit; tests/test_arith_probe_gpu.py runs
them on the device."""
import functools
import os
import random
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import pyref as pr  # noqa: E402
from test_miller_formulas import line_f12  # noqa: E402  (placement of c0, c3, c5)

P = pr.P
R = 1 << 384
RP = R % P                       # the field's 1 in device form
RINV = pow(R, -1, P)
PINV_R = pow(P, -1, R)
U = -pr.Z                        # |z| = 0xd201000000010000
SEED = "hbls-arith-cases-1"


def tm(x):
    """field element -> device limbs (Montgomery form)"""
    return x * R % P


def fm(v):
    """device limbs -> field element"""
    return v * RINV % P


def rng(tag):
    return random.Random("%s:%s" % (SEED, tag))


def premont(x, y):
    """the unique value a CIOS multiplier holds before its final conditional
    subtraction: t = (x y + m p) / R with m = -x y / p mod R"""
    m = (-x * y * PINV_R) % R
    t, rem = divmod(x * y + m * P, R)
    assert rem == 0
    return t


# ------------------------------------------------------------------ Fp pool
KS = tuple(range(32, 353, 32))
ALL_ONES = (0x1a0111e9 << 352) | ((1 << 352) - 1)        # every 32-bit limb ones, top 0x1a0111e9
ALT_EVEN = sum(0xffffffff << (32 * i) for i in range(0, 12, 2))   # limbs 0,2,..,10 ones, rest 0
# the other phase: limbs 1,3,..,9 ones; limb 11 cannot be ones below p, so it
# takes the largest top limb that keeps every lower pattern < p
ALT_ODD = sum(0xffffffff << (32 * i) for i in range(1, 11, 2)) | (0x1a0111e9 << 352)
FP_EDGES = ([0, 1, RP, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 380]
            + [(1 << k) - 1 for k in KS] + [P - (1 << k) for k in KS]
            + [ALL_ONES, ALT_EVEN, ALT_ODD])


@functools.lru_cache(None)
def fp_pool():
    r = rng("fp")
    pool = FP_EDGES + [r.randrange(P) for _ in range(64)]
    assert all(0 <= v < P for v in pool)
    return tuple(pool)


@functools.lru_cache(None)
def fp_unary():
    return tuple((v,) for v in fp_pool())


@functools.lru_cache(None)
def fp_addsub():
    """sums of exactly p, p-1 and p+1, differences of exactly 0"""
    out = []
    for x in fp_pool():
        out += [(x, (P - x) % P), (x, x), (x, P - 1 - x)]
        if x >= 2:
            out.append((x, P + 1 - x))
    r = rng("fp-addsub")
    pool = fp_pool()
    out += [(r.choice(pool), r.choice(pool)) for _ in range(32)]
    return tuple(out)


MUL_TARGETS = (0, 1, P - 1, (1 << 64) - 1, 1 << 380)


@functools.lru_cache(None)
def fp_mul():
    """for each raw target r and pool x != 0 the partner y = r R / x, so the
    device result is exactly r; then p-1 squared and seeded pairs"""
    out = []
    for r_ in MUL_TARGETS:
        for x in fp_pool():
            if x:
                out.append((x, r_ * R * pow(x, -1, P) % P))
    out.append((P - 1, P - 1))
    r = rng("fp-mul")
    pool = fp_pool()
    out += [(r.choice(pool), r.choice(pool)) for _ in range(32)]
    return tuple(out)


@functools.lru_cache(None)
def fp_inv():
    return tuple((v,) for v in fp_pool() if v)[:64]


@functools.lru_cache(None)
def fp_sqrt():
    """edges, squares of edges and seeded values: both outcomes occur"""
    r = rng("fp-sqrt")
    vals = [0, 1, RP, P - 1, tm(P - 1), (P - 1) // 2, 1 << 380, ALL_ONES, ALT_EVEN, ALT_ODD]
    vals += [tm(fm(v) ** 2 % P) for v in (P - 1, P - 2, ALL_ONES, 1 << 380, (1 << 64) - 1)]
    vals += [r.randrange(P) for _ in range(64 - len(vals))]
    return tuple((v,) for v in vals)


@functools.lru_cache(None)
def fp_le48_in():
    """plain integers as 48 little-endian bytes, >= p included"""
    big = [P, P + 1, P + (1 << 64), (1 << 381) - 1, 1 << 381, 1 << 383, (1 << 384) - 1,
           (0x1a0111ea << 352) | ((1 << 352) - 1), P | 0xffffffff]
    assert all(P <= v < R for v in big)
    return tuple((v,) for v in tuple(fp_pool()) + tuple(big))


# ------------------------------------------------------------------ Fp2 pool
F2_EDGE_COMP = (0, 1, P - 1, ALL_ONES)


@functools.lru_cache(None)
def f2_pool():
    r = rng("fp2")
    pool = [(a, b) for a in F2_EDGE_COMP for b in F2_EDGE_COMP]
    pool += [(r.randrange(P), r.randrange(P)) for _ in range(32)]
    return tuple(pool)


@functools.lru_cache(None)
def f2_unary():
    return tuple(x for x in f2_pool())


@functools.lru_cache(None)
def f2_binary():
    pool = f2_pool()
    out = [x + y for x in pool[:16] for y in pool[:16]]
    out += [pool[16 + i] + pool[16 + (i + 1) % 32] for i in range(32)]
    return tuple(out)


@functools.lru_cache(None)
def f2_mul():
    """f2_binary plus operands built for cvr_fp2_mul's third product, which
    multiplies the UNREDUCED sums a+b and c+d: both sums >= p, exactly one
    >= p, and the named worst case a = b = c = d = p-1 (in f2_binary)"""
    r = rng("fp2-mul")
    hi = lambda: r.randrange(P // 2 + 1, P)
    lo = lambda: r.randrange(0, P // 2)
    out = list(f2_binary())
    out += [(hi(), hi(), hi(), hi()) for _ in range(48)]
    out += [(hi(), hi(), lo(), lo()) for _ in range(12)]
    out += [(lo(), lo(), hi(), hi()) for _ in range(12)]
    out += [(P - 1, P - 1, hi(), lo()), (P - 1, P - 2, P - 2, P - 1)]
    return tuple(out)


CVR_WORST = (P - 1, P - 1, P - 1, P - 1)


@functools.lru_cache(None)
def f2_mul_fp():
    pool, fps = f2_pool(), fp_pool()
    out = [x + (s,) for x in pool[:16] for s in F2_EDGE_COMP]
    out += [x + (fps[(7 * i) % len(fps)],) for i, x in enumerate(pool)]
    return tuple(out)


@functools.lru_cache(None)
def f2_inv():
    return tuple(x for x in f2_pool() if x != (0, 0))


def f2_sqrt_class(x):
    """x a field element (not limbs).  b = 0: 'qr' / 'nqr' by a in Fp (every
    such x is a square in Fp2; the two classes are the two branches of the
    b = 0 path, root (s, 0) or (0, s)).  b != 0: 'sq' / 'nsq' in Fp2."""
    a, b = x
    if b == 0:
        return "qr" if pr.fp_sqrt(a) is not None else "nqr"
    return "sq" if pr.f2_sqrt(x) is not None else "nsq"


@functools.lru_cache(None)
def f2_sqrt():
    """0, -1, and at least 8 of each class of f2_sqrt_class; at most 64"""
    r = rng("fp2-sqrt")
    want = {"qr": 9, "nqr": 9, "sq": 12, "nsq": 12}
    out = [(0, 0), (P - 1, 0), (1, 0), (0, 1), (P - 1, P - 1), (1, P - 1)]
    for x in out:
        c = f2_sqrt_class(x)
        want[c] = max(0, want[c] - 1)
    while any(want.values()):
        x = (r.randrange(P), 0 if r.random() < 0.5 else r.randrange(P))
        c = f2_sqrt_class(x)
        if want[c]:
            want[c] -= 1
            out.append(x)
    # squares of edge-limb elements, so roots with extreme limbs occur too
    out += [pr.f2_sqr((fm(a), fm(b))) for a, b in ((P - 1, ALL_ONES), (ALL_ONES, 1), (1, P - 1))]
    assert len(out) <= 64
    return tuple((tm(a), tm(b)) for a, b in out)


# ------------------------------------------------------------------ Fp6 / Fp12
Z2 = (0, 0)
ONE2 = (RP, 0)
MAX2 = (P - 1, P - 1)


def _tower_elems(n, tag):
    """n fp2 coefficients: 0, 1, a single non-zero coefficient in each
    position, the upper half zero (the subfield below), all (p-1, p-1),
    16 seeded"""
    r = rng(tag)
    rf2 = lambda: (r.randrange(P), r.randrange(P))
    el = [(Z2,) * n, (ONE2,) + (Z2,) * (n - 1)]
    for i in range(n):
        el.append(tuple(rf2() if j == i else Z2 for j in range(n)))
    half = n // 2 if n == 6 else 1
    el.append(tuple(rf2() if j < half else Z2 for j in range(n)))
    el.append(tuple(MAX2 if j < half else Z2 for j in range(n)))
    if n == 3:
        el.append((rf2(), Z2, rf2()))            # c1 = 0
    el.append((MAX2,) * n)
    el += [tuple(rf2() for _ in range(n)) for _ in range(16)]
    return tuple(el)


def _flat(el):
    return tuple(c for f2 in el for c in f2)


@functools.lru_cache(None)
def f6_elems():
    return _tower_elems(3, "fp6")


@functools.lru_cache(None)
def f12_elems():
    return _tower_elems(6, "fp12")


def _pairs(elems):
    n = len(elems)
    out = []
    for i, e in enumerate(elems):
        out += [(e, elems[(3 * i + 1) % n]), (e, e), (e, elems[-17])]   # -17: all (p-1, p-1)
    return tuple(_flat(a) + _flat(b) for a, b in out)


@functools.lru_cache(None)
def f6_unary():
    return tuple(_flat(e) for e in f6_elems())


@functools.lru_cache(None)
def f6_binary():
    return _pairs(f6_elems())


@functools.lru_cache(None)
def f6_inv():
    return tuple(_flat(e) for e in f6_elems() if any(c != Z2 for c in e))


@functools.lru_cache(None)
def f12_unary():
    return tuple(_flat(e) for e in f12_elems())


@functools.lru_cache(None)
def f12_binary():
    return _pairs(f12_elems())


@functools.lru_cache(None)
def f12_inv():
    return tuple(_flat(e) for e in f12_elems() if any(c != Z2 for c in e))


@functools.lru_cache(None)
def _lines():
    r = rng("lines")
    rf2 = lambda: (r.randrange(P), r.randrange(P))
    ls = [(MAX2, MAX2, MAX2), (Z2, Z2, Z2), (ONE2, Z2, Z2), (Z2, rf2(), Z2), (Z2, Z2, rf2()),
          (rf2(), Z2, Z2), ((ALL_ONES, P - 1), (1, ALL_ONES), (P - 1, 0))]
    ls += [(rf2(), rf2(), rf2()) for _ in range(9)]
    return tuple(ls)


@functools.lru_cache(None)
def f12_line():
    ls = _lines()
    return tuple(_flat(e) + _flat(ls[i % len(ls)]) for i, e in enumerate(f12_elems())) + \
        tuple(_flat(f12_elems()[-1 - i]) + _flat(l) for i, l in enumerate(ls))


@functools.lru_cache(None)
def f12_line2():
    ls = _lines()
    n = len(ls)
    return tuple(_flat(e) + _flat(ls[i % n]) + _flat(ls[(5 * i + 3) % n])
                 for i, e in enumerate(f12_elems()))


def f12_of(v, i=0):
    """12 raw limbs values from v[i:] -> pyref Fp12"""
    c = [(fm(v[i + 2 * k]), fm(v[i + 2 * k + 1])) for k in range(6)]
    return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))


def f12_raw(x):
    return [tm(c) for half in x for f2 in half for c in f2]


def f6_of(v, i=0):
    return tuple((fm(v[i + 2 * k]), fm(v[i + 2 * k + 1])) for k in range(3))


def f6_raw(x):
    return [tm(c) for f2 in x for c in f2]


def f2_of(v, i=0):
    return (fm(v[i]), fm(v[i + 1]))


def f2_raw(x):
    return [tm(x[0]), tm(x[1])]


def f12_frob2(x):
    return pr.f12_frobenius(pr.f12_frobenius(x))


def easy_part(f):
    """f^((p^6-1)(p^2+1)): lands in the cyclotomic subgroup"""
    g = pr.f12_mul(pr.f12_conj(f), pr.f12_inv(f))
    return pr.f12_mul(f12_frob2(g), g)


@functools.lru_cache(None)
def f12_cyclotomic():
    """1 and the easy part of 8 seeded elements"""
    seeded = f12_elems()[-8:]
    out = [tuple(f12_raw(pr.F12_ONE))]
    out += [tuple(f12_raw(easy_part(f12_of(_flat(e))))) for e in seeded]
    return tuple(out)


@functools.lru_cache(None)
def final_exp_in():
    """1, an Fp2-subfield element, an Fp6-subfield element, a sparse element
    (line shaped), four seeded elements; none zero"""
    el = f12_elems()
    r = rng("fexp")
    rf2 = lambda: (r.randrange(P), r.randrange(P))
    sparse = (rf2(), Z2, Z2, Z2, rf2(), rf2())
    fp2sub = (rf2(),) + (Z2,) * 5
    fp6sub = (rf2(), rf2(), rf2(), Z2, Z2, Z2)
    picks = [el[1], fp2sub, fp6sub, sparse] + list(el[-4:])
    assert all(any(c != Z2 for c in e) for e in picks)
    return tuple(_flat(e) for e in picks)


@functools.lru_cache(None)
def final_exp_expected():
    """The device chain computes the CUBE of pyref's FINAL_EXP power (see
    test_arith_cases.test_final_exp_exponent).  About 0.4 s per element in
    pure Python: computed once per session, shared by the three
    implementations."""
    return tuple(tuple(f12_raw(pr.f12_pow(f12_of(v), 3 * pr.FINAL_EXP))) for v in final_exp_in())


# ------------------------------------------------------------------ group law
def _jac(F2, pt, z):
    """affine field-element point -> Jacobian raw limbs with the given Z (a
    field element); None -> infinity under an arbitrary x, y"""
    if F2:
        mul, sqr = pr.f2_mul, pr.f2_sqr
        x, y = pt
        z2 = sqr(z)
        X, Y = mul(x, z2), mul(y, mul(z2, z))
        return tuple(tm(c) for c in X + Y + z)
    x, y = pt
    return (tm(x * z * z % P), tm(y * z * z * z % P), tm(z))


def jac_to_affine(F2, v):
    """raw Jacobian limbs -> pyref affine point, None when Z == 0"""
    if F2:
        X, Y, Zc = f2_of(v, 0), f2_of(v, 2), f2_of(v, 4)
        if Zc == (0, 0):
            return None
        zi = pr.f2_inv(Zc)
        zi2 = pr.f2_sqr(zi)
        return (pr.f2_mul(X, zi2), pr.f2_mul(Y, pr.f2_mul(zi2, zi)))
    X, Y, Zc = fm(v[0]), fm(v[1]), fm(v[2])
    if Zc == 0:
        return None
    zi = pr.fp_inv(Zc)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


GroupCase = namedtuple("GroupCase", "name item expect degenerate")


def _group_cases(F2, tag):
    """(add cases, dbl cases, madd cases).  The same affine point appears
    under different Jacobian representatives (random non-trivial Z)."""
    r = rng(tag)
    if F2:
        gen, mul, add, neg = pr.G2_GEN, pr.g2_mul, pr.g2_add, pr.g2_neg
        rz = lambda: (r.randrange(1, P), r.randrange(1, P))
        one, zero = (1, 0), (0, 0)
        n = 6
    else:
        gen, mul, add, neg = pr.G1_GEN, pr.g1_mul, pr.g1_add, pr.g1_neg
        rz = lambda: r.randrange(2, P)
        one, zero = 1, 0
        n = 3
    pts = [mul(gen, r.randrange(2, pr.R)) for _ in range(5)]
    A, B, C, D, E = pts
    J = lambda pt, z: _jac(F2, pt, z)
    flat = (lambda pt: tuple(tm(c) for f in pt for c in f)) if F2 else \
        (lambda pt: tuple(tm(c) for c in pt))
    inf_std = flat((one, one, zero))                 # the library's own (1, 1, 0)
    inf_odd = flat((C[0], C[1], zero))               # x, y of a real point, Z = 0
    adds = [
        GroupCase("generic", J(A, rz()) + J(B, rz()), add(A, B), False),
        GroupCase("generic_z1_one", J(C, one) + J(D, rz()), add(C, D), False),
        GroupCase("generic_z2_one", J(D, rz()) + J(E, one), add(D, E), False),
        GroupCase("generic_both_one", J(A, one) + J(E, one), add(A, E), False),
        GroupCase("generic_neg", J(B, rz()) + J(neg(C), rz()), add(B, neg(C)), False),
        GroupCase("same_point_z_differs", J(A, rz()) + J(A, rz()), add(A, A), True),
        GroupCase("same_point_z_one", J(B, one) + J(B, rz()), add(B, B), True),
        GroupCase("negation_z_differs", J(A, rz()) + J(neg(A), rz()), None, True),
        GroupCase("negation_z_one", J(D, rz()) + J(neg(D), one), None, True),
        GroupCase("inf_plus_p", inf_std + J(B, rz()), B, True),
        GroupCase("p_plus_inf", J(B, rz()) + inf_std, B, True),
        GroupCase("inf_odd_plus_p", inf_odd + J(E, rz()), E, True),
        GroupCase("p_plus_inf_odd", J(E, rz()) + inf_odd, E, True),
        GroupCase("inf_plus_inf", inf_std + inf_odd, None, True),
    ]
    dbls = [GroupCase("dbl_%d" % i, J(p_, rz() if i else one), add(p_, p_), False)
            for i, p_ in enumerate(pts)]
    dbls += [GroupCase("dbl_inf", inf_std, None, True), GroupCase("dbl_inf_odd", inf_odd, None, True)]
    aff = flat
    madds = [
        GroupCase("generic", J(A, rz()) + aff(B), add(A, B), False),
        GroupCase("generic_z_one", J(C, one) + aff(D), add(C, D), False),
        GroupCase("acc_equals_table_point", J(B, rz()) + aff(B), add(B, B), True),
        GroupCase("acc_is_negated_table_point", J(neg(D), rz()) + aff(D), None, True),
        GroupCase("acc_inf", inf_std + aff(E), E, True),
        GroupCase("acc_inf_odd", inf_odd + aff(A), A, True),
    ]
    for c in adds + dbls + madds:
        assert all(0 <= v < P for v in c.item)
    assert all(len(c.item) == 2 * n for c in adds) and all(len(c.item) == n for c in dbls)
    return tuple(adds), tuple(dbls), tuple(madds)


@functools.lru_cache(None)
def g1_cases():
    return _group_cases(False, "g1")


@functools.lru_cache(None)
def g2_cases():
    return _group_cases(True, "g2")


# ------------------------------------------------------------------ references
# each takes one item (tuple of raw integers) and returns (raw outputs, flag
# or None).  Outputs are the exact wire integers the device must return.
def _fp1(f):
    return lambda v: ([tm(f(fm(v[0])))], None)


def _fp2_(f):
    return lambda v: ([tm(f(fm(v[0]), fm(v[1])))], None)


INV2 = (P + 1) // 2
ref_fp_mul = _fp2_(lambda x, y: x * y % P)


def ref_fp_sqrt(v):
    s = pr.fp_sqrt(fm(v[0]))
    return ([0 if s is None else tm(s)], int(s is not None))


def ref_fp_legendre(v):
    x = fm(v[0])
    return ([], 0 if x == 0 else (1 if pow(x, (P - 1) // 2, P) == 1 else -1))


def ref_fp_from_le48(v):
    return ([tm(v[0]) if v[0] < P else 0], int(v[0] < P))


def _f2u(f):
    return lambda v: (f2_raw(f(f2_of(v))), None)


def _f2b(f):
    return lambda v: (f2_raw(f(f2_of(v, 0), f2_of(v, 2))), None)


ref_fp2_mul = _f2b(pr.f2_mul)
ref_fp2_sqr = _f2u(pr.f2_sqr)


def ref_fp2_sqrt(v):
    s = pr.f2_sqrt(f2_of(v))
    return ([0, 0] if s is None else f2_raw(s), int(s is not None))


ref_fp6_mul = lambda v: (f6_raw(pr.f6_mul(f6_of(v, 0), f6_of(v, 6))), None)
ref_fp12_mul = lambda v: (f12_raw(pr.f12_mul(f12_of(v, 0), f12_of(v, 12))), None)


def _f12u(f):
    return lambda v: (f12_raw(f(f12_of(v))), None)


ref_fp12_sqr = _f12u(pr.f12_sqr)
ref_fp12_inv = _f12u(pr.f12_inv)
ref_fp12_frob = _f12u(pr.f12_frobenius)
ref_fp12_frob2 = _f12u(f12_frob2)
ref_fp12_pow_u = _f12u(lambda x: pr.f12_pow(x, U))


def _line_of(v, i):
    return line_f12((f2_of(v, i), f2_of(v, i + 2), f2_of(v, i + 4)))


ref_mul_line = lambda v: (f12_raw(pr.f12_mul(f12_of(v), _line_of(v, 12))), None)
ref_mul_line2 = lambda v: (f12_raw(pr.f12_mul(pr.f12_mul(f12_of(v), _line_of(v, 12)),
                                              _line_of(v, 18))), None)


def ref_final_exp(v):
    return (list(final_exp_expected()[final_exp_in().index(tuple(v))]), None)


# ------------------------------------------------------------------ the table
# name, fp elements in / out, base (the operation a † implementation must
# match byte for byte), case list, reference, kind:
#   exact  outputs and flag equal the reference's
#   any    fp2_sqrt_any: flag, r^2 == x and canonical form only
#   g1/g2  GroupCase lists; compared after normalising to affine
#   addj   g2 cases through cv_g2_addj: edge flag on every degenerate case,
#          on no generic one; result checked where the flag is clear
Op = namedtuple("Op", "name n_in n_out base cases ref kind")


def _op(name, n_in, n_out, cases, ref, base=None, kind="exact"):
    return Op(name, n_in, n_out, base, cases, ref, kind)


_g = lambda which, idx: (lambda: (g2_cases() if which == 2 else g1_cases())[idx])

OPS = (
    _op("fp_add", 2, 1, fp_addsub, _fp2_(lambda x, y: (x + y) % P)),
    _op("fp_sub", 2, 1, fp_addsub, _fp2_(lambda x, y: (x - y) % P)),
    _op("fp_neg", 1, 1, fp_unary, _fp1(lambda x: -x % P)),
    _op("fp_dbl", 1, 1, fp_unary, _fp1(lambda x: 2 * x % P)),
    _op("fp_half", 1, 1, fp_unary, _fp1(lambda x: x * INV2 % P)),
    _op("fp_mul", 2, 1, fp_mul, ref_fp_mul),
    _op("fp_mul_inl", 2, 1, fp_mul, ref_fp_mul, "fp_mul"),
    _op("fp_mul_c", 2, 1, fp_mul, ref_fp_mul, "fp_mul"),
    _op("fp_mul_asm", 2, 1, fp_mul, ref_fp_mul, "fp_mul"),
    _op("fp_mul_rs", 2, 1, fp_mul, ref_fp_mul, "fp_mul"),
    _op("fp_sqr", 1, 1, fp_unary, _fp1(lambda x: x * x % P)),
    _op("fp_inv", 1, 1, fp_inv, _fp1(pr.fp_inv)),
    _op("fp_sqrt", 1, 1, fp_sqrt, ref_fp_sqrt),
    _op("fp_legendre", 1, 0, fp_sqrt, ref_fp_legendre),
    _op("fp_is_odd", 1, 0, fp_unary, lambda v: ([], fm(v[0]) & 1)),
    _op("fp_to_mont", 1, 1, fp_unary, lambda v: ([tm(v[0])], None)),
    _op("fp_from_mont", 1, 1, fp_unary, lambda v: ([fm(v[0])], None)),
    _op("fp_from_le48", 1, 1, fp_le48_in, ref_fp_from_le48),
    _op("fp_to_le48", 1, 1, fp_unary, lambda v: ([fm(v[0])], None)),
    _op("fp2_add", 4, 2, f2_binary, _f2b(pr.f2_add)),
    _op("fp2_sub", 4, 2, f2_binary, _f2b(pr.f2_sub)),
    _op("fp2_neg", 2, 2, f2_unary, _f2u(pr.f2_neg)),
    _op("fp2_conj", 2, 2, f2_unary, _f2u(pr.f2_conj)),
    _op("fp2_half", 2, 2, f2_unary, _f2u(lambda x: pr.f2_muls(x, INV2))),
    _op("fp2_mul", 4, 2, f2_mul, ref_fp2_mul),
    _op("fp2_mul_ri", 4, 2, f2_mul, ref_fp2_mul, "fp2_mul"),
    _op("cvr_fp2_mul", 4, 2, f2_mul, ref_fp2_mul, "fp2_mul"),
    _op("fp2_sqr", 2, 2, f2_unary, ref_fp2_sqr),
    _op("cvr_fp2_sqr", 2, 2, f2_unary, ref_fp2_sqr, "fp2_sqr"),
    _op("fp2_mul_fp", 3, 2, f2_mul_fp, lambda v: (f2_raw(pr.f2_muls(f2_of(v), fm(v[2]))), None)),
    _op("fp2_mul_xi", 2, 2, f2_unary, _f2u(pr.f2_mul_xi)),
    _op("fp2_inv", 2, 2, f2_inv, _f2u(pr.f2_inv)),
    _op("fp2_sqrt", 2, 2, f2_sqrt, ref_fp2_sqrt),
    _op("fp2_sqrt_any", 2, 2, f2_sqrt, ref_fp2_sqrt, kind="any"),
    _op("fp6_mul", 12, 6, f6_binary, ref_fp6_mul),
    _op("fp6_mul_rs6", 12, 6, f6_binary, ref_fp6_mul, "fp6_mul"),
    _op("fp6_mul_v", 6, 6, f6_unary, lambda v: (f6_raw(pr.f6_mul_v(f6_of(v))), None)),
    _op("fp6_inv", 6, 6, f6_inv, lambda v: (f6_raw(pr.f6_inv(f6_of(v))), None)),
    _op("fp12_mul", 24, 12, f12_binary, ref_fp12_mul),
    _op("fp12_mul_6", 24, 12, f12_binary, ref_fp12_mul, "fp12_mul"),
    _op("fp12_sqr", 12, 12, f12_unary, ref_fp12_sqr),
    _op("fp12_sqr_6", 12, 12, f12_unary, ref_fp12_sqr, "fp12_sqr"),
    _op("fp12_inv", 12, 12, f12_inv, ref_fp12_inv),
    _op("fp12_conj", 12, 12, f12_unary, _f12u(pr.f12_conj)),
    _op("fp12_frob", 12, 12, f12_unary, ref_fp12_frob),
    _op("fp12_frob2", 12, 12, f12_unary, ref_fp12_frob2),
    _op("fp12_mul_line", 18, 12, f12_line, ref_mul_line),
    _op("fp12_mul_line_6", 18, 12, f12_line, ref_mul_line, "fp12_mul_line"),
    _op("fp12_mul_line2", 24, 12, f12_line2, ref_mul_line2),
    _op("fp12_cyc_sqr", 12, 12, f12_cyclotomic, ref_fp12_sqr),
    _op("fp12_pow_u", 12, 12, f12_cyclotomic, ref_fp12_pow_u),
    _op("fp12_pow_u_6", 12, 12, f12_cyclotomic, ref_fp12_pow_u, "fp12_pow_u"),
    _op("final_exp", 12, 12, final_exp_in, ref_final_exp),
    _op("final_exp_6", 12, 12, final_exp_in, ref_final_exp, "final_exp"),
    _op("g1_dbl", 3, 3, _g(1, 1), None, kind="g1"),
    _op("g1_add", 6, 3, _g(1, 0), None, kind="g1"),
    _op("g1_madd", 5, 3, _g(1, 2), None, kind="g1"),
    _op("g2_dbl", 6, 6, _g(2, 1), None, kind="g2"),
    _op("g2_add", 12, 6, _g(2, 0), None, kind="g2"),
    _op("cv_fp6_mul", 12, 6, f6_binary, ref_fp6_mul, "fp6_mul"),
    _op("cv_fp12_mul", 24, 12, f12_binary, ref_fp12_mul, "fp12_mul"),
    _op("cv_fp12_sqr", 12, 12, f12_unary, ref_fp12_sqr, "fp12_sqr"),
    _op("cv_fp12_inv_q0", 12, 12, f12_inv, ref_fp12_inv, "fp12_inv"),
    _op("cv_fp12_frob_q0", 12, 12, f12_unary, ref_fp12_frob, "fp12_frob"),
    _op("cv_fp12_frob2_q0", 12, 12, f12_unary, ref_fp12_frob2, "fp12_frob2"),
    _op("cv_fp12_mul_line", 18, 12, f12_line, ref_mul_line, "fp12_mul_line"),
    _op("cv_fp12_cyc_sqr", 12, 12, f12_cyclotomic, ref_fp12_sqr, "fp12_cyc_sqr"),
    _op("cv_pow_u", 12, 12, f12_cyclotomic, ref_fp12_pow_u, "fp12_pow_u"),
    _op("cv_final_exp", 12, 12, final_exp_in, ref_final_exp, "final_exp"),
    _op("cv_g2_dbl_plain", 6, 6, _g(2, 1), None, "g2_dbl", kind="g2"),
    _op("cv_g2_addj", 12, 6, _g(2, 0), None, "g2_add", kind="addj"),
)
OP_INDEX = {o.name: i for i, o in enumerate(OPS)}
COOP_OPS = tuple(o.name for o in OPS if o.name.startswith("cv_"))
COOP_COUNTS = (1, 15, 16, 17, 33)


def items_of(op):
    """the raw operand tuples of an operation (group ops: the cases' items)"""
    cs = op.cases()
    return tuple(c.item for c in cs) if op.kind in ("g1", "g2", "addj") else cs


def pack(items):
    return b"".join(v.to_bytes(48, "little") for it in items for v in it)


def unpack(buf, n_fp):
    """bytes -> list of per-item lists of n_fp integers"""
    vals = [int.from_bytes(buf[i:i + 48], "little") for i in range(0, len(buf), 48)]
    return [vals[i:i + n_fp] for i in range(0, len(vals), n_fp)] if n_fp else []
