"""Inputs and expected results for the stage probe (hbls_probe.inc,
DESIGN.md §4j): the two byte-to-point stages at the head of every verify
pipeline, hash-to-G2 and G2 decompress with its subgroup check.  Plain
Python, no GPU import; everything comes from oracle/pyref.py and a fixed
seed, built once per process.

tests/test_stage_cases.py asserts from the reference alone that the sets
cover what they claim; tests/test_stage_probe_gpu.py runs them on both
kernels of each stage.

The low-order points are the adversarial inputs of the decompress stage: a
signature is attacker-chosen bytes, and #E'(Fp2) = h2 r with
h2 = 13^2 23^2 2713 11953 262069 q, so curve points of those small orders
exist and are cheap to build: multiply any curve point by #E'/m (by #E'/m^2
for m = 13, 23, whose parts are not cyclic: #E'/13 kills every point)."""
import functools
import os
import random
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import pyref as pr  # noqa: E402
from arith_cases import tm  # noqa: E402  (field element -> device Montgomery limbs)

P = pr.P
INV2 = (P + 1) // 2
U = -pr.Z                        # |z|, the scalar of cv_g2_mul_u
N = 64                           # payloads / signatures of the square-root path sets
SEED = "hbls-stage-cases-1"
ORDER_E2 = pr.H2 * pr.R          # #E'(Fp2)
LOW_ORDERS = (13, 23, 2713, 11953, 262069)
H2_Q = pr.H2 // (13 ** 2 * 23 ** 2 * 2713 * 11953 * 262069)     # the 448-bit rest of h2
ORDER_E1 = pr.H1 * pr.R          # #E(Fp)
G1_LOW_ORDERS = (11, 10177)      # h1 = 3 11^2 10177^2 ...; order 3 is (0, +-2)


def rng(tag):
    return random.Random("%s:%s" % (SEED, tag))


# ------------------------------------------------------- path classification
def sqrt_branch(x):
    """0: (a+w)/2 is the square; 1: (a-w)/2 is (pyref.f2_sqrt, b != 0 path)"""
    a, b = x
    assert b != 0
    w = pr.fp_sqrt((a * a + b * b) % P)
    assert w is not None
    return 0 if pr.fp_sqrt((a + w) * INV2 % P) is not None else 1


def g2_rhs(x):
    return pr.f2_add(pr.f2_mul(pr.f2_sqr(x), x), pr.B2)


def classify_map(msg):
    """(candidate index, sqrt branch) that pyref.ft_map_g2 takes for msg"""
    t2 = (pr.set_array_mask(msg), 0)
    w = pr.f2_add(pr.f2_sqr(t2), pr.B2)
    w = ((w[0] + 1) % P, w[1])
    w = pr.f2_muls(pr.f2_mul(pr.f2_inv(w), t2), pr.FT_C1)
    x1 = pr.f2_neg(pr.f2_mul(t2, w))
    x1 = ((x1[0] + pr.FT_C2) % P, x1[1])
    x2 = pr.f2_neg(x1)
    x2 = ((x2[0] - 1) % P, x2[1])
    x3 = pr.f2_inv(pr.f2_sqr(w))
    x3 = ((x3[0] + 1) % P, x3[1])
    for i, x in enumerate((x1, x2, x3)):
        y2 = g2_rhs(x)
        if pr.f2_sqrt(y2) is not None:
            assert pr.ft_map_g2(t2)[0] == x
            return i, sqrt_branch(y2)
    raise AssertionError("no candidate")


def classify_sig(sig):
    """(sqrt branch, encoded parity, root flipped) of one compressed point"""
    odd = (sig[95] & 0x80) != 0
    raw = bytearray(sig)
    raw[95] &= 0x7F
    x = (int.from_bytes(raw[:48], "little"), int.from_bytes(raw[48:], "little"))
    y2 = g2_rhs(x)
    y = pr.f2_sqrt(y2)
    assert y is not None
    return sqrt_branch(y2), int(odd), int(bool(pr.f2_is_odd(y)) != odd)


# ---------------------------------------------------------------- hash cases
HashCase = namedtuple("HashCase", "name msg")
LENGTHS = (1, 31, 32, 47, 48, 49, 64)


@functools.lru_cache(None)
def payloads():
    """the 64 commit payloads of test_sqrt_paths_gpu.py (48 bytes each)"""
    return tuple(pr.construct_commit_payload(j, pr.synth_msg(j), j + 1) for j in range(N))


@functools.lru_cache(None)
def hash_map_cases():
    return tuple(HashCase("map%02d" % j, m) for j, m in enumerate(payloads()))


@functools.lru_cache(None)
def hash_length_cases():
    """one message per length.  The 48-, 49- and 64-byte ones share their
    first 48 bytes, whose byte 47 has its whole high nibble set: the 380-bit
    mask and the truncation at 48 bytes both change what is hashed."""
    r = rng("lengths")
    base = bytearray(r.getrandbits(8) | 1 for _ in range(48))
    base[47] |= 0xF0
    tail = bytes(r.getrandbits(8) | 1 for _ in range(16))
    out = []
    for n in LENGTHS:
        if n < 48:
            m = bytes(r.getrandbits(8) | 1 for _ in range(n))
        else:
            m = bytes(base) + tail[:n - 48]
        assert len(m) == n
        out.append(HashCase("len%d" % n, m))
    return tuple(out)


@functools.lru_cache(None)
def hash_zero_cases():
    """t == 0: the map has no image and the stage reports ok = 0"""
    return (HashCase("zero32", bytes(32)), HashCase("zero48", bytes(48)),
            HashCase("zero48_high_nibble", bytes(47) + b"\xf0"))


@functools.lru_cache(None)
def hash_cases():
    return hash_map_cases() + hash_length_cases() + hash_zero_cases()


@functools.lru_cache(None)
def hash_groups():
    """{message length: cases}: one probe call hashes messages of one length"""
    out = {}
    for c in hash_cases():
        out.setdefault(len(c.msg), []).append(c)
    return {k: tuple(v) for k, v in out.items()}


@functools.lru_cache(None)
def hash_expected(msg, fast):
    """(96 serialized bytes, ok) from pyref alone; zero bytes where ok is 0"""
    pt = pr.hash_to_g2(msg, fast_cofactor=fast)
    if pt is None:
        return bytes(96), 0
    return pr.g2_serialize(pt), 1


@functools.lru_cache(None)
def hash_pyref_picks():
    """names of the cases whose expected value the GPU test takes from pyref
    itself, not from the C oracle: the first payload of each map candidate,
    the shortest and the longest message, the masked 48-byte one and a
    t == 0 message"""
    first = {}
    for c in hash_map_cases():
        first.setdefault(classify_map(c.msg)[0], c.name)
    assert sorted(first) == [0, 1, 2]
    return tuple(first[i] for i in range(3)) + ("len1", "len48", "len64", "zero48")


# ---------------------------------------------------------- decompress cases
DecCase = namedtuple("DecCase", "name sig flag point")


def ref_decompress(sig):
    """(flag, affine point or None) of pyref.g2_deserialize with its full
    [r]Q membership test: 0 rejected, 1 a point, 2 the identity"""
    try:
        pt = pr.g2_deserialize(sig)
    except ValueError:
        return 0, None
    return (2, None) if pt is None else (1, pt)


def _case(name, sig):
    sig = bytes(sig)
    assert len(sig) == 96
    flag, pt = ref_decompress(sig)
    return DecCase(name, sig, flag, pt)


def aff_limbs(pt):
    """affine G2 point -> the probe's 4 raw Montgomery limbs values"""
    (xa, xb), (ya, yb) = pt
    return (tm(xa), tm(xb), tm(ya), tm(yb))


@functools.lru_cache(None)
def valid_sig_points():
    """the 64 signatures of test_sqrt_paths_gpu.py: key j signs payload j"""
    return tuple(pr.sign_hash(pr.synth_sk(j), m) for j, m in enumerate(payloads()))


@functools.lru_cache(None)
def valid_sigs():
    return tuple(pr.g2_serialize(s) for s in valid_sig_points())


@functools.lru_cache(None)
def dec_valid_cases():
    return tuple(_case("valid%02d" % j, s) for j, s in enumerate(valid_sigs()))


@functools.lru_cache(None)
def dec_identity_case():
    return _case("identity", bytes(96))


def _le48(v):
    return v.to_bytes(48, "little")


@functools.lru_cache(None)
def swept_points():
    """the first two curve points (c, 1), c = 1, 2, ... outside the subgroup
    (the sweep of test_g2_subgroup_method_equivalence) and the first such x
    whose right-hand side is no square"""
    pts, nonres, c = [], None, 1
    while len(pts) < 2 or nonres is None:
        x = (c, 1)
        y = pr.f2_sqrt(g2_rhs(x))
        if y is None:
            nonres = nonres or x
        elif len(pts) < 2 and pr.g2_mul((x, y), pr.R) is not None:
            pts.append((x, y))
        c += 1
    return tuple(pts), nonres


@functools.lru_cache(None)
def dec_boundary_cases():
    s = valid_sigs()[0]
    xa, xb = s[:48], s[48:]
    keep = bytes([xb[47] & 0x80])                   # the parity flag of byte 95
    (big, _), nonres = swept_points()
    out = [
        _case("xa_eq_p", _le48(P) + xb),
        _case("xa_eq_p_minus_1", _le48(P - 1) + xb),
        _case("xb_eq_p", xa + _le48(P)[:47] + bytes([_le48(P)[47] | keep[0]])),
        _case("byte47_bit7", xa[:47] + bytes([xa[47] | 0x80]) + xb),
        _case("x_zero", bytes(96)),
        _case("x_zero_parity", bytes(95) + b"\x80"),
        _case("rhs_non_residue", _le48(nonres[0]) + _le48(nonres[1])),
        _case("large_order_outside", pr.g2_serialize(big)),
    ]
    return tuple(out)


def low_order_point(base, m):
    """a point of exact order m on E'(Fp2) from a curve point base"""
    k = 2 if m in (13, 23) else 1
    t = pr.g2_mul(base, ORDER_E2 // m ** k)
    assert t is not None and pr.g2_mul(t, m) is None
    return t


@functools.lru_cache(None)
def low_order_points():
    """{name: (order, point)}: one point per order of LOW_ORDERS from the
    first swept point and a second point of order 13 from the next one"""
    (q1, q2), _ = swept_points()
    out = {"T%d" % m: (m, low_order_point(q1, m)) for m in LOW_ORDERS}
    out["T13b"] = (13, low_order_point(q2, 13))
    return out


def _flip_parity(sig):
    return sig[:95] + bytes([sig[95] ^ 0x80])


@functools.lru_cache(None)
def dec_low_order_cases():
    """every T, T13 + T23, every -T, and S + T for the valid signature S of
    index 0 in both parity encodings (the flipped one is -(S + T))"""
    ts = low_order_points()
    s0 = valid_sig_points()[0]
    out = [_case(n, pr.g2_serialize(t)) for n, (_m, t) in ts.items()]
    out.append(_case("T13+T23", pr.g2_serialize(pr.g2_add(ts["T13"][1], ts["T23"][1]))))
    out += [_case("-" + n, pr.g2_serialize(pr.g2_neg(t))) for n, (_m, t) in ts.items()]
    for n, (_m, t) in ts.items():
        enc = pr.g2_serialize(pr.g2_add(s0, t))
        out += [_case("S+" + n, enc), _case("-(S+%s)" % n, _flip_parity(enc))]
    return tuple(out)


@functools.lru_cache(None)
def dec_cases():
    return (dec_valid_cases() + (dec_identity_case(),) + dec_boundary_cases()
            + dec_low_order_cases())


def case_point(sig):
    """the curve point a compressed encoding stands for, subgroup or not"""
    return pr.g2_deserialize(sig, check_subgroup=False)


def chain_degenerates(pt):
    """Model of cv_g2_mul_u on one point: the double-and-add chain over the
    bits of |z| below the top one.  True if an addition meets an operand at
    infinity or two operands of equal x, the cases cv_g2_addj flags for the
    exact recompute.  A doubling never degenerates (no 2-torsion on E')."""
    acc = pt
    for bit in range(U.bit_length() - 2, -1, -1):
        acc = pr.g2_add(acc, acc)
        if (U >> bit) & 1:
            if acc is None or acc[0] == pt[0]:
                return True
            acc = pr.g2_add(acc, pt)
    assert acc == pr.g2_mul(pt, U)
    return False


# ------------------------------------------------------------- G1 low orders
@functools.lru_cache(None)
def g1_low_order_points():
    """{name: (order, point)} on E(Fp): (0, -2) of order 3 ((0, 2) serializes
    to the all-zero identity encoding) and one point each of order 11 and
    10177, from the first curve point x = 1, 2, ... outside the subgroup"""
    x = 1
    while True:
        y = pr.fp_sqrt((x * x * x + pr.B1) % P)
        if y is not None and pr.g1_mul((x, y), pr.R) is not None:
            break
        x += 1
    out = {"G1_T3": (3, (0, P - 2))}
    for m in G1_LOW_ORDERS:
        t = pr.g1_mul((x, y), ORDER_E1 // m ** 2)
        assert t is not None
        while pr.g1_mul(t, m) is not None:          # the m-part may be cyclic of order m^2
            t = pr.g1_mul(t, m)
        out["G1_T%d" % m] = (m, t)
    return out
