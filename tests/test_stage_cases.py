"""CPU checks of tests/stage_cases.py: the inputs of the stage probe must
cover what they claim.  Everything here follows from oracle/pyref.py alone:
every path is shown to occur, not assumed to, so a weak case set cannot hide
a device fault behind a passing GPU test."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stage_cases as sc  # noqa: E402
from oracle import pyref as pr  # noqa: E402

P = sc.P


# ------------------------------------------------------------------ hash
def test_hash_map_paths():
    cls = [sc.classify_map(c.msg) for c in sc.hash_map_cases()]
    assert len(cls) == 64
    cand = [sum(1 for c, _ in cls if c == i) for i in range(3)]
    branch = [sum(1 for _, b in cls if b == i) for i in range(2)]
    print("map candidates", cand, "sqrt branches", branch)
    assert min(cand) >= 8 and min(branch) >= 8
    assert all(len(c.msg) == 48 for c in sc.hash_map_cases())


def test_hash_lengths_mask_and_truncation():
    by = {len(c.msg): c.msg for c in sc.hash_length_cases()}
    assert sorted(by) == [1, 31, 32, 47, 48, 49, 64] == list(sc.LENGTHS)
    m48 = by[48]
    assert m48[47] & 0xF0 == 0xF0
    # the mask bites: the 48 bytes as an integer are not what is hashed, and
    # every bit of the high nibble matters
    t = pr.set_array_mask(m48)
    assert t == int.from_bytes(m48, "little") & ((1 << 380) - 1)
    assert t != int.from_bytes(m48, "little")
    assert t != int.from_bytes(m48, "little") & ((1 << 381) - 1)
    # truncation bites: the longer messages carry non-zero bytes past 48 and
    # hash like their first 48 bytes
    for n in (49, 64):
        assert by[n][:48] == m48 and all(by[n][48:])
        assert pr.set_array_mask(by[n]) == t
        assert int.from_bytes(by[n], "little") != int.from_bytes(m48, "little")
    assert sc.hash_expected(by[64], True) == sc.hash_expected(m48, True)
    # the short ones are zero padded: their last byte counts
    for n in (1, 31, 32, 47):
        assert by[n][-1] != 0 and pr.set_array_mask(by[n]) == int.from_bytes(by[n], "little")
    ts = [pr.set_array_mask(m) for m in by.values()]
    assert len(set(ts)) == 5 and 0 not in ts


def test_hash_zero_cases_fail_in_the_reference():
    zs = sc.hash_zero_cases()
    assert [len(c.msg) for c in zs] == [32, 48, 48]
    assert zs[0].msg == bytes(32) and zs[1].msg == bytes(48)
    assert zs[2].msg[:47] == bytes(47) and zs[2].msg[47] == 0xF0
    for c in zs:
        assert pr.set_array_mask(c.msg) == 0
        assert pr.ft_map_g2((0, 0)) is None
        for fast in (True, False):
            assert pr.hash_to_g2(c.msg, fast_cofactor=fast) is None
            assert sc.hash_expected(c.msg, fast) == (bytes(96), 0)


def test_hash_groups_and_picks():
    groups = sc.hash_groups()
    assert sorted(groups) == [1, 31, 32, 47, 48, 49, 64]
    assert sum(len(v) for v in groups.values()) == len(sc.hash_cases()) == 64 + 7 + 3
    assert len(groups[48]) == 64 + 1 + 2 and len(groups[32]) == 2
    names = [c.name for c in sc.hash_cases()]
    assert len(set(names)) == len(names)
    picks = sc.hash_pyref_picks()
    assert len(picks) >= 6 and set(picks) <= set(names)
    by = {c.name: c.msg for c in sc.hash_cases()}
    assert [sc.classify_map(by[n])[0] for n in picks[:3]] == [0, 1, 2]
    # the two cofactor modes give different points in the same subgroup
    fast, full = (pr.hash_to_g2(by[picks[0]], fast_cofactor=f) for f in (True, False))
    assert fast != full and pr.g2_in_subgroup(fast) and pr.g2_in_subgroup(full)


# ------------------------------------------------------------ decompress
def test_valid_signatures_cover_the_sqrt_paths():
    cases = sc.dec_valid_cases()
    assert len(cases) == 64
    cls = [sc.classify_sig(c.sig) for c in cases]
    for k, name in enumerate(("sqrt branch", "parity", "root flipped")):
        cnt = [sum(1 for c in cls if c[k] == v) for v in (0, 1)]
        print(name, cnt)
        assert min(cnt) >= 8, name
    for c, s in zip(cases, sc.valid_sig_points()):
        assert c.flag == 1 and c.point == s
    # Montgomery limbs of the expected point: v = x R mod p
    limbs = sc.aff_limbs(cases[0].point)
    rinv = pow(1 << 384, -1, P)
    assert tuple(v * rinv % P for v in limbs) == cases[0].point[0] + cases[0].point[1]


def test_identity_and_boundary_encodings():
    assert sc.dec_identity_case().sig == bytes(96) and sc.dec_identity_case().flag == 2
    by = {c.name: c for c in sc.dec_boundary_cases()}
    s = sc.valid_sigs()[0]
    le = lambda b: int.from_bytes(b, "little")
    assert le(by["xa_eq_p"].sig[:48]) == P and by["xa_eq_p"].sig[48:] == s[48:]
    assert le(by["xa_eq_p_minus_1"].sig[:48]) == P - 1
    xb = bytearray(by["xb_eq_p"].sig[48:])
    xb[47] &= 0x7F
    assert le(xb) == P and by["xb_eq_p"].sig[:48] == s[:48]
    assert by["byte47_bit7"].sig[47] == s[47] | 0x80 and s[47] & 0x80 == 0
    assert by["byte47_bit7"].sig[:47] + by["byte47_bit7"].sig[48:] == s[:47] + s[48:]
    assert by["x_zero"].sig == bytes(96)
    assert by["x_zero_parity"].sig == bytes(95) + b"\x80"
    x = (le(by["rhs_non_residue"].sig[:48]), le(by["rhs_non_residue"].sig[48:]))
    assert x[0] < P and x[1] < P and pr.f2_sqrt(sc.g2_rhs(x)) is None
    big = sc.case_point(by["large_order_outside"].sig)
    assert pr.g2_on_curve(big) and pr.g2_mul(big, pr.R) is not None
    # not of low order either: h2's cofactor part does not kill it
    assert pr.g2_mul(big, pr.H2 // sc.H2_Q) is not None
    # the flags are pyref's, whatever they are; these follow from the encoding
    for n in ("xa_eq_p", "xb_eq_p", "byte47_bit7", "rhs_non_residue", "large_order_outside"):
        assert by[n].flag == 0, n
    assert by["x_zero"].flag == 2
    print({n: c.flag for n, c in by.items()})
    assert all(c.flag == sc.ref_decompress(c.sig)[0] for c in by.values())


def test_cofactor_factorisation():
    assert pr.H2 == 13 ** 2 * 23 ** 2 * 2713 * 11953 * 262069 * sc.H2_Q
    assert sc.H2_Q.bit_length() == 448
    assert sc.ORDER_E2 == pr.H2 * pr.R
    assert all(sc.H2_Q % m for m in sc.LOW_ORDERS)


def test_low_order_points():
    ts = sc.low_order_points()
    assert sorted(m for m, _t in ts.values()) == sorted(sc.LOW_ORDERS + (13,))
    for name, (m, t) in ts.items():
        assert t is not None and pr.g2_on_curve(t), name
        assert pr.g2_mul(t, m) is None, name          # m prime: the order is exactly m
        assert pr.g2_mul(t, pr.R) is not None, name
    # the second point of order 13 is no multiple of the first: the 13-part
    # of E'(Fp2) is not cyclic
    t13, t13b = ts["T13"][1], ts["T13b"][1]
    assert all(pr.g2_mul(t13, k) != t13b for k in range(1, 13))


def test_low_order_cases():
    cases = sc.dec_low_order_cases()
    names = [c.name for c in cases]
    ts = sc.low_order_points()
    assert len(set(names)) == len(names) == 4 * len(ts) + 1
    assert len(set(c.sig for c in cases)) == len(cases)
    by = {c.name: c for c in cases}
    s0 = sc.valid_sig_points()[0]
    for n, (_m, t) in ts.items():
        assert sc.case_point(by[n].sig) == t
        assert sc.case_point(by["-" + n].sig) == pr.g2_neg(t)
        st = sc.case_point(by["S+" + n].sig)
        assert st == pr.g2_add(s0, t)
        assert sc.case_point(by["-(S+%s)" % n].sig) == pr.g2_neg(st)
        assert by["S+" + n].sig[:95] == by["-(S+%s)" % n].sig[:95]
        assert by["S+" + n].sig[95] ^ by["-(S+%s)" % n].sig[95] == 0x80
    assert sc.case_point(by["T13+T23"].sig) == pr.g2_add(ts["T13"][1], ts["T23"][1])
    # pyref's full [r]Q == infinity test rejects every one of them
    assert all(c.flag == 0 and c.point is None for c in cases)
    # and so does the psi criterion psi(Q) == [z]Q the device uses
    for n in ("T13", "T23", "T2713", "S+T13"):
        q = sc.case_point(by[n].sig)
        assert pr.g2_psi(q) != pr.g2_mul(q, pr.Z)


def test_chain_model_reaches_both_paths():
    """k_g2_decompress_coop judges a point on its straight path unless an
    addition of the |z| chain degenerates, and then on the scalar recompute:
    the low-order cases must reach both"""
    cases = sc.dec_low_order_cases()
    deg = [c.name for c in cases if sc.chain_degenerates(sc.case_point(c.sig))]
    straight = [c.name for c in cases if c.name not in deg]
    print("degenerate chains", len(deg), deg, "straight chains", len(straight))
    assert len(deg) >= 3 and len(straight) >= 3
    # order 13: the second addition of the chain is 12T + T
    assert sc.U >> 60 == 0b1101
    assert {"T13", "-T13", "T13b", "-T13b"} <= set(deg)
    assert {"T23", "T2713", "S+T13", "-(S+T13)"} <= set(straight)
    # no honest point degenerates
    assert not any(sc.chain_degenerates(c.point) for c in sc.dec_valid_cases()[:4])


def test_all_decompress_cases():
    cases = sc.dec_cases()
    assert len(cases) == 64 + 1 + 8 + len(sc.dec_low_order_cases())
    flags = [c.flag for c in cases]
    assert flags.count(1) >= 64 and flags.count(2) == 2 and flags.count(0) >= 30
    assert all((c.flag == 1) == (c.point is not None) for c in cases)


# -------------------------------------------------------------------- G1
def test_g1_low_order_points():
    assert pr.H1 % (3 * 11 ** 2 * 10177 ** 2) == 0
    ts = sc.g1_low_order_points()
    assert sorted(m for m, _t in ts.values()) == [3, 11, 10177]
    for name, (m, t) in ts.items():
        assert t is not None and pr.g1_on_curve(t), name
        assert pr.g1_mul(t, m) is None, name
        enc = pr.g1_serialize(t)
        assert enc != bytes(48), name
        try:
            pr.g1_deserialize(enc)
            raise AssertionError("pyref accepts " + name)
        except ValueError as e:
            assert "subgroup" in str(e), name
        assert pr.g1_deserialize(enc, check_subgroup=False) == t
    # the other point of order 3 has no encoding of its own
    assert pr.g1_on_curve((0, 2)) and pr.g1_mul((0, 2), 3) is None
    assert pr.g1_serialize((0, 2)) == bytes(48)
