"""GPU parity for the Fp2 square-root paths of the scalar (thread-per-item)
kernels: k_hash_to_g2 (map candidates x1/x2/x3, both sqrt branches) and
k_g2_decompress (both sqrt branches, both parities, root flipped or kept).
The inputs are classified with the pure-Python oracle so that every path is
shown to occur, not assumed to."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from oracle import pyref as pr  # noqa: E402


def _gpu_available():
    try:
        from harmony_amd import core
        return core.device_count() > 0
    except Exception:
        return False


if not os.environ.get("HBLS_FORCE_GPU_TESTS"):
    pytestmark = [pytest.mark.gpu,
                  pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]

N = 64
P = pr.P
INV2 = (P + 1) // 2


@pytest.fixture(scope="module")
def core():
    from harmony_amd import core as c
    c.init(-1 if c.device_count() == 0 else 0)
    return c


@pytest.fixture(scope="module")
def capi(oracle_lib):
    return oracle_lib


def sk_bytes(i):
    return pr.fr_serialize(pr.synth_sk(i))


@pytest.fixture(scope="module")
def payloads():
    return [pr.construct_commit_payload(j, pr.synth_msg(j), j + 1) for j in range(N)]


@pytest.fixture(scope="module")
def sigs(capi, payloads):
    return [capi.sign_hash(sk_bytes(j), payloads[j]) for j in range(N)]


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


def test_hash_to_g2_all_paths(core, capi, payloads):
    cls = [classify_map(m) for m in payloads]
    cand = [sum(1 for c, _ in cls if c == i) for i in range(3)]
    branch = [sum(1 for _, b in cls if b == i) for i in range(2)]
    print("map candidates", cand, "sqrt branches", branch)
    assert min(cand) >= 8 and min(branch) >= 8
    mlen = len(payloads[0])
    assert all(len(m) == mlen for m in payloads)
    for fast in (True, False):
        core.set_g2_cofactor_mode(fast)
        capi.set_g2_cofactor_mode(fast)
        try:
            got = core.batch_hash_to_g2(b"".join(payloads), mlen, N)
            for j, m in enumerate(payloads):
                assert got[96 * j:96 * j + 96] == capi.hash_to_g2(m), (fast, j)
        finally:
            core.set_g2_cofactor_mode(True)
            capi.set_g2_cofactor_mode(True)


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


def test_g2_decompress_all_paths(core, capi, sigs):
    cls = [classify_sig(s) for s in sigs]
    for k, name in enumerate(("sqrt branch", "parity", "root flipped")):
        cnt = [sum(1 for c in cls if c[k] == v) for v in (0, 1)]
        print(name, cnt)
        assert min(cnt) >= 8, name
    for k in range(N // 2):
        a, b = sigs[2 * k], sigs[2 * k + 1]
        assert core.g2_add(a, b) == capi.g2_add(a, b), k


def test_g2_check_mutated_encodings(core, capi, sigs):
    for j in range(16):
        m = bytearray(sigs[j])
        m[(7 * j + 3) % 95] ^= 1 << (j % 8)      # an x bit, never the parity flag
        m = bytes(m)
        assert core.g2_check(m) == capi.g2_check(m), j
