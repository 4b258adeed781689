"""GPU parity for the Fp2 square-root paths of hash-to-G2 (map candidates
x1/x2/x3, both sqrt branches) and of G2 decompress (both sqrt branches, both
parities, root flipped or kept).  The inputs are classified with the
pure-Python oracle (tests/stage_cases.py) so that every path is shown to
occur, not assumed to.

Which kernel each test reaches: test_hash_to_g2_all_paths runs k_hash_to_g2
(hbls_batch_hash_to_g2 never takes the cooperative hash);
test_g2_decompress_all_paths runs g2_deserialize inside k_g2_addsub through
core.g2_add, and k_g2_decompress and k_g2_decompress_coop through the stage
probe; test_g2_check_mutated_encodings runs k_g2_check.  The cooperative
hash on the same payloads is in test_stage_probe_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import arith_cases as ac  # noqa: E402
import stage_cases as sc  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from stage_cases import classify_map, classify_sig, sqrt_branch  # noqa: E402,F401


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


def test_g2_decompress_all_paths(core, capi, sigs):
    cls = [classify_sig(s) for s in sigs]
    for k, name in enumerate(("sqrt branch", "parity", "root flipped")):
        cnt = [sum(1 for c in cls if c[k] == v) for v in (0, 1)]
        print(name, cnt)
        assert min(cnt) >= 8, name
    for k in range(N // 2):
        a, b = sigs[2 * k], sigs[2 * k + 1]
        assert core.g2_add(a, b) == capi.g2_add(a, b), k
    # the decompress kernels themselves, thread-per-item and cooperative:
    # flag and affine point of every signature against pyref.g2_deserialize
    cases = sc.dec_valid_cases()
    assert sigs == [c.sig for c in cases]
    for kernel, name in enumerate(core.STAGE_KERNELS):
        aff, flags = core.g2_decompress_probe(b"".join(sigs), N, kernel)
        assert flags == [1] * N, name
        for j, (c, got) in enumerate(zip(cases, ac.unpack(aff, 4))):
            assert tuple(got) == sc.aff_limbs(c.point), (name, j)


def test_g2_check_mutated_encodings(core, capi, sigs):
    for j in range(16):
        m = bytearray(sigs[j])
        m[(7 * j + 3) % 95] ^= 1 << (j % 8)      # an x bit, never the parity flag
        m = bytes(m)
        assert core.g2_check(m) == capi.g2_check(m), j
