"""Verdict parity of the scalar (thread-per-item) pairing kernel k_verify on a
small mixed batch: the coop threshold is forced to 0 so the scalar kernel
runs at a batch the wave-cooperative kernel would normally take, and the
same batch through the cooperative kernel must agree."""
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

N = 16
BATCH = 8
BMLEN = (N + 7) // 8


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


def bitmap(signers):
    bm = bytearray(BMLEN)
    for i in signers:
        bm[i >> 3] |= 1 << (i & 7)
    return bytes(bm)


@pytest.fixture(scope="module")
def mixed_batch(core, capi):
    sks = [sk_bytes(i) for i in range(N)]
    pks = core.batch_pk_from_sk(b"".join(sks), N)
    msgs = [pr.construct_commit_payload(j, pr.synth_msg(j), j + 1) for j in range(BATCH)]

    def agg(signers, msg):
        return capi.aggregate_sigs([capi.sign_hash(sks[i], msg) for i in signers])

    sets = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10],
            [1, 3, 5, 7, 9, 11, 13, 15],
            [15],
            list(range(N))]
    items = [(bitmap(s), agg(s, msgs[j])) for j, s in enumerate(sets)]      # four valid
    s = [2, 4, 6, 8, 10, 12]
    items.append((bitmap(s[:-1] + [13]), agg(s, msgs[4])))                # wrong signer set
    items.append((bitmap(s), agg(s, msgs[0])))                            # wrong message
    items.append((bitmap(s), b"\x00" * 96))                               # identity sig, mask set
    items.append((bitmap([]), b"\x00" * 96))                              # empty mask + identity
    bms = b"".join(b for b, _ in items)
    sigs = b"".join(g for _, g in items)
    want = capi.Committee(pks, N).batch_agg_verify(bms, sigs, b"".join(msgs), 48, BATCH)
    return pks, bms, sigs, b"".join(msgs), want


def test_reference_verdicts(mixed_batch):
    # herumi: both-identity accepts; everything else about items 4..6 rejects
    assert mixed_batch[4] == [1, 1, 1, 1, 0, 0, 0, 1]


@pytest.mark.parametrize("threshold", [0, 10 ** 9], ids=["scalar", "coop"])
def test_mixed_batch_verdicts(core, mixed_batch, threshold):
    pks, bms, sigs, msgs, want = mixed_batch
    gc = core.Committee(pks, N)
    core.set_coop_threshold(threshold)
    try:
        got = gc.batch_agg_verify(bms, sigs, msgs, 48, BATCH)
    finally:
        core.set_coop_threshold(-1)
    assert got == want
