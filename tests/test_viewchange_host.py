"""harmony_amd.viewchange on the host: the collector, driven
through a backend over the CPU oracle, against a per-message restatement of
the reference's rule that makes one oracle call per check.  No GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from harmony_amd import viewchange as vcm  # noqa: E402
import viewchange_cases as vc  # noqa: E402


@pytest.fixture(scope="module")
def keys(oracle_lib):
    return vc.Keys(oracle_lib)


@pytest.fixture(scope="module")
def collected(oracle_lib, keys):
    """both batches through the collector and through the restatement, once"""
    backend = vc.OracleBackend(oracle_lib, keys)
    col = vcm.ViewChange(keys.pks_cat, vc.N, backend=backend)
    ref = vc.Restated(oracle_lib, keys)
    msgs, P, want = vc.first_batch(keys)
    codes = col.process(msgs)
    calls1 = dict(backend.calls)
    ref_codes = [ref.on_message(m) for m in msgs]
    msgs2 = vc.second_batch(keys, P)
    codes2 = col.process(msgs2)
    calls2 = dict(backend.calls)
    ref_codes2 = [ref.on_message(m) for m in msgs2]
    return dict(col=col, ref=ref, backend=backend, P=P, want=want, codes=codes,
                ref_codes=ref_codes, codes2=codes2, ref_codes2=ref_codes2,
                calls1=calls1, calls2=calls2)


def test_codes_follow_the_reference_order(collected):
    assert collected["ref_codes"] == collected["want"]
    assert collected["codes"] == collected["want"]
    assert collected["codes2"] == collected["ref_codes2"] == [vcm.VC_OK] * 3


def test_state_equals_the_restatement(collected):
    col, ref = collected["col"], collected["ref"]
    for view in (vc.VIEW, vc.VIEW2):
        assert col.bitmaps(view) == ref.bitmaps(view)
        assert col.get_m2_bitmap(view) == (ref.aggregate("m2", view), ref.bitmaps(view)[1])
        assert col.get_m3_bitmap(view) == (ref.aggregate("m3", view), ref.bitmaps(view)[2])
    assert col.bitmaps(vc.VIEW) == (vc.bitmap_of([0, 1, 3, 4, 7]), vc.bitmap_of([2, 8]),
                                    vc.bitmap_of([0, 1, 2, 3, 4, 7, 8]))
    assert col.m1_payload == ref.m1_payload == collected["P"]
    # the second view ID kept its own state
    assert col.bitmaps(vc.VIEW2) == (vc.bitmap_of([2]), vc.bitmap_of([0, 1]),
                                     vc.bitmap_of([0, 1, 2]))
    assert col.get_m2_bitmap(7) == (None, None) and col.get_m3_bitmap(7) == (None, None)


def test_one_backend_call_per_method_per_batch(collected):
    assert collected["calls1"] == {"verify_msgs": 1, "verify_seals": 1}
    # the second batch's only proof was accepted in the first: no seal call
    assert collected["calls2"] == {"verify_msgs": 2, "verify_seals": 1}


def test_message_table_holds_each_string_once(oracle_lib, keys):
    seen = {}

    class Spy(vc.OracleBackend):
        def verify_msgs(self, key_idx, sigs, msg_idx, msgs):
            seen.update(key_idx=list(key_idx), msg_idx=list(msg_idx), msgs=list(msgs))
            return super().verify_msgs(key_idx, sigs, msg_idx, msgs)

        def verify_seals(self, blobs, msgs, quorum):
            seen.update(blobs=list(blobs), quorum=quorum)
            return super().verify_seals(blobs, msgs, quorum)

    msgs, P, want = vc.first_batch(keys)
    col = vcm.ViewChange(keys.pks_cat, vc.N, backend=Spy(oracle_lib, keys))
    assert col.process(msgs) == want
    assert len(seen["key_idx"]) == 2 * 12           # sender 9 never reaches the backend
    assert len(set(seen["msgs"])) == len(seen["msgs"]) == 5
    assert set(seen["msgs"]) >= {vcm.NIL, vc.VIEW.to_bytes(8, "little"), P}
    assert seen["quorum"] is True and len(seen["blobs"]) == 3   # P, the 6-signer one, the bad one
    assert col.process([]) == [] and col.process([msgs[9]]) == [vcm.ERR_SENDER]


def test_verify_block_refusal_comes_before_the_m1_checks(oracle_lib, keys):
    msgs, P, _ = vc.first_batch(keys)
    col = vcm.ViewChange(keys.pks_cat, vc.N, backend=vc.OracleBackend(oracle_lib, keys),
                         verify_block=lambda payload: payload != P)
    codes = col.process(msgs[:4])
    assert codes == [vcm.ERR_BLOCK, vcm.ERR_BLOCK, vcm.VC_OK, vcm.ERR_BLOCK]
    assert col.bitmaps(vc.VIEW) == (bytes(2), vc.bitmap_of([2]), vc.bitmap_of([2]))
    assert col.m1_payload is None


def test_new_view(collected, keys):
    col, P = collected["col"], collected["P"]
    m3_sig, m3_bm = col.get_m3_bitmap(vc.VIEW)
    m2_sig, m2_bm = col.get_m2_bitmap(vc.VIEW)
    before = dict(collected["backend"].calls)
    assert col.verify_new_view(vc.VIEW, m3_sig, m3_bm, m2_sig, m2_bm, P) == vcm.NV_OK
    after = collected["backend"].calls
    assert after["verify_seals"] == before["verify_seals"] + 1
    assert after["verify_msgs"] == before["verify_msgs"]

    flipped = bytes([m3_bm[0] ^ 0x20, m3_bm[1]])
    vid = vc.VIEW.to_bytes(8, "little")
    few = list(range(6))
    few_sig, few_bm = keys.agg(few, vid), vc.bitmap_of(few)
    nv = col.verify_new_view
    assert nv(vc.VIEW, None, m3_bm, m2_sig, m2_bm, P) == vcm.NV_ERR_M3_MISSING
    assert nv(vc.VIEW, m3_sig, flipped, m2_sig, m2_bm, P) == vcm.NV_ERR_M3_SIG
    assert nv(vc.VIEW, few_sig, few_bm, m2_sig, m2_bm, P) == vcm.NV_ERR_M3_QUORUM
    assert nv(vc.VIEW, m3_sig, m3_bm, m3_sig, m2_bm, P) == vcm.NV_ERR_M2_SIG
    assert nv(vc.VIEW, m3_sig, m3_bm, m2_sig, m2_bm, P[:100]) == vcm.NV_ERR_M1_FORMAT
    # the first failure wins: M3 signature, M2 signature, M3 quorum, then M1
    assert nv(vc.VIEW, m3_sig, flipped, m3_sig, m2_bm, P[:100]) == vcm.NV_ERR_M3_SIG
    assert nv(vc.VIEW, few_sig, few_bm, m3_sig, m2_bm, P[:100]) == vcm.NV_ERR_M2_SIG
    assert nv(vc.VIEW, few_sig, few_bm, m2_sig, m2_bm, P[:100]) == vcm.NV_ERR_M3_QUORUM
    # M1 is due without an M2 part, and a wrong proof is a signature failure
    assert nv(vc.VIEW, m3_sig, m3_bm, None, None, P) == vcm.NV_OK
    wrong = P[:32] + keys.agg(range(7), vid) + P[128:]
    assert nv(vc.VIEW, m3_sig, m3_bm, None, None, wrong) == vcm.NV_ERR_M1_SIG
    # M1 is not looked at when M2 holds as many bits as M3
    vid2 = vc.VIEW2.to_bytes(8, "little")
    all7 = list(range(7))
    assert nv(vc.VIEW2, keys.agg(all7, vid2), vc.bitmap_of(all7), keys.agg(all7, vcm.NIL),
              vc.bitmap_of(all7), b"") == vcm.NV_OK
