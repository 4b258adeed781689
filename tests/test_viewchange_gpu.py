"""harmony_amd.viewchange on the device: the batch of
test_viewchange_host.py through DeviceBackend and through the oracle backend;
codes, bitmaps and aggregates must be equal, and the NEWVIEW round trip runs on
the device."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from harmony_amd import viewchange as vcm  # noqa: E402
import viewchange_cases as vc  # noqa: E402


def _gpu_available():
    try:
        from harmony_amd import core
        return core.device_count() > 0
    except Exception:
        return False


if not os.environ.get("HBLS_FORCE_GPU_TESTS"):
    pytestmark = [pytest.mark.gpu,
                  pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]


def test_device_backend_equals_oracle_backend(oracle_lib):
    keys = vc.Keys(oracle_lib)
    dev = vcm.ViewChange(keys.pks_cat, vc.N)                # DeviceBackend
    ora = vcm.ViewChange(keys.pks_cat, vc.N, backend=vc.OracleBackend(oracle_lib, keys))
    msgs, P, want = vc.first_batch(keys)
    assert ora.process(msgs) == want
    assert dev.process(msgs) == want
    msgs2 = vc.second_batch(keys, P)
    assert dev.process(msgs2) == ora.process(msgs2) == [vcm.VC_OK] * 3
    for view in (vc.VIEW, vc.VIEW2):
        assert dev.bitmaps(view) == ora.bitmaps(view)
        assert dev.get_m2_bitmap(view) == ora.get_m2_bitmap(view)
        assert dev.get_m3_bitmap(view) == ora.get_m3_bitmap(view)
    assert dev.m1_payload == ora.m1_payload == P

    # NEWVIEW, verified on the device
    m3_sig, m3_bm = dev.get_m3_bitmap(vc.VIEW)
    m2_sig, m2_bm = dev.get_m2_bitmap(vc.VIEW)
    vid = vc.VIEW.to_bytes(8, "little")
    few = list(range(6))
    few_sig, few_bm = keys.agg(few, vid), vc.bitmap_of(few)
    flipped = bytes([m3_bm[0] ^ 0x20, m3_bm[1]])
    cases = [
        (m3_sig, m3_bm, m2_sig, m2_bm, P),
        (m3_sig, flipped, m2_sig, m2_bm, P),
        (few_sig, few_bm, m2_sig, m2_bm, P),
        (m3_sig, m3_bm, m3_sig, m2_bm, P),
        (m3_sig, m3_bm, m2_sig, m2_bm, P[:100]),
        (m3_sig, m3_bm, None, None, P),
        (m3_sig, m3_bm, None, None, P[:32] + keys.agg(range(7), vid) + P[128:]),
        (m3_sig, m3_bm, None, None, P + b"\x00"),           # proof of a wrong length
    ]
    want_nv = [vcm.NV_OK, vcm.NV_ERR_M3_SIG, vcm.NV_ERR_M3_QUORUM, vcm.NV_ERR_M2_SIG,
               vcm.NV_ERR_M1_FORMAT, vcm.NV_OK, vcm.NV_ERR_M1_SIG, vcm.NV_ERR_M1_FORMAT]
    assert [ora.verify_new_view(vc.VIEW, *c) for c in cases] == want_nv
    assert [dev.verify_new_view(vc.VIEW, *c) for c in cases] == want_nv
