"""Host side of the epoch-context engine: the epoch-context
LRU, the commit payload by epoch, the verified-seal cache and the first-failure
index of harmony_amd.engine, driven with a stub verifier, and core.pack_blobs.
No GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402
from harmony_amd import engine as eng  # noqa: E402

N = 5
STAKING_EPOCH = 100


class _Stub:
    """records every verifier call; an item is accepted unless its signature
    starts with a zero byte"""

    def __init__(self):
        self.calls = []

    def __call__(self, contexts, ctx_idx, blobs, msgs, quorum):
        self.calls.append(dict(keys=[c.key for c in contexts], ctx_idx=list(ctx_idx),
                               blobs=list(blobs), msgs=list(msgs), quorum=quorum))
        return [0 if b[0] == 0 else 1 for b in blobs]


class _Loader:
    def __init__(self):
        self.loads = []

    def __call__(self, shard_id, epoch):
        self.loads.append((shard_id, epoch))
        return bytes([shard_id]) * (48 * N), N, None, epoch >= STAKING_EPOCH


def _item(shard, epoch, j, good=True, bitmap=b"\x1f"):
    sig = bytes([1 if good else 0]) + bytes([j % 256]) * 95
    return eng.SealItem(shard, epoch, pr.synth_msg(j), 1000 + j, 2000 + j, sig, bitmap)


def test_epoch_context_lru():
    loader, stub = _Loader(), _Stub()
    e = eng.Engine(loader, verifier=stub)
    for ep in range(20):
        e.epoch_context(0, ep)
    assert loader.loads == [(0, ep) for ep in range(20)]
    e.epoch_context(0, 0)                       # a hit: now the most recent
    assert len(loader.loads) == 20
    e.epoch_context(1, 0)                       # the 21st evicts the oldest: (0, 1)
    assert len(e.resident_contexts()) == 20
    assert (0, 1) not in e.resident_contexts() and (0, 0) in e.resident_contexts()
    e.epoch_context(0, 1)                       # reload
    assert loader.loads[-2:] == [(1, 0), (0, 1)]
    assert (0, 2) not in e.resident_contexts()
    ctx = e.epoch_context(0, 1)
    assert (ctx.n, ctx.power, ctx.is_staking, len(ctx.pks)) == (N, None, False, 48 * N)
    assert len(loader.loads) == 22


def test_payload_by_epoch():
    for staking in (False, True):
        for j in range(3):
            h = pr.synth_msg(j)
            want = pr.construct_commit_payload(7 + j, h, 9 + j, staking=staking)
            assert eng.construct_commit_payload(7 + j, h, 9 + j, staking) == want
            assert len(want) == (48 if staking else 40)
    stub = _Stub()
    e = eng.Engine(_Loader(), verifier=stub)
    items = [_item(0, STAKING_EPOCH - 1, 1), _item(0, STAKING_EPOCH, 2), _item(3, 5, 3)]
    res = e.verify_headers(items)
    assert res == ([1, 1, 1], None)
    call, = stub.calls
    assert [len(m) for m in call["msgs"]] == [40, 48, 40]
    for it, msg, blob in zip(items, call["msgs"], call["blobs"]):
        staking = it.epoch >= STAKING_EPOCH
        assert msg == pr.construct_commit_payload(it.number, it.block_hash, it.view_id,
                                                  staking=staking)
        assert blob == it.sig + it.bitmap
    # one call for the window; every item names its own context
    assert [call["keys"][i] for i in call["ctx_idx"]] == [(0, 99), (0, 100), (3, 5)]
    assert call["quorum"] is True


def test_verified_cache_and_first_failure():
    stub = _Stub()
    e = eng.Engine(_Loader(), verifier=stub)
    items = [_item(0, 1, 1), _item(0, 1, 2, good=False), _item(1, 1, 3), _item(0, 2, 4, good=False)]
    res = e.verify_headers(items)
    assert res.codes == [1, 0, 1, 0] and res.first_failure == 1
    assert len(stub.calls) == 1 and len(stub.calls[0]["blobs"]) == 4
    # accepted items hit the cache; rejected ones are verified again
    res = e.verify_headers(items)
    assert res.codes == [1, 0, 1, 0] and res.first_failure == 1
    assert len(stub.calls) == 2
    assert stub.calls[1]["blobs"] == [items[1].sig + items[1].bitmap,
                                      items[3].sig + items[3].bitmap]
    # all hits: the verifier is not called
    res = e.verify_crosslinks([items[2], items[0]])
    assert res == ([1, 1], None) and len(stub.calls) == 2
    assert e.verify_headers([]) == ([], None)
    # a cross-link of block number <= 1 is refused on the host
    low = _item(0, 1, 9)._replace(number=1)
    res = e.verify_crosslinks([items[0], low])
    assert res.codes == [1, eng.HBLS_ERR_BADINPUT] and res.first_failure == 1
    assert len(stub.calls) == 2


def test_cache_keys_on_whole_bitmap():
    """two bitmaps that differ only after byte 64 are distinct cache keys (the
    reference's fixed 64-byte key would merge them)"""
    stub = _Stub()
    e = eng.Engine(_Loader(), verifier=stub)
    a = _item(0, 1, 1, bitmap=b"\xff" * 64 + b"\x01")
    b = a._replace(bitmap=b"\xff" * 64 + b"\x02")
    assert e.verify_headers([a]).codes == [1]
    assert e.verify_headers([b]).codes == [1]
    assert len(stub.calls) == 2
    assert e.verify_headers([a, b]).codes == [1, 1]
    assert len(stub.calls) == 2


def test_window_wider_than_the_context_cache():
    """a window over more contexts than the LRU holds still goes out in one
    call, with every context of the window present"""
    loader, stub = _Loader(), _Stub()
    e = eng.Engine(loader, verifier=stub)
    items = [_item(0, ep, ep) for ep in range(30)]
    assert e.verify_headers(items) == ([1] * 30, None)
    call, = stub.calls
    assert [call["keys"][i] for i in call["ctx_idx"]] == [(0, ep) for ep in range(30)]
    assert len(e.resident_contexts()) == 20


def test_pack_blobs():
    from harmony_amd.core import BadInputError, pack_blobs
    assert pack_blobs([]) == (b"", [0])
    cat, off = pack_blobs([b"abc", b"", b"de"])
    assert cat == b"abcde" and off == [0, 3, 3, 5]

    class Big:
        def __len__(self):
            return 1 << 31

    with pytest.raises(BadInputError):
        pack_blobs([Big(), Big()])
    with pytest.raises(BadInputError):
        pack_blobs([b"x", Big(), Big()])
