"""Host side of the multi-key votes: the CSR packing helper
and the pure-Python model of the ordered all-or-nothing rule, checked against
quorum.BallotBox.submit_vote — the mirror of the reference's
drop-if-any-key-voted rule.  No GPU needed."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_pack_key_lists():
    from harmony_amd.core import pack_key_lists
    assert pack_key_lists([]) == ([0], [])
    assert pack_key_lists([], 0) == ([0], [])
    off, idx = pack_key_lists([[3], [], [1, 2, 9], (7, 8)])
    assert off == [0, 1, 1, 4, 6]
    assert idx == [3, 1, 2, 9, 7, 8]
    # lists are passed as they are: order and repeats are the device's verdict
    assert pack_key_lists([[5, 5], [7, 3]], 2) == ([0, 2, 4], [5, 5, 7, 3])
    with pytest.raises(ValueError):
        pack_key_lists([[1], [2]], 3)
    with pytest.raises(ValueError):
        pack_key_lists([[1]], 0)
    with pytest.raises(ValueError):
        pack_key_lists([[-1]])
    with pytest.raises(ValueError):
        pack_key_lists([[1 << 32]])


def test_model_example():
    from harmony_amd.stream import ordered_claim_model
    res, bms = ordered_claim_model([bytes(5)], [(0, [1, 2], True), (0, [2, 3], True),
                                                (0, [3, 4], True), (0, [31, 32], True)])
    assert res == [1, 2, 1, 1]             # B loses to A, C wins: B set nothing
    assert bms == [bytes([0x1E, 0, 0, 0x80, 0x01])]
    res, bms2 = ordered_claim_model(bms, [(0, [4, 5], True), (0, [6, 7], False),
                                          (0, [6], 1), (0, [9], -3)])
    assert res == [2, 0, 1, -3]
    assert bms2 == [bytes([0x5E, 0, 0, 0x80, 0x01])]
    assert bms == [bytes([0x1E, 0, 0, 0x80, 0x01])]     # inputs are left alone


def test_model_matches_ballot_box():
    """seeded sequence of overlapping signer sets over two rounds, fed in
    ticks to the model and one by one to a BallotBox per round"""
    from harmony_amd import quorum
    from harmony_amd.stream import ordered_claim_model
    rng = random.Random(17)
    n, rounds = 24, 2
    boxes = [quorum.BallotBox() for _ in range(rounds)]
    bitmaps = [bytes((n + 7) // 8)] * rounds
    outcomes = set()
    for _ in range(6):
        tick = [(rng.randrange(rounds), sorted(rng.sample(range(n), rng.randint(1, 4))),
                 rng.random() >= 0.15) for _ in range(12)]
        res, bitmaps = ordered_claim_model(bitmaps, tick)
        for (r, keys, valid), got in zip(tick, res):
            if not valid:                  # never reaches the ballot box
                assert got == 0
                continue
            try:
                boxes[r].submit_vote(quorum.COMMIT, [bytes([k]) for k in keys],
                                     b"h", b"s", 1)
                want = 1
            except ValueError:
                want = 2
            assert got == want, (r, keys)
            outcomes.add(got)
        for r in range(rounds):
            voted = {k[0] for k in boxes[r]._votes[quorum.COMMIT]}
            assert bitmaps[r] == bytes(
                sum(1 << (k & 7) for k in voted if k >> 3 == b) for b in range((n + 7) // 8))
    assert outcomes == {1, 2}
