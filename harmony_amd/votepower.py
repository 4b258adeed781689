"""harmony_amd.votepower — integer mirror of numeric.Dec (numeric/decimal.go)
and of votepower.Compute (consensus/votepower/roster.go:158-238).

A Dec is held as the plain `int` inside it: the value times 10**18
(Precision = 18, decimal.go:22).  That integer is the unit in which voting
power crosses the C-ABI (hbls_committee_set_quorum), so the list compute()
returns goes to Committee.set_quorum unchanged.  Pure Python, no GPU.

shard.Schedule is not mirrored: the epoch's HarmonyVotePercent and
ExternalVotePercent are parameters.
"""

PRECISION = 18
ONE = 10 ** PRECISION                     # numeric.OneDec()
_HALF = ONE // 2                          # fivePrecision


class VotingPowerNotEqualOne(ValueError):
    """ErrVotingPowerNotEqualOne (roster.go:23)"""

    def __init__(self):
        super().__init__("voting power not equal to one")


def new_dec(i: int) -> int:
    """numeric.NewDec(i)"""
    return i * ONE


def _quo_trunc(a: int, b: int) -> int:
    """big.Int.Quo: truncated towards zero (Python's // floors)"""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def _chop_round(d: int) -> int:
    """chopPrecisionAndRound (decimal.go:458-489): drop 18 digits, round the
    dropped part half-to-even"""
    if d < 0:
        return -_chop_round(-d)
    quo, rem = divmod(d, ONE)
    if rem < _HALF:
        return quo
    if rem > _HALF:
        return quo + 1
    return quo if quo % 2 == 0 else quo + 1


def dec_mul(a: int, b: int) -> int:
    """Dec.Mul (decimal.go:255-263)"""
    return _chop_round(a * b)


def dec_quo(a: int, b: int) -> int:
    """Dec.Quo (decimal.go:297-310): precision applied twice, integer
    quotient, then chop-and-round"""
    return _chop_round(_quo_trunc(a * ONE * ONE, b))


TWO_THIRDS = dec_quo(new_dec(2), new_dec(3))   # twoThird, one-node-staked-vote.go:23


def compute(effective_stakes, harmony_percent: int, external_percent: int):
    """votepower.Compute: OverallPercent of every slot, as Dec integers, in
    slot order.

    effective_stakes[i] is None for a Harmony slot, else the slot's
    EffectiveStake as a Dec integer.  Harmony slots get
    harmony_percent.Quo(slot count); stakers get
    stake.Quo(total stake).Mul(external_percent); what is missing to exactly
    one goes to the last staked voter (roster.go:215-224).  Raises
    VotingPowerNotEqualOne as the reference returns its error."""
    total = sum(e for e in effective_stakes if e is not None)
    hmy_slots = new_dec(sum(1 for e in effective_stakes if e is None))
    out = []
    ours = theirs = 0
    last_staked = None
    for i, e in enumerate(effective_stakes):
        if e is not None:
            overall = dec_mul(dec_quo(e, total), external_percent)
            theirs += overall
            last_staked = i
        else:
            overall = dec_quo(harmony_percent, hmy_slots)
            ours += overall
        out.append(overall)
    diff = ONE - (ours + theirs)
    if diff != 0 and last_staked is not None:
        out[last_staked] += diff
        theirs += diff
    if last_staked is not None and ours + theirs != ONE:
        raise VotingPowerNotEqualOne()
    return out
