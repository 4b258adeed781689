"""The switches of the combined aggregate verify, without a
GPU: what each setter accepts and rejects, what -1 restores, the two batch-size
rules at their thresholds, what each environment variable resolves to (fresh
child processes: a variable is read once, on first use), and
core.aggrlc_switches.  All through the hook hbls_aggrlc_switch_value."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from harmony_amd import core  # noqa: E402

RULE = "rule"       # default of sigleg and early: 1 from a batch size on
# name: (variable, raw setter, accepted, default, some rejected values)
TABLE = {
    "mode": ("HBLS_AGG_VERIFY_MODE", core.set_agg_verify_mode, (0, 1), -1, (2, -2, 7)),
    "final": ("HBLS_AGGRLC_FINAL", core.set_aggrlc_final, (0, 8, 16), 16, (4, 1, -2, 7)),
    "sigleg": ("HBLS_AGGRLC_SIGLEG", core.set_aggrlc_sigleg, (0, 1), RULE, (2, -2, 7)),
    "early": ("HBLS_AGGRLC_EARLY", core.set_aggrlc_early, (0, 1), RULE, (2, -2, 7)),
    "miller": ("HBLS_AGGRLC_MILLER", core.set_aggrlc_miller, (0, 1, 2), 2, (3, -2, 7)),
    "chunkleg": ("HBLS_AGGRLC_CHUNKLEG", core.set_aggrlc_chunkleg, (0, 16), 16, (8, 1, -2, 7)),
}
RULE_FROM = {"sigleg": 16384, "early": 262144}
SIZES = (0, 1, 16383, 16384, 262143, 262144, 1 << 20)


def _expected(name, value, batch):
    """what `name` resolves to at `batch` when it holds `value`"""
    if value == RULE:
        return 1 if batch >= RULE_FROM[name] else 0
    return value


def _snapshot(value_of=core.aggrlc_switch_value):
    return {name: [value_of(name, b) for b in SIZES] for name in TABLE}


def _defaults():
    return {name: [_expected(name, TABLE[name][3], b) for b in SIZES] for name in TABLE}


def test_hook_names_match_the_setters():
    assert tuple(TABLE) == core.AGGRLC_SWITCHES
    assert core._lib.hbls_aggrlc_switch_value(-1, 0) == core.HBLS_ERR_BADINPUT
    assert core._lib.hbls_aggrlc_switch_value(len(TABLE), 0) == core.HBLS_ERR_BADINPUT


@pytest.mark.parametrize("name", list(TABLE))
def test_setter_table(name):
    _, setter, accepted, default, rejected = TABLE[name]
    try:
        for v in accepted:
            setter(v)
            assert [core.aggrlc_switch_value(name, b) for b in SIZES] == [v] * len(SIZES)
            for bad in rejected:
                with pytest.raises(core.BadInputError):
                    setter(bad)
                # the rejected call changed nothing
                assert core.aggrlc_switch_value(name, 0) == v
            setter(-1)
            assert _snapshot() == _defaults()
    finally:
        setter(-1)


def test_rules_at_their_thresholds():
    for name, first in RULE_FROM.items():
        TABLE[name][1](-1)
        assert core.aggrlc_switch_value(name, first - 1) == 0
        assert core.aggrlc_switch_value(name, first) == 1
    assert RULE_FROM == {"sigleg": 16384, "early": 262144}
    # the sizes the issue names, spelled out
    assert core.aggrlc_switch_value("sigleg", 16383) == 0
    assert core.aggrlc_switch_value("sigleg", 16384) == 1
    assert core.aggrlc_switch_value("early", 262143) == 0
    assert core.aggrlc_switch_value("early", 262144) == 1


def test_context_manager_sets_and_restores():
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=0, early=1, miller=0, final=8,
                              chunkleg=0):
        got = _snapshot()
        want = {"mode": 1, "final": 8, "sigleg": 0, "early": 1, "miller": 0, "chunkleg": 0}
        assert got == {k: [v] * len(SIZES) for k, v in want.items()}
        # a setter used inside is put back too, since its switch was named
        core.set_aggrlc_miller(1)
    assert _snapshot() == _defaults()
    with pytest.raises(RuntimeError):
        with core.aggrlc_switches(sigleg=1, miller=1):
            assert core.aggrlc_switch_value("sigleg", 0) == 1
            raise RuntimeError("body failed")
    assert _snapshot() == _defaults()


def test_context_manager_applies_nothing_when_a_value_is_rejected():
    with pytest.raises(core.BadInputError):
        with core.aggrlc_switches(sigleg=1, final=8, miller=5):
            pytest.fail("the body must not run")
    assert _snapshot() == _defaults()
    with pytest.raises(TypeError):
        with core.aggrlc_switches(sigleg=1, millre=1):
            pytest.fail("the body must not run")
    assert _snapshot() == _defaults()


# ------------------------------------------------------------ the environment
_CHILD = ("import json; from harmony_amd import core; "
          "print(json.dumps({n: [core.aggrlc_switch_value(n, b) for b in %r] "
          "for n in core.AGGRLC_SWITCHES}))" % (SIZES,))


def _env_cases():
    """(variable or None, string, switch, value it must resolve to)"""
    cases = [(None, None, None, None)]
    for name, (var, _, accepted, default, _) in TABLE.items():
        cases += [(var, str(v), name, v) for v in accepted]
        cases.append((var, "7", name, default))
    cases += [("HBLS_AGGRLC_MILLER", s, "miller", 2) for s in ("02", "2x")]
    return cases


@pytest.mark.parametrize("var,text,name,value", _env_cases(),
                         ids=["%s=%s" % (c[0], c[1]) for c in _env_cases()])
def test_environment(var, text, name, value):
    env = {k: v for k, v in os.environ.items() if k not in {t[0] for t in TABLE.values()}}
    if var:
        env[var] = text
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=REPO, env=env, check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    got = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    want = _defaults()
    if var:
        want[name] = [_expected(name, value, b) for b in SIZES]
    assert got == want
