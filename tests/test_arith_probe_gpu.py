"""Device field, tower and group arithmetic against big-integer references,
one operation at a time (hbls_arith_probe).

Every production function is run on raw limb operands built to hit carries
and boundaries (tests/arith_cases.py; what the sets cover is asserted on the
CPU in tests/test_arith_cases.py) and compared EXACTLY with oracle/pyref.py.
Alternative implementations (asm / inline / register-ABI multipliers, the
fp6-granular tower, the cooperative cv_* layer) must also return the same
bytes as the operation they stand in for, which is what verdict parity
between the kernels rests on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import arith_cases as ac  # noqa: E402
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

P = ac.P
OP_NAMES = [o.name for o in ac.OPS]


@pytest.fixture(scope="module")
def core():
    from harmony_amd import core as c
    c.init(-1 if c.device_count() == 0 else 0)
    return c


@pytest.fixture(scope="module")
def run(core):
    """run(name) -> (out bytes, flags) of the operation on its whole case
    list; one device call per operation per session"""
    cache = {}

    def go(name):
        if name not in cache:
            op = ac.OPS[ac.OP_INDEX[name]]
            items = ac.items_of(op)
            cache[name] = core.arith_probe(ac.OP_INDEX[name], ac.pack(items), len(items), op.n_out)
        return cache[name]
    return go


def _check_canonical(name, outs):
    for j, o in enumerate(outs):
        for k, v in enumerate(o):
            assert v < P, "%s item %d: output limb vector %d is not reduced (%#x)" % (name, j, k, v)


def _check_exact(op, items, outs, flags):
    for j, it in enumerate(items):
        want, wflag = op.ref(it)
        if op.n_out:
            assert outs[j] == want, "%s item %d %r: got %r, want %r (field values: %r vs %r)" % (
                op.name, j, it, outs[j], want, [ac.fm(v) for v in outs[j]], [ac.fm(v) for v in want])
        assert flags[j] == (0 if wflag is None else wflag), "%s item %d %r: flag" % (op.name, j, it)


def _check_sqrt_any(op, items, outs, flags):
    for j, it in enumerate(items):
        x = ac.f2_of(it)
        assert flags[j] == int(pr.f2_sqrt(x) is not None), "%s item %d: flag" % (op.name, j)
        if flags[j]:
            assert pr.f2_sqr(ac.f2_of(outs[j])) == x, "%s item %d: not a root" % (op.name, j)


def _check_group(op, cases, outs, flags):
    F2 = op.kind != "g1"
    for j, c in enumerate(cases):
        if op.kind == "addj":
            assert flags[j] == int(c.degenerate), "%s %s: edge flag %d" % (op.name, c.name, flags[j])
            if flags[j]:
                continue               # the kernel recomputes flagged items on the scalar path
        else:
            assert flags[j] == 0
        got = ac.jac_to_affine(F2, outs[j])
        assert got == c.expect, "%s %s: got %r, want %r" % (op.name, c.name, got, c.expect)


@pytest.mark.parametrize("name", OP_NAMES)
def test_op(run, name):
    op = ac.OPS[ac.OP_INDEX[name]]
    out, flags = run(name)
    items = ac.items_of(op)
    outs = ac.unpack(out, op.n_out)
    assert len(flags) == len(items) and (not op.n_out or len(outs) == len(items))
    _check_canonical(name, outs)       # fp_to_le48's serialized integer included
    if op.kind == "exact":
        _check_exact(op, items, outs, flags)
    elif op.kind == "any":
        _check_sqrt_any(op, items, outs, flags)
    else:
        _check_group(op, op.cases(), outs, flags)
    if op.base is not None:
        bout, bflags = run(op.base)
        if op.kind == "exact":
            assert out == bout and flags == bflags, "%s differs from %s" % (name, op.base)
        else:
            # group law: same Jacobian representative wherever the formulas
            # apply (no operand at infinity, distinct x)
            n = op.n_out * 48
            for j, c in enumerate(op.cases()):
                if not c.degenerate:
                    assert out[j * n:(j + 1) * n] == bout[j * n:(j + 1) * n], \
                        "%s differs from %s on %s" % (name, op.base, c.name)


def test_fp_le48_round_trip(core):
    """48 bytes -> fp_from_le48 -> fp_to_le48 gives the bytes back for every
    value below p; values >= p are rejected"""
    items = ac.fp_le48_in()
    out, flags = core.arith_probe(ac.OP_INDEX["fp_from_le48"], ac.pack(items), len(items), 1)
    assert flags == [int(v[0] < P) for v in items]
    assert 0 in flags and 1 in flags
    good = [j for j, f in enumerate(flags) if f]
    mont = b"".join(out[48 * j:48 * (j + 1)] for j in good)
    back, _ = core.arith_probe(ac.OP_INDEX["fp_to_le48"], mont, len(good), 1)
    assert back == ac.pack([items[j] for j in good])


@pytest.mark.parametrize("name", ac.COOP_OPS)
def test_coop_counts(core, run, name):
    """partial last blocks and a second block: 1, 15, 16, 17 and 33 items
    (16 items per block); results must not depend on the count"""
    op = ac.OPS[ac.OP_INDEX[name]]
    items = ac.items_of(op)
    ref_out, ref_flags = run(name)
    w = op.n_out * 48
    for n in ac.COOP_COUNTS:
        idx = [(7 * j + 3) % len(items) for j in range(n)]
        out, flags = core.arith_probe(ac.OP_INDEX[name], ac.pack([items[i] for i in idx]), n,
                                      op.n_out)
        assert out == b"".join(ref_out[i * w:(i + 1) * w] for i in idx), (name, n)
        assert flags == [ref_flags[i] for i in idx], (name, n)


@pytest.mark.parametrize("bad", [P, P + 1, (1 << 384) - 1, 1 << 381])
def test_operand_not_below_p_is_rejected(core, bad):
    for name, pos in (("fp_add", 0), ("fp_add", 1), ("fp12_mul", 23), ("cv_fp12_mul", 13),
                      ("g2_add", 5), ("fp_to_le48", 0)):
        op = ac.OPS[ac.OP_INDEX[name]]
        good = list(ac.items_of(op)[0])
        item = list(good)
        item[pos] = bad
        with pytest.raises(core.BadInputError):
            core.arith_probe(ac.OP_INDEX[name], ac.pack([good, item]), 2, op.n_out)


def test_zero_is_rejected_where_undefined(core):
    for name in ("fp_inv", "fp2_inv", "fp6_inv", "fp12_inv", "cv_fp12_inv_q0",
                 "final_exp", "final_exp_6", "cv_final_exp"):
        op = ac.OPS[ac.OP_INDEX[name]]
        with pytest.raises(core.BadInputError):
            core.arith_probe(ac.OP_INDEX[name], ac.pack([(0,) * op.n_in]), 1, op.n_out)


def test_unknown_operation_is_rejected(core):
    for op in (-1, len(ac.OPS), 1 << 20):
        with pytest.raises(core.BadInputError):
            core.arith_probe(op, bytes(48 * 24), 1, 12)


def test_coop_selftest(core):
    rc = core.coop_selftest()
    assert rc == 0, "cooperative stages that differ from their scalar twins: %s (rc %d)" % (
        core.coop_selftest_failed_stages(rc) if rc > 0 else "launch failed", rc)


def test_fpmul_asm_check(core):
    assert core.fpmul_asm_check() == 0


def test_table_matches_library(core):
    """an operation cannot be added to the probe's switch without a test:
    the Python table and the library's list agree name by name"""
    assert core.arith_probe_ops() == OP_NAMES
    assert all(ac.OP_INDEX[o.base] < i for i, o in enumerate(ac.OPS) if o.base)
