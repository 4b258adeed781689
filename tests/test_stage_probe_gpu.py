"""The two byte-to-point stages at the head of every verify pipeline, per
kernel variant, against the reference at value level:
k_hash_to_g2 / k_hash_to_g2_coop and k_g2_decompress / k_g2_decompress_coop
through the stage probe of hbls_probe.inc.  The cases and their expected
results are tests/stage_cases.py's (checked on the CPU by
tests/test_stage_cases.py): every map path, the message mask and truncation,
t == 0, both cofactor modes; valid, identity, boundary and low-order
signature encodings, on the straight and on the degenerate-chain path of the
cooperative membership check."""
import contextlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import arith_cases as ac  # noqa: E402
import stage_cases as sc  # noqa: E402
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

KERNELS = pytest.mark.parametrize("kernel", [0, 1], ids=["scalar", "coop"])
MODES = pytest.mark.parametrize("fast", [True, False], ids=["fast", "full"])
BATCHES = (1, 15, 16, 17, 33)            # the cooperative kernels hold 16 items per block
BAD = -3                                 # HBLS_ERR_BADINPUT


@pytest.fixture(scope="module")
def core():
    from harmony_amd import core as c
    c.init(-1 if c.device_count() == 0 else 0)
    return c


@pytest.fixture(scope="module")
def capi(oracle_lib):
    return oracle_lib


@contextlib.contextmanager
def cofactor_mode(core, capi, fast):
    core.set_g2_cofactor_mode(fast)
    capi.set_g2_cofactor_mode(fast)
    try:
        yield
    finally:
        core.set_g2_cofactor_mode(True)
        capi.set_g2_cofactor_mode(True)


# ------------------------------------------------------------------ hash
def _oracle_hash(capi, msg):
    """(96 bytes, ok) from the C oracle; it fails in its own way on t == 0"""
    try:
        return capi.hash_to_g2(msg), 1
    except ValueError:
        return bytes(96), 0


@MODES
@KERNELS
def test_hash_to_g2(core, capi, kernel, fast):
    picks = set(sc.hash_pyref_picks())
    assert len(picks) >= 6
    n_ok = 0
    with cofactor_mode(core, capi, fast):
        core.hash_edge_reset()
        assert core.hash_edge_count() == 0
        for mlen, cases in sorted(sc.hash_groups().items()):
            out, ok = core.hash_to_g2_probe(b"".join(c.msg for c in cases), mlen, len(cases),
                                            kernel)
            for j, c in enumerate(cases):
                want = sc.hash_expected(c.msg, fast) if c.name in picks \
                    else _oracle_hash(capi, c.msg)
                assert (out[96 * j:96 * j + 96], ok[j]) == want, (c.name, mlen)
                n_ok += want[1]
        edges = core.hash_edge_count()
    assert n_ok == len(sc.hash_cases()) - len(sc.hash_zero_cases())
    # the exact recompute of the cooperative kernel: no map output degenerates
    # the fast chain; the full-cofactor mode sends every mapped item there
    assert edges == (n_ok if kernel == 1 and not fast else 0)


def test_hash_references_agree(capi):
    """the two references on the cases each of them judges alone above"""
    by = {c.name: c.msg for c in sc.hash_cases()}
    for fast in (True, False):
        capi.set_g2_cofactor_mode(fast)
        try:
            for n in sc.hash_pyref_picks():
                assert _oracle_hash(capi, by[n]) == sc.hash_expected(by[n], fast), (n, fast)
        finally:
            capi.set_g2_cofactor_mode(True)


def _layout(batch, good, bad, special=()):
    """a batch of `batch` items: good ones in turn, a bad one in the last slot
    of every full block of 16 and in the last slot of the batch, the special
    ones at slots 2, 4, ... between good ones"""
    items = [good[i % len(good)] for i in range(batch)]
    for k, s in enumerate(special):
        if 2 * k + 3 < batch:
            items[2 * k + 2] = s
    if batch > 1:
        for i in list(range(15, batch, 16)) + [batch - 1]:
            items[i] = bad
    return items


@KERNELS
def test_hash_to_g2_geometry(core, kernel):
    """items 16 to a block: the parked dummy of a t == 0 item and the edge
    flag are per item, so every neighbour hashes as it does alone"""
    good = [c.msg for c in sc.hash_map_cases()[:7]]
    bad = sc.hash_zero_cases()[1].msg
    assert all(len(m) == 48 for m in good + [bad])
    alone = {m: core.hash_to_g2_probe(m, 48, 1, kernel) for m in good + [bad]}
    assert alone[bad] == (bytes(96), [0])
    assert all(alone[m][1] == [1] for m in good)
    for batch in BATCHES:
        items = _layout(batch, good, bad)
        if batch > 1:
            assert items[-1] == bad and (batch < 16 or items[15] == bad)
        out, ok = core.hash_to_g2_probe(b"".join(items), 48, batch, kernel)
        for j, m in enumerate(items):
            assert (out[96 * j:96 * j + 96], [ok[j]]) == alone[m], (batch, j)


# ------------------------------------------------------------ decompress
def _check_decompress(cases, aff, flags, what):
    assert len(flags) == len(cases)
    for c, got, fl in zip(cases, ac.unpack(aff, 4), flags):
        assert fl == c.flag, (what, c.name)
        if c.flag == 1:
            assert tuple(got) == sc.aff_limbs(c.point), (what, c.name)


@KERNELS
def test_g2_decompress(core, kernel):
    cases = sc.dec_cases()
    aff, flags = core.g2_decompress_probe(b"".join(c.sig for c in cases), len(cases), kernel)
    _check_decompress(cases, aff, flags, kernel)


def test_g2_decompress_oracle_agrees(capi):
    """the C oracle's verdict on every encoding pyref judged"""
    for c in sc.dec_cases():
        assert capi.g2_check(c.sig) == (c.flag != 0), c.name


@KERNELS
def test_g2_decompress_geometry(core, kernel):
    """rejected encodings in the last slot of a full block and of the ragged
    last block, low-order points (degenerate and straight chains) and the
    identity between valid signatures: every item decodes as it does alone"""
    low = {c.name: c for c in sc.dec_low_order_cases()}
    good = list(sc.dec_valid_cases()[:7])
    bad = sc.dec_boundary_cases()[0]
    special = [low["T13"], low["T23"], sc.dec_identity_case(), low["S+T13"], low["-T13b"],
               low["T2713"]]
    assert bad.flag == 0 and [c.flag for c in special] == [0, 0, 2, 0, 0, 0]
    alone = {}
    for c in good + [bad] + special:
        alone[c.name] = core.g2_decompress_probe(c.sig, 1, kernel)
        _check_decompress([c], *alone[c.name], what="alone")
    for batch in BATCHES:
        items = _layout(batch, good, bad, special)
        if batch >= 15:
            assert [c.name for c in items[1:4]] == [good[1].name, "T13", good[3].name]
        aff, flags = core.g2_decompress_probe(b"".join(c.sig for c in items), batch, kernel)
        _check_decompress(items, aff, flags, batch)
        for j, c in enumerate(items):
            if c.flag == 1:
                assert (aff[192 * j:192 * j + 192], [flags[j]]) == alone[c.name], (batch, j)


# ------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def votes(core, capi):
    """a committee of 16 and 8 single-key votes: item 2 is S + T13, item 5 is
    T2713 alone, the rest valid; the expected codes are the oracle's"""
    n = 16
    sks = [pr.fr_serialize(pr.synth_sk(i)) for i in range(n)]
    pk = [capi.pk_from_sk(sk) for sk in sks]
    committee = core.Committee(b"".join(pk), n)
    msgs = [pr.construct_commit_payload(j, pr.synth_msg(700 + j), j + 1) for j in range(8)]
    keys = [0, 3, 5, 15, 2, 7, 9, 11]
    sigs = [capi.sign_hash(sks[k], m) for k, m in zip(keys, msgs)]
    ts = sc.low_order_points()
    s2 = pr.g2_deserialize(sigs[2])
    sigs[2] = pr.g2_serialize(pr.g2_add(s2, ts["T13"][1]))
    sigs[5] = pr.g2_serialize(ts["T2713"][1])
    want = []
    for k, s, m in zip(keys, sigs, msgs):
        try:
            want.append(1 if capi.verify_hash(pk[k], s, m) else 0)
        except ValueError:
            want.append(BAD)
    assert want == [1, 1, BAD, 1, 1, BAD, 1, 1]
    return committee, keys, sigs, msgs


@pytest.mark.parametrize("threshold", [0, 10 ** 9], ids=["scalar", "coop"])
def test_batch_verify_votes_rejects_low_order(core, votes, threshold):
    committee, keys, sigs, msgs = votes
    core.set_coop_threshold(threshold)
    try:
        got = committee.batch_verify_votes(keys, b"".join(sigs), b"".join(msgs), len(msgs[0]))
    finally:
        core.set_coop_threshold(-1)
    assert got == [1, 1, BAD, 1, 1, BAD, 1, 1]


# ------------------------------------------------------------ G1 low order
def test_g1_low_order_points_rejected(core, capi):
    """points of order 3, 11 and 10177 on E(Fp): pyref's [r]P test rejects
    them, so must g1_check and the committee table"""
    n = 16
    pks = [capi.pk_from_sk(pr.fr_serialize(pr.synth_sk(i))) for i in range(n)]
    assert all(core.g1_check(pk) for pk in pks)
    core.Committee(b"".join(pks), n)                  # the honest table builds
    for name, (_m, t) in sc.g1_low_order_points().items():
        enc = pr.g1_serialize(t)
        with pytest.raises(ValueError):
            pr.g1_deserialize(enc)
        assert not capi.g1_check(enc), name
        assert not core.g1_check(enc), name
        with pytest.raises(ValueError):
            core.Committee(b"".join(pks[:9] + [enc] + pks[10:]), n)
