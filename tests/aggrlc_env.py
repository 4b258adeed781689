"""What the combined aggregate-verify GPU tests (test_aggrlc*_gpu.py) share:
the skip mark, the `core` fixture body, and one committee with its valid
items.  A helper module like arith_cases.py, not collected."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402

N = 64                      # committee
CHUNK = 64
BAD = -1                    # any negative code (the oracle and the library number them apart)


def _gpu_available():
    try:
        from harmony_amd import core
        return core.device_count() > 0
    except Exception:
        return False


def gpu_marks():
    """a test module's pytestmark"""
    if os.environ.get("HBLS_FORCE_GPU_TESTS"):
        return pytest.mark.gpu
    return [pytest.mark.gpu, pytest.mark.skipif(not _gpu_available(), reason="no AMD GPU")]


def init_core():
    """body of a module's `core` fixture"""
    from harmony_amd import core as c
    c.init(-1 if c.device_count() == 0 else 0)
    return c


def _norm(res):
    return [BAD if v < 0 else v for v in res]


def _chunks(batch):
    return (batch + CHUNK - 1) // CHUNK


class Env:
    """64 keys and `total` valid (mask, message, aggregate signature) items
    plus D, the forged signature the tests add and subtract — built once,
    never modified; tests work on copies of the lists.  An item's aggregate
    signature is one signature under the sum of its signers' secret keys (BLS
    is linear in the key).  The masks depend on `seed` alone."""

    def __init__(self, capi, core, seed, total=130, sk_base=300, msg_base=500):
        self.core = core
        self.capi = capi
        self.total = total
        rng = random.Random(seed)
        sk = [pr.synth_sk(sk_base + i) for i in range(N)]
        self.pks = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in sk), N)
        self.committee = core.Committee(self.pks, N)
        self.oracle = capi.Committee(self.pks, N)
        self.bmlen = (N + 7) // 8
        self.masks, self.msgs, agg_sk = [], [], []
        for j in range(total):
            signers = rng.sample(range(N), rng.randrange(1, N + 1))
            bm = bytearray(self.bmlen)
            for i in signers:
                bm[i >> 3] |= 1 << (i & 7)
            self.masks.append(bytes(bm))
            self.msgs.append(pr.construct_commit_payload(j, pr.synth_msg(msg_base + j), j + 1))
            agg_sk.append(sum(sk[i] for i in signers) % pr.R)
        self.mlen = len(self.msgs[0])
        cat = core.batch_sign(b"".join(pr.fr_serialize(k) for k in agg_sk),
                              b"".join(self.msgs), self.mlen, total)
        self.sigs = [cat[96 * j:96 * (j + 1)] for j in range(total)]
        self.D = capi.sign_hash(pr.fr_serialize(pr.synth_sk(999)), self.msgs[0])
        assert core.aggrlc_chunk_size() == CHUNK

    def args(self, batch, sigs=None, masks=None, msgs=None):
        """batch_agg_verify's arguments for the first `batch` items"""
        sigs = self.sigs if sigs is None else sigs
        masks = self.masks if masks is None else masks
        msgs = self.msgs if msgs is None else msgs
        return (b"".join(masks[:batch]), b"".join(sigs[:batch]), b"".join(msgs[:batch]),
                self.mlen, batch)

    def oracle_run(self, batch, sigs=None, masks=None, msgs=None):
        return _norm(self.oracle.batch_agg_verify(*self.args(batch, sigs, masks, msgs)))

    def configured(self, call, **switches):
        """(normalised results, stats, stage slots 0..8) of call() at
        threshold 1 under the given core.aggrlc_switches"""
        core = self.core
        with core.aggrlc_switches(threshold=1, **switches):
            res = call()
            stats = core.aggrlc_last_stats()
            slots = [core.last_stage_ns(i) for i in range(9)]
        return _norm(res), stats, slots

    def run(self, batch, sigs=None, masks=None, msgs=None, **switches):
        a = self.args(batch, sigs, masks, msgs)
        # Env's own, whatever signature a test module gives its `configured`
        return Env.configured(self, lambda: self.committee.batch_agg_verify(*a), **switches)

    def cancelling(self, a, b):
        """sig_a + D and sig_b - D: the unweighted sum of the two signatures is
        that of the valid ones, the weighted one must not be"""
        sigs = list(self.sigs)
        sigs[a] = self.capi.g2_add(self.sigs[a], self.D)
        sigs[b] = self.capi.g2_add(self.sigs[b], self.D, sub=True)
        return sigs

    def two_committees(self, n=66):
        """(ContextSet, idx, blobs, messages, expected) for one seal_verify call
        over two committees: the second lists the same keys in reverse order,
        so its items carry the mirrored mask; item 65 has a wrong signature"""
        pk = [self.pks[48 * i:48 * (i + 1)] for i in range(N)]
        second = self.core.Committee(b"".join(reversed(pk)), N)
        cs = self.core.ContextSet([self.committee, second])

        def mirrored(mask):
            out = bytearray(self.bmlen)
            for i in range(N):
                if mask[i >> 3] >> (i & 7) & 1:
                    out[(N - 1 - i) >> 3] |= 1 << ((N - 1 - i) & 7)
            return bytes(out)

        idx = [j & 1 for j in range(n)]
        sigs = list(self.sigs[:n])
        sigs[65] = self.sigs[0]
        blobs = [sigs[j] + (mirrored(self.masks[j]) if idx[j] else self.masks[j])
                 for j in range(n)]
        want = [1] * n
        want[65] = 0
        return cs, idx, blobs, self.msgs[:n], want
