"""Shared by test_viewchange_host.py and test_viewchange_gpu.py: a committee of
9 under the uniform policy (quorum needs 7), a backend over the CPU oracle, a
plain per-message restatement of onViewChangeSanityCheck + ProcessViewChangeMsg
that calls the oracle one message at a time, and one batch of VIEWCHANGE
messages that reaches every refusal."""
from collections import Counter

from oracle import pyref as pr
from harmony_amd import viewchange as vcm

N = 9
NBYTES = 2
QUORUM_ABOVE = 2 * N // 3       # 6: quorum is popcount > 6
BAD = -3
NOQUORUM = -4


def bitmap_of(keys):
    bm = bytearray(NBYTES)
    for k in keys:
        bm[k >> 3] |= 1 << (k & 7)
    return bytes(bm)


def count_in_range(bitmap):
    return sum(1 for i in range(N) if bitmap[i >> 3] >> (i & 7) & 1)


class Keys:
    def __init__(self, capi):
        self.capi = capi
        self.sks = [pr.fr_serialize(pr.synth_sk(100 + i)) for i in range(N)]
        self.pks = [capi.pk_from_sk(sk) for sk in self.sks]
        self.pks_cat = b"".join(self.pks)
        self._sigs = {}

    def sign(self, i, msg):
        if (i, msg) not in self._sigs:
            self._sigs[(i, msg)] = self.capi.sign_hash(self.sks[i], msg)
        return self._sigs[(i, msg)]

    def agg(self, signers, msg):
        return self.capi.aggregate_sigs([self.sign(i, msg) for i in signers])

    def m1_payload(self, block_hash, signers, bits=None):
        """block hash || aggregated prepared signature || bitmap"""
        bits = signers if bits is None else bits
        return block_hash + self.agg(signers, block_hash) + bitmap_of(bits)


class OracleBackend:
    """the viewchange backend over the CPU oracle; counts its calls"""

    def __init__(self, capi, keys):
        self.capi, self.keys = capi, keys
        self.committee = capi.Committee(keys.pks_cat, N)
        self.calls = Counter()

    def verify_msgs(self, key_idx, sigs, msg_idx, msgs):
        self.calls["verify_msgs"] += 1
        out = []
        for k, sig, m in zip(key_idx, sigs, msg_idx):
            try:
                out.append(1 if self.capi.verify_hash(self.keys.pks[k], sig, msgs[m]) else 0)
            except ValueError:
                out.append(BAD)
        return out

    def verify_seals(self, blobs, msgs, quorum):
        self.calls["verify_seals"] += 1
        out = []
        for blob, msg in zip(blobs, msgs):
            if len(blob) != 96 + NBYTES:
                out.append(BAD)
            elif quorum and not count_in_range(blob[96:]) > QUORUM_ABOVE:
                out.append(NOQUORUM)
            else:
                try:
                    out.append(1 if self.committee.agg_verify(blob[96:], blob[:96], msg) else 0)
                except ValueError:
                    out.append(BAD)
        return out

    def aggregate(self, sigs):
        self.calls["aggregate"] += 1
        return self.capi.aggregate_sigs(list(sigs))

    def mask_power(self, bitmap):
        self.calls["mask_power"] += 1
        c = count_in_range(bitmap)
        return c, c, c > QUORUM_ABOVE


class Restated:
    """onViewChangeSanityCheck's signature leg, then ProcessViewChangeMsg, one
    message at a time, each check a single oracle call where it stands in the
    reference"""

    def __init__(self, capi, keys):
        self.capi, self.keys = capi, keys
        self.committee = capi.Committee(keys.pks_cat, N)
        self.m1, self.m2, self.m3 = {}, {}, {}      # view -> {sender: sig}
        self.m1_payload = None

    def _verify(self, sender, sig, msg):
        try:
            return self.capi.verify_hash(self.keys.pks[sender], sig, msg)
        except ValueError:
            return False

    def on_message(self, msg):
        sender, view_id, payload, has_block, vc_sig, id_sig = msg
        if sender >= N:
            return vcm.ERR_SENDER
        if not self._verify(sender, id_sig, view_id.to_bytes(8, "little")):
            return vcm.ERR_VIEWID_SIG
        if sender in self.m3.get(view_id, {}):
            return vcm.ERR_DUP_M3
        if len(payload) >= 128 and has_block:
            if sender in self.m1.get(view_id, {}):
                return vcm.ERR_DUP_M1
            if not self._verify(sender, vc_sig, payload):
                return vcm.ERR_VERIFY_M1
            blob = payload[32:]
            if len(blob) != 96 + NBYTES or not self.capi.g2_check(blob[:96]):
                return vcm.ERR_PROOF_FORMAT
            if not count_in_range(blob[96:]) > QUORUM_ABOVE:
                return vcm.ERR_NO_QUORUM
            if not self.committee.agg_verify(blob[96:], blob[:96], payload[:32]):
                return vcm.ERR_M1_PAYLOAD
            self.m1.setdefault(view_id, {})[sender] = vc_sig
            self.m3.setdefault(view_id, {})[sender] = id_sig
            if self.m1_payload is None:
                self.m1_payload = payload
            return vcm.VC_OK
        if sender in self.m2.get(view_id, {}):
            return vcm.ERR_DUP_M2
        if not self._verify(sender, vc_sig, vcm.NIL):
            return vcm.ERR_VERIFY_M2
        self.m2.setdefault(view_id, {})[sender] = vc_sig
        self.m3.setdefault(view_id, {})[sender] = id_sig
        return vcm.VC_OK

    def bitmaps(self, view_id):
        return tuple(bitmap_of(m.get(view_id, {})) for m in (self.m1, self.m2, self.m3))

    def aggregate(self, which, view_id):
        sigs = list(getattr(self, which).get(view_id, {}).values())
        return self.capi.aggregate_sigs(sigs) if sigs else None


VIEW = 5
VIEW2 = 6


def first_batch(keys):
    """(messages, payload P).  Five M1 messages share P, whose proof is signed
    by 7 keys; two M2 messages; and one message per refusal."""
    h = pr.synth_msg(900)
    P = keys.m1_payload(h, range(7))
    P6 = keys.m1_payload(pr.synth_msg(901), range(6))                   # no quorum
    PBAD = keys.m1_payload(pr.synth_msg(902), range(6), bits=range(7))  # bad aggregate
    vid = VIEW.to_bytes(8, "little")

    def m1(s, payload=P):
        return (s, VIEW, payload, True, keys.sign(s, payload), keys.sign(s, vid))

    def m2(s):
        return (s, VIEW, b"", False, keys.sign(s, vcm.NIL), keys.sign(s, vid))

    other = VIEW2.to_bytes(8, "little")
    msgs = [
        m1(0), m1(1), m2(2), m1(3),
        m2(1),                                                          # repeated sender
        (4, VIEW, b"", False, keys.sign(4, vcm.NIL), keys.sign(4, other)),  # bad view-ID sig
        m1(5, P6),
        m1(6, PBAD),
        (7, VIEW, P, True, keys.sign(7, vcm.NIL), keys.sign(7, vid)),   # M1 signing NIL
        (9, VIEW, b"", False, keys.sign(0, vcm.NIL), keys.sign(0, vid)),    # no such sender
        m1(4), m2(8), m1(7),
    ]
    want = [vcm.VC_OK, vcm.VC_OK, vcm.VC_OK, vcm.VC_OK, vcm.ERR_DUP_M3, vcm.ERR_VIEWID_SIG,
            vcm.ERR_NO_QUORUM, vcm.ERR_M1_PAYLOAD, vcm.ERR_VERIFY_M1, vcm.ERR_SENDER,
            vcm.VC_OK, vcm.VC_OK, vcm.VC_OK]
    return msgs, P, want


def second_batch(keys, P):
    """another view ID: two M2 messages and an M1 that carries the proof the
    first batch accepted"""
    vid = VIEW2.to_bytes(8, "little")
    return [
        (0, VIEW2, b"", False, keys.sign(0, vcm.NIL), keys.sign(0, vid)),
        (1, VIEW2, b"", False, keys.sign(1, vcm.NIL), keys.sign(1, vid)),
        (2, VIEW2, P, True, keys.sign(2, P), keys.sign(2, vid)),
    ]
