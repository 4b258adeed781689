"""harmony_amd.viewchange — host mirror of the view-change collector
(consensus/view_change_construct.go) and of the two sanity legs around it
(onViewChangeSanityCheck, consensus/checks.go:178-192; onNewView,
consensus/view_change.go:477-500), re-built around two device calls per batch
of VIEWCHANGE messages.

The reference verifies one message at a time while the chain is halted: the
view-ID signature, the view-change signature over NIL or the M1 payload, and
for an M1 message the aggregated prepared proof inside the payload.  Here a
batch of messages is resolved on the host and goes to the device as

  one verify_msgs call   two items per message over a table that holds each
                         distinct byte string once (ContextSet.verify_msgs,
                         DESIGN.md §4p), and
  one verify_seals call  over the distinct M1 payloads not yet known good
                         (ContextSet.seal_verify with quorum, §4i).

The reference's rule is then applied per message, in arrival order, on the
host.  This is bookkeeping only.  The backend is injectable, so everything in
this module can be exercised without a GPU; the default one runs on the device.

m1_payload is one field of the collector, not one per view ID, as vc.m1Payload
is in the reference.

One ordering difference is inherited from the quorum entries (include/hbls.h
at hbls_batch_agg_verify_quorum): an M1 proof without quorum whose signature
does not decode reports ERR_NO_QUORUM here, where the reference reports the
decoding error first.  Both refuse the message.
"""

HBLS_OK = 1
HBLS_FALSE = 0
HBLS_ERR_BADINPUT = -3
NOQUORUM = -4

NIL = b"\x01"               # consensus/view_change.go: NIL payload of an M2 message
VALID_PAYLOAD_LENGTH = 128  # ValidPayloadLength: 32 hash + 96 signature, then the bitmap

# process(): one code per message, the first reason in the reference's order
VC_OK = 1
ERR_SENDER = -10            # sender index >= n (never reaches the device)
ERR_VIEWID_SIG = -11        # onViewChangeSanityCheck: view-ID signature
ERR_DUP_M3 = -12            # errDupM3
ERR_BLOCK = -13             # verifyBlock refused the prepared block
ERR_DUP_M1 = -14            # errDupM1
ERR_VERIFY_M1 = -15         # errVerifyM1
ERR_PROOF_FORMAT = -16      # ReadSignatureBitmapByPublicKeys: length or encoding
ERR_NO_QUORUM = -17         # errNoQuorum
ERR_M1_PAYLOAD = -18        # errM1Payload
ERR_DUP_M2 = -19            # errDupM2
ERR_VERIFY_M2 = -20         # errVerifyM2

# verify_new_view()
NV_OK = 1
NV_ERR_M3_MISSING = -30
NV_ERR_M3_SIG = -31
NV_ERR_M2_SIG = -32
NV_ERR_M3_QUORUM = -33
NV_ERR_M1_FORMAT = -34
NV_ERR_M1_SIG = -35


def view_id_bytes(view_id: int) -> bytes:
    return view_id.to_bytes(8, "little")


def _popcount(bitmap: bytes) -> int:
    """utils.CountOneBits: every set bit of the raw bytes"""
    return sum(bin(b).count("1") for b in bitmap)


class DeviceBackend:
    """the default backend: one committee, its quorum policy and a
    one-committee ContextSet on the device"""

    def __init__(self, pks: bytes, n: int, power=None):
        from . import core
        self._core = core
        self.n = n
        self._power = None if power is None else list(power)
        self.committee = core.Committee(pks, n)
        self.committee.set_quorum(self._power)
        self.ctxset = core.ContextSet([self.committee])

    def verify_msgs(self, key_idx, sigs, msg_idx, msgs):
        batch = len(key_idx)
        return self.ctxset.verify_msgs([0] * batch, [[k] for k in key_idx], b"".join(sigs),
                                       msg_idx, msgs)

    def verify_seals(self, blobs, msgs, quorum):
        return self.ctxset.seal_verify([0] * len(blobs), blobs, msgs, quorum=quorum)

    def aggregate(self, sigs):
        return self._core.g2_aggregate(b"".join(sigs), len(sigs))

    def mask_power(self, bitmap):
        powers, counts = self.committee.mask_power(bitmap, 1)
        if self._power is None:
            quorum = counts[0] > 2 * self.n // 3
        else:
            quorum = powers[0] > self._core.TWO_THIRDS_DEC
        return powers[0], counts[0], quorum


class _ViewState:
    """bhpSigs/bhpBitmap (M1), nilSigs/nilBitmap (M2), viewIDSigs/viewIDBitmap
    (M3) of one view ID; the signature maps keep arrival order"""

    def __init__(self, n):
        nbytes = (n + 7) >> 3
        self.m1_sigs, self.m2_sigs, self.m3_sigs = {}, {}, {}
        self.m1_bitmap = bytearray(nbytes)
        self.m2_bitmap = bytearray(nbytes)
        self.m3_bitmap = bytearray(nbytes)


def _set_bit(bitmap, i):
    bitmap[i >> 3] |= 1 << (i & 7)


class ViewChange:
    """pks: n concatenated 48-byte keys; power None is the uniform policy,
    else n voting powers (votepower.compute).  backend: an object with
    verify_msgs(key_idx, sigs, msg_idx, msgs) -> codes,
    verify_seals(blobs, msgs, quorum) -> codes, aggregate(sigs) -> sig96 and
    mask_power(bitmap) -> (power, count, quorum); the default runs on the
    device.  verify_block(payload) -> truthy when the prepared block that
    comes with an M1 message is acceptable (default: always)."""

    def __init__(self, pks: bytes, n: int, power=None, backend=None, verify_block=None):
        if len(pks) != 48 * n:
            raise ValueError(f"expected {48 * n} key bytes got {len(pks)}")
        self.n = n
        self._backend = DeviceBackend(pks, n, power) if backend is None else backend
        self._verify_block = verify_block
        self._views = {}
        self._m1_payload = None
        self._good_proofs = set()

    @property
    def m1_payload(self):
        """the first accepted M1 payload (vc.m1Payload), or None"""
        return self._m1_payload

    def bitmaps(self, view_id):
        """(M1, M2, M3) bitmaps of a view ID; all-zero where nothing arrived"""
        st = self._views.get(view_id) or _ViewState(self.n)
        return bytes(st.m1_bitmap), bytes(st.m2_bitmap), bytes(st.m3_bitmap)

    @staticmethod
    def _is_m1(payload, has_block):
        return len(payload) >= VALID_PAYLOAD_LENGTH and bool(has_block)

    def process(self, messages):
        """messages, in arrival order: (sender_idx, view_id, payload, has_block,
        viewchange_sig, viewid_sig).  One code per message: VC_OK, or the first
        reason of ProcessViewChangeMsg behind onViewChangeSanityCheck."""
        messages = list(messages)
        codes = [None] * len(messages)
        table, table_pos = [], {}

        def entry(data):
            data = bytes(data)
            if data not in table_pos:
                table_pos[data] = len(table)
                table.append(data)
            return table_pos[data]

        key_idx, sigs, msg_idx, live = [], [], [], []
        proofs, proof_pos = [], {}
        for j, (sender, view_id, payload, has_block, vc_sig, id_sig) in enumerate(messages):
            if not 0 <= sender < self.n:
                codes[j] = ERR_SENDER
                continue
            if len(vc_sig) != 96 or len(id_sig) != 96:
                raise ValueError(f"message {j}: signatures must be 96 bytes")
            payload = bytes(payload)
            m1 = self._is_m1(payload, has_block)
            live.append(j)
            key_idx += [sender, sender]
            sigs += [bytes(id_sig), bytes(vc_sig)]
            msg_idx += [entry(view_id_bytes(view_id)), entry(payload if m1 else NIL)]
            if m1 and payload not in self._good_proofs and payload not in proof_pos:
                proof_pos[payload] = len(proofs)
                proofs.append(payload)
        if not live:
            return codes
        sig_codes = self._backend.verify_msgs(key_idx, sigs, msg_idx, table)
        if len(sig_codes) != len(key_idx):
            raise RuntimeError("backend returned a wrong number of codes")
        proof_codes = []
        if proofs:
            proof_codes = self._backend.verify_seals([p[32:] for p in proofs],
                                                     [p[:32] for p in proofs], True)
            if len(proof_codes) != len(proofs):
                raise RuntimeError("backend returned a wrong number of codes")
        for k, j in enumerate(live):
            sender, view_id, payload, has_block, vc_sig, id_sig = messages[j]
            payload = bytes(payload)
            proof = None
            if payload in proof_pos:
                proof = proof_codes[proof_pos[payload]]
            elif payload in self._good_proofs:
                proof = HBLS_OK
            codes[j] = self._apply(sender, view_id, payload, has_block, bytes(vc_sig),
                                   bytes(id_sig), sig_codes[2 * k], sig_codes[2 * k + 1],
                                   proof)
        return codes

    def _apply(self, sender, view_id, payload, has_block, vc_sig, id_sig, id_code, vc_code,
               proof):
        if id_code != HBLS_OK:
            return ERR_VIEWID_SIG
        st = self._views.get(view_id)
        if st is not None and sender in st.m3_sigs:
            return ERR_DUP_M3
        if self._is_m1(payload, has_block):
            if self._verify_block is not None and not self._verify_block(payload):
                return ERR_BLOCK
            if st is not None and sender in st.m1_sigs:
                return ERR_DUP_M1
            if vc_code != HBLS_OK:
                return ERR_VERIFY_M1
            if proof == NOQUORUM:
                return ERR_NO_QUORUM
            if proof == HBLS_FALSE:
                return ERR_M1_PAYLOAD
            if proof != HBLS_OK:
                return ERR_PROOF_FORMAT
            self._good_proofs.add(payload)
            st = self._views.setdefault(view_id, _ViewState(self.n))
            st.m1_sigs[sender] = vc_sig
            _set_bit(st.m1_bitmap, sender)
            st.m3_sigs[sender] = id_sig
            _set_bit(st.m3_bitmap, sender)
            if self._m1_payload is None:
                self._m1_payload = payload
            return VC_OK
        if st is not None and sender in st.m2_sigs:
            return ERR_DUP_M2
        if vc_code != HBLS_OK:
            return ERR_VERIFY_M2
        st = self._views.setdefault(view_id, _ViewState(self.n))
        st.m2_sigs[sender] = vc_sig
        _set_bit(st.m2_bitmap, sender)
        st.m3_sigs[sender] = id_sig
        _set_bit(st.m3_bitmap, sender)
        return VC_OK

    # -- GetM2Bitmap / GetM3Bitmap (view_change_construct.go:121-151)
    def get_m2_bitmap(self, view_id):
        st = self._views.get(view_id)
        if st is None or not st.m2_sigs:
            return None, None
        return self._backend.aggregate(list(st.m2_sigs.values())), bytes(st.m2_bitmap)

    def get_m3_bitmap(self, view_id):
        st = self._views.get(view_id)
        if st is None or not st.m3_sigs:
            return None, None
        return self._backend.aggregate(list(st.m3_sigs.values())), bytes(st.m3_bitmap)

    def verify_new_view(self, view_id, m3_sig, m3_bitmap, m2_sig, m2_bitmap, payload):
        """VerifyNewViewMsg (view_change_construct.go:154-203) and the checks
        onNewView makes behind it (view_change.go:477-500) on a NEWVIEW message,
        with one verify_seals call over the aggregates that are present.
        NV_OK, or the first failure in the reference's order."""
        if m3_sig is None or m3_bitmap is None:
            return NV_ERR_M3_MISSING
        payload = b"" if payload is None else bytes(payload)
        m1_due = m2_bitmap is None or _popcount(m3_bitmap) > _popcount(m2_bitmap)
        m1_sent = m1_due and len(payload) >= VALID_PAYLOAD_LENGTH
        blobs = [bytes(m3_sig) + bytes(m3_bitmap)]
        msgs = [view_id_bytes(view_id)]
        if m2_sig is not None:
            blobs.append(bytes(m2_sig) + bytes(m2_bitmap or b""))
            msgs.append(NIL)
        if m1_sent:
            blobs.append(payload[32:])
            msgs.append(payload[:32])
        codes = list(self._backend.verify_seals(blobs, msgs, False))
        if len(codes) != len(blobs):
            raise RuntimeError("backend returned a wrong number of codes")
        if codes.pop(0) != HBLS_OK:
            return NV_ERR_M3_SIG
        if m2_sig is not None and codes.pop(0) != HBLS_OK:
            return NV_ERR_M2_SIG
        if not self._backend.mask_power(bytes(m3_bitmap))[2]:
            return NV_ERR_M3_QUORUM
        if m1_due:
            if not m1_sent:
                return NV_ERR_M1_FORMAT
            code = codes.pop(0)
            if code == HBLS_FALSE:
                return NV_ERR_M1_SIG
            if code != HBLS_OK:
                return NV_ERR_M1_FORMAT
        return NV_OK
