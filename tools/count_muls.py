"""Measure the GPU path's OWN fp_mul counts per operation (instrumented
libhbls_count.so, -DHBLS_COUNT_MULS): settles the roofline denominator
against the oracle's op-counter and locates algorithmic-work levers.

Run on a GPU box:  python tools/count_muls.py [OUT.json]
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import pyref as pr  # noqa: E402

lib = ctypes.CDLL(os.path.join(REPO, "harmony_amd", "libhbls_count.so"))
lib.hbls_mulcount_read.restype = ctypes.c_uint64
lib.hbls_committee_build.restype = ctypes.c_void_p
lib.hbls_committee_build.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
lib.hbls_agg_verify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                ctypes.c_char_p, ctypes.c_size_t]
lib.hbls_mask_aggregate_g1.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]

assert lib.hbls_init(-1) == 1


def count(fn):
    lib.hbls_mulcount_reset()
    fn()
    return int(lib.hbls_mulcount_read())


out = {}
n = 4096
sks = b"".join(pr.fr_serialize(pr.synth_sk(i)) for i in range(n))
pks = ctypes.create_string_buffer(48 * n)
assert lib.hbls_batch_pk_from_sk(sks, n, pks) == 1
out["keygen_per_key"] = count(lambda: lib.hbls_batch_pk_from_sk(sks, n, pks)) // n
com = lib.hbls_committee_build(pks.raw, n)
assert com
out["committee_build_4096_total"] = count(
    lambda: None)  # build already done; placeholder 0

import random
rng = random.Random(42)
bm = bytearray(n // 8)
signers = [i for i in range(n) if rng.random() < 0.9]
for i in signers:
    bm[i >> 3] |= 1 << (i & 7)
bm = bytes(bm)
msg = pr.construct_commit_payload(1000, pr.synth_msg(1000), 17)
sk_sum = sum(pr.synth_sk(i) for i in signers) % pr.R
sig = ctypes.create_string_buffer(96)
assert lib.hbls_sign_hash(pr.fr_serialize(sk_sum), msg, len(msg), sig) == 1
sig = sig.raw

outp = ctypes.create_string_buffer(48)
out["mask_aggregate_4096_b09"] = count(
    lambda: lib.hbls_mask_aggregate_g1(com, bm, outp))
h96 = ctypes.create_string_buffer(96)
out["hash_to_g2"] = count(lambda: lib.hbls_hash_to_g2(msg, len(msg), h96))
out["g2_check_sig"] = count(lambda: lib.hbls_g2_check(sig))
out["g1_check_pk"] = count(lambda: lib.hbls_g1_check(pks.raw[:48]))

for thr, name in ((0, "scalar"), (1 << 30, "coop")):
    lib.hbls_set_coop_threshold(thr)
    out[f"agg_verify_total_{name}"] = count(
        lambda: lib.hbls_agg_verify(com, bm, sig, msg, len(msg)))
lib.hbls_set_coop_threshold(-1)

# aggregate verify, fp-mul per item: one all-valid batch of 64 (one chunk)
# through the thread-per-item kernels, exact (mode 0, a final exponentiation
# per item) against combined (mode 1, one per chunk).  Both
# figures are whole-pipeline; their difference is the verify stage's saving.
lib.hbls_batch_agg_verify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                      ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_int32)]
nb = 64
bres = (ctypes.c_int32 * nb)()
lib.hbls_set_coop_threshold(0)
lib.hbls_set_aggrlc_threshold(1)
for mode, name in ((0, "exact"), (1, "combined")):
    assert lib.hbls_set_agg_verify_mode(mode) == 1
    out[f"agg_verify_per_item_{name}"] = count(
        lambda: lib.hbls_batch_agg_verify(com, bm * nb, sig * nb, msg * nb, len(msg),
                                          nb, bres)) // nb
    assert list(bres) == [1] * nb, name
astats = (ctypes.c_uint32 * 3)()
lib.hbls_aggrlc_last_stats(astats)
out["agg_verify_combined_stats"] = list(astats)
assert list(astats) == [1, 0, 0]
out["verify_stage_saving_per_item"] = (out["agg_verify_per_item_exact"] -
                                       out["agg_verify_per_item_combined"])
# the combined path with the signature leg per item (leg 0) and once per chunk
# (leg 1), same batch.  The front (mask, hash, decompress) is
# the same launches in every mode, so the legs' difference is the verify
# stage's; the verify-stage figures subtract the front as counted by the
# single-item entries above.  The counter adds up what each lane's own control
# flow performs: it does not see the additions a wave executes for the other
# lanes' scalar bits in the bit-serial g1_mul / g2_mul.
front = out["mask_aggregate_4096_b09"] + out["hash_to_g2"] + out["g2_check_sig"]
out["front_per_item"] = front
assert lib.hbls_set_agg_verify_mode(1) == 1
for leg in (0, 1):
    assert lib.hbls_set_aggrlc_sigleg(leg) == 1
    out[f"agg_verify_per_item_combined_leg{leg}"] = count(
        lambda: lib.hbls_batch_agg_verify(com, bm * nb, sig * nb, msg * nb, len(msg),
                                          nb, bres)) // nb
    assert list(bres) == [1] * nb, leg
    out[f"verify_stage_per_item_combined_leg{leg}"] = (
        out[f"agg_verify_per_item_combined_leg{leg}"] - front)
out["verify_stage_per_item_exact"] = out["agg_verify_per_item_exact"] - front
# leg 1 under each item Miller kernel: 0 = affine arguments
# and the product kernel, 1 = Jacobian arguments, 2 = Jacobian arguments and
# the product across the wave (every lane multiplies in each of six rounds,
# where the product kernel's tree does 63 multiplications per chunk)
assert lib.hbls_set_aggrlc_sigleg(1) == 1
for lvl in (0, 1, 2):
    assert lib.hbls_set_aggrlc_miller(lvl) == 1
    out[f"agg_verify_per_item_combined_leg1_miller{lvl}"] = count(
        lambda: lib.hbls_batch_agg_verify(com, bm * nb, sig * nb, msg * nb, len(msg),
                                          nb, bres)) // nb
    assert list(bres) == [1] * nb, lvl
    out[f"verify_stage_per_item_combined_leg1_miller{lvl}"] = (
        out[f"agg_verify_per_item_combined_leg1_miller{lvl}"] - front)
lib.hbls_set_aggrlc_miller(-1)
lib.hbls_set_aggrlc_sigleg(-1)
lib.hbls_set_agg_verify_mode(-1)
lib.hbls_set_aggrlc_threshold(-1)
lib.hbls_set_coop_threshold(-1)

# vote verification, fp-mul per vote: one all-valid single-group tick of 4096
# through the stream, per-item pairing (mode 0) against random-combination
# batching (mode 1).  Both figures include the signature decompress.
lib.hbls_stream_create.restype = ctypes.c_void_p
lib.hbls_stream_create.argtypes = [ctypes.c_void_p, ctypes.c_int]
lib.hbls_stream_free.argtypes = [ctypes.c_void_p]
lib.hbls_stream_set_rounds.argtypes = [
    ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
    ctypes.c_char_p, ctypes.c_size_t]
lib.hbls_stream_set_verify_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
lib.hbls_stream_process.argtypes = [
    ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
    ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p,
    ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
    ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
vsigs = ctypes.create_string_buffer(96 * n)
assert lib.hbls_batch_sign(sks, msg * n, ctypes.c_size_t(len(msg)),
                           ctypes.c_size_t(n), vsigs) == 1
kidx = (ctypes.c_uint32 * n)(*range(n))
ridx = (ctypes.c_uint32 * n)()
slot0 = (ctypes.c_uint32 * 1)(0)
vres = (ctypes.c_int32 * n)()
# thread-per-item kernels throughout: the wave-cooperative kernels carry
# their own multiplier, which the counter does not see
lib.hbls_set_coop_threshold(0)
for mode, name in ((0, "item"), (1, "batched")):
    st = lib.hbls_stream_create(com, 1)
    assert st
    assert lib.hbls_stream_set_rounds(st, slot0, 1, msg, len(msg)) == 1
    assert lib.hbls_stream_set_verify_mode(st, mode) == 1
    out[f"vote_verify_per_vote_{name}"] = count(
        lambda: lib.hbls_stream_process(st, kidx, ridx, vsigs.raw, slot0, 1, n, vres)) // n
    assert list(vres) == [1] * n, name
    lib.hbls_stream_free(st)
lib.hbls_set_coop_threshold(-1)
stats =(ctypes.c_uint32 * 4)()
lib.hbls_rlc_last_stats(stats)
out["vote_verify_batched_rlc_stats"] = list(stats)
assert out["vote_verify_per_vote_batched"] < out["vote_verify_per_vote_item"]

# oracle comparison
from oracle import capi
capi.reset_op_count()
oc = capi.Committee(pks.raw, n)
capi.reset_op_count()
assert oc.agg_verify(bm, sig, msg) is True
out["oracle_agg_verify_total"] = capi.op_count()

print(json.dumps(out, indent=1))
if len(sys.argv) > 1:      # optional: also keep the counts in a file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
