"""ctypes binding of libhbls.so — THE PRODUCT PATH (HIP/CDNA4 kernels behind
the C-ABI in include/hbls.h).

Fails loudly if the library is missing or no AMD GPU is present: there is NO
CPU fallback here.  The CPU oracle under oracle/ is test infrastructure only.
"""
import contextlib
import ctypes
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("HBLS_SO", os.path.join(_DIR, "libhbls.so"))

HBLS_OK = 1
HBLS_FALSE = 0
HBLS_ERR = -1
HBLS_ERR_NOGPU = -2
HBLS_ERR_BADINPUT = -3
HBLS_NOQUORUM = -4
NOQUORUM = HBLS_NOQUORUM                 # per-item result of the *_quorum entries
TWO_THIRDS_DEC = 666666666666666667      # numeric.NewDec(2).Quo(numeric.NewDec(3)), 1e-18 units


class HblsError(RuntimeError):
    pass


class NoGpuError(HblsError):
    pass


class BadInputError(HblsError, ValueError):
    """HBLS_ERR_BADINPUT; a ValueError, as it has always been raised"""


def _load():
    if not os.path.exists(_SO):
        raise HblsError(
            f"libhbls.so not found at {_SO}: build it with "
            "`python -m harmony_amd.build` (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(_SO)
    lib.hbls_version.restype = ctypes.c_char_p
    lib.hbls_last_kernel_ns.restype = ctypes.c_uint64
    lib.hbls_last_stage_ns.restype = ctypes.c_uint64
    lib.hbls_mad_peak_ops.restype = ctypes.c_double
    lib.hbls_committee_build.restype = ctypes.c_void_p
    lib.hbls_committee_build.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.hbls_committee_free.argtypes = [ctypes.c_void_p]
    lib.hbls_committee_size.argtypes = [ctypes.c_void_p]
    lib.hbls_committee_size.restype = ctypes.c_size_t
    lib.hbls_mask_aggregate_g1.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.hbls_agg_verify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                    ctypes.c_char_p, ctypes.c_size_t]
    lib.hbls_batch_agg_verify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                          ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_batch_verify_votes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                            ctypes.c_char_p, ctypes.c_char_p,
                                            ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_construct_commit_payload.argtypes = [ctypes.c_uint64, ctypes.c_char_p,
                                                  ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p]
    lib.hbls_batch_seal_verify.argtypes = [
        ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
        ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_mask_partials.argtypes = [ctypes.c_void_p, ctypes.c_char_p,
                                       ctypes.c_size_t, ctypes.c_char_p]
    lib.hbls_msm_g1_committee.argtypes = [ctypes.c_void_p, ctypes.c_char_p,
                                          ctypes.c_char_p]
    lib.hbls_batch_agg_verify_partials.argtypes = [
        ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
        ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_stream_create.restype = ctypes.c_void_p
    lib.hbls_stream_create.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.hbls_stream_free.argtypes = [ctypes.c_void_p]
    lib.hbls_stream_set_rounds.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ctypes.c_char_p, ctypes.c_size_t]
    lib.hbls_stream_process.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p,
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_stream_check.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_stream_check_submit.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    lib.hbls_stream_check_poll.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_stream_get.argtypes = [ctypes.c_void_p, ctypes.c_uint32,
                                    ctypes.c_char_p, ctypes.c_char_p]
    lib.hbls_stream_set_verify_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.hbls_batch_verify_votes_grouped.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_char_p,
        ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_vote_key_sums.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_char_p,
        ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_batch_verify_votes_multi.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_char_p,
        ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_stream_process_multi.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
        ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
    lib.hbls_rlc_last_stats.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    lib.hbls_rlc_last_stats.restype = None
    lib.hbls_set_agg_verify_mode.argtypes = [ctypes.c_int]
    lib.hbls_set_aggrlc_threshold.argtypes = [ctypes.c_int]
    lib.hbls_set_aggrlc_threshold.restype = None
    lib.hbls_aggrlc_last_stats.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    lib.hbls_aggrlc_last_stats.restype = None
    lib.hbls_set_aggrlc_final.argtypes = [ctypes.c_int]
    lib.hbls_aggrlc_final_selftest.argtypes = [ctypes.c_int]
    lib.hbls_set_aggrlc_sigleg.argtypes = [ctypes.c_int]
    lib.hbls_set_aggrlc_early.argtypes = [ctypes.c_int]
    lib.hbls_set_aggrlc_chunkleg.argtypes = [ctypes.c_int]
    lib.hbls_set_aggrlc_miller.argtypes = [ctypes.c_int]
    lib.hbls_aggrlc_probe.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                      ctypes.c_char_p]
    lib.hbls_aggrlc_switch_value.argtypes = [ctypes.c_int, ctypes.c_size_t]
    lib.hbls_last_host_ns.restype = ctypes.c_uint64
    lib.hbls_last_host_ns.argtypes = [ctypes.c_int]
    u64p, u32p, i32p = (ctypes.POINTER(t) for t in
                        (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32))
    lib.hbls_committee_set_quorum.argtypes = [ctypes.c_void_p, u64p, ctypes.c_uint64]
    lib.hbls_mask_power.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                    u64p, u32p]
    lib.hbls_agg_verify_quorum.argtypes = lib.hbls_agg_verify.argtypes
    lib.hbls_batch_agg_verify_quorum.argtypes = lib.hbls_batch_agg_verify.argtypes
    lib.hbls_batch_seal_verify_quorum.argtypes = lib.hbls_batch_seal_verify.argtypes
    lib.hbls_stream_power.argtypes = [ctypes.c_void_p, u32p, ctypes.c_int,
                                      u64p, u32p, i32p]
    lib.hbls_last_stage_ns.argtypes = [ctypes.c_int]
    lib.hbls_copy_bench_ns.restype = ctypes.c_uint64
    lib.hbls_copy_bench_ns.argtypes = [ctypes.c_size_t]
    lib.hbls_fpmul_bench_waves.restype = ctypes.c_double
    lib.hbls_fpmul_bench_waves.argtypes = [ctypes.c_int, ctypes.c_int]
    # test hooks (not in include/hbls.h): device self-tests and the
    # operation-level arithmetic probe
    lib.hbls_coop_selftest.restype = ctypes.c_int
    lib.hbls_fpmul_asm_check.restype = ctypes.c_longlong
    lib.hbls_arith_probe.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.c_char_p, i32p]
    lib.hbls_arith_probe_op_name.argtypes = [ctypes.c_int]
    lib.hbls_arith_probe_op_name.restype = ctypes.c_char_p
    # the stage probe: hash-to-G2 and G2 decompress per kernel variant
    lib.hbls_hash_to_g2_probe.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.c_int, ctypes.c_char_p, i32p]
    lib.hbls_g2_decompress_probe.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                             ctypes.c_char_p, i32p]
    # epoch contexts; guarded so that an older library loads
    if hasattr(lib, "hbls_ctxset_create"):
        lib.hbls_ctxset_create.restype = ctypes.c_void_p
        lib.hbls_ctxset_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        lib.hbls_ctxset_free.argtypes = [ctypes.c_void_p]
        lib.hbls_ctxset_free.restype = None
        lib.hbls_ctxset_size.argtypes = [ctypes.c_void_p]
        lib.hbls_ctxset_size.restype = ctypes.c_size_t
        lib.hbls_batch_seal_verify_ctx.argtypes = [
            ctypes.c_void_p, u32p, ctypes.c_char_p, u32p, ctypes.c_char_p, u32p,
            ctypes.c_size_t, ctypes.c_int, i32p]
        lib.hbls_ctx_mask_sums.argtypes = [
            ctypes.c_void_p, u32p, ctypes.c_char_p, u32p, ctypes.c_size_t,
            ctypes.c_char_p, u64p, u32p, i32p]
    # signed-message windows
    if hasattr(lib, "hbls_batch_verify_msgs_ctx"):
        lib.hbls_batch_verify_msgs_ctx.argtypes = [
            ctypes.c_void_p, u32p, u32p, u32p, ctypes.c_char_p, u32p, ctypes.c_char_p,
            u32p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, i32p]
    return lib


_lib = _load()


def _check(rc, what):
    if rc == HBLS_ERR_NOGPU:
        raise NoGpuError(f"{what}: no AMD GPU available (product path requires gfx950)")
    if rc == HBLS_ERR_BADINPUT:
        raise BadInputError(f"{what}: bad input")
    if rc < 0:
        raise HblsError(f"{what}: error {rc}")
    return rc


def version() -> str:
    return _lib.hbls_version().decode()


def device_count() -> int:
    return _lib.hbls_device_count()


def init(device=-1):
    _check(_lib.hbls_init(device), "hbls_init")


def last_kernel_ns() -> int:
    return _lib.hbls_last_kernel_ns()


def last_stage_ns(i: int) -> int:
    """device time of stage i of the last aggregate-verify call on this
    thread: 0 mask aggregate, 1 hash-to-G2, 2 decompress, 3 pairing,
    7 quorum by mask (k_mask_power; for ContextSet.seal_verify the front:
    prepare and quorum by mask); in the plain entries 7 is the combined
    path's signature scaling and chunk sums"""
    return _lib.hbls_last_stage_ns(i)


def set_g2_cofactor_mode(fast: bool):
    _lib.hbls_set_g2_cofactor_mode(int(fast))


def set_coop_threshold(n: int):
    """batches <= n use the wave-cooperative (latency) kernels; larger use
    thread-per-item (throughput).  -1 restores the env/default value."""
    _lib.hbls_set_coop_threshold(n)


def rlc_chunk_size() -> int:
    """votes per refinement chunk of the batched (random-combination) path"""
    return _lib.hbls_rlc_chunk_size()


def rlc_last_stats():
    """[groups pairing-checked, groups failed, chunks re-checked, votes sent
    per-item] of the last batched call on this thread"""
    out = (ctypes.c_uint32 * 4)()
    _lib.hbls_rlc_last_stats(out)
    return list(out)


def set_agg_verify_mode(mode: int):
    """pairing stage of batch_agg_verify / batch_seal_verify: 0 exact (one
    final exponentiation per item), 1 combined (one per chunk of
    aggrlc_chunk_size() items, from the threshold up), -1 auto (default)"""
    _check(_lib.hbls_set_agg_verify_mode(mode), "set_agg_verify_mode")


def set_aggrlc_threshold(n: int):
    """smallest batch that takes the combined aggregate-verify path; -1
    restores the default"""
    _lib.hbls_set_aggrlc_threshold(n)


def aggrlc_chunk_size() -> int:
    """items that share one final exponentiation on the combined path"""
    return _lib.hbls_aggrlc_chunk_size()


def aggrlc_last_stats():
    """[chunks checked, chunks failed, items re-checked per item] of the last
    aggregate-verify call on this thread; zeros when it ran the exact path"""
    out = (ctypes.c_uint32 * 3)()
    _lib.hbls_aggrlc_last_stats(out)
    return list(out)


def set_aggrlc_final(kernel: int):
    """kernel of the combined path's final exponentiations: 16 or 8 = four
    lanes per chunk, that many chunks per block; 0 = one lane per chunk; -1
    restores the default.  Verdicts do not depend on it."""
    _check(_lib.hbls_set_aggrlc_final(kernel), "set_aggrlc_final")


def aggrlc_final_selftest(nchunks: int) -> int:
    """chunks on which the cooperative final kernels and the one-lane kernel
    disagree over nchunks deterministic chunk products (0 = parity)"""
    return _check(_lib.hbls_aggrlc_final_selftest(nchunks), "aggrlc_final_selftest")


def set_aggrlc_sigleg(leg: int):
    """where the combined path pairs the signatures: 0 = one
    Miller leg per item, 1 = one per chunk on the chunk's scaled signature
    sum, -1 = the default rule.  Verdicts and stats do not depend on it."""
    _check(_lib.hbls_set_aggrlc_sigleg(leg), "set_aggrlc_sigleg")


def set_aggrlc_early(early: int):
    """when the chunk-level signature leg is paired: 0 =
    inside the Miller kernel, behind the items; 1 = hoisted: the signature
    chain runs ahead of the mask kernel and the chunk legs beside it on a
    side stream (plain, seal and quorum entries; ContextSet.seal_verify keeps
    the sequence of 0); -1 = the default rule.  Verdicts and stats do not
    depend on it.  last_stage_ns(8) is the chunk-leg kernel's own interval,
    zero when nothing was hoisted."""
    _check(_lib.hbls_set_aggrlc_early(early), "set_aggrlc_early")


def set_aggrlc_chunkleg(kernel: int):
    """kernel of the hoisted chunk legs: 16 = four lanes per
    chunk, 16 chunks per block; 0 = one lane per chunk; -1 restores the
    default.  Verdicts do not depend on it."""
    _check(_lib.hbls_set_aggrlc_chunkleg(kernel), "set_aggrlc_chunkleg")


def set_aggrlc_miller(level: int):
    """level of the chunk-level leg's item kernel, k_aggrlc_item (DESIGN.md
    §4m, §4n): 0 = affine arguments and a product kernel of its own; 1 =
    Jacobian arguments, no inversion; 2 = that, and the chunk product inside
    the item kernel; -1 restores the default.  Verdicts and stats do not
    depend on it."""
    _check(_lib.hbls_set_aggrlc_miller(level), "set_aggrlc_miller")


_AGGRLC_SETTERS = {"mode": set_agg_verify_mode, "threshold": set_aggrlc_threshold,
                   "sigleg": set_aggrlc_sigleg, "early": set_aggrlc_early,
                   "miller": set_aggrlc_miller, "final": set_aggrlc_final,
                   "chunkleg": set_aggrlc_chunkleg}
AGGRLC_SWITCHES = ("mode", "final", "sigleg", "early", "miller", "chunkleg")


@contextlib.contextmanager
def aggrlc_switches(**values):
    """Set the given switches of the combined path (mode, threshold, sigleg,
    early, miller, final, chunkleg: the arguments of the set_* functions
    above) for the body of a `with`, and put every one of them back to -1 on
    the way out, exceptions included.  The switches are process-global, so a
    missed restore would reach every later call.  If a setter rejects a value
    nothing stays applied and its BadInputError is raised."""
    unknown = set(values) - set(_AGGRLC_SETTERS)
    if unknown:
        raise TypeError("aggrlc_switches: unknown switch %s" % sorted(unknown))
    try:
        for name, v in values.items():
            _AGGRLC_SETTERS[name](v)
        yield
    finally:
        for name in values:
            _AGGRLC_SETTERS[name](-1)


def aggrlc_switch_value(name: str, batch: int = 0) -> int:
    """Test hook (needs no GPU): what switch `name` of AGGRLC_SWITCHES resolves
    to for a call over `batch` items — the value set or read from the
    environment, with the sigleg and early rules applied to `batch`; -1 is
    the mode's auto."""
    return _lib.hbls_aggrlc_switch_value(AGGRLC_SWITCHES.index(name), batch)


AGGRLC_PROBE_OPS = {"g1_mul64w": (0, 3 * 48 + 8, 3 * 48),
                    "g2_mul64w": (1, 6 * 48 + 8, 6 * 48),
                    "miller1_fe": (2, 6 * 48, 12 * 48),
                    "miller1j_fe": (3, 9 * 48, 12 * 48),
                    "wave_prod": (4, 64 * 12 * 48, 2 * 12 * 48)}


def aggrlc_probe(name: str, data: bytes, n_items: int) -> bytes:
    """Test hook: run g1_mul64w / g2_mul64w (Jacobian
    point and a little-endian u64 scalar per item), miller1_fe (affine Q,
    affine P), miller1j_fe (Jacobian Q, Jacobian P) or wave_prod (64 fp12 per
    item; the product as held by lane 0 and by lane 63) on raw device-domain
    limbs; returns the raw results."""
    op, in_b, out_b = AGGRLC_PROBE_OPS[name]
    if len(data) != n_items * in_b:
        raise ValueError("aggrlc_probe: operand size")
    out = ctypes.create_string_buffer(max(1, n_items * out_b))
    _check(_lib.hbls_aggrlc_probe(op, data, n_items, out), "aggrlc_probe")
    return out.raw[:n_items * out_b]


def last_host_ns(i: int) -> int:
    """host-side time of the last aggregate-verify call on this thread:
    0 device allocations, 1 inside upload calls, 2 first launch to results
    on the host, 3 frees, 4 the whole call"""
    return _lib.hbls_last_host_ns(i)


def pk_from_sk(sk32: bytes) -> bytes:
    out = ctypes.create_string_buffer(48)
    _check(_lib.hbls_pk_from_sk(sk32, out), "pk_from_sk")
    return out.raw


def batch_pk_from_sk(sks: bytes, batch: int) -> bytes:
    out = ctypes.create_string_buffer(48 * batch)
    _check(_lib.hbls_batch_pk_from_sk(sks, batch, out), "batch_pk_from_sk")
    return out.raw


def sign_hash(sk32: bytes, msg: bytes) -> bytes:
    out = ctypes.create_string_buffer(96)
    _check(_lib.hbls_sign_hash(sk32, msg, len(msg), out), "sign_hash")
    return out.raw


def batch_sign(sks: bytes, msgs: bytes, mlen: int, batch: int) -> bytes:
    out = ctypes.create_string_buffer(96 * batch)
    _check(_lib.hbls_batch_sign(sks, msgs, mlen, batch, out), "batch_sign")
    return out.raw


def hash_to_g2(msg: bytes) -> bytes:
    out = ctypes.create_string_buffer(96)
    _check(_lib.hbls_hash_to_g2(msg, len(msg), out), "hash_to_g2")
    return out.raw


def batch_hash_to_g2(msgs: bytes, mlen: int, batch: int) -> bytes:
    out = ctypes.create_string_buffer(96 * batch)
    _check(_lib.hbls_batch_hash_to_g2(msgs, mlen, batch, out), "batch_hash_to_g2")
    return out.raw


def verify_hash(pk48: bytes, sig96: bytes, msg: bytes) -> bool:
    rc = _lib.hbls_verify_hash(pk48, sig96, msg, len(msg))
    return _check(rc, "verify_hash") == HBLS_OK


def g1_add(a: bytes, b: bytes) -> bytes:
    out = ctypes.create_string_buffer(48)
    _check(_lib.hbls_g1_add(a, b, out), "g1_add")
    return out.raw


def g1_sub(a: bytes, b: bytes) -> bytes:
    out = ctypes.create_string_buffer(48)
    _check(_lib.hbls_g1_sub(a, b, out), "g1_sub")
    return out.raw


def g2_add(a: bytes, b: bytes) -> bytes:
    out = ctypes.create_string_buffer(96)
    _check(_lib.hbls_g2_add(a, b, out), "g2_add")
    return out.raw


def g1_check(p48: bytes) -> bool:
    return _check(_lib.hbls_g1_check(p48), "g1_check") == HBLS_OK


def g2_check(p96: bytes) -> bool:
    return _check(_lib.hbls_g2_check(p96), "g2_check") == HBLS_OK


def msm_g1(points: bytes, scalars: bytes, n: int) -> bytes:
    out = ctypes.create_string_buffer(48)
    _check(_lib.hbls_msm_g1(points, scalars, n, out), "msm_g1")
    return out.raw


def g2_aggregate(sigs_cat: bytes, n: int) -> bytes:
    out = ctypes.create_string_buffer(96)
    _check(_lib.hbls_g2_aggregate(sigs_cat, n, out), "g2_aggregate")
    return out.raw


def batch_keccak256(msgs: bytes, mlen: int, batch: int) -> bytes:
    out = ctypes.create_string_buffer(32 * batch)
    _check(_lib.hbls_batch_keccak256(msgs, mlen, batch, out), "batch_keccak")
    return out.raw


COOP_SELFTEST_STAGES = ("fp12_mul", "fp12_sqr", "mul_line", "cyc_sqr", "dbl_step",
                        "add_step", "pow_u", "final_exp")


def coop_selftest() -> int:
    """k_coop_selftest: every cooperative building block against its scalar
    twin on the device.  0 = all equal; bit i set = stage i of
    COOP_SELFTEST_STAGES differs; negative = the launch failed."""
    return _lib.hbls_coop_selftest()


def coop_selftest_failed_stages(mask: int):
    return [s for i, s in enumerate(COOP_SELFTEST_STAGES) if mask >> i & 1]


def fpmul_asm_check() -> int:
    """mismatches between the generated asm CIOS core and the C body over
    dependent chains of random operands; 0 = bit-exact, -1 = launch failed"""
    return _lib.hbls_fpmul_asm_check()


def arith_probe_ops():
    """names of the probe's operations, by operation number"""
    return [_lib.hbls_arith_probe_op_name(i).decode()
            for i in range(_lib.hbls_arith_probe_op_count())]


def arith_probe(op: int, data: bytes, n_items: int, out_fp: int):
    """Test hook: run operation `op` on n_items operand sets
    of raw device-domain limbs.  Returns (out bytes, n_items x out_fp x 48;
    flags, one int per item)."""
    out = ctypes.create_string_buffer(max(1, n_items * out_fp * 48))
    flags = (ctypes.c_int32 * max(1, n_items))()
    _check(_lib.hbls_arith_probe(op, data, n_items, out, flags), "arith_probe")
    return out.raw[:n_items * out_fp * 48], list(flags)[:n_items]


STAGE_KERNELS = ("scalar", "coop")      # the stage probe's kernel numbers 0 and 1


def hash_to_g2_probe(msgs: bytes, mlen: int, batch: int, kernel: int):
    """Test hook: hash batch messages of mlen bytes with
    k_hash_to_g2 (kernel 0) or k_hash_to_g2_coop through its production
    launcher (kernel 1), in the current cofactor mode.  Returns (batch x 96
    serialized bytes, zero where ok is 0; the per-item ok flags)."""
    if len(msgs) != mlen * batch:
        raise ValueError("hash_to_g2_probe: %d bytes for %d x %d" % (len(msgs), batch, mlen))
    out = ctypes.create_string_buffer(max(1, 96 * batch))
    ok = (ctypes.c_int32 * max(1, batch))()
    _check(_lib.hbls_hash_to_g2_probe(msgs, mlen, batch, kernel, out, ok), "hash_to_g2_probe")
    return out.raw[:96 * batch], list(ok)[:batch]


def g2_decompress_probe(sigs: bytes, batch: int, kernel: int):
    """Test hook: decompress and subgroup-check batch
    signatures with k_g2_decompress (kernel 0) or k_g2_decompress_coop
    (kernel 1).  Returns (batch x 4 x 48 bytes, the affine x.a, x.b, y.a, y.b
    as raw Montgomery limbs, meaningful where the flag is 1; the per-item
    flags: 0 bad, 1 ok, 2 infinity)."""
    if len(sigs) != 96 * batch:
        raise ValueError("g2_decompress_probe: %d bytes for %d signatures" % (len(sigs), batch))
    out = ctypes.create_string_buffer(max(1, 192 * batch))
    flags = (ctypes.c_int32 * max(1, batch))()
    _check(_lib.hbls_g2_decompress_probe(sigs, batch, kernel, out, flags),
           "g2_decompress_probe")
    return out.raw[:192 * batch], list(flags)[:batch]


def hash_edge_count() -> int:
    """items k_hash_to_g2_coop has sent down its exact scalar recompute since
    the last reset (a degenerate addition in the cofactor chain, or the
    full-cofactor mode); -1 if the counter cannot be read"""
    return _lib.hbls_hash_edge_count()


def hash_edge_reset():
    if not _lib.hbls_hash_edge_reset():
        raise HblsError("hash_edge_reset failed")


def construct_commit_payload(block_num: int, hash32: bytes, view_id: int,
                             staking: bool = True) -> bytes:
    out = ctypes.create_string_buffer(48)
    n = _lib.hbls_construct_commit_payload(block_num, hash32, view_id, int(staking), out)
    return out.raw[:n]


def parse_commit_sig_bitmap(payload: bytes):
    sig = ctypes.create_string_buffer(96)
    bm = ctypes.create_string_buffer(max(len(payload), 96) - 96 + 1)
    n = _lib.hbls_parse_commit_sig_bitmap(payload, len(payload), sig, bm, len(payload))
    if n < 0:
        raise ValueError("payload too short")
    return sig.raw, bm.raw[:n]


def pack_key_lists(key_lists, batch=None):
    """Signer sets in the CSR form of the multi-key entries:
    returns (key_off, key_idx) with vote j signed by
    key_idx[key_off[j]:key_off[j + 1]].  Lists are taken as they are — whether
    one is well formed (non-empty, in range, strictly ascending) is the
    device's per-vote verdict.  batch, when given, is the number of votes the
    caller's other arrays hold; a different number of lists raises ValueError.
    Needs no GPU."""
    if batch is not None and len(key_lists) != batch:
        raise ValueError(f"expected {batch} key lists got {len(key_lists)}")
    key_off, key_idx = [0], []
    for keys in key_lists:
        for k in keys:
            if not 0 <= k < 1 << 32:
                raise ValueError(f"key index {k} is not a uint32")
            key_idx.append(k)
        key_off.append(len(key_idx))
    if key_off[-1] >= 1 << 31:
        raise ValueError("too many key indices for one call")
    return key_off, key_idx


def pack_blobs(blobs):
    """Byte strings of any lengths in the CSR form of the epoch-context
    entries: returns (cat, off) with item j at
    cat[off[j]:off[j + 1]]; off holds len(blobs) + 1 uint32 values.  Raises
    BadInputError when the total exceeds 2^32 - 1.  Needs no GPU."""
    off, total = [0], 0
    for b in blobs:
        total += len(b)
        if total > 0xffffffff:
            raise BadInputError("pack_blobs: more than 2^32 - 1 bytes in one call")
        off.append(total)
    return b"".join(blobs), off


def _csr_arrays(key_lists, batch, csr=None):
    """ctypes (key_off, key_idx, batch) of key_lists, or of a caller's raw
    csr=(key_off, key_idx) pair, which is passed on unchecked but for its
    length"""
    if csr is None:
        key_off, key_idx = pack_key_lists(key_lists, batch)
    else:
        key_off, key_idx = csr
        if not key_off or (batch is not None and len(key_off) != batch + 1):
            raise ValueError("key_off must hold batch + 1 entries")
        if any(o > len(key_idx) for o in key_off):
            raise ValueError("key_off points past key_idx")
    return ((ctypes.c_uint32 * len(key_off))(*key_off),
            (ctypes.c_uint32 * max(len(key_idx), 1))(*key_idx), len(key_off) - 1)


class Committee:
    """Device-resident, validated pubkey table (UpdateParticipants equivalent)."""

    def __init__(self, pks_cat: bytes, n: int):
        self._h = _lib.hbls_committee_build(pks_cat, n)
        if not self._h:
            if device_count() == 0:
                raise NoGpuError("committee_build: no AMD GPU")
            raise ValueError("committee_build: invalid pubkey in table")
        self.n = n
        self._quorum_set = False

    def _bitmap_len(self) -> int:
        return (self.n + 7) >> 3

    def _check_bitmaps(self, bitmaps: bytes, batch: int, what: str):
        """Mask.SetMask errors on a length mismatch (crypto/bls/mask.go:113-118);
        the FFI memcpys ceil(n/8) bytes per item, so a short buffer would read
        out of bounds.  Validate before crossing the ABI."""
        want = self._bitmap_len() * batch
        if len(bitmaps) != want:
            raise ValueError(
                f"{what}: mismatching bitmap lengths expected {want} got {len(bitmaps)}")

    def mask_aggregate(self, bitmap: bytes) -> bytes:
        self._check_bitmaps(bitmap, 1, "mask_aggregate")
        out = ctypes.create_string_buffer(48)
        _check(_lib.hbls_mask_aggregate_g1(self._h, bitmap, out), "mask_aggregate")
        return out.raw

    def agg_verify(self, bitmap: bytes, sig96: bytes, msg: bytes) -> bool:
        self._check_bitmaps(bitmap, 1, "agg_verify")
        rc = _lib.hbls_agg_verify(self._h, bitmap, sig96, msg, len(msg))
        return _check(rc, "agg_verify") == HBLS_OK

    def batch_agg_verify(self, bitmaps: bytes, sigs: bytes, msgs: bytes,
                         mlen: int, batch: int):
        self._check_bitmaps(bitmaps, batch, "batch_agg_verify")
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_agg_verify(self._h, bitmaps, sigs, msgs, mlen,
                                          batch, res), "batch_agg_verify")
        return list(res)

    def mask_partials(self, bitmaps: bytes, batch: int) -> bytes:
        self._check_bitmaps(bitmaps, batch, "mask_partials")
        out = ctypes.create_string_buffer(48 * batch)
        _check(_lib.hbls_mask_partials(self._h, bitmaps, batch, out), "mask_partials")
        return out.raw

    def batch_agg_verify_partials(self, bitmaps: bytes, ext48s: bytes, n_ext: int,
                                  sigs: bytes, msgs: bytes, mlen: int, batch: int):
        self._check_bitmaps(bitmaps, batch, "batch_agg_verify_partials")
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_agg_verify_partials(
            self._h, bitmaps, ext48s, n_ext, sigs, msgs, mlen, batch, res),
            "batch_agg_verify_partials")
        return list(res)

    def batch_seal_verify(self, sig_bitmaps: bytes, blob_len: int,
                          msgs: bytes, mlen: int, batch: int):
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_seal_verify(self._h, sig_bitmaps, blob_len,
                                           msgs, mlen, batch, res),
               "batch_seal_verify")
        return list(res)

    # -- quorum by mask
    def set_quorum(self, power=None, threshold=None):
        """the epoch's qrVerifier (engine.go:644-659).  power None: uniform
        policy, quorum is popcount > floor(2n/3).  Otherwise n voting powers
        in 1e-18 units (votepower.compute) and quorum is masked sum >
        threshold (default TWO_THIRDS_DEC).  Call before sharing the
        committee between threads."""
        if power is None:
            rc = _lib.hbls_committee_set_quorum(self._h, None, 0)
        else:
            if len(power) != self.n:
                raise ValueError(f"set_quorum: expected {self.n} powers got {len(power)}")
            if any(p < 0 or p >> 64 for p in power):
                raise BadInputError("set_quorum: power out of range")
            arr = (ctypes.c_uint64 * self.n)(*power)
            rc = _lib.hbls_committee_set_quorum(
                self._h, arr, TWO_THIRDS_DEC if threshold is None else threshold)
        _check(rc, "set_quorum")
        self._quorum_set = True

    def mask_power(self, bitmaps: bytes, batch: int):
        """(powers, counts): masked voting-power sum and in-range popcount
        of each bitmap (ComputeTotalPowerByMask / CountOneBits)"""
        self._check_bitmaps(bitmaps, batch, "mask_power")
        pw = (ctypes.c_uint64 * batch)()
        cn = (ctypes.c_uint32 * batch)()
        _check(_lib.hbls_mask_power(self._h, bitmaps, batch, pw, cn), "mask_power")
        return list(pw), list(cn)

    def agg_verify_quorum(self, bitmap: bytes, sig96: bytes, msg: bytes) -> int:
        """verifySignature (engine.go:619-642): 1 accept, 0 reject, NOQUORUM;
        other negative codes raise"""
        self._check_bitmaps(bitmap, 1, "agg_verify_quorum")
        rc = _lib.hbls_agg_verify_quorum(self._h, bitmap, sig96, msg, len(msg))
        return rc if rc == NOQUORUM else _check(rc, "agg_verify_quorum")

    def batch_agg_verify_quorum(self, bitmaps: bytes, sigs: bytes, msgs: bytes,
                                mlen: int, batch: int):
        """batch_agg_verify behind the quorum-by-mask gate: items without
        quorum get NOQUORUM and never reach the pairing"""
        self._check_bitmaps(bitmaps, batch, "batch_agg_verify_quorum")
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_agg_verify_quorum(self._h, bitmaps, sigs, msgs, mlen,
                                                 batch, res), "batch_agg_verify_quorum")
        return list(res)

    def batch_seal_verify_quorum(self, sig_bitmaps: bytes, blob_len: int,
                                 msgs: bytes, mlen: int, batch: int):
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_seal_verify_quorum(self._h, sig_bitmaps, blob_len,
                                                  msgs, mlen, batch, res),
               "batch_seal_verify_quorum")
        return list(res)

    def msm(self, scalars_cat: bytes) -> bytes:
        """Pippenger MSM over the resident validated table: sum s_i * pk_i"""
        if len(scalars_cat) != 32 * self.n:
            raise ValueError("msm: scalars must be n*32 bytes")
        out = ctypes.create_string_buffer(48)
        _check(_lib.hbls_msm_g1_committee(self._h, scalars_cat, out), "msm_committee")
        return out.raw

    def batch_verify_votes(self, key_idx, sigs: bytes, msgs: bytes, mlen: int):
        batch = len(key_idx)
        idx = (ctypes.c_uint32 * batch)(*key_idx)
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_verify_votes(self._h, idx, sigs, msgs, mlen,
                                            batch, res), "batch_verify_votes")
        return list(res)

    def batch_verify_votes_grouped(self, key_idx, group_idx, sigs: bytes,
                                   msgs: bytes, mlen: int):
        """batch_verify_votes for votes that share messages: vote j signs
        msgs[group_idx[j]]; one pairing per group (random combination), same
        per-vote codes.  An out-of-range group index gives HBLS_ERR_BADINPUT
        for that vote."""
        batch = len(key_idx)
        if len(group_idx) != batch or len(sigs) != 96 * batch:
            raise ValueError("key_idx/group_idx/sigs length mismatch")
        if mlen <= 0 or len(msgs) % mlen:
            raise ValueError("msgs must be n_groups * mlen bytes")
        idx = (ctypes.c_uint32 * batch)(*key_idx)
        grp = (ctypes.c_uint32 * batch)(*group_idx)
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_verify_votes_grouped(
            self._h, idx, grp, sigs, msgs, mlen, len(msgs) // mlen, batch, res),
            "batch_verify_votes_grouped")
        return list(res)

    # -- multi-key votes
    def vote_key_sums(self, key_lists, csr=None):
        """(sums, ok): the serialized key sum of each vote's signer set
        (signerPubKey, leader.go:165-172) and 1 / HBLS_ERR_BADINPUT per vote.
        An infinity sum and a malformed vote's block are 48 zero bytes."""
        off, idx, batch = _csr_arrays(key_lists, None, csr)
        if batch == 0:
            return [], []
        out = ctypes.create_string_buffer(48 * batch)
        ok = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_vote_key_sums(self._h, off, idx, batch, out, ok),
               "vote_key_sums")
        return [out.raw[48 * j:48 * (j + 1)] for j in range(batch)], list(ok)

    def batch_verify_votes_multi(self, key_lists, sigs: bytes, msgs: bytes, mlen: int):
        """batch_verify_votes for signer sets: vote j is checked against the
        sum of its keys; a malformed key list gives HBLS_ERR_BADINPUT for
        that vote."""
        if len(sigs) % 96:
            raise ValueError("sigs must be batch * 96 bytes")
        off, idx, batch = _csr_arrays(key_lists, len(sigs) // 96)
        if mlen <= 0 or len(msgs) != mlen * batch:
            raise ValueError("msgs must be batch * mlen bytes")
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_verify_votes_multi(self._h, off, idx, sigs, msgs, mlen,
                                                  batch, res), "batch_verify_votes_multi")
        return list(res)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.hbls_committee_free(self._h)
        except Exception:
            pass


class ContextSet:
    """Device-resident table of epoch contexts: several
    committees behind one batch call.  Item j of a call names its committee by
    ctx_idx[j], the position in `committees`.  Each committee's set_quorum, if
    it is to be used, must have been called before the set is built."""

    def __init__(self, committees):
        if not hasattr(_lib, "hbls_ctxset_create"):
            raise HblsError("this libhbls.so has no epoch-context entries: rebuild it")
        self.committees = list(committees)    # keep alive: the set borrows them
        n = len(self.committees)
        arr = (ctypes.c_void_p * max(n, 1))(*[c._h for c in self.committees])
        self._h = _lib.hbls_ctxset_create(arr, n)
        if not self._h:
            if device_count() == 0:
                raise NoGpuError("ctxset_create: no AMD GPU")
            raise BadInputError("ctxset_create: empty set or invalid committee")

    def __len__(self):
        return _lib.hbls_ctxset_size(self._h)

    @staticmethod
    def _u32(values, what):
        if any(not 0 <= v <= 0xffffffff for v in values):
            raise BadInputError(f"{what}: not a uint32")
        return (ctypes.c_uint32 * max(len(values), 1))(*values)

    def seal_verify(self, ctx_idx, blobs, msgs, quorum=False, offsets=None):
        """verifySignature over a window that mixes contexts: blobs[j] is the
        raw commitSigAndBitmap of item j, msgs[j] its payload (any length),
        ctx_idx[j] its committee.  Per item 1 accept, 0 reject,
        HBLS_ERR_BADINPUT (context index out of range, or a blob that is not
        96 + ceil(n/8) bytes of its committee) and, with quorum=True,
        NOQUORUM.  offsets=(blob_off, msg_off) replaces the offsets computed
        from the lists (passed on as they are)."""
        batch = len(ctx_idx)
        if len(blobs) != batch or len(msgs) != batch:
            raise ValueError("ctx_idx/blobs/msgs length mismatch")
        if batch == 0:
            return []
        bcat, boff = pack_blobs(blobs)
        mcat, moff = pack_blobs(msgs)
        if offsets is not None:
            boff, moff = offsets
            if len(boff) != batch + 1 or len(moff) != batch + 1:
                raise ValueError("offsets must hold batch + 1 entries")
            if max(boff) > len(bcat) or max(moff) > len(mcat):
                raise ValueError("offsets point past the data")
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_batch_seal_verify_ctx(
            self._h, self._u32(ctx_idx, "ctx_idx"), bcat, self._u32(boff, "blob_off"),
            mcat, self._u32(moff, "msg_off"), batch, int(bool(quorum)), res),
            "batch_seal_verify_ctx")
        return list(res)

    def mask_sums(self, ctx_idx, bitmaps):
        """(sums, powers, counts, ok) of bare bitmaps against their contexts:
        serialized masked key sum (48 zero bytes = infinity), masked voting
        power, in-range popcount, and 1 / HBLS_ERR_BADINPUT per item (a bad
        item has a zero block, power 0 and count 0)."""
        batch = len(ctx_idx)
        if len(bitmaps) != batch:
            raise ValueError("ctx_idx/bitmaps length mismatch")
        if batch == 0:
            return [], [], [], []
        cat, off = pack_blobs(bitmaps)
        out = ctypes.create_string_buffer(48 * batch)
        pw = (ctypes.c_uint64 * batch)()
        cn = (ctypes.c_uint32 * batch)()
        ok = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_ctx_mask_sums(
            self._h, self._u32(ctx_idx, "ctx_idx"), cat, self._u32(off, "bm_off"), batch,
            out, pw, cn, ok), "ctx_mask_sums")
        return ([out.raw[48 * j:48 * (j + 1)] for j in range(batch)], list(pw), list(cn),
                list(ok))

    def verify_msgs(self, ctx_idx, key_lists, sigs: bytes, msg_idx, msgs, digest=None,
                    csr=None):
        """Single verifies over a window that mixes committees and messages
        (DESIGN.md §4p): item j is sigs[96 * j:96 * (j + 1)] by the keys
        key_lists[j] of committee ctx_idx[j] over msgs[msg_idx[j]].  msgs is a
        list of byte strings of any lengths, each hashed to G2 once; where
        digest[i] is true the message signed is keccak256(msgs[i]), computed on
        the device.  Per item 1 accept, 0 reject, HBLS_ERR_BADINPUT (context or
        message index out of range, malformed key list, undecodable signature,
        a message that does not hash).  csr=(key_off, key_idx) replaces
        key_lists, csr=(key_off, key_idx, msg_off) the message offsets too
        (key_off None keeps key_lists); they are passed on as they are.  An
        empty batch, an empty message table and offsets that do not start at 0
        or that decrease raise BadInputError."""
        if not hasattr(_lib, "hbls_batch_verify_msgs_ctx"):
            raise HblsError("this libhbls.so has no signed-message entry: rebuild it")
        batch = len(ctx_idx)
        if len(sigs) != 96 * batch or len(msg_idx) != batch:
            raise ValueError("ctx_idx/sigs/msg_idx length mismatch")
        if digest is not None and len(digest) != len(msgs):
            raise ValueError("digest must hold one flag per message")
        key_csr = None if csr is None or csr[0] is None else (csr[0], csr[1])
        off, idx, _ = _csr_arrays(key_lists, batch, key_csr)
        mcat, moff = pack_blobs(msgs)
        if csr is not None and len(csr) > 2:
            moff = list(csr[2])
            if len(moff) != len(msgs) + 1:
                raise ValueError("msg_off must hold len(msgs) + 1 entries")
            if max(moff) > len(mcat):
                raise ValueError("msg_off points past the data")
        flags = None if digest is None else bytes(1 if d else 0 for d in digest)
        res = (ctypes.c_int32 * max(batch, 1))()
        _check(_lib.hbls_batch_verify_msgs_ctx(
            self._h, self._u32(ctx_idx, "ctx_idx"), off, idx, sigs,
            self._u32(msg_idx, "msg_idx"), mcat, self._u32(moff, "msg_off"), len(msgs),
            flags, batch, res), "batch_verify_msgs_ctx")
        return list(res)[:batch]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.hbls_ctxset_free(self._h)
        except Exception:
            pass


class Stream:
    """Device-resident FBFT vote stream (config 5): per-round hash points,
    bitmaps and running G2 aggregates live in HBM; one hbls_stream_process
    call per tick.  Mirrors the leader's per-message loop
    (consensus/leader.go:221-309) — see include/hbls.h."""

    def __init__(self, committee: "Committee", max_rounds: int):
        self.committee = committee        # keep alive: C ctx borrows its table
        self.n = committee.n
        self.max_rounds = max_rounds
        self._h = _lib.hbls_stream_create(committee._h, max_rounds)
        if not self._h:
            if device_count() == 0:
                raise NoGpuError("stream_create: no AMD GPU")
            raise HblsError("stream_create failed")

    def set_rounds(self, slots, payloads_cat: bytes, payload_len: int):
        k = len(slots)
        if payload_len * k != len(payloads_cat):
            raise ValueError("payloads must be k * payload_len bytes")
        arr = (ctypes.c_uint32 * k)(*slots)
        _check(_lib.hbls_stream_set_rounds(self._h, arr, k, payloads_cat,
                                           payload_len), "stream_set_rounds")

    def set_verify_mode(self, mode: int):
        """0: one pairing per vote (default); 1: batched, one pairing per
        round present in a tick.  Results are the same either way."""
        _check(_lib.hbls_stream_set_verify_mode(self._h, mode),
               "stream_set_verify_mode")

    def process(self, key_idx, round_idx, sigs_cat: bytes):
        batch = len(key_idx)
        if len(round_idx) != batch or len(sigs_cat) != 96 * batch:
            raise ValueError("key_idx/round_idx/sigs length mismatch")
        active = sorted(set(round_idx))
        ki = (ctypes.c_uint32 * batch)(*key_idx)
        ri = (ctypes.c_uint32 * batch)(*round_idx)
        act = (ctypes.c_uint32 * len(active))(*active)
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_stream_process(self._h, ki, ri, sigs_cat, act,
                                        len(active), batch, res), "stream_process")
        return list(res)

    def process_multi(self, key_lists, round_idx, sigs_cat: bytes):
        """process() for multi-key votes: vote j is signed by the keys
        key_lists[j] (ascending committee indices) with one summed signature.
        Per vote: 1 accepted (all bits set, signature added once), 2 valid but
        one of its keys had voted (nothing set), 0 invalid, <0 malformed.
        Votes take effect in list order."""
        batch = len(round_idx)
        if len(sigs_cat) != 96 * batch:
            raise ValueError("key_lists/round_idx/sigs length mismatch")
        off, idx, _ = _csr_arrays(key_lists, batch)
        active = sorted(set(round_idx))
        ri = (ctypes.c_uint32 * batch)(*round_idx)
        act = (ctypes.c_uint32 * len(active))(*active)
        res = (ctypes.c_int32 * batch)()
        _check(_lib.hbls_stream_process_multi(self._h, off, idx, ri, sigs_cat, act,
                                              len(active), batch, res),
               "stream_process_multi")
        return list(res)

    def check(self, slots):
        k = len(slots)
        arr = (ctypes.c_uint32 * k)(*slots)
        ok = (ctypes.c_int32 * k)()
        _check(_lib.hbls_stream_check(self._h, arr, k, ok), "stream_check")
        return [bool(v == 1) for v in ok]

    def check_submit(self, slots):
        """async check: snapshots the rounds and runs the pairing chain on a
        side stream (overlaps later process() ticks); one in flight."""
        k = len(slots)
        arr = (ctypes.c_uint32 * k)(*slots)
        _check(_lib.hbls_stream_check_submit(self._h, arr, k), "stream_check_submit")
        self._pending_check = list(slots)

    def check_poll(self):
        """waits for the in-flight check; returns {slot: bool} (empty if none)"""
        slots = getattr(self, "_pending_check", None)
        if not slots:
            return {}
        ok = (ctypes.c_int32 * len(slots))()
        k = _check(_lib.hbls_stream_check_poll(self._h, ok), "stream_check_poll")
        self._pending_check = None
        return {s: bool(ok[i] == 1) for i, s in enumerate(slots[:k])}

    def power(self, slots):
        """(power, count, quorum) lists for the given round slots, tallied
        on the device from the resident bitmaps (IsQuorumAchieved).  quorum
        is None until the committee's set_quorum has been called."""
        k = len(slots)
        arr = (ctypes.c_uint32 * k)(*slots)
        pw = (ctypes.c_uint64 * k)()
        cn = (ctypes.c_uint32 * k)()
        qr = (ctypes.c_int32 * k)() if self.committee._quorum_set else None
        _check(_lib.hbls_stream_power(self._h, arr, k, pw, cn, qr), "stream_power")
        return list(pw), list(cn), (list(qr) if qr is not None else None)

    def get(self, slot: int):
        """returns (bitmap bytes, serialized aggregate sig 96B)"""
        bm = ctypes.create_string_buffer((self.n + 7) // 8)
        agg = ctypes.create_string_buffer(96)
        _check(_lib.hbls_stream_get(self._h, slot, bm, agg), "stream_get")
        return bm.raw, agg.raw

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.hbls_stream_free(self._h)
        except Exception:
            pass
