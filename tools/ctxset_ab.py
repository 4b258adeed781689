"""A/B of the epoch-context entry: one ContextSet.seal_verify
call over a window that mixes committees, against the loop a caller has to
write without it — split the window by committee and make one
Committee.batch_seal_verify call per committee.  The loop runs entry points
that exist without this feature: it is the yardstick, not code under test.

  python tools/ctxset_ab.py --out profiles/ctxset_ab.json

Shapes:
  a   the epoch chain: 64 contexts of 250 keys, one item each
  b   cross-links: 4 contexts of 250 keys, 64 items each, interleaved
  c48 sync across an epoch boundary: 2 contexts of 4096 keys, 10240 items
      each, first one committee then the other — the whole window is above
      the combined mode's threshold (16384), each half below it; 48-byte
      payloads throughout
  c40 the same with 40-byte payloads before the boundary

Both legs start from the same Python lists (context index, blob, payload per
item) and end with the per-item verdicts in window order, so the split and
the packing are inside the timed region of the leg that needs them.  Reported
per leg: median wall time, median device time (hbls_last_kernel_ns, summed
over the calls of the loop), and the chunk counts of
hbls_aggrlc_last_stats — shape c must show chunks for the single call and
none for the halves — and, for the single call, the stage times.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

MASK_POOL = 32      # distinct masks per context (messages are distinct per item)


def mask_of(n, signers):
    bm = bytearray((n + 7) // 8)
    for i in signers:
        bm[i >> 3] |= 1 << (i & 7)
    return bytes(bm)


def build_window(core, pr, sizes, ctx_of_item, mlen_of_ctx, seed):
    """committees of disjoint synthetic keys and a valid window: item j
    belongs to context ctx_of_item[j]; ~90 % participation masks from a small
    pool per context, one signature under the sum of the signers' keys"""
    rng = random.Random(seed)
    sk = [[pr.synth_sk(50000 + 8192 * c + i) for i in range(n)] for c, n in enumerate(sizes)]
    flat = [k for ks in sk for k in ks]
    cat = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in flat), len(flat))
    committees, at = [], 0
    for n in sizes:
        committees.append(core.Committee(cat[48 * at:48 * (at + n)], n))
        at += n
    pools = []
    for c, n in enumerate(sizes):
        pool = []
        for _ in range(MASK_POOL):
            signers = [i for i in range(n) if rng.random() < 0.9] or [0]
            pool.append((mask_of(n, signers),
                         pr.fr_serialize(sum(sk[c][i] for i in signers) % pr.R)))
        pools.append(pool)
    batch = len(ctx_of_item)
    msgs, masks, sks = [], [], []
    for j, c in enumerate(ctx_of_item):
        mask, agg = pools[c][rng.randrange(MASK_POOL)]
        msgs.append(pr.construct_commit_payload(j, pr.synth_msg(j), j + 1)[:mlen_of_ctx[c]])
        masks.append(mask)
        sks.append(agg)
    blobs = [None] * batch
    for mlen in sorted(set(mlen_of_ctx)):
        pick = [j for j in range(batch) if len(msgs[j]) == mlen]
        sig = core.batch_sign(b"".join(sks[j] for j in pick), b"".join(msgs[j] for j in pick),
                              mlen, len(pick))
        for k, j in enumerate(pick):
            blobs[j] = sig[96 * k:96 * (k + 1)] + masks[j]
    return committees, blobs, msgs


def run_shape(core, pr, name, sizes, ctx_of_item, mlen_of_ctx, steps, warmup):
    committees, blobs, msgs = build_window(core, pr, sizes, ctx_of_item, mlen_of_ctx, 7)
    ctxset = core.ContextSet(committees)
    batch = len(ctx_of_item)
    stages = []     # of the single call: front (prepare, power), hash, decompress, key sums, pairing

    def single():
        res = ctxset.seal_verify(ctx_of_item, blobs, msgs)
        stages.append([core.last_stage_ns(i) / 1e6 for i in (7, 1, 2, 0, 3)])
        return res, core.last_kernel_ns(), core.aggrlc_last_stats()[0]

    def loop():
        groups = {}
        for j, c in enumerate(ctx_of_item):
            groups.setdefault(c, []).append(j)
        res, dev, chunks = [None] * batch, 0, 0
        for c, pick in groups.items():
            sub = committees[c].batch_seal_verify(
                b"".join(blobs[j] for j in pick), len(blobs[pick[0]]),
                b"".join(msgs[j] for j in pick), mlen_of_ctx[c], len(pick))
            dev += core.last_kernel_ns()
            chunks += core.aggrlc_last_stats()[0]
            for j, r in zip(pick, sub):
                res[j] = r
        return res, dev, chunks

    rec = {"contexts": len(sizes), "keys": sizes[0], "batch": batch,
           "payload_bytes": sorted(set(mlen_of_ctx))}
    for leg, fn in (("loop", loop), ("single", single)):
        wall, dev = [], []
        for it in range(warmup + steps):
            t0 = time.perf_counter_ns()
            res, d, chunks = fn()
            t1 = time.perf_counter_ns()
            if it >= warmup:
                wall.append((t1 - t0) / 1e6)
                dev.append(d / 1e6)
        rec[leg] = {"wall_ms": wall, "wall_ms_median": statistics.median(wall),
                    "kernel_ms_median": statistics.median(dev),
                    "aggrlc_chunks": chunks,
                    "mismatches": sum(1 for r in res if r != 1)}
    rec["single"]["stage_ms_median"] = dict(zip(
        ("front", "hash", "decompress", "key_sums", "pairing"),
        (statistics.median(c) for c in zip(*stages[warmup:]))))
    rec["wall_ratio_loop_over_single"] = (rec["loop"]["wall_ms_median"] /
                                          rec["single"]["wall_ms_median"])
    print(json.dumps({name: {k: (rec[k]["wall_ms_median"], rec[k]["kernel_ms_median"],
                                 rec[k]["aggrlc_chunks"], rec[k]["mismatches"])
                             for k in ("loop", "single")}}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c48,c40")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--half", type=int, default=10240, help="items per side of shape c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from harmony_amd import core
    from oracle import pyref as pr
    core.init(0)
    half = args.half
    shapes = {
        "a": ([250] * 64, list(range(64)), [48] * 64),
        "b": ([250] * 4, [j % 4 for j in range(256)], [48] * 4),
        "c48": ([4096] * 2, [0] * half + [1] * half, [48, 48]),
        "c40": ([4096] * 2, [0] * half + [1] * half, [40, 48]),
    }
    out = {"version": core.version(), "steps": args.steps, "warmup": args.warmup,
           "agg_verify_mode": "auto (library default)", "shapes": {}}
    for name in args.shapes.split(","):
        sizes, ctx_of_item, mlens = shapes[name]
        out["shapes"][name] = run_shape(core, pr, name, sizes, ctx_of_item, mlens,
                                        args.steps, args.warmup)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
