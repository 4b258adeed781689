"""A/B of the quorum gate in front of batch aggregate verify.

Inputs are the benchmark's own (bench.build_inputs): committee 4096, batch
262144, Bernoulli(0.9) masks — every one of which has quorum under both
policies used here.  One process per leg, so a tree of the parent commit and
this tree can alternate in one session:

  python tools/quorum_ab.py --leg plain --tree ../parent --out a1.json
  python tools/quorum_ab.py --leg gated --out b1.json

`--tree DIR` imports harmony_amd and bench from DIR (default: this tree).
The plain leg calls only batch_agg_verify, so it runs against an older tree.
The gated leg times, on one set of inputs:
  plain          batch_agg_verify
  gated_uniform  batch_agg_verify_quorum, uniform policy
  gated_staked   the same with weights from votepower.compute
  gather_10pct   staked, every 10th item given a one-signer mask (no quorum)
and reports k_mask_power's own device time (hbls_last_stage_ns(7)) next to a
device-to-device copy of the same bitmap bytes (hbls_copy_bench_ns).

`--cache DIR` keeps the built inputs (bitmaps, messages, signatures, public
keys) between processes; they take longer to build than the legs to run.
"""
import argparse
import json
import os
import pickle
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(core, bench, pr, batch, cache):
    path = os.path.join(cache, f"quorum_ab_{batch}.pkl") if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    sks, bitmaps, sk_sums, msgs = bench.build_inputs(0, batch)
    pks = core.batch_pk_from_sk(sks, bench.COMMITTEE)
    msgs_cat = b"".join(msgs)
    sigs = core.batch_sign(b"".join(pr.fr_serialize(s) for s in sk_sums), msgs_cat,
                           bench.MSG_LEN, batch)
    data = {"pks": pks, "bitmaps": bitmaps, "msgs": msgs_cat, "sigs": sigs}
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path + ".tmp", "wb") as f:
            pickle.dump(data, f, protocol=4)
        os.replace(path + ".tmp", path)
    return data


def timed(core, fn, steps, warmup, want, stage7=False):
    wall, dev, st, s7 = [], [], [], []
    for it in range(warmup + steps):
        t0 = time.perf_counter_ns()
        res = fn()
        t1 = time.perf_counter_ns()
        if it >= warmup:
            wall.append((t1 - t0) / 1e6)
            dev.append(core.last_kernel_ns() / 1e6)
            st.append([core._lib.hbls_last_stage_ns(i) / 1e6 for i in range(4)])
            if stage7:
                s7.append(core._lib.hbls_last_stage_ns(7) / 1e6)
    bad = sum(1 for a, b in zip(res, want) if a != b)
    rec = {"wall_ms": wall, "wall_ms_median": statistics.median(wall),
           "pipeline_ms_median": statistics.median(dev),
           "stage_ms_median": [statistics.median(c) for c in zip(*st)],
           "mismatches": bad}
    if stage7:
        rec["mask_power_ms"] = s7
        rec["mask_power_ms_median"] = statistics.median(s7)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("plain", "gated"), required=True)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import bench
    from harmony_amd import core
    from oracle import pyref as pr
    assert os.path.dirname(os.path.abspath(bench.__file__)) == tree
    core.init(0)

    B, n, mlen = args.batch, bench.COMMITTEE, bench.MSG_LEN
    d = build(core, bench, pr, B, args.cache)
    committee = core.Committee(d["pks"], n)
    bmlen = n // 8
    out = {"leg": args.leg, "tree": tree, "committee": n, "batch": B,
           "steps": args.steps, "warmup": args.warmup, "version": core.version(),
           "bitmap_bytes": B * bmlen}

    def plain():
        return committee.batch_agg_verify(d["bitmaps"], d["sigs"], d["msgs"], mlen, B)

    out["plain"] = timed(core, plain, args.steps, args.warmup, [1] * B)
    print(json.dumps({"plain": out["plain"]["wall_ms_median"]}), flush=True)

    if args.leg == "gated":
        from harmony_amd import votepower as vp

        def gated(bitmaps=d["bitmaps"]):
            return committee.batch_agg_verify_quorum(bitmaps, d["sigs"], d["msgs"], mlen, B)

        committee.set_quorum()
        out["gated_uniform"] = timed(core, gated, args.steps, args.warmup, [1] * B, True)

        rng = random.Random(1)
        stakes = [None if rng.random() < 0.2 else rng.randrange(1, 10 ** 6) * 10 ** 15
                  for _ in range(n)]
        stakes[-1] = 10 ** 18
        e18 = 10 ** 18
        committee.set_quorum(vp.compute(stakes, 49 * e18 // 100, 51 * e18 // 100))
        out["gated_staked"] = timed(core, gated, args.steps, args.warmup, [1] * B, True)

        bm = bytearray(d["bitmaps"])
        want = [1] * B
        for j in range(0, B, 10):
            bm[j * bmlen:(j + 1) * bmlen] = bytes([1]) + bytes(bmlen - 1)
            want[j] = core.NOQUORUM
        bm = bytes(bm)
        out["gather_10pct"] = timed(core, lambda: gated(bm), args.steps, args.warmup, want, True)
        out["gather_10pct"]["quorumless"] = want.count(core.NOQUORUM)

        copies = [core._lib.hbls_copy_bench_ns(B * bmlen) / 1e6 for _ in range(args.steps)]
        out["d2d_copy_ms"] = copies
        out["d2d_copy_ms_median"] = statistics.median(copies)
        for k in ("gated_uniform", "gated_staked", "gather_10pct"):
            print(json.dumps({k: out[k]["wall_ms_median"],
                              "mask_power_ms": out[k]["mask_power_ms_median"]}), flush=True)
        print(json.dumps({"d2d_copy_ms": out["d2d_copy_ms_median"]}), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
