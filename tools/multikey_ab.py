"""A/B of the stream's multi-key entry against the single-key
entry it stands beside.

Committee of 4096, 16 open rounds, ticks of 512, 4096 and 16384 votes (the
last past the size at which the verify stage leaves the cooperative kernels)
spread evenly over the rounds, all valid and without overlaps; the rounds are
re-opened before every tick so each tick does the same work.  Legs:

  old_single   hbls_stream_process, one key per vote
  new_single   hbls_stream_process_multi, the same votes as one-key lists
  new_mixed    hbls_stream_process_multi, keys per vote drawn from {1, 2, 4};
               the signature is the sum of the keys' signatures

One process per run, so a tree of the parent commit and this tree can
alternate in one session:

  python tools/multikey_ab.py --leg old --tree ../parent --out parent_1.json
  python tools/multikey_ab.py --leg new --out this_1.json
  python tools/multikey_ab.py --summarize DIR --out profiles/multikey_ab.json

`--leg old` runs old_single only and uses nothing newer than the stream
itself, so it runs against an older tree (`--tree DIR` imports harmony_amd
from DIR).  `--leg new` runs all three.  `--summarize DIR` reads the
parent_*.json and this_*.json of DIR and writes median and spread over the
runs of every leg's per-run median, and the new entry's votes/s and keys/s
against the parent's old_single median.
"""
import argparse
import glob
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROUNDS = 4096, 16
TICKS = (512, 4096, 16384)


def build_ticks(core, pr, payloads, T):
    """(single-key tick, mixed tick): each (key_lists, rounds, sigs).  Votes
    of a round take consecutive keys, so no two votes of a tick overlap."""
    mlen = len(payloads[0])
    rng = random.Random(T)
    out = []
    for sizes in ((1,), (1, 2, 4)):
        cursor = [0] * ROUNDS
        lists, rounds, sk_sums = [], [], []
        for j in range(T):
            r = j % ROUNDS
            k = rng.choice(sizes)
            keys = list(range(cursor[r], cursor[r] + k))
            cursor[r] += k
            assert cursor[r] <= N
            lists.append(keys)
            rounds.append(r)
            # the sum of the keys' signatures is the signature of the summed secret
            sk_sums.append(pr.fr_serialize(sum(pr.synth_sk(i) for i in keys)))
        sigs = core.batch_sign(b"".join(sk_sums), b"".join(payloads[r] for r in rounds),
                               mlen, T)
        out.append((lists, rounds, sigs))
    return out


def timed(core, st, reopen, fn, T, ticks, warmup):
    dev, wall = [], []
    for it in range(warmup + ticks):
        reopen()
        t0 = time.perf_counter_ns()
        res = fn()
        t1 = time.perf_counter_ns()
        assert res == [1] * T
        if it >= warmup:
            dev.append(core.last_kernel_ns() / 1e6)
            wall.append((t1 - t0) / 1e6)
    return {"kernel_ms_median": statistics.median(dev), "kernel_ms_min": min(dev),
            "wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall)}


def run(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    from harmony_amd import core
    from oracle import pyref as pr
    assert os.path.dirname(os.path.dirname(os.path.abspath(core.__file__))) == tree
    core.init(0)
    sks = b"".join(pr.fr_serialize(pr.synth_sk(i)) for i in range(N))
    committee = core.Committee(core.batch_pk_from_sk(sks, N), N)
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(900 + r), r + 1)
                for r in range(ROUNDS)]
    st = core.Stream(committee, ROUNDS)

    def reopen():
        st.set_rounds(list(range(ROUNDS)), b"".join(payloads), len(payloads[0]))

    out = {"leg": args.leg, "tree": tree, "committee": N, "rounds": ROUNDS,
           "measured_ticks": args.ticks, "warmup_ticks": args.warmup,
           "version": core.version(), "legs": []}
    for T in TICKS:
        single, mixed = build_ticks(core, pr, payloads, T)
        flat = [k[0] for k in single[0]]
        legs = [("old_single", lambda: st.process(flat, single[1], single[2]), T)]
        if args.leg == "new":
            legs.append(("new_single",
                         lambda: st.process_multi(single[0], single[1], single[2]), T))
            legs.append(("new_mixed",
                         lambda: st.process_multi(mixed[0], mixed[1], mixed[2]),
                         sum(len(k) for k in mixed[0])))
        for name, fn, nkeys in legs:
            rec = {"tick": T, "leg": name, "keys": nkeys}
            rec.update(timed(core, st, reopen, fn, T, args.ticks, args.warmup))
            rec["votes_per_s_wall"] = T / (rec["wall_ms_median"] / 1e3)
            rec["keys_per_s_wall"] = nkeys / (rec["wall_ms_median"] / 1e3)
            out["legs"].append(rec)
            print(json.dumps(rec), flush=True)
    return out


def summarize(d):
    """median and spread over the runs of each leg's per-run medians"""
    out = {"committee": N, "rounds": ROUNDS, "runs": {}, "legs": []}
    acc = {}
    for side in ("parent", "this"):
        files = sorted(glob.glob(os.path.join(d, side + "_*.json")))
        out["runs"][side] = len(files)
        for f in files:
            with open(f) as fh:
                run = json.load(fh)
            out.setdefault("measured_ticks", run["measured_ticks"])
            for rec in run["legs"]:
                acc.setdefault((side, rec["leg"], rec["tick"], rec["keys"]), []).append(rec)
    base = {}
    for (side, leg, T, nkeys), recs in sorted(acc.items()):
        row = {"tree": side, "leg": leg, "tick": T, "keys": nkeys, "runs": len(recs)}
        for key in ("wall_ms_median", "kernel_ms_median"):
            v = [r[key] for r in recs]
            med = statistics.median(v)
            row[key] = {"median": med, "min": min(v), "max": max(v),
                        "spread_pct": 100.0 * (max(v) - min(v)) / med}
        w = row["wall_ms_median"]["median"]
        row["votes_per_s_wall"] = T / (w / 1e3)
        row["keys_per_s_wall"] = nkeys / (w / 1e3)
        if side == "parent" and leg == "old_single":
            base[T] = row
        out["legs"].append(row)
    for row in out["legs"]:
        b = base.get(row["tick"])
        if b is not None and row["tree"] == "this":
            row["votes_per_s_vs_parent_old"] = row["votes_per_s_wall"] / b["votes_per_s_wall"]
            row["keys_per_s_vs_parent_old"] = row["keys_per_s_wall"] / b["keys_per_s_wall"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("old", "new"))
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--ticks", type=int, default=10, help="measured ticks per leg")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--summarize", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarize:
        out = summarize(args.summarize)
    elif args.leg:
        out = run(args)
    else:
        ap.error("one of --leg and --summarize is required")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    else:
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
