"""A/B of the signed-message entry: one ContextSet.verify_msgs
call over a window that mixes committees and messages, against the
composition a caller has to write without it — split the window by committee
and message length, make one Committee.batch_verify_votes_multi call per
group with the group's message repeated per item, and where the signed bytes
are a Keccak digest, run core.batch_keccak256 first and bring the digests
back to the host.  The composition runs entry points that exist without this
feature, from a tree of the parent commit: it is the yardstick, not code
under test.

  python tools/msgs_ab.py --parent ../parent --out profiles/msgs_ab.json
  python tools/msgs_ab.py --bench --parent ../parent --out profiles/msgs_bench_ab.json

Workloads (seeded, the same in both trees):
  viewchange  committee of 4096, one VIEWCHANGE message per key: 8192 items
              (view-ID signature and view-change signature) over a table of 3
              messages: NIL, the view ID, a 640-byte M1 payload signed by every
              fourth sender
  tick        4096 votes spread over 4 committees of 1024, each committee
              voting on its own 48-byte commit payload
  auth        sender authentication: 4096 signatures of one committee of 4096,
              each over the Keccak-256 digest of its own 200-byte message
Every workload holds a few items with another item's signature.

The driver starts every leg in a fresh process.  First each tree computes the
verdicts of every workload; the driver asserts that they are equal, item by
item, and that the planted items and no others are refused — before anything
is timed.  Then the trees alternate, `--runs` times; every timed process
checks its verdicts against the recorded ones again before it times a
workload.  Reported per workload and tree: the per-run medians of wall time
and device time (hbls_last_kernel_ns, summed over the calls of the
composition), their median and range over the runs, parent side first.

--bench runs `bench.py --gpus 1 --steps 10 --warmup 3` from both trees,
alternating, and applies the project's rule: this tree's step times must lie
inside the parent's range widened by its width.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIL = b"\x01"
VIEW_ID = 41
WORKLOADS = ("viewchange", "tick", "auth")


# ------------------------------------------------------------------ workloads

def _sign(core, pr, sk_ints, msgs):
    """one device signing call per message length; sk_ints[j] signs msgs[j]"""
    sigs = [None] * len(msgs)
    for mlen in sorted(set(len(m) for m in msgs)):
        pick = [j for j in range(len(msgs)) if len(msgs[j]) == mlen]
        cat = core.batch_sign(b"".join(pr.fr_serialize(sk_ints[j]) for j in pick),
                              b"".join(msgs[j] for j in pick), mlen, len(pick))
        for k, j in enumerate(pick):
            sigs[j] = cat[96 * k:96 * (k + 1)]
    return sigs


def _committee(core, pr, base, n):
    sks = [pr.synth_sk(base + i) for i in range(n)]
    pks = core.batch_pk_from_sk(b"".join(pr.fr_serialize(k) for k in sks), n)
    return sks, core.Committee(pks, n)


def _plant(sigs, every):
    """item j (j % every == every - 1) carries its neighbour's signature"""
    bad = [j for j in range(len(sigs)) if j % every == every - 1]
    for j in bad:
        sigs[j] = sigs[j - 1]
    return set(bad)


def build(core, pr, keccak, name):
    """dict(committees, ctx, keys, sigs, msg_idx, table, digest, signed, bad):
    item j is key keys[j] of committee ctx[j] on table[msg_idx[j]]; signed[i] is
    what a signer of entry i signs (its bytes, or their digest)"""
    if name == "viewchange":
        n = 4096
        sks, committee = _committee(core, pr, 0, n)
        payload = pr.synth_msg(77) + bytes(96) + bytes(n // 8)     # hash || proof: 640 bytes
        table = [NIL, VIEW_ID.to_bytes(8, "little"), payload]
        ctx, keys, msg_idx = [], [], []
        for s in range(n):
            ctx += [0, 0]
            keys += [s, s]
            msg_idx += [1, 2 if s % 4 == 0 else 0]
        committees, digest, every = [committee], [False] * 3, 1000
        sk_of = [sks[k] for k in keys]
    elif name == "tick":
        parts = [_committee(core, pr, 50000 + 2048 * c, 1024) for c in range(4)]
        committees = [p[1] for p in parts]
        table = [pr.construct_commit_payload(900 + c, pr.synth_msg(900 + c), c + 1)
                 for c in range(4)]
        ctx = [j % 4 for j in range(4096)]
        keys = [j // 4 for j in range(4096)]
        msg_idx = list(ctx)
        digest, every = [False] * 4, 500
        sk_of = [parts[c][0][k] for c, k in zip(ctx, keys)]
    elif name == "auth":
        n = 4096
        sks, committee = _committee(core, pr, 0, n)
        table = [(pr.synth_msg(3000 + j) * 7)[:200] for j in range(n)]
        ctx, keys, msg_idx = [0] * n, list(range(n)), list(range(n))
        committees, digest, every = [committee], [True] * n, 500
        sk_of = sks
    else:
        raise SystemExit("unknown workload " + name)
    signed = [keccak(m) if d else m for m, d in zip(table, digest)]
    sigs = _sign(core, pr, sk_of, [signed[i] for i in msg_idx])
    bad = _plant(sigs, every)
    return dict(committees=committees, ctx=ctx, keys=keys, sigs=sigs, msg_idx=msg_idx,
                table=table, digest=digest, bad=bad)


def leg_new(core, w, state):
    if "set" not in state:                      # built once per epoch, like a committee
        state["set"] = core.ContextSet(w["committees"])
    res = state["set"].verify_msgs(w["ctx"], [[k] for k in w["keys"]], b"".join(w["sigs"]),
                                   w["msg_idx"], w["table"],
                                   w["digest"] if any(w["digest"]) else None)
    return res, core.last_kernel_ns()


def leg_parent(core, w, state):
    """what a caller writes without the entry; the split and the packing are
    part of the call, as the packing is part of verify_msgs"""
    table, dev = w["table"], 0
    signed = list(table)
    dig = [i for i, d in enumerate(w["digest"]) if d]
    by_len = {}
    for i in dig:
        by_len.setdefault(len(table[i]), []).append(i)
    for mlen, pick in by_len.items():           # digests come back to the host
        out = core.batch_keccak256(b"".join(table[i] for i in pick), mlen, len(pick))
        dev += core.last_kernel_ns()
        for k, i in enumerate(pick):
            signed[i] = out[32 * k:32 * (k + 1)]
    groups = {}
    for j, (c, mi) in enumerate(zip(w["ctx"], w["msg_idx"])):
        groups.setdefault((c, len(signed[mi])), []).append(j)
    res = [None] * len(w["ctx"])
    for (c, mlen), pick in groups.items():
        sub = w["committees"][c].batch_verify_votes_multi(
            [[w["keys"][j]] for j in pick], b"".join(w["sigs"][j] for j in pick),
            b"".join(signed[w["msg_idx"][j]] for j in pick), mlen)
        dev += core.last_kernel_ns()
        for j, r in zip(pick, sub):
            res[j] = r
    return res, dev


def child(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    from harmony_amd import core
    from oracle import capi, pyref as pr
    assert os.path.dirname(os.path.dirname(os.path.abspath(core.__file__))) == tree
    core.init(0)
    fn = leg_new if args.child == "new" else leg_parent
    expect = None
    if args.expect:
        with open(args.expect) as f:
            expect = json.load(f)
    out = {"leg": args.child, "tree": tree, "version": core.version(), "workloads": {}}
    for name in args.workloads.split(","):
        w = build(core, pr, capi.keccak256, name)
        state = {}
        res, _ = fn(core, w, state)
        rec = {"items": len(res), "table": len(w["table"]), "contexts": len(w["committees"]),
               "refused": sum(1 for r in res if r != 1)}
        want = [0 if j in w["bad"] else 1 for j in range(len(res))]
        assert res == want, name + ": verdicts differ from the planted pattern"
        if expect is None:
            rec["verdicts"] = res
        else:
            assert res == expect["workloads"][name]["verdicts"], name + ": verdicts differ"
            wall, dev = [], []
            for it in range(args.warmup + args.steps):
                t0 = time.perf_counter_ns()
                res, d = fn(core, w, state)
                t1 = time.perf_counter_ns()
                assert res == want
                if it >= args.warmup:
                    wall.append((t1 - t0) / 1e6)
                    dev.append(d / 1e6)
            rec.update(wall_ms=wall, wall_ms_median=statistics.median(wall),
                       kernel_ms_median=statistics.median(dev))
        out["workloads"][name] = rec
        print(json.dumps({name: {k: v for k, v in rec.items()
                                 if k not in ("verdicts", "wall_ms")}}), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f)


# --------------------------------------------------------------------- driver

def _spawn(tree, leg, out, args, expect=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--tree", tree,
           "--out", out, "--workloads", args.workloads, "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    if expect:
        cmd += ["--expect", expect]
    p = subprocess.run(cmd, timeout=args.child_timeout)
    if p.returncode != 0:
        raise SystemExit("%s leg failed in %s (exit %d)" % (leg, tree, p.returncode))
    with open(out) as f:
        return json.load(f)


def _stats(v):
    med = statistics.median(v)
    return {"median": med, "min": min(v), "max": max(v),
            "spread_pct": 100.0 * (max(v) - min(v)) / med, "per_run": v}


def drive(args):
    parent = os.path.abspath(args.parent)
    legs = (("parent", parent, "parent"), ("this", HERE, "new"))
    with tempfile.TemporaryDirectory() as tmp:
        verd = {}
        for side, tree, leg in legs:
            verd[side] = _spawn(tree, leg, os.path.join(tmp, side + "_v.json"), args)
        out = {"what": "ContextSet.verify_msgs (this tree) against one "
                       "batch_verify_votes_multi call per committee and message length, "
                       "batch_keccak256 through the host where entries are digested "
                       "(parent commit's tree); fresh processes, trees alternating",
               "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
               "version": verd["this"]["version"], "workloads": {}}
        for name in args.workloads.split(","):
            a, b = (verd[s]["workloads"][name] for s in ("parent", "this"))
            assert a["verdicts"] == b["verdicts"], name + ": parent and this tree disagree"
            out["workloads"][name] = {
                "items": b["items"], "table": b["table"], "contexts": b["contexts"],
                "refused": b["refused"], "verdicts_equal": True,
                "verdicts_sha256": hashlib.sha256(bytes(b["verdicts"])).hexdigest()}
        print("verdicts equal in both trees; timing", flush=True)
        runs = {"parent": [], "this": []}
        for r in range(args.runs):
            for side, tree, leg in legs:
                runs[side].append(_spawn(tree, leg, os.path.join(tmp, "%s_%d.json" % (side, r)),
                                         args, expect=os.path.join(tmp, side + "_v.json")))
        for name, rec in out["workloads"].items():
            for side in ("parent", "this"):
                rec[side] = {key: _stats([run["workloads"][name][key] for run in runs[side]])
                             for key in ("wall_ms_median", "kernel_ms_median")}
            rec["wall_ratio_parent_over_this"] = (rec["parent"]["wall_ms_median"]["median"] /
                                                  rec["this"]["wall_ms_median"]["median"])
    return out


def bench(args):
    parent = os.path.abspath(args.parent)
    extra = ["--gpus", "1", "--steps", "10", "--warmup", "3"]
    out = {"what": "python bench.py " + " ".join(extra) + ", one MI355X, fresh processes, "
                   "parent commit's tree and this tree alternating in one session",
           "runs": []}
    sha = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(args.runs):
            for side, tree in (("parent", parent), ("this", HERE)):
                dump = os.path.join(tmp, side)
                p = subprocess.run([sys.executable, "bench.py"] + extra +
                                   ["--dump-outputs", dump], cwd=tree, timeout=args.child_timeout,
                                   stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    raise SystemExit("bench.py failed in %s (exit %d)" % (tree, p.returncode))
                line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
                res = json.loads(line)
                out["runs"].append({"leg": side, "run": r + 1, "ms_per_step": res["ms_per_step"],
                                    "value": res["value"]})
                with open(os.path.join(dump, "verify_results.npy"), "rb") as f:
                    sha[side] = hashlib.sha256(f.read()).hexdigest()
                print(json.dumps(out["runs"][-1]), flush=True)
    summary = {}
    for side in ("parent", "this"):
        v = [x["ms_per_step"] for x in out["runs"] if x["leg"] == side]
        summary[side] = {"ms_per_step_min": min(v), "ms_per_step_max": max(v), "ms_per_step": v}
    lo, hi = summary["parent"]["ms_per_step_min"], summary["parent"]["ms_per_step_max"]
    summary["allowed_range_ms"] = [round(lo - (hi - lo), 3), round(hi + (hi - lo), 3)]
    summary["this_within_allowed_range"] = all(
        summary["allowed_range_ms"][0] <= x <= summary["allowed_range_ms"][1]
        for x in summary["this"]["ms_per_step"])
    out["summary"] = summary
    out["verify_results_sha256"] = sha
    out["verify_results_identical"] = sha["parent"] == sha["this"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a tree of the parent commit, built")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--runs", type=int, default=3, help="alternations")
    ap.add_argument("--steps", type=int, default=7, help="measured calls per run")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--child-timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("parent", "new"), help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--expect", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent:
        ap.error("--parent is required")
    out = bench(args) if args.bench else drive(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    else:
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
