"""A/B of where the combined aggregate verify pairs the signatures
(DESIGN.md §4k): per item (leg 0) or once per chunk (leg 1).

  bench   `python bench.py` at its defaults in fresh processes, three legs
          alternating `--rounds` times: the parent commit's tree (--parent
          DIR, built), this tree with HBLS_AGGRLC_SIGLEG=0 and with =1; then a
          second alternating session with --full --skip-cpu-baseline for the
          stage times, whose first round also dumps the verdicts
          (--dump-outputs) and compares verify_results.npy with the parent's.
            python tools/aggrlc_sigleg_ab.py bench --parent DIR \
                --out profiles/aggrlc_sigleg_bench_ab.json

  sweep   one process, the benchmark's own inputs (bench.build_inputs), each
          size a prefix of the full batch; per size legs 0 and 1 alternate
          `--rounds` times after a warm-up round and every call records wall
          time, the verify stage, g_stage_ns[4..7] (Miller, chunk products,
          final exponentiation, signature scaling + sums); the exact path
          (mode 0) runs alongside for the combined path's own threshold.
          Then one bad item in the full batch, once per leg.
            python tools/aggrlc_sigleg_ab.py sweep \
                --out profiles/aggrlc_sigleg_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))


def _spread(v):
    return [round(min(v), 3), round(max(v), 3)]


# ---------------------------------------------------------------- bench legs
def bench_once(tree, env_leg, extra):
    env = dict(os.environ)
    env.pop("HBLS_AGGRLC_SIGLEG", None)
    if env_leg is not None:
        env["HBLS_AGGRLC_SIGLEG"] = str(env_leg)
    p = subprocess.run([sys.executable, "bench.py"] + extra, cwd=tree, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if p.returncode != 0:
        raise SystemExit("bench.py failed in %s (exit %d): %s\n%s"
                         % (tree, p.returncode, p.stdout[-400:].decode(errors="replace"),
                            p.stderr[-1200:].decode(errors="replace")))
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def run_bench(args):
    import numpy as np
    legs = (("parent", os.path.abspath(args.parent), None), ("leg0", HERE, 0), ("leg1", HERE, 1))
    out = {"what": "python bench.py, committee 4096, batch 262144, one MI355X; legs alternate "
                   "in one session. parent = the parent commit's tree; leg0 / leg1 = this "
                   "tree with HBLS_AGGRLC_SIGLEG=0 / 1",
           "headline_session_1": [], "full_session_2": [], "summary": {}}
    for rnd in range(1, args.rounds + 1):
        for name, tree, leg in legs:
            r = bench_once(tree, leg, [])
            rec = {"leg": name, "run": rnd, "ms_per_step": r["ms_per_step"], "value": r["value"]}
            out["headline_session_1"].append(rec)
            print(json.dumps(rec), flush=True)
    dumps = {}
    for rnd in range(1, args.full_rounds + 1):
        for name, tree, leg in legs:
            extra = ["--full", "--skip-cpu-baseline"]
            if rnd == 1:
                dumps[name] = os.path.join(os.path.abspath(args.dump_dir), name)
                extra += ["--dump-outputs", dumps[name]]
            r = bench_once(tree, leg, extra)
            rec = {"leg": name, "run": rnd, "ms_per_step": r["ms_per_step"], "value": r["value"],
                   "stages_ms_per_launch": r["roofline"]["stages_ms_per_launch"]}
            out["full_session_2"].append(rec)
            print(json.dumps(rec), flush=True)
    if dumps:
        ref = np.load(os.path.join(dumps["parent"], "verify_results.npy"))
        out["verify_results_identical_to_parent"] = {
            name: bool(np.array_equal(ref, np.load(os.path.join(dumps[name],
                                                                "verify_results.npy"))))
            for name in ("leg0", "leg1")}
    if args.merge:          # a headline session recorded by an earlier invocation
        with open(args.merge) as f:
            out["headline_session_1"] = json.load(f)["headline_session_1"]
    if not out["headline_session_1"]:
        return out
    for name, _, _ in legs:
        ms = [r["ms_per_step"] for r in out["headline_session_1"] if r["leg"] == name]
        vs = [r["value"] for r in out["headline_session_1"] if r["leg"] == name]
        out["summary"][name] = {"ms_per_step": _spread(ms), "verifies_per_s": _spread(vs)}

    def beats(a, b):
        """a's range wholly below b's, by at least three times the wider spread"""
        (alo, ahi), (blo, bhi) = out["summary"][a]["ms_per_step"], out["summary"][b]["ms_per_step"]
        return ahi < blo and blo - ahi >= 3 * max(ahi - alo, bhi - blo)
    out["summary"]["leg1_beats_parent"] = beats("leg1", "parent")
    out["summary"]["leg1_beats_leg0"] = beats("leg1", "leg0")
    out["summary"]["leg0_beats_parent"] = beats("leg0", "parent")
    print(json.dumps(out["summary"]), flush=True)
    return out


# ---------------------------------------------------------------- per-call sweep
def one_call(core, committee, d, mlen, bmlen, b, sigs=None):
    bm, ms = d["bitmaps"][:b * bmlen], d["msgs"][:b * mlen]
    sg = (sigs if sigs is not None else d["sigs"])[:b * 96]
    t0 = time.perf_counter_ns()
    res = committee.batch_agg_verify(bm, sg, ms, mlen, b)
    t1 = time.perf_counter_ns()
    st = [core._lib.hbls_last_stage_ns(i) / 1e6 for i in range(8)]
    return {"wall_ms": (t1 - t0) / 1e6, "verify_ms": st[3], "miller_ms": st[4],
            "chunk_prod_ms": st[5], "final_ms": st[6], "sig_ms": st[7],
            "stats": core.aggrlc_last_stats(), "bad": sum(1 for v in res if v != 1)}


SWEEP_LEGS = (("leg0", 1, 0), ("leg1", 1, 1), ("exact", 0, -1))


def run_sweep(args):
    import bench
    import quorum_ab
    from harmony_amd import core
    from oracle import pyref as pr
    core.init(0)
    B, n, mlen = args.batch, bench.COMMITTEE, bench.MSG_LEN
    bmlen = n // 8
    d = quorum_ab.build(core, bench, pr, B, args.cache)
    committee = core.Committee(d["pks"], n)
    sizes = [int(s) for s in args.sizes.split(",") if int(s) <= B]
    out = {"committee": n, "batch": B, "rounds": args.rounds, "version": core.version(),
           "legs": [name for name, _, _ in SWEEP_LEGS], "sizes": {}}
    # the legs set mode and sigleg themselves; everything goes back on the way out
    with core.aggrlc_switches(threshold=1, mode=-1, sigleg=-1):
        for b in sizes:
            rec = {name: [] for name, _, _ in SWEEP_LEGS}
            for rnd in range(args.rounds + 1):          # round 0 warms up
                k = rnd % len(SWEEP_LEGS)
                for name, mode, leg in SWEEP_LEGS[k:] + SWEEP_LEGS[:k]:
                    core.set_agg_verify_mode(mode)
                    core.set_aggrlc_sigleg(leg)
                    r = one_call(core, committee, d, mlen, bmlen, b)
                    if rnd:
                        rec[name].append(r)
            summary = {}
            for name, calls in rec.items():
                summary[name] = {k: _spread([c[k] for c in calls])
                                 for k in ("wall_ms", "verify_ms", "miller_ms", "chunk_prod_ms",
                                           "final_ms", "sig_ms")}
                summary[name]["wall_ms_median"] = statistics.median(c["wall_ms"] for c in calls)
                summary[name]["bad"] = sum(c["bad"] for c in calls)
            out["sizes"][str(b)] = {"summary": summary, "calls": rec}
            print(json.dumps({"batch": b, **{k: {"wall": v["wall_ms"], "verify": v["verify_ms"]}
                                             for k, v in summary.items()}}), flush=True)
        # one bad item (a valid point, the wrong signature) in the full batch
        sigs = bytearray(d["sigs"])
        j = B // 2 + 17
        sigs[96 * j:96 * (j + 1)] = d["sigs"][96 * (j + 1):96 * (j + 2)]
        sigs = bytes(sigs)
        core.set_agg_verify_mode(1)
        out["one_bad_item"] = {}
        for name, leg in (("leg0", 0), ("leg1", 1)):
            core.set_aggrlc_sigleg(leg)
            good = [one_call(core, committee, d, mlen, bmlen, B) for _ in range(2)][-1]
            bad = one_call(core, committee, d, mlen, bmlen, B, sigs=sigs)
            out["one_bad_item"][name] = {"all_valid": good, "one_bad": bad,
                                         "extra_wall_ms": bad["wall_ms"] - good["wall_ms"]}
            print(json.dumps({"one_bad_item": name, "stats": bad["stats"], "bad": bad["bad"],
                              "extra_wall_ms": round(bad["wall_ms"] - good["wall_ms"], 2)}),
                  flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    pb = sub.add_parser("bench")
    pb.add_argument("--parent", required=True, help="the parent commit's tree, built")
    pb.add_argument("--rounds", type=int, default=3)
    pb.add_argument("--full-rounds", type=int, default=2)
    pb.add_argument("--dump-dir", default="sigleg_ab_dump")
    pb.add_argument("--merge", default=None,
                    help="with --rounds 0: take the headline session from this earlier output")
    pb.add_argument("--out", default=None)
    ps = sub.add_parser("sweep")
    ps.add_argument("--batch", type=int, default=262144)
    ps.add_argument("--sizes", default="16384,32768,65536,131072,262144")
    ps.add_argument("--rounds", type=int, default=3)
    ps.add_argument("--cache", default=None)
    ps.add_argument("--out", default=None)
    args = ap.parse_args()
    out = run_bench(args) if args.cmd == "bench" else run_sweep(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
