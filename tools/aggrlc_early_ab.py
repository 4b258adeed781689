"""A/B of when the combined aggregate verify pairs the chunk sums of the
signatures: inside the Miller kernel, behind the items
(early 0), or hoisted beside the mask kernel on a side stream (early 1).

  step0   leg 1 at two sizes, 4032 chunks (one exact round of Miller waves
          with the chunk entries in it) against 4096 (64 waves over): one
          process, a warm-up round, then `--rounds` alternating rounds; records
          hbls_last_stage_ns(4).  Runs on a tree without the early switch too.
            python tools/aggrlc_early_ab.py step0 --out profiles/aggrlc_early_step0.json

  sweep   one process, the benchmark's own inputs, each size a prefix of the
          full batch; early 0, early 1 and early 1 with the one-lane chunk-leg
          kernel alternate `--rounds` times after a warm-up round; every call
          records wall time and stage slots 0..8.  Then one bad item and one
          dirty chunk in the full batch, once per setting.
            python tools/aggrlc_early_ab.py sweep --out profiles/aggrlc_early_ab.json

  bench   `python bench.py` at its defaults in fresh processes, three legs
          alternating `--rounds` times: the parent commit's tree (--parent DIR,
          built), this tree with HBLS_AGGRLC_EARLY=0 and this tree at its
          default; the first round also dumps the verdicts (--dump-outputs)
          and compares verify_results.npy with the parent's.
            python tools/aggrlc_early_ab.py bench --parent DIR \
                --out profiles/aggrlc_early_bench_ab.json
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

SLOT_NAMES = ("mask_ms", "hash_ms", "decompress_ms", "verify_ms", "miller_ms",
              "chunk_prod_ms", "final_ms", "sig_ms", "chunkleg_ms")


def _spread(v):
    return [round(min(v), 3), round(max(v), 3)]


def _beats(a, b):
    """range a wholly below range b, by at least three times the wider spread"""
    (alo, ahi), (blo, bhi) = a, b
    return ahi < blo and blo - ahi >= 3 * max(ahi - alo, bhi - blo)


def one_call(core, committee, d, mlen, bmlen, b, sigs=None, bitmaps=None):
    bm = (bitmaps if bitmaps is not None else d["bitmaps"])[:b * bmlen]
    ms = d["msgs"][:b * mlen]
    sg = (sigs if sigs is not None else d["sigs"])[:b * 96]
    t0 = time.perf_counter_ns()
    res = committee.batch_agg_verify(bm, sg, ms, mlen, b)
    t1 = time.perf_counter_ns()
    rec = {"wall_ms": (t1 - t0) / 1e6, "kernel_ms": core.last_kernel_ns() / 1e6}
    for i, name in enumerate(SLOT_NAMES):
        rec[name] = core._lib.hbls_last_stage_ns(i) / 1e6
    rec["stats"] = core.aggrlc_last_stats()
    rec["bad"] = sum(1 for v in res if v != 1)
    return rec


def _setup(args):
    import bench
    import quorum_ab
    from harmony_amd import core
    from oracle import pyref as pr
    core.init(0)
    B, n, mlen = args.batch, bench.COMMITTEE, bench.MSG_LEN
    d = quorum_ab.build(core, bench, pr, B, args.cache)
    return core, core.Committee(d["pks"], n), d, B, n, mlen, n // 8


def _summary(calls):
    keys = ("wall_ms", "kernel_ms") + SLOT_NAMES
    s = {k: _spread([c[k] for c in calls]) for k in keys}
    s["wall_ms_median"] = statistics.median(c["wall_ms"] for c in calls)
    s["bad"] = sum(c["bad"] for c in calls)
    return s


# ---------------------------------------------------------------- step 0
def run_step0(args):
    core, committee, d, B, n, mlen, bmlen = _setup(args)
    sizes = [int(s) for s in args.sizes.split(",")]
    out = {"what": "leg 1 with the chunk entries inside the Miller kernel; sizes alternate in "
                   "one process after a warm-up round; miller_ms = hbls_last_stage_ns(4)",
           "committee": n, "rounds": args.rounds, "version": core.version(), "sizes": {}}
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=1, early=0):
        rec = {b: [] for b in sizes}
        for rnd in range(args.rounds + 1):
            k = rnd % len(sizes)
            for b in sizes[k:] + sizes[:k]:
                r = one_call(core, committee, d, mlen, bmlen, b)
                if rnd:
                    rec[b].append(r)
        for b in sizes:
            waves = (b + (b + 63) // 64 + 63) // 64
            out["sizes"][str(b)] = {"miller_waves": waves, "summary": _summary(rec[b]),
                                    "calls": rec[b]}
            print(json.dumps({"batch": b, "waves": waves,
                              "miller_ms": out["sizes"][str(b)]["summary"]["miller_ms"]}),
                  flush=True)
        lo, hi = (out["sizes"][str(b)]["summary"]["miller_ms"] for b in sizes[:2])
        gap = hi[0] - lo[1]
        wider = max(lo[1] - lo[0], hi[1] - hi[0])
        out["gap_ms"] = round(gap, 3)
        out["wider_spread_ms"] = round(wider, 3)
        out["gap_at_least_3x_spread"] = bool(gap >= 3 * wider)
        print(json.dumps({k: out[k] for k in ("gap_ms", "wider_spread_ms",
                                              "gap_at_least_3x_spread")}), flush=True)
    return out


# ---------------------------------------------------------------- per-call sweep
# (name, early, chunk-leg kernel): the default kernel (four lanes per chunk)
# and the one-lane kernel it was measured against
SWEEP_LEGS = (("early0", 0, -1), ("early1", 1, -1), ("early1_onelane", 1, 0))


def run_sweep(args):
    core, committee, d, B, n, mlen, bmlen = _setup(args)
    sizes = [int(s) for s in args.sizes.split(",") if int(s) <= B]
    out = {"committee": n, "batch": B, "rounds": args.rounds, "version": core.version(),
           "legs": [name for name, _, _ in SWEEP_LEGS], "slots": list(SLOT_NAMES), "sizes": {}}
    # the legs set early and chunkleg themselves; everything goes back on the way out
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=1, early=-1, chunkleg=-1):
        for b in sizes:
            rec = {name: [] for name, _, _ in SWEEP_LEGS}
            for rnd in range(args.rounds + 1):          # round 0 warms up
                k = rnd % len(SWEEP_LEGS)
                for name, early, kern in SWEEP_LEGS[k:] + SWEEP_LEGS[:k]:
                    core.set_aggrlc_early(early)
                    core.set_aggrlc_chunkleg(kern)
                    r = one_call(core, committee, d, mlen, bmlen, b)
                    if rnd:
                        rec[name].append(r)
            summary = {name: _summary(calls) for name, calls in rec.items()}
            w0, w1 = summary["early0"]["wall_ms"], summary["early1"]["wall_ms"]
            summary["early1_beats_early0"] = _beats(w1, w0)
            summary["early0_beats_early1"] = _beats(w0, w1)
            summary["early1_beats_early1_onelane"] = _beats(
                w1, summary["early1_onelane"]["wall_ms"])
            out["sizes"][str(b)] = {"summary": summary, "calls": rec}
            print(json.dumps({"batch": b, **{k: {"wall": v["wall_ms"], "mask": v["mask_ms"],
                                                 "miller": v["miller_ms"],
                                                 "chunkleg": v["chunkleg_ms"]}
                                             for k, v in summary.items() if isinstance(v, dict)},
                              "early1_beats_early0": summary["early1_beats_early0"],
                              "early0_beats_early1": summary["early0_beats_early1"]}),
                  flush=True)
        # one bad item (a valid point, the wrong signature), then one dirty
        # chunk (an empty mask under a real signature) in the full batch
        j = B // 2 + 17
        sigs = bytearray(d["sigs"])
        sigs[96 * j:96 * (j + 1)] = d["sigs"][96 * (j + 1):96 * (j + 2)]
        sigs = bytes(sigs)
        bms = bytearray(d["bitmaps"])
        bms[bmlen * j:bmlen * (j + 1)] = bytes(bmlen)
        bms = bytes(bms)
        out["one_bad_item"], out["one_dirty_chunk"] = {}, {}
        for name, early, kern in SWEEP_LEGS:
            core.set_aggrlc_early(early)
            core.set_aggrlc_chunkleg(kern)
            good = [one_call(core, committee, d, mlen, bmlen, B) for _ in range(2)][-1]
            bad = one_call(core, committee, d, mlen, bmlen, B, sigs=sigs)
            dirty = one_call(core, committee, d, mlen, bmlen, B, bitmaps=bms)
            out["one_bad_item"][name] = {"all_valid": good, "one_bad": bad,
                                         "extra_wall_ms": bad["wall_ms"] - good["wall_ms"]}
            out["one_dirty_chunk"][name] = {"all_valid": good, "one_dirty": dirty,
                                            "extra_wall_ms": dirty["wall_ms"] - good["wall_ms"]}
            print(json.dumps({"leg": name, "bad_stats": bad["stats"], "bad": bad["bad"],
                              "bad_extra_wall_ms": round(bad["wall_ms"] - good["wall_ms"], 2),
                              "dirty_stats": dirty["stats"], "dirty_bad": dirty["bad"],
                              "dirty_extra_wall_ms": round(dirty["wall_ms"] - good["wall_ms"], 2)}),
                  flush=True)
    return out


# ---------------------------------------------------------------- bench legs
def bench_once(tree, early, extra):
    env = dict(os.environ)
    env.pop("HBLS_AGGRLC_EARLY", None)
    if early is not None:
        env["HBLS_AGGRLC_EARLY"] = str(early)
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
    legs = (("parent", os.path.abspath(args.parent), None), ("early0", HERE, 0),
            ("default", HERE, None))
    out = {"what": "python bench.py, committee 4096, batch 262144, one MI355X; legs alternate "
                   "in one session. parent = the parent commit's tree; early0 = this tree with "
                   "HBLS_AGGRLC_EARLY=0; default = this tree, no switch set",
           "headline": [], "summary": {}}
    dumps = {}
    for rnd in range(1, args.rounds + 1):
        for name, tree, early in legs:
            extra = []
            if rnd == 1:
                dumps[name] = os.path.join(os.path.abspath(args.dump_dir), name)
                extra = ["--dump-outputs", dumps[name]]
            r = bench_once(tree, early, extra)
            rec = {"leg": name, "run": rnd, "ms_per_step": r["ms_per_step"], "value": r["value"]}
            out["headline"].append(rec)
            print(json.dumps(rec), flush=True)
    ref = np.load(os.path.join(dumps["parent"], "verify_results.npy"))
    out["verify_results_identical_to_parent"] = {
        name: bool(np.array_equal(ref, np.load(os.path.join(dumps[name], "verify_results.npy"))))
        for name in ("early0", "default")}
    out["verify_results_items"] = int(ref.size)
    for name, _, _ in legs:
        ms = [r["ms_per_step"] for r in out["headline"] if r["leg"] == name]
        vs = [r["value"] for r in out["headline"] if r["leg"] == name]
        out["summary"][name] = {"ms_per_step": _spread(ms), "verifies_per_s": _spread(vs)}
    rng = {k: v["ms_per_step"] for k, v in out["summary"].items()}
    out["summary"]["default_beats_parent"] = _beats(rng["default"], rng["parent"])
    out["summary"]["default_beats_early0"] = _beats(rng["default"], rng["early0"])
    out["summary"]["early0_differs_from_parent"] = (_beats(rng["early0"], rng["parent"])
                                                    or _beats(rng["parent"], rng["early0"]))
    print(json.dumps(out["summary"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p0 = sub.add_parser("step0")
    p0.add_argument("--batch", type=int, default=262144)
    p0.add_argument("--sizes", default="258048,262144")
    p0.add_argument("--rounds", type=int, default=5)
    p0.add_argument("--cache", default=None)
    p0.add_argument("--out", default=None)
    ps = sub.add_parser("sweep")
    ps.add_argument("--batch", type=int, default=262144)
    ps.add_argument("--sizes", default="16384,32768,65536,131072,258048,262144")
    ps.add_argument("--rounds", type=int, default=5)
    ps.add_argument("--cache", default=None)
    ps.add_argument("--out", default=None)
    pb = sub.add_parser("bench")
    pb.add_argument("--parent", required=True, help="the parent commit's tree, built")
    pb.add_argument("--rounds", type=int, default=3)
    pb.add_argument("--dump-dir", default="early_ab_dump")
    pb.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"step0": run_step0, "sweep": run_sweep, "bench": run_bench}[args.cmd](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
