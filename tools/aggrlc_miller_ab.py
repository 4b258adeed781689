"""A/B of the item Miller kernel of the combined aggregate verify (DESIGN.md
§4m): level 0 = affine arguments and a product kernel of its own, level 1 =
Jacobian arguments (no inversion), level 2 = Jacobian arguments and the chunk
product inside the Miller kernel.

  sweep   one process, the benchmark's own inputs, each size a prefix of the
          full batch; the three levels alternate `--rounds` times after a
          warm-up round; every call records wall time and stage slots 0..8.
          Then one bad item and one dirty chunk in the full batch, once per
          level.  The default level is the highest whose wall-clock range at
          the full batch beats the next lower level's (`_beats`).
            python tools/aggrlc_miller_ab.py sweep --out profiles/aggrlc_miller_ab.json

  bench   `python bench.py` at its defaults in fresh processes, three legs
          alternating `--rounds` times: the parent commit's tree (--parent DIR,
          built), this tree with HBLS_AGGRLC_MILLER=0 and this tree at its
          default; the first round also dumps the verdicts (--dump-outputs)
          and compares verify_results.npy with the parent's.
            python tools/aggrlc_miller_ab.py bench --parent DIR \
                --out profiles/aggrlc_miller_bench_ab.json
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

from aggrlc_early_ab import SLOT_NAMES, _beats, _setup, _spread, _summary, one_call  # noqa: E402

LEVELS = (0, 1, 2)


def _name(level):
    return "level%d" % level


def run_sweep(args):
    core, committee, d, B, n, mlen, bmlen = _setup(args)
    sizes = [int(s) for s in args.sizes.split(",") if int(s) <= B]
    out = {"committee": n, "batch": B, "rounds": args.rounds, "version": core.version(),
           "legs": [_name(v) for v in LEVELS], "slots": list(SLOT_NAMES),
           "what": "batch_agg_verify on the combined path, chunk-level leg, the early rule at "
                   "its default; levels alternate in one process after a warm-up round",
           "sizes": {}}
    # the legs set the level themselves; everything goes back on the way out
    with core.aggrlc_switches(mode=1, threshold=1, sigleg=1, miller=-1):
        for b in sizes:
            rec = {_name(v): [] for v in LEVELS}
            for rnd in range(args.rounds + 1):          # round 0 warms up
                k = rnd % len(LEVELS)
                for v in LEVELS[k:] + LEVELS[:k]:
                    core.set_aggrlc_miller(v)
                    r = one_call(core, committee, d, mlen, bmlen, b)
                    if rnd:
                        rec[_name(v)].append(r)
            summary = {name: _summary(calls) for name, calls in rec.items()}
            w = [summary[_name(v)]["wall_ms"] for v in LEVELS]
            summary["level1_beats_level0"] = _beats(w[1], w[0])
            summary["level2_beats_level1"] = _beats(w[2], w[1])
            summary["level2_beats_level0"] = _beats(w[2], w[0])
            out["sizes"][str(b)] = {"summary": summary, "calls": rec}
            print(json.dumps({"batch": b,
                              **{k: {"wall": v["wall_ms"], "miller": v["miller_ms"],
                                     "prod": v["chunk_prod_ms"], "bad": v["bad"]}
                                 for k, v in summary.items() if isinstance(v, dict)},
                              **{k: v for k, v in summary.items() if isinstance(v, bool)}}),
                  flush=True)
        full = out["sizes"][str(B)]["summary"] if str(B) in out["sizes"] else None
        if full:
            pick = 0
            if full["level1_beats_level0"]:
                pick = 1
            if full["level2_beats_level1"] and (pick == 1 or full["level2_beats_level0"]):
                pick = 2
            out["default_level_by_rule"] = pick
            print(json.dumps({"default_level_by_rule": pick}), flush=True)
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
        for v in LEVELS:
            core.set_aggrlc_miller(v)
            good = [one_call(core, committee, d, mlen, bmlen, B) for _ in range(2)][-1]
            bad = one_call(core, committee, d, mlen, bmlen, B, sigs=sigs)
            dirty = one_call(core, committee, d, mlen, bmlen, B, bitmaps=bms)
            out["one_bad_item"][_name(v)] = {"all_valid": good, "one_bad": bad,
                                             "extra_wall_ms": bad["wall_ms"] - good["wall_ms"]}
            out["one_dirty_chunk"][_name(v)] = {"all_valid": good, "one_dirty": dirty,
                                                "extra_wall_ms": dirty["wall_ms"] - good["wall_ms"]}
            print(json.dumps({"leg": _name(v), "bad_stats": bad["stats"], "bad": bad["bad"],
                              "bad_extra_wall_ms": round(bad["wall_ms"] - good["wall_ms"], 2),
                              "dirty_stats": dirty["stats"], "dirty_bad": dirty["bad"],
                              "dirty_extra_wall_ms": round(dirty["wall_ms"] - good["wall_ms"], 2)}),
                  flush=True)
    return out


def bench_once(tree, level, extra):
    env = dict(os.environ)
    env.pop("HBLS_AGGRLC_MILLER", None)
    if level is not None:
        env["HBLS_AGGRLC_MILLER"] = str(level)
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
    legs = (("parent", os.path.abspath(args.parent), None), ("level0", HERE, 0),
            ("default", HERE, None))
    out = {"what": "python bench.py, committee 4096, batch 262144, one MI355X; legs alternate "
                   "in one session. parent = the parent commit's tree; level0 = this tree with "
                   "HBLS_AGGRLC_MILLER=0; default = this tree, no switch set",
           "headline": [], "summary": {}}
    dumps = {}
    for rnd in range(1, args.rounds + 1):
        for name, tree, level in legs:
            extra = []
            if rnd == 1:
                dumps[name] = os.path.join(os.path.abspath(args.dump_dir), name)
                extra = ["--dump-outputs", dumps[name]]
            r = bench_once(tree, level, extra)
            rec = {"leg": name, "run": rnd, "ms_per_step": r["ms_per_step"], "value": r["value"]}
            out["headline"].append(rec)
            print(json.dumps(rec), flush=True)
    ref = np.load(os.path.join(dumps["parent"], "verify_results.npy"))
    out["verify_results_identical_to_parent"] = {
        name: bool(np.array_equal(ref, np.load(os.path.join(dumps[name], "verify_results.npy"))))
        for name in ("level0", "default")}
    out["verify_results_items"] = int(ref.size)
    for name, _, _ in legs:
        ms = [r["ms_per_step"] for r in out["headline"] if r["leg"] == name]
        vs = [r["value"] for r in out["headline"] if r["leg"] == name]
        out["summary"][name] = {"ms_per_step": _spread(ms), "verifies_per_s": _spread(vs)}
    rng = {k: v["ms_per_step"] for k, v in out["summary"].items()}
    out["summary"]["default_beats_parent"] = _beats(rng["default"], rng["parent"])
    out["summary"]["default_beats_level0"] = _beats(rng["default"], rng["level0"])
    out["summary"]["level0_differs_from_parent"] = (_beats(rng["level0"], rng["parent"])
                                                    or _beats(rng["parent"], rng["level0"]))
    print(json.dumps(out["summary"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    ps = sub.add_parser("sweep")
    ps.add_argument("--batch", type=int, default=262144)
    ps.add_argument("--sizes", default="16384,32768,65536,131072,258048,262144")
    ps.add_argument("--rounds", type=int, default=5)
    ps.add_argument("--cache", default=None)
    ps.add_argument("--out", default=None)
    pb = sub.add_parser("bench")
    pb.add_argument("--parent", required=True, help="the parent commit's tree, built")
    pb.add_argument("--rounds", type=int, default=3)
    pb.add_argument("--dump-dir", default="miller_ab_dump")
    pb.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"sweep": run_sweep, "bench": run_bench}[args.cmd](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
