"""A/B of the final kernels of the combined aggregate verify and the sweep
behind its auto threshold.

Inputs are the benchmark's own (bench.build_inputs): committee 4096,
Bernoulli(0.9) masks; each size is a prefix of the full batch.  One process;
per size the legs alternate `--rounds` times, each round starting one leg
later in the order

  exact   mode 0, one final exponentiation per item
  coop16  mode 1, k_aggrlc_final_coop<16>  (the default)
  coop8   mode 1, k_aggrlc_final_coop<8>
  lane    mode 1, k_aggrlc_final (one lane per chunk)

and every call records wall time, the four stage times, g_stage_ns[4..6]
(Miller, chunk products, final exponentiation) and hbls_last_host_ns(0..4).

  python tools/aggrlc_tail_ab.py --out profiles/aggrlc_tail_ab.json

`--cache DIR` keeps the built inputs between processes (shared with
tools/quorum_ab.py).
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

LEGS = (("exact", 0, -1), ("coop16", 1, 16), ("coop8", 1, 8), ("lane", 1, 0))


def one_call(core, committee, d, mlen, bmlen, b):
    bm, sg, ms = d["bitmaps"][:b * bmlen], d["sigs"][:b * 96], d["msgs"][:b * mlen]
    t0 = time.perf_counter_ns()
    res = committee.batch_agg_verify(bm, sg, ms, mlen, b)
    t1 = time.perf_counter_ns()
    st = [core._lib.hbls_last_stage_ns(i) / 1e6 for i in range(7)]
    return {"wall_ms": (t1 - t0) / 1e6,
            "pipeline_ms": core.last_kernel_ns() / 1e6,
            "stage_ms": st[:4], "miller_ms": st[4], "chunk_prod_ms": st[5],
            "final_ms": st[6],
            "host_ms": [core.last_host_ns(i) / 1e6 for i in range(5)],
            "bad": sum(1 for v in res if v != 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--sizes", default="16384,32768,65536,131072,262144")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
           "legs": [name for name, _, _ in LEGS], "sizes": {}}

    # the legs set mode and final themselves; everything goes back on the way out
    with core.aggrlc_switches(threshold=1, mode=-1, final=-1):
        for b in sizes:
            rec = {name: [] for name, _, _ in LEGS}
            for rnd in range(args.rounds + 1):          # round 0 warms up
                # each round starts one leg later, so that no leg always
                # follows the same neighbour
                k = rnd % len(LEGS)
                for name, mode, final in LEGS[k:] + LEGS[:k]:
                    core.set_agg_verify_mode(mode)
                    core.set_aggrlc_final(final)
                    r = one_call(core, committee, d, mlen, bmlen, b)
                    if rnd:
                        rec[name].append(r)
            summary = {}
            for name, calls in rec.items():
                wall = [c["wall_ms"] for c in calls]
                summary[name] = {"wall_ms": wall, "wall_ms_median": statistics.median(wall),
                                 "final_ms": [c["final_ms"] for c in calls],
                                 "verify_ms": [c["stage_ms"][3] for c in calls],
                                 "bad": sum(c["bad"] for c in calls)}
            out["sizes"][str(b)] = {"summary": summary, "calls": rec}
            print(json.dumps({"batch": b, **{k: [round(min(v["wall_ms"]), 2),
                                                  round(max(v["wall_ms"]), 2),
                                                  round(statistics.median(v["final_ms"]), 2)]
                                             for k, v in summary.items()}}), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
