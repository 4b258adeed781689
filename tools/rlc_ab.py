"""A/B of the stream's two verify modes: per-item pairing (`--mode item`,
today's default) against random-combination batching (`--mode batched`).

Committee of 4096, 16 open rounds, ticks of 64 / 512 / 4096 votes (and one of
16384, past the size at which the per-item path stops being latency-bound)
spread evenly over the rounds; two legs per tick size: all votes valid, and one bad
vote per tick (a valid point signing another round's payload).  Inputs are
built once, outside the timed region; the rounds are re-opened before every
tick so each tick does the same work.  Reports the median over the measured
ticks of hbls_last_kernel_ns and of the wall clock around
hbls_stream_process.  One process per mode:

  python tools/rlc_ab.py --mode item    --out item.json
  python tools/rlc_ab.py --mode batched --out batched.json

The item leg uses only entry points that predate the batched mode, so it
also runs against an older build of the library.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import pyref as pr  # noqa: E402

N, ROUNDS = 4096, 16
TICKS = (64, 512, 4096, 16384)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("item", "batched"), required=True)
    ap.add_argument("--ticks", type=int, default=20, help="measured ticks per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from harmony_amd import core
    core.init(0)
    sks = [pr.fr_serialize(pr.synth_sk(i)) for i in range(N)]
    pks = core.batch_pk_from_sk(b"".join(sks), N)
    committee = core.Committee(pks, N)
    payloads = [pr.construct_commit_payload(r, pr.synth_msg(900 + r), r + 1)
                for r in range(ROUNDS)]
    mlen = len(payloads[0])
    pl_cat = b"".join(payloads)
    slots = list(range(ROUNDS))
    # vote j: key j // 16 in round j % 16; the next round's signature makes it bad
    V = max(TICKS)
    all_keys = [j // ROUNDS for j in range(V)]
    rounds = [j % ROUNDS for j in range(V)]
    sks_cat = b"".join(sks[k] for k in all_keys)
    good = core.batch_sign(sks_cat, b"".join(payloads[r] for r in rounds), mlen, V)
    wrong = core.batch_sign(sks_cat, b"".join(payloads[(r + 1) % ROUNDS] for r in rounds),
                            mlen, V)

    st = core.Stream(committee, ROUNDS)
    if args.mode == "batched":
        st.set_verify_mode(1)

    out = {"mode": args.mode, "committee": N, "rounds": ROUNDS,
           "measured_ticks": args.ticks, "warmup_ticks": args.warmup,
           "version": core.version(), "legs": []}
    for T in TICKS:
        for leg in ("all_valid", "one_bad"):
            keys, rnds = all_keys[:T], rounds[:T]
            sigs = good[:96 * T]
            want = [1] * T
            if leg == "one_bad":
                b = T // 2
                sigs = sigs[:96 * b] + wrong[96 * b:96 * (b + 1)] + sigs[96 * (b + 1):]
                want[b] = 0
            dev_ns, wall_ns, stats = [], [], None
            for it in range(args.warmup + args.ticks):
                st.set_rounds(slots, pl_cat, mlen)
                t0 = time.perf_counter_ns()
                res = st.process(keys, rnds, sigs)
                t1 = time.perf_counter_ns()
                assert res == want, (T, leg)
                if it >= args.warmup:
                    dev_ns.append(core.last_kernel_ns())
                    wall_ns.append(t1 - t0)
            if args.mode == "batched":
                stats = core.rlc_last_stats()
            rec = {"tick": T, "leg": leg,
                   "kernel_ms_median": statistics.median(dev_ns) / 1e6,
                   "kernel_ms_min": min(dev_ns) / 1e6,
                   "wall_ms_median": statistics.median(wall_ns) / 1e6,
                   "wall_ms_min": min(wall_ns) / 1e6,
                   "votes_per_s_wall": T / (statistics.median(wall_ns) / 1e9),
                   "rlc_stats": stats}
            out["legs"].append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
