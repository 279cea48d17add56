#!/usr/bin/env python3
"""Ragged scrub against one scrub per length and against the ragged check, its
floor (not shipped).

The ragged batch's own workload (tools/ragged_bench.py): one geometry (rs, k
sources, `rows` parity rows); stripe lengths drawn with a fixed seed from 64
distinct values between 4 KiB and 1 MiB (not all multiples of 16), as many
stripes as make the source bytes total --gib GiB, encoded by Ragged.encode.
Three routes over the same shards, each on consistent stripes and (`_corrupt`)
on a second allocation where 1 % of the stripes carry one flipped byte (a
seeded choice of stripe, shard and column):

  ragged      one isal_amd.Scrub.ragged run over all stripes
  per_length  one uniform isal_amd.Scrub per distinct length on the same
              shards: the route a caller has without the ragged scrub
  check       one isal_amd.Ragged.check on the same shards: the same reads
              with no location step, the floor

Every route reads (k + rows) * lens[s] bytes per stripe and writes nothing but
its result words. Before anything is timed the verdicts of both scrub routes
are compared with the planted corruption and with each other, and the check's
words with them. Timing: HIP events around `steps` back-to-back runs on the
current stream, after a warm-up of every route; the routes are interleaved
round by round, each round starting with another route, so that they share
whatever else the machine is doing. One JSON line per (route, round), to
stdout and to --out; a last line per route pair gives the ratio of the
medians and each route's spread.

  tools/scrub_ragged_bench.py --out profiles/scrub_ragged_ab.jsonl
  tools/scrub_ragged_bench.py --routes check     # the floor alone
"""
import argparse
import json
import os
import random
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isa-l_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from ragged_bench import Shards, draw_lengths, time_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--gib", type=float, default=10.0, help="source bytes per step, GiB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--routes", default="ragged,per_length,check",
                    help="comma-separated subset of ragged, per_length, check")
    ap.add_argument("--label", default=None, help="copied into every JSON line (which build was measured)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("scrub_ragged_bench: needs the GPU (no timing without one)")
    picked = args.routes.split(",")
    if not picked or set(picked) - {"ragged", "per_length", "check"}:
        raise SystemExit("scrub_ragged_bench: --routes takes ragged, per_length, check")
    k, rows = args.k, args.rows
    m = k + rows
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    a = isal_amd.gf_gen_rs_matrix(m, k)
    tbls = isal_amd.ec_init_tables(k, rows, a[k * k:])
    lens = draw_lengths(args.seed, int(args.gib * (1 << 30)) // k)
    S = len(lens)
    by_len = {}
    for s, n in enumerate(lens):
        by_len.setdefault(n, []).append(s)

    # two encoded allocations; the second gets the flips
    rng = random.Random(args.seed)
    hit = sorted(rng.sample(range(S), max(1, S // 100)))
    want = [-1] * S
    states = {}
    for state in ("clean", "corrupt"):
        sh = Shards(torch, dev, gen, k, rows, lens)
        enc = isal_amd.Ragged(k, rows, tbls, lens, sh.data, sh.coding)
        enc.encode(0)
        torch.cuda.synchronize()
        if state == "corrupt":
            base = sh.buf.data_ptr()
            for s in hit:
                i, col = rng.randrange(m), rng.randrange(lens[s])
                at = (sh.data[s * k + i] if i < k else sh.coding[s * rows + i - k]) - base + col
                sh.buf[at] ^= 1 << rng.randrange(8)
                want[s] = i
            torch.cuda.synchronize()
        states[state] = (sh, enc)

    routes, results, objects = [], {}, []
    for state, (sh, enc) in states.items():
        suffix = "" if state == "clean" else "_corrupt"
        if "ragged" in picked:
            sc = isal_amd.Scrub.ragged(k, rows, tbls, lens, sh.data, sh.coding)
            v = torch.zeros(S, dtype=torch.int32, device=dev)
            objects.append(sc)
            results["ragged" + suffix] = v
            routes.append(("ragged" + suffix, lambda sc=sc, v=v: sc.run(v, 0)))
        if "per_length" in picked:
            per = []
            for n, ss in sorted(by_len.items()):
                sc = isal_amd.Scrub(n, k, rows, tbls, len(ss), [sh.data[s * k + j] for s in ss for j in range(k)],
                                    [sh.coding[s * rows + l] for s in ss for l in range(rows)])
                per.append((sc, torch.zeros(len(ss), dtype=torch.int32, device=dev), ss))
                objects.append(sc)
            results["per_length" + suffix] = per

            def per_length(per=per):
                for sc, v, _ in per:
                    sc.run(v, 0)

            routes.append(("per_length" + suffix, per_length))
        if "check" in picked:
            bad = torch.zeros(S, dtype=torch.int64, device=dev)
            results["check" + suffix] = bad
            routes.append(("check" + suffix, lambda enc=enc, bad=bad: enc.check(bad, 0)))

    # the routes answer what they should before anything is timed
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    for name, res in results.items():
        expect = want if name.endswith("_corrupt") else [-1] * S
        if name.startswith("ragged"):
            got = res.cpu().tolist()
        elif name.startswith("per_length"):
            got = [None] * S
            for _, v, ss in res:
                for s, w in zip(ss, v.cpu().tolist()):
                    got[s] = w
        else:  # the check tells consistent from not
            got = [-1 if w == -1 else expect[s] for s, w in enumerate(res.cpu().tolist())]
        wrong = [s for s in range(S) if got[s] != expect[s]]
        if wrong:
            s = wrong[0]
            raise SystemExit(f"scrub_ragged_bench: {name}: stripe {s} (len {lens[s]}): {got[s]}, want {expect[s]}")

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        if args.label:
            rec["label"] = args.label
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    launches = {}
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        n0 = isal_amd.kernel_launches()
        fn()
        launches[name] = isal_amd.kernel_launches() - n0
    torch.cuda.synchronize()
    nbytes = m * sum(lens)
    ms_of = {name: [] for name, _ in routes}
    common = {"tool": "scrub_ragged_bench", "gen": "rs", "k": k, "rows": rows, "stripes": S,
              "distinct_lengths": len(by_len), "min_len": min(lens), "max_len": max(lens)}
    for rnd in range(args.rounds):
        for name, fn in routes[rnd % len(routes):] + routes[:rnd % len(routes)]:  # every route leads a round
            ms = time_steps(torch, fn, args.steps)
            ms_of[name].append(ms)
            emit(dict(common, corrupt_stripes=len(hit) if name.endswith("_corrupt") else 0, route=name, round=rnd,
                      steps=args.steps, launches_per_step=launches[name], ms_per_step=round(ms, 5),
                      bytes_per_step=nbytes, GBps=round(nbytes / ms / 1e6, 1)))
    for suffix in ("", "_corrupt"):
        for other in ("per_length", "check"):
            x, y = ms_of.get("ragged" + suffix), ms_of.get(other + suffix)
            if x and y:
                emit(dict(common, summary=f"ragged{suffix} / {other}{suffix}",
                          ratio_of_medians=round(statistics.median(x) / statistics.median(y), 4),
                          ragged_ms_min_max=[round(min(x), 5), round(max(x), 5)],
                          other_ms_min_max=[round(min(y), 5), round(max(y), 5)]))
    for sc in objects:
        sc.close()


if __name__ == "__main__":
    main()
