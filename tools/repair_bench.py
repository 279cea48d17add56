#!/usr/bin/env python3
"""Repair batch against per-pattern batches and the uniform ceiling (not shipped).

For one geometry and shard size, with the stripes spread over N distinct
erasure patterns, three routes rebuild the same device-resident bytes:

  repair   one isal_amd.Repair over every stripe (one launch per pass)
  batches  one isal_amd.Batch per distinct pattern with that pattern's decode
           tables, run back to back on one stream (what the API offered
           before the repair batch)
  ceiling  one Batch over every stripe with a single pattern's tables: the
           same bytes moved, no indirection, the 0/1-mask path where it applies

Timing: HIP events around `steps` back-to-back runs on the current stream,
after a warm-up of every route; the routes are interleaved round by round so
that they share whatever else the machine is doing. Bytes per step =
(k + nerrs) * len * nstripes (bench.py's decode convention). One JSON line
per (shape, patterns, route, round), to stdout and to --out.

  tools/repair_bench.py --out profiles/repair_ab.jsonl
  tools/repair_bench.py --len 65536 --stripes 16384 --patterns 364
"""
import argparse
import itertools
import json
import os
import random
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isa-l_amd"))


def decode_tables(isal_amd, a, k, pat):
    ret, c, surv = isal_amd.decode_matrix(a, k, pat)
    if ret != 0:
        raise SystemExit(f"pattern {pat} is not decodable ({ret})")
    return isal_amd.ec_init_tables(k, len(pat), c), surv


def time_steps(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def run_shape(args, torch, isal_amd, len_, S, npat, emit):
    k, m, nerrs = args.k, args.m, args.nerrs
    a = isal_amd.gf_gen_rs_matrix(m, k) if args.gen == "rs" else isal_amd.gf_gen_cauchy1_matrix(m, k)
    every = list(itertools.combinations(range(m), nerrs))
    rng = random.Random(args.seed)
    pats = every if npat >= len(every) else rng.sample(every, npat)
    npat = len(pats)
    of = [pats[s % npat] for s in range(S)]
    rng.shuffle(of)

    dev = torch.device("cuda:0")
    buf = torch.empty((S * m, len_), dtype=torch.uint8, device=dev)
    buf.random_(generator=torch.Generator(device=dev).manual_seed(args.seed))
    base, pitch = buf.data_ptr(), len_
    assert base % 16 == 0 and pitch % 16 == 0
    shards = [base + r * pitch for r in range(S * m)]

    repair = isal_amd.Repair(len_, k, m, a, nerrs, S, [e for p in of for e in p], shards)
    assert repair.npatterns() == npat
    tables = {p: decode_tables(isal_amd, a, k, p) for p in pats}
    batches = []
    for p in pats:
        tb, surv = tables[p]
        rows = [s for s in range(S) if of[s] == p]
        batches.append(isal_amd.Batch(len_, k, nerrs, tb, len(rows),
                                      [shards[s * m + i] for s in rows for i in surv],
                                      [shards[s * m + e] for s in rows for e in p]))
    tb, surv = tables[pats[0]]
    ceiling = isal_amd.Batch(len_, k, nerrs, tb, S, [shards[s * m + i] for s in range(S) for i in surv],
                             [shards[s * m + e] for s in range(S) for e in pats[0]])

    def run_batches():
        for b in batches:
            b.encode(0)

    routes = [("repair", lambda: repair.run(0)), ("batches", run_batches), ("ceiling", lambda: ceiling.encode(0))]

    # the two routes under comparison compute the same bytes (the ceiling
    # route then overwrites the destinations of pats[0] in every stripe: it is
    # timed, not checked, and runs last in every round)
    repair.run(0)
    want = int(buf.view(torch.int64).sum().item())
    buf[torch.tensor([s * m + e for s in range(S) for e in of[s]], device=dev)] = 0xA5
    run_batches()
    got = int(buf.view(torch.int64).sum().item())
    if want != got:
        raise SystemExit(f"repair and per-pattern batches disagree ({want} != {got})")

    launches = {}
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        n0 = isal_amd.kernel_launches()
        fn()
        launches[name] = isal_amd.kernel_launches() - n0
    torch.cuda.synchronize()
    nbytes = (k + nerrs) * len_ * S
    for rnd in range(args.rounds):
        for name, fn in routes:
            ms = time_steps(torch, fn, args.steps)
            emit({"tool": "repair_bench", "gen": args.gen, "k": k, "m": m, "nerrs": nerrs, "len": len_,
                  "stripes": S, "patterns": npat, "route": name, "round": rnd, "steps": args.steps,
                  "launches_per_step": launches[name], "ms_per_step": round(ms, 5),
                  "bytes_per_step": nbytes, "GBps": round(nbytes / ms / 1e6, 1)})
    for b in batches + [ceiling]:
        b.close()
    repair.close()
    del buf
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gen", choices=("rs", "cauchy"), default="rs")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--m", type=int, default=14)
    ap.add_argument("--nerrs", type=int, default=3)
    ap.add_argument("--len", type=int, default=None, help="bytes per shard (default: both issue shapes)")
    ap.add_argument("--stripes", type=int, default=None)
    ap.add_argument("--patterns", type=int, nargs="*", default=[1, 14, 364])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("repair_bench: needs the GPU (no timing without one)")
    shapes = [(args.len, args.stripes)] if args.len else [(1 << 20, 1024), (1 << 16, 16384)]
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for len_, S in shapes:
        for npat in args.patterns:
            run_shape(args, torch, isal_amd, len_, S or 1024, npat, emit)


if __name__ == "__main__":
    main()
