#!/usr/bin/env python3
"""Scrub batch against the batch check, its ceiling (not shipped).

For one geometry and shard size three routes run over the same
device-resident, correctly encoded stripes:

  scrub_clean    one isal_amd.Scrub.run on consistent stripes: the verify plus
                 a fill of the verdict words
  check          one isal_amd.Batch.check on the same shards: the ceiling (the
                 same reads, no location branch in the kernel)
  scrub_corrupt  Scrub.run with one byte flipped in 1 % of the stripes (a
                 seeded choice of stripe, shard and column): the cold path runs
                 in one lane of each such stripe
  check_corrupt  Batch.check on those corrupt shards: scrub_corrupt's ceiling
                 on the same allocation (the corrupt route keeps shards of its
                 own, and a route's rate moves by a few per cent with the
                 allocation it reads)

Every route reads (k + rows) * len bytes per stripe and writes nothing but
its result words. Timing: HIP events around `steps` back-to-back runs on the
current stream, after a warm-up of every route; the routes are interleaved
round by round, each round starting with another route, so that they share
whatever else the machine is doing. The clean routes never see a flip.
One JSON line per (shape, route, round), to stdout and to --out.

  tools/scrub_bench.py --out profiles/scrub_ab.jsonl
  tools/scrub_bench.py --len 65536 --stripes 16384
"""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isa-l_amd"))


def time_steps(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def run_shape(args, torch, isal_amd, len_, S, emit):
    k, rows = args.k, args.rows
    m = k + rows
    a = isal_amd.gf_gen_rs_matrix(m, k)
    tbls = isal_amd.ec_init_tables(k, rows, a[k * k:])
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)

    def encoded():
        """S stripes (S, m, len_), parity from Batch.encode; pointer lists."""
        sh = torch.empty((S, m, len_), dtype=torch.uint8, device=dev)
        sh[:, :k].random_(generator=gen)
        base = sh.data_ptr()
        data = [base + (s * m + j) * len_ for s in range(S) for j in range(k)]
        coding = [base + (s * m + k + l) * len_ for s in range(S) for l in range(rows)]
        b = isal_amd.Batch(len_, k, rows, tbls, S, data, coding)
        b.encode(0)
        torch.cuda.synchronize()
        return sh, data, coding, b

    assert len_ % 16 == 0
    clean, c_data, c_coding, check = encoded()
    dirty, d_data, d_coding, check_dirty = encoded()
    rng = random.Random(args.seed)
    hit = sorted(rng.sample(range(S), max(1, S // 100)))
    want = {}
    for s in hit:
        i, col = rng.randrange(m), rng.randrange(len_)
        dirty[s, i, col] ^= 1 << rng.randrange(8)
        want[s] = i
    torch.cuda.synchronize()

    scrub_clean = isal_amd.Scrub(len_, k, rows, tbls, S, c_data, c_coding)
    scrub_dirty = isal_amd.Scrub(len_, k, rows, tbls, S, d_data, d_coding)
    v_clean = torch.zeros(S, dtype=torch.int32, device=dev)
    v_dirty = torch.zeros(S, dtype=torch.int32, device=dev)
    bad = torch.zeros(S, dtype=torch.int64, device=dev)
    bad_dirty = torch.zeros(S, dtype=torch.int64, device=dev)
    routes = [("scrub_clean", lambda: scrub_clean.run(v_clean, 0)), ("check", lambda: check.check(bad, 0)),
              ("scrub_corrupt", lambda: scrub_dirty.run(v_dirty, 0)),
              ("check_corrupt", lambda: check_dirty.check(bad_dirty, 0))]

    # the routes answer what they should before anything is timed
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    if int((v_clean != -1).sum().item()) or int((bad != -1).sum().item()):
        raise SystemExit("scrub_bench: the clean stripes do not verify")
    got = v_dirty.cpu().tolist()
    for s in range(S):
        if got[s] != want.get(s, -1):
            raise SystemExit(f"scrub_bench: stripe {s}: verdict {got[s]}, want {want.get(s, -1)}")

    launches = {}
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        n0 = isal_amd.kernel_launches()
        fn()
        launches[name] = isal_amd.kernel_launches() - n0
    torch.cuda.synchronize()
    nbytes = m * len_ * S
    for rnd in range(args.rounds):
        for name, fn in routes[rnd % len(routes):] + routes[:rnd % len(routes)]:  # every route leads a round
            ms = time_steps(torch, fn, args.steps)
            emit({"tool": "scrub_bench", "gen": "rs", "k": k, "rows": rows, "len": len_, "stripes": S,
                  "corrupt_stripes": len(hit) if name.endswith("_corrupt") else 0, "route": name, "round": rnd,
                  "steps": args.steps, "launches_per_step": launches[name], "ms_per_step": round(ms, 5),
                  "bytes_per_step": nbytes, "GBps": round(nbytes / ms / 1e6, 1)})
    check.close()
    check_dirty.close()
    scrub_clean.close()
    scrub_dirty.close()
    del clean, dirty
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--len", type=int, default=None, help="bytes per shard (default: both issue shapes)")
    ap.add_argument("--stripes", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("scrub_bench: needs the GPU (no timing without one)")
    shapes = [(args.len, args.stripes)] if args.len else [(1 << 20, 1024), (1 << 16, 16384)]
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for len_, S in shapes:
        run_shape(args, torch, isal_amd, len_, S or 1024, emit)


if __name__ == "__main__":
    main()
