#!/usr/bin/env python3
"""Overwrite batch against the composed route and the update ceiling (not shipped).

For one geometry and shard size, with one rewritten data shard per stripe
(nw = 1) whose index is the same in every stripe ("uniform") or spread over
all k values ("mixed"), three routes run over the same device-resident bytes:

  overwrite  one isal_amd.Overwrite.run(commit=True): parity ^= C * (old ^ new)
             and new stored over old, one launch per pass
  composed   what the API offered before: torch.bitwise_xor(old, new,
             out=scratch), one isal_amd.Batch.update per distinct index over
             that index's stripes, then old.copy_(new)
  ceiling    one uniform-index Batch.update over the same parity: the memory
             skeleton of a parity read-modify-write without the old / new
             traffic; compare by bytes moved

Bytes per step and stripe, for P parity rows: overwrite (2 + P) reads +
(P + 1) writes, composed 3 (xor) + (1 + 2 P) (update) + 2 (copy), ceiling
1 + 2 P. Timing: HIP events around `steps` back-to-back runs on the current
stream, after a warm-up of every route; the routes are interleaved round by
round so that they share whatever else the machine is doing. One JSON line
per (shape, index mode, route, round), to stdout and to --out.

  tools/overwrite_bench.py --out profiles/overwrite_ab.jsonl
  tools/overwrite_bench.py --len 65536 --stripes 16384 --index mixed
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


def run_shape(args, torch, isal_amd, len_, S, mode, emit):
    k, rows = args.k, args.rows
    a = isal_amd.gf_gen_rs_matrix(k + rows, k)
    tbls = isal_amd.ec_init_tables(k, rows, a[k * k:])
    rng = random.Random(args.seed)
    idx = [args.vec_i] * S if mode == "uniform" else [s % k for s in range(S)]
    rng.shuffle(idx)

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    old = torch.empty((S, len_), dtype=torch.uint8, device=dev).random_(generator=gen)
    new = torch.empty((S, len_), dtype=torch.uint8, device=dev).random_(generator=gen)
    parity = torch.empty((S * rows, len_), dtype=torch.uint8, device=dev).random_(generator=gen)
    scratch = torch.empty((S, len_), dtype=torch.uint8, device=dev)
    old0, parity0 = old.clone(), parity.clone()
    assert all(t.data_ptr() % 16 == 0 for t in (old, new, parity, scratch)) and len_ % 16 == 0
    p_old = [old.data_ptr() + s * len_ for s in range(S)]
    p_new = [new.data_ptr() + s * len_ for s in range(S)]
    p_par = [parity.data_ptr() + r * len_ for r in range(S * rows)]
    p_scr = [scratch.data_ptr() + s * len_ for s in range(S)]

    over = isal_amd.Overwrite(len_, k, rows, tbls, 1, S, idx, p_old, p_new, p_par)
    # update(j) reads data[s*k + j] only: every slot of a stripe names its scratch row
    batches = []
    for j in sorted(set(idx)):
        ss = [s for s in range(S) if idx[s] == j]
        batches.append((j, isal_amd.Batch(len_, k, rows, tbls, len(ss), [p_scr[s] for s in ss for _ in range(k)],
                                          [p_par[s * rows + l] for s in ss for l in range(rows)])))
    ceiling = isal_amd.Batch(len_, k, rows, tbls, S, [p_scr[s] for s in range(S) for _ in range(k)], p_par)

    def run_composed():
        torch.bitwise_xor(old, new, out=scratch)
        for j, b in batches:
            b.update(j, 0)
        old.copy_(new)

    routes = [("overwrite", lambda: over.run(commit=True, stream=0)), ("composed", run_composed),
              ("ceiling", lambda: ceiling.update(args.vec_i, 0))]

    # the two routes under comparison compute the same bytes from the same start
    over.run(commit=True, stream=0)
    want = (int(parity.view(torch.int64).sum().item()), int(old.view(torch.int64).sum().item()))
    old.copy_(old0)
    parity.copy_(parity0)
    run_composed()
    got = (int(parity.view(torch.int64).sum().item()), int(old.view(torch.int64).sum().item()))
    if want != got or not torch.equal(old, new):
        raise SystemExit(f"overwrite and the composed route disagree ({want} != {got})")
    del old0, parity0

    launches = {}
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        n0 = isal_amd.kernel_launches()
        fn()
        launches[name] = isal_amd.kernel_launches() - n0
    launches["composed"] += 2  # the xor and the copy are torch's kernels
    torch.cuda.synchronize()
    per = {"overwrite": 2 + rows + rows + 1, "composed": 3 + (1 + 2 * rows) + 2, "ceiling": 1 + 2 * rows}
    for rnd in range(args.rounds):
        for name, fn in routes:
            ms = time_steps(torch, fn, args.steps)
            nbytes = per[name] * len_ * S
            emit({"tool": "overwrite_bench", "gen": "rs", "k": k, "rows": rows, "nw": 1, "len": len_, "stripes": S,
                  "index": mode, "distinct": len(batches), "route": name, "round": rnd, "steps": args.steps,
                  "launches_per_step": launches[name], "ms_per_step": round(ms, 5), "bytes_per_step": nbytes,
                  "GBps": round(nbytes / ms / 1e6, 1)})
    for _, b in batches:
        b.close()
    ceiling.close()
    over.close()
    del old, new, parity, scratch
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--vec-i", type=int, default=3, help="the uniform index (and the ceiling's)")
    ap.add_argument("--len", type=int, default=None, help="bytes per shard (default: both issue shapes)")
    ap.add_argument("--stripes", type=int, default=None)
    ap.add_argument("--index", choices=("uniform", "mixed"), nargs="*", default=["uniform", "mixed"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("overwrite_bench: needs the GPU (no timing without one)")
    shapes = [(args.len, args.stripes)] if args.len else [(1 << 20, 1024), (1 << 16, 16384)]
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for len_, S in shapes:
        for mode in args.index:
            run_shape(args, torch, isal_amd, len_, S or 1024, mode, emit)


if __name__ == "__main__":
    main()
