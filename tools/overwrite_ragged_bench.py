#!/usr/bin/env python3
"""Ragged overwrite against one overwrite batch per (length, count) pair and
against a uniform overwrite batch (not shipped).

One geometry (rs, k data shards, `rows` parity rows); tools/ragged_bench.py's
stripe lengths (64 distinct values between 4 KiB and 1 MiB, as many stripes as
make the data bytes total --gib GiB); every stripe rewrites 1 to --max-nw of
its data shards over its whole length, count and indices drawn with the same
seed. Four routes:

  ragged        one isal_amd.Overwrite.ragged run over all stripes
  per_pair      one isal_amd.Overwrite per (length, count) pair on the same
                shards: the route a caller has without the ragged overwrite
  uniform       one Overwrite over as many stripes of one length (the mean,
                rounded to 16) that all rewrite --uniform-nw shards, in an
                allocation of its own: the ceiling
  ragged_equal  Overwrite.ragged with those equal lengths and counts on
                uniform's shards: what the item, length and count lookups
                themselves cost

Before anything is timed the image the ragged run leaves is compared byte for
byte with the one per_pair leaves on the same (re-uploaded) shards, and
ragged_equal's with uniform's, without and with commit. Timing: HIP events
around `steps` back-to-back runs without commit on the current stream (each
run folds the same delta in again, so the bytes moved never change), after a
warm-up of every route; the routes are interleaved round by round, each round
starting with another route, so that they share whatever else the machine is
doing. One JSON line per (route, round), to stdout and to --out.

  tools/overwrite_ragged_bench.py --out profiles/overwrite_ragged_ab.jsonl
"""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isa-l_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from ragged_bench import draw_lengths, time_steps  # noqa: E402


class Shards:
    """Stripes of the given lengths in one device allocation, every shard
    16-byte aligned and random: per stripe its k data shards, its rows parity
    rows, then one `new` buffer per slot of sets[s]."""

    def __init__(self, torch, dev, gen, k, rows, lens, sets):
        self.old, self.new, self.coding = [], [], []
        at = 0
        spans = [(n + 15) // 16 * 16 for n in lens]
        total = sum(sp * (k + rows + len(ix)) for sp, ix in zip(spans, sets))
        self.buf = torch.empty(total, dtype=torch.uint8, device=dev)
        self.buf.random_(generator=gen)
        base = self.buf.data_ptr()
        assert base % 16 == 0
        for sp, ix in zip(spans, sets):
            self.old.append([base + at + j * sp for j in ix])
            self.coding += [base + at + (k + l) * sp for l in range(rows)]
            self.new.append([base + at + (k + rows + i) * sp for i in range(len(ix))])
            at += sp * (k + rows + len(ix))


def same_image(torch, sh, first, second, what):
    """Both routes leave the same bytes on the same upload, for both flags."""
    orig = sh.buf.clone()
    for commit in (False, True):
        first(commit)
        torch.cuda.synchronize()
        ref = sh.buf.clone()
        if torch.equal(ref, orig):
            raise SystemExit(f"overwrite_ragged_bench: the first route changed nothing (commit={commit})")
        sh.buf.copy_(orig)
        second(commit)
        torch.cuda.synchronize()
        if not torch.equal(sh.buf, ref):
            raise SystemExit(f"overwrite_ragged_bench: {what} (commit={commit})")
        sh.buf.copy_(orig)
        del ref
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--max-nw", type=int, default=3)
    ap.add_argument("--uniform-nw", type=int, default=2, help="the uniform routes' count (the mean of 1..max-nw)")
    ap.add_argument("--gib", type=float, default=10.0, help="data bytes of the stripes, GiB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("overwrite_ragged_bench: needs the GPU (no timing without one)")
    k, rows, W, U = args.k, args.rows, args.max_nw, args.uniform_nw
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    a = isal_amd.gf_gen_rs_matrix(k + rows, k)
    tbls = isal_amd.ec_init_tables(k, rows, a[k * k:])
    lens = draw_lengths(args.seed, int(args.gib * (1 << 30)) // k)
    S = len(lens)
    mean = (sum(lens) // S + 15) // 16 * 16
    rng = random.Random(args.seed + 1)
    sets = [rng.sample(range(k), rng.randint(1, W)) for _ in range(S)]
    sets_eq = [rng.sample(range(k), U) for _ in range(S)]

    rag = Shards(torch, dev, gen, k, rows, lens, sets)
    uni = Shards(torch, dev, gen, k, rows, [mean] * S, sets_eq)

    def flat(rows_):
        return [x for r in rows_ for x in r]

    ragged = isal_amd.Overwrite.ragged(k, rows, tbls, lens, sets, rag.old, rag.new, rag.coding)
    pairs = {}
    for s, (n, ix) in enumerate(zip(lens, sets)):
        pairs.setdefault((n, len(ix)), []).append(s)
    per_pair = [isal_amd.Overwrite(n, k, rows, tbls, c, len(ss), flat(sets[s] for s in ss),
                                   flat(rag.old[s] for s in ss), flat(rag.new[s] for s in ss),
                                   [rag.coding[s * rows + l] for s in ss for l in range(rows)])
                for (n, c), ss in sorted(pairs.items())]
    uniform = isal_amd.Overwrite(mean, k, rows, tbls, U, S, flat(sets_eq), flat(uni.old), flat(uni.new), uni.coding)
    ragged_equal = isal_amd.Overwrite.ragged(k, rows, tbls, [mean] * S, sets_eq, uni.old, uni.new, uni.coding)

    def per_pair_run(commit=False):
        for o in per_pair:
            o.run(commit, 0)

    routes = [("ragged", lambda commit=False: ragged.run(commit, 0)), ("per_pair", per_pair_run),
              ("uniform", lambda commit=False: uniform.run(commit, 0)),
              ("ragged_equal", lambda commit=False: ragged_equal.run(commit, 0))]

    same_image(torch, rag, routes[0][1], routes[1][1], "the ragged image differs from the per-pair batches'")
    same_image(torch, uni, routes[3][1], routes[2][1], "ragged_equal's image differs from the uniform batch's")

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    # bytes a step moves: old and new of every slot read, every parity row read and written
    moved = {"rag": sum(n * (2 * len(ix) + 2 * rows) for n, ix in zip(lens, sets)), "uni": S * mean * (2 * U + 2 * rows)}
    launches = {}
    for name, fn in routes:
        for _ in range(args.warmup):
            fn()
        n0 = isal_amd.kernel_launches()
        fn()
        launches[name] = isal_amd.kernel_launches() - n0
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, fn in routes[rnd % len(routes):] + routes[:rnd % len(routes)]:  # every route leads a round
            ms = time_steps(torch, fn, args.steps)
            nbytes = moved["uni" if name in ("uniform", "ragged_equal") else "rag"]
            emit({"tool": "overwrite_ragged_bench", "gen": "rs", "k": k, "rows": rows, "max_nw": W, "uniform_nw": U,
                  "stripes": S, "distinct_lengths": len(set(lens)), "pairs": len(pairs), "min_len": min(lens),
                  "max_len": max(lens), "uniform_len": mean, "route": name, "round": rnd, "steps": args.steps,
                  "launches_per_step": launches[name], "ms_per_step": round(ms, 5), "bytes_per_step": nbytes,
                  "GBps": round(nbytes / ms / 1e6, 1)})


if __name__ == "__main__":
    main()
