#!/usr/bin/env python3
"""Ragged repair against one repair batch per (length, count) pair and against
a uniform repair batch (not shipped).

One geometry (rs, k of m shards); tools/ragged_bench.py's stripe lengths (64
distinct values between 4 KiB and 1 MiB, as many stripes as make the source
bytes total --gib GiB); every stripe loses 1 to --max-errs shards, count and
pattern drawn with the same seed from all patterns of each count. Four routes:

  ragged        one isal_amd.Repair.ragged run over all stripes
  per_pair      one isal_amd.Repair per (length, count) pair on the same
                shards: the route a caller has without the ragged repair
  uniform       one Repair over as many stripes of one length (the mean,
                rounded to 16) that all lost --max-errs shards, in an
                allocation of its own: the ceiling
  ragged_equal  Repair.ragged with those equal lengths and counts on uniform's
                shards: what the item and length lookups themselves cost

Before anything is timed the image the ragged run leaves is compared byte for
byte with the one per_pair leaves on the same shards (the erased shards filled
with other bytes in between), and ragged_equal's with uniform's. Timing: HIP
events around `steps` back-to-back runs on the current stream, after a warm-up
of every route; the routes are interleaved round by round, each round starting
with another route, so that they share whatever else the machine is doing. One
JSON line per (route, round), to stdout and to --out.

  tools/repair_ragged_bench.py --out profiles/repair_ragged_ab.jsonl
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
    """Stripes of the given lengths in one device allocation: every shard
    16-byte aligned and random; shards[s*m + i]."""

    def __init__(self, torch, dev, gen, m, lens):
        self.m, self.lens = m, lens
        self.span = [(n + 15) // 16 * 16 for n in lens]
        self.off, at = [], 0
        for sp in self.span:
            self.off.append(at)
            at += m * sp
        self.buf = torch.empty(at, dtype=torch.uint8, device=dev)
        self.buf.random_(generator=gen)
        base = self.buf.data_ptr()
        assert base % 16 == 0
        self.shards = [base + o + i * sp for o, sp in zip(self.off, self.span) for i in range(m)]

    def scribble(self, errs, value):
        """Other bytes into every erased shard: a route that then leaves the
        reference image has written all of them."""
        for s, row in enumerate(errs):
            for e in row:
                at = self.off[s] + e * self.span[s]
                self.buf[at:at + self.lens[s]] = value


def same_image(torch, sh, errs, first, second, what):
    first()
    torch.cuda.synchronize()
    ref = sh.buf.clone()
    sh.scribble(errs, 0x5A)
    second()
    torch.cuda.synchronize()
    if not torch.equal(sh.buf, ref):
        raise SystemExit(f"repair_ragged_bench: {what}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--m", type=int, default=14)
    ap.add_argument("--max-errs", type=int, default=3)
    ap.add_argument("--gib", type=float, default=10.0, help="source bytes per step, GiB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("repair_ragged_bench: needs the GPU (no timing without one)")
    k, m, E = args.k, args.m, args.max_errs
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    a = isal_amd.gf_gen_rs_matrix(m, k)
    lens = draw_lengths(args.seed, int(args.gib * (1 << 30)) // k)
    S = len(lens)
    mean = (sum(lens) // S + 15) // 16 * 16
    rng = random.Random(args.seed + 1)
    errs = [rng.sample(range(m), rng.randint(1, E)) for _ in range(S)]
    errs_eq = [rng.sample(range(m), E) for _ in range(S)]

    rag = Shards(torch, dev, gen, m, lens)
    uni = Shards(torch, dev, gen, m, [mean] * S)

    ragged = isal_amd.Repair.ragged(k, m, a, lens, errs, rag.shards)
    pairs = {}
    for s, (n, row) in enumerate(zip(lens, errs)):
        pairs.setdefault((n, len(row)), []).append(s)
    per_pair = [isal_amd.Repair(n, k, m, a, c, len(ss), [e for s in ss for e in errs[s]],
                                [rag.shards[s * m + i] for s in ss for i in range(m)])
                for (n, c), ss in sorted(pairs.items())]
    uniform = isal_amd.Repair(mean, k, m, a, E, S, [e for row in errs_eq for e in row], uni.shards)
    ragged_equal = isal_amd.Repair.ragged(k, m, a, [mean] * S, errs_eq, uni.shards)

    def per_pair_run():
        for r in per_pair:
            r.run(0)

    routes = [("ragged", lambda: ragged.run(0)), ("per_pair", per_pair_run), ("uniform", lambda: uniform.run(0)),
              ("ragged_equal", lambda: ragged_equal.run(0))]

    same_image(torch, rag, errs, routes[0][1], routes[1][1], "the ragged image differs from the per-pair batches'")
    same_image(torch, uni, errs_eq, routes[3][1], routes[2][1], "ragged_equal's image differs from the uniform batch's")

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    # bytes a step moves: k survivors read and the erased shards written
    moved = {"rag": sum(n * (k + len(row)) for n, row in zip(lens, errs)), "uni": S * mean * (k + E)}
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
            emit({"tool": "repair_ragged_bench", "gen": "rs", "k": k, "m": m, "max_errs": E, "stripes": S,
                  "distinct_lengths": len(set(lens)), "pairs": len(pairs), "patterns": ragged.npatterns(),
                  "min_len": min(lens), "max_len": max(lens), "uniform_len": mean, "route": name, "round": rnd,
                  "steps": args.steps, "launches_per_step": launches[name], "ms_per_step": round(ms, 5),
                  "bytes_per_step": nbytes, "GBps": round(nbytes / ms / 1e6, 1)})


if __name__ == "__main__":
    main()
