#!/usr/bin/env python3
"""Ragged batch against one batch per length and against a uniform batch (not
shipped).

One geometry (rs, k sources, `rows` parity rows); stripe lengths drawn with a
fixed seed from 64 distinct values between 4 KiB and 1 MiB (not all multiples
of 16), as many stripes as make the source bytes total --gib GiB. Four routes
for the encode and the same four for the check:

  ragged        one isal_amd.Ragged.encode / .check over all stripes
  per_length    one isal_amd.Batch.encode / .check per distinct length on the
                same shards: the route a caller has without the ragged batch
  uniform       one Batch over as many stripes of one length (the mean,
                rounded to 16) in an allocation of its own: the ceiling
  ragged_equal  Ragged with all lengths equal on uniform's shards: what the
                item lookup itself costs

Before anything is timed the ragged parity is compared byte for byte with the
per-length batches' on the same shards, ragged_equal's with uniform's, and
every check must report every stripe consistent. Timing: HIP events around
`steps` back-to-back runs on the current stream, after a warm-up of every
route; the routes are interleaved round by round, each round starting with
another route, so that they share whatever else the machine is doing. One JSON
line per (op, route, round), to stdout and to --out.

  tools/ragged_bench.py --out profiles/ragged_ab.jsonl
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


def draw_lengths(seed, total):
    """64 distinct lengths in [4 KiB, 1 MiB], then stripes cycling through
    them in a shuffled order until their sum reaches total."""
    rng = random.Random(seed)
    values = rng.sample(range(4096, (1 << 20) + 1), 64)
    assert any(v % 16 for v in values)
    lens, at = [], 0
    while at < total:
        lens.append(values[len(lens) % 64])
        at += lens[-1]
    rng.shuffle(lens)
    return lens


class Shards:
    """Stripes of the given lengths in one device allocation: every shard
    16-byte aligned, sources random, parity zero."""

    def __init__(self, torch, dev, gen, k, rows, lens):
        m = k + rows
        self.k, self.rows, self.lens = k, rows, lens
        off, at = [], 0
        for n in lens:
            span = (n + 15) // 16 * 16
            off.append(at)
            at += m * span
        self.buf = torch.empty(at, dtype=torch.uint8, device=dev)
        self.buf.random_(generator=gen)
        base = self.buf.data_ptr()
        assert base % 16 == 0
        self.data, self.coding = [], []
        for n, o in zip(lens, off):
            span = (n + 15) // 16 * 16
            self.data += [base + o + j * span for j in range(k)]
            self.coding += [base + o + (k + l) * span for l in range(rows)]
        self.bytes = m * sum(lens)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
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
        raise SystemExit("ragged_bench: needs the GPU (no timing without one)")
    k, rows = args.k, args.rows
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    a = isal_amd.gf_gen_rs_matrix(k + rows, k)
    tbls = isal_amd.ec_init_tables(k, rows, a[k * k:])
    lens = draw_lengths(args.seed, int(args.gib * (1 << 30)) // k)
    S = len(lens)
    mean = (sum(lens) // S + 15) // 16 * 16

    rag = Shards(torch, dev, gen, k, rows, lens)
    uni = Shards(torch, dev, gen, k, rows, [mean] * S)

    ragged = isal_amd.Ragged(k, rows, tbls, lens, rag.data, rag.coding)
    by_len = {}
    for s, n in enumerate(lens):
        by_len.setdefault(n, []).append(s)
    per_length = []
    for n, ss in sorted(by_len.items()):
        b = isal_amd.Batch(n, k, rows, tbls, len(ss), [rag.data[s * k + j] for s in ss for j in range(k)],
                           [rag.coding[s * rows + l] for s in ss for l in range(rows)])
        per_length.append((b, torch.zeros(len(ss), dtype=torch.int64, device=dev)))
    uniform = isal_amd.Batch(mean, k, rows, tbls, S, uni.data, uni.coding)
    ragged_equal = isal_amd.Ragged(k, rows, tbls, [mean] * S, uni.data, uni.coding)
    bad = {name: torch.zeros(S, dtype=torch.int64, device=dev) for name in ("ragged", "uniform", "ragged_equal")}

    def per_length_encode():
        for b, _ in per_length:
            b.encode(0)

    def per_length_check():
        for b, w in per_length:
            b.check(w, 0)

    routes = {
        "encode": [("ragged", lambda: ragged.encode(0)), ("per_length", per_length_encode),
                   ("uniform", lambda: uniform.encode(0)), ("ragged_equal", lambda: ragged_equal.encode(0))],
        "check": [("ragged", lambda: ragged.check(bad["ragged"], 0)), ("per_length", per_length_check),
                  ("uniform", lambda: uniform.check(bad["uniform"], 0)),
                  ("ragged_equal", lambda: ragged_equal.check(bad["ragged_equal"], 0))],
    }

    # the routes compute the same bytes before anything is timed: the ragged
    # route writes over the random bytes the parity shards start with, then
    # the batches write over that
    for sh, ragged_fn, batch_fn in ((rag, routes["encode"][0][1], per_length_encode),
                                    (uni, routes["encode"][3][1], routes["encode"][2][1])):
        ragged_fn()
        torch.cuda.synchronize()
        ref = sh.buf.clone()
        batch_fn()
        torch.cuda.synchronize()
        if not torch.equal(sh.buf, ref):
            raise SystemExit("ragged_bench: the ragged parity differs from the batch's")
        del ref
    for _, fn in routes["check"]:
        fn()
    torch.cuda.synchronize()
    words = [w for w in bad.values()] + [w for _, w in per_length]
    if any(int((w != -1).sum().item()) for w in words):
        raise SystemExit("ragged_bench: encoded stripes do not verify")

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for op, rts in routes.items():
        launches = {}
        for name, fn in rts:
            for _ in range(args.warmup):
                fn()
            n0 = isal_amd.kernel_launches()
            fn()
            launches[name] = isal_amd.kernel_launches() - n0
        torch.cuda.synchronize()
        for rnd in range(args.rounds):
            for name, fn in rts[rnd % len(rts):] + rts[:rnd % len(rts)]:  # every route leads a round
                ms = time_steps(torch, fn, args.steps)
                nbytes = (uni if name in ("uniform", "ragged_equal") else rag).bytes
                emit({"tool": "ragged_bench", "op": op, "gen": "rs", "k": k, "rows": rows, "stripes": S,
                      "distinct_lengths": len(by_len), "min_len": min(lens), "max_len": max(lens), "uniform_len": mean,
                      "route": name, "round": rnd, "steps": args.steps, "launches_per_step": launches[name],
                      "ms_per_step": round(ms, 5), "bytes_per_step": nbytes, "GBps": round(nbytes / ms / 1e6, 1)})


if __name__ == "__main__":
    main()
