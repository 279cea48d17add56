#!/usr/bin/env python3
"""Ragged CRC64 against one batch CRC64 per length and against the uniform
batch, its floor (not shipped).

The workload of tools/ragged_crc_bench.py (profiles/ragged_crc_ab.jsonl): one
geometry (rs, k sources, `rows` parity rows); stripe lengths drawn with a fixed
seed from 64 distinct values between 4 KiB and 1 MiB (not all multiples of
16), as many stripes as make the source bytes total --gib GiB, encoded by
Ragged.encode. Three routes, each crc64_<variant> of every source and parity
shard, for one reflected and one normal flavour (--variants):

  ragged      one isal_amd.Ragged.crc64 over all stripes (2 launches)
  per_length  one uniform isal_amd.Batch.crc64 per distinct length on the same
              shards: the route a caller has without the ragged checksum
              (2 launches per length, and a table set per length)
  uniform     one isal_amd.Batch.crc64 over as many stripes of one length (the
              mean) with the same total bytes: the floor

Before anything is timed the ragged and the per-length words are compared with
each other, a sample of shards of the ragged and of the uniform route with
crc64_<variant> on the host, and every route's launch count is taken. Timing:
HIP events around `steps` back-to-back runs on the current stream, after a
warm-up of every route; the routes are interleaved round by round, each round
starting with another route. One JSON line per (variant, route, round), to
stdout and to --out; a last line per route pair gives the ratio of the medians
and each route's range. --routes ragged --rounds 1 is the run to put under a
kernel trace for the times of the pass and the combine alone.

  tools/ragged_crc64_bench.py --out profiles/ragged_crc64_ab.jsonl
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

INIT = 0x9E3779B97F4A7C15


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--gib", type=float, default=10.0, help="source bytes per step, GiB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--variants", default="rocksoft_refl,ecma_norm", help="CRC64_VARIANTS names, comma-separated")
    ap.add_argument("--routes", default="ragged,per_length,uniform", help="routes to time, comma-separated")
    ap.add_argument("--sample", type=int, default=48, help="shards per route checked on the host")
    ap.add_argument("--label", default=None, help="copied into every JSON line (which build was measured)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("ragged_crc64_bench: needs the GPU (no timing without one)")
    k, rows = args.k, args.rows
    m = k + rows
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    a = isal_amd.gf_gen_rs_matrix(m, k)
    tbls = isal_amd.ec_init_tables(k, rows, a[k * k:])
    lens = draw_lengths(args.seed, int(args.gib * (1 << 30)) // k)
    S = len(lens)
    mean = (sum(lens) // S + 15) // 16 * 16
    by_len = {}
    for s, n in enumerate(lens):
        by_len.setdefault(n, []).append(s)
    timed = args.routes.split(",")

    rag = Shards(torch, dev, gen, k, rows, lens)
    uni = Shards(torch, dev, gen, k, rows, [mean] * S)
    ragged = isal_amd.Ragged(k, rows, tbls, lens, rag.data, rag.coding)
    ragged.encode(0)
    uniform = isal_amd.Batch(mean, k, rows, tbls, S, uni.data, uni.coding)
    uniform.encode(0)
    per_length = []
    for n, ss in sorted(by_len.items()):
        b = isal_amd.Batch(n, k, rows, tbls, len(ss), [rag.data[s * k + j] for s in ss for j in range(k)],
                           [rag.coding[s * rows + l] for s in ss for l in range(rows)])
        per_length.append((b, torch.zeros(len(ss) * m, dtype=torch.int64, device=dev), ss))
    words = {name: torch.zeros(S * m, dtype=torch.int64, device=dev) for name in ("ragged", "uniform")}
    torch.cuda.synchronize()

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        if args.label:
            rec["label"] = args.label
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for vname in args.variants.split(","):
        variant = isal_amd.CRC64_VARIANTS.index(vname)

        def run_per_length():
            for b, w, _ in per_length:
                b.crc64(variant, INIT, w, 0)

        routes = [("ragged", lambda: ragged.crc64(variant, INIT, words["ragged"], 0)), ("per_length", run_per_length),
                  ("uniform", lambda: uniform.crc64(variant, INIT, words["uniform"], 0))]

        # the routes answer what they should before anything is timed
        for _, fn in routes:
            fn()
        torch.cuda.synchronize()
        got = {name: w.cpu().numpy().view(np.uint64) for name, w in words.items()}
        scattered = np.zeros(S * m, np.uint64)
        for _, w, ss in per_length:
            v = w.cpu().numpy().view(np.uint64).reshape(len(ss), m)
            for row, s in zip(v, ss):
                scattered[s * m:(s + 1) * m] = row
        if not np.array_equal(got["ragged"], scattered):
            pos = int(np.nonzero(got["ragged"] != scattered)[0][0])
            raise SystemExit(f"ragged_crc64_bench: {vname}: stripe {pos // m} (len {lens[pos // m]}) shard {pos % m}: "
                             f"ragged {int(got['ragged'][pos]):#018x}, per_length {int(scattered[pos]):#018x}")
        rng = random.Random(args.seed)
        for name, sh, ln in (("ragged", rag, lens), ("uniform", uni, [mean] * S)):
            base = sh.buf.data_ptr()
            for _ in range(args.sample):
                s, i = rng.randrange(S), rng.randrange(m)
                at = (sh.data[s * k + i] if i < k else sh.coding[s * rows + i - k]) - base
                host = sh.buf[at:at + ln[s]].cpu().numpy()
                want = isal_amd.crc64(variant, INIT, host, ln[s])
                if int(got[name][s * m + i]) != want:
                    raise SystemExit(f"ragged_crc64_bench: {vname}: {name}: stripe {s} (len {ln[s]}) shard {i}: "
                                     f"{int(got[name][s * m + i]):#018x}, host crc64 {want:#018x}")

        routes = [r for r in routes if r[0] in timed]
        launches = {}
        for name, fn in routes:
            for _ in range(args.warmup):
                fn()
            n0 = isal_amd.kernel_launches()
            fn()
            launches[name] = isal_amd.kernel_launches() - n0
        torch.cuda.synchronize()
        nbytes = {"ragged": m * sum(lens), "per_length": m * sum(lens), "uniform": m * mean * S}
        ms_of = {name: [] for name, _ in routes}
        common = {"tool": "ragged_crc64_bench", "variant": vname, "gen": "rs", "k": k, "rows": rows, "stripes": S,
                  "distinct_lengths": len(by_len), "min_len": min(lens), "max_len": max(lens), "uniform_len": mean}
        for rnd in range(args.rounds):
            for name, fn in routes[rnd % len(routes):] + routes[:rnd % len(routes)]:  # every route leads a round
                ms = time_steps(torch, fn, args.steps)
                ms_of[name].append(ms)
                emit(dict(common, route=name, round=rnd, steps=args.steps, launches_per_step=launches[name],
                          ms_per_step=round(ms, 5), bytes_per_step=nbytes[name],
                          GBps=round(nbytes[name] / ms / 1e6, 1)))
        x = ms_of.get("ragged")
        for other in ("per_length", "uniform"):
            y = ms_of.get(other)
            if x and y:
                emit(dict(common, summary=f"ragged / {other}",
                          ratio_of_medians=round(statistics.median(x) / statistics.median(y), 4),
                          ragged_ms_min_max=[round(min(x), 5), round(max(x), 5)],
                          other_ms_min_max=[round(min(y), 5), round(max(y), 5)]))
    ragged.close()
    uniform.close()
    for b, _, _ in per_length:
        b.close()


if __name__ == "__main__":
    main()
