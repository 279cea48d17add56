#!/usr/bin/env python3
"""T10 protection information per sector against the CRC32C sector pass over
the same bytes (not shipped).

The sector checksums' workload (tools/sector_crc_bench.py): rs, k sources and
`rows` parity rows, stripe lengths drawn with a fixed seed from 64 distinct
values between 4 KiB and 1 MiB, as many stripes as make the source bytes total
--gib GiB, encoded by Ragged.encode. For each sector size four routes over the
same shards:

  guard      isal_amd.Ragged.sector_t10dif: a 16-bit word per sector, 1 launch
  generate   isal_amd.Ragged.dif_generate: an 8-byte tuple per sector (type 1,
             a reference tag per shard), 1 launch
  verify     isal_amd.Ragged.dif_verify of those tuples, all clean: a fill of
             the per-shard words and 1 launch
  crc32c     isal_amd.Ragged.sector_crc: the yardstick, 1 launch

Before anything is timed a sample of guard words, short last sectors included,
is compared with a bytewise crc16_t10dif on the host, every tuple is decoded
and compared with its guard word and its tags, and verify must answer clean
for every shard. Timing: HIP events around `steps` back-to-back calls after a
warm-up, routes interleaved round by round, each round led by another route.
One JSON line per (sector, route, round), then one summary line per route
against crc32c.

  tools/dif_bench.py --out profiles/dif_ab.jsonl
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

INIT32, SEED16, APP_TAG = 0x9E3779B9, 0x1D0F, 0xA5C3


def crc16_t10dif(seed, data):
    crc = seed
    for b in data:
        crc ^= int(b) << 8
        for _ in range(8):
            crc = ((crc << 1) ^ (0x8BB7 if crc & 0x8000 else 0)) & 0xFFFF
    return crc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--gib", type=float, default=10.0, help="source bytes per step, GiB")
    ap.add_argument("--sectors", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--sample", type=int, default=64, help="sectors per case checked on the host")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import isal_amd

    if not torch.cuda.is_available():
        raise SystemExit("dif_bench: needs the GPU (no timing without one)")
    k, rows = args.k, args.rows
    m = k + rows
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    tbls = isal_amd.ec_init_tables(k, rows, isal_amd.gf_gen_rs_matrix(m, k)[k * k:])
    lens = draw_lengths(args.seed, int(args.gib * (1 << 30)) // k)
    S = len(lens)
    sh = Shards(torch, dev, gen, k, rows, lens)
    ragged = isal_amd.Ragged(k, rows, tbls, lens, sh.data, sh.coding)
    ragged.encode(0)
    torch.cuda.synchronize()
    base = sh.buf.data_ptr()
    shard_ptr = [[sh.data[s * k + j] if j < k else sh.coding[s * rows + j - k] for j in range(m)] for s in range(S)]
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    common = {"tool": "dif_bench", "gen": "rs", "k": k, "rows": rows, "stripes": S,
              "distinct_lengths": len(set(lens)), "min_len": min(lens), "max_len": max(lens)}
    rng = random.Random(args.seed)
    ref0_host = np.random.default_rng(args.seed).integers(0, 1 << 32, S * m, dtype=np.uint64).astype(np.uint32)
    ref0 = torch.from_numpy(ref0_host.view(np.int32).copy()).to(dev)
    for sector in args.sectors:
        first, total = isal_amd.ragged_sector_offsets(lens, sector)
        nsec = m * total
        w16 = torch.zeros(nsec, dtype=torch.int16, device=dev)
        w32 = torch.zeros(nsec, dtype=torch.int32, device=dev)
        pi = torch.zeros(nsec, dtype=torch.int64, device=dev)
        bad = torch.zeros(S * m, dtype=torch.int32, device=dev)
        kw = dict(type=isal_amd.DIF_TYPE1, app_tag=APP_TAG, seed=SEED16, ref0=ref0)
        routes = [("guard", lambda: ragged.sector_t10dif(sector, SEED16, w16, 0)),
                  ("generate", lambda: ragged.dif_generate(sector, pi, **kw)),
                  ("verify", lambda: ragged.dif_verify(sector, pi, bad, **kw)),
                  ("crc32c", lambda: ragged.sector_crc(sector, INIT32, w32, 0))]
        for _, fn in routes:
            fn()
        torch.cuda.synchronize()
        case = dict(common, sector=sector)
        words = w16.cpu().numpy().view(np.uint16)
        for t in range(args.sample):
            s = rng.randrange(S)
            j, ns = rng.randrange(m), -(-lens[s] // sector)
            i = ns - 1 if t % 2 else rng.randrange(ns)  # every other one a last sector
            n = min(sector, lens[s] - i * sector)
            at = shard_ptr[s][j] - base + i * sector
            want = crc16_t10dif(SEED16, sh.buf[at:at + n].cpu().numpy())
            word = int(words[m * int(first[s]) + j * ns + i])
            if word != want:
                raise SystemExit(f"dif_bench: sector {sector}: stripe {s} (len {lens[s]}) shard {j} sector {i}: "
                                 f"{word:#x}, host {want:#x}")
        # every tuple: its guard word, the application tag, ref0 of its shard + the sector's index
        tup = pi.cpu().numpy().view(np.uint8).reshape(-1, 8)
        guard = tup[:, 0].astype(np.uint16) << 8 | tup[:, 1]
        app = tup[:, 2].astype(np.uint16) << 8 | tup[:, 3]
        ref = tup[:, 4:8].astype(np.uint32) @ np.array([1 << 24, 1 << 16, 1 << 8, 1], dtype=np.uint32)
        want_ref = np.concatenate([(ref0_host[s * m + j] + np.arange(-(-n // sector), dtype=np.uint32)).astype(np.uint32)
                                   for s, n in enumerate(lens) for j in range(m)])
        if not (np.array_equal(guard, words) and (app == APP_TAG).all() and np.array_equal(ref, want_ref)):
            raise SystemExit(f"dif_bench: sector {sector}: a generated tuple differs from its guard word or its tags")
        if not (bad.cpu().numpy().view(np.uint32) == isal_amd.DIF_CLEAN).all():
            raise SystemExit(f"dif_bench: sector {sector}: verify of the generated tuples is not clean")
        launches = {}
        for rname, fn in routes:
            for _ in range(args.warmup):
                fn()
            n0 = isal_amd.kernel_launches()
            fn()
            launches[rname] = isal_amd.kernel_launches() - n0
        torch.cuda.synchronize()
        nbytes = m * sum(lens)
        ms_of = {rname: [] for rname, _ in routes}
        for rnd in range(args.rounds):
            lead = rnd % len(routes)
            for rname, fn in routes[lead:] + routes[:lead]:  # every route leads a round
                ms = time_steps(torch, fn, args.steps)
                ms_of[rname].append(ms)
                emit(dict(case, route=rname, round=rnd, steps=args.steps, launches_per_step=launches[rname],
                          sectors=int(nsec), ms_per_step=round(ms, 5), bytes_per_step=int(nbytes),
                          GBps=round(nbytes / ms / 1e6, 1)))
        y = ms_of["crc32c"]
        for rname, _ in routes[:3]:
            x = ms_of[rname]
            emit(dict(case, summary=f"{rname} / crc32c",
                      ratio_of_medians=round(statistics.median(x) / statistics.median(y), 4),
                      ms_min_max=[round(min(x), 5), round(max(x), 5)],
                      crc32c_ms_min_max=[round(min(y), 5), round(max(y), 5)]))
        del w16, w32, pi, bad
        torch.cuda.empty_cache()
    ragged.close()


if __name__ == "__main__":
    main()
