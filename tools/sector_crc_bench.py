#!/usr/bin/env python3
"""Sector checksums against the whole-shard checksum of the same bytes and
against what a caller could do without them (not shipped).

The ragged checksum's workload (tools/ragged_crc_bench.py): rs, k sources and
`rows` parity rows, stripe lengths drawn with a fixed seed from 64 distinct
values between 4 KiB and 1 MiB, as many stripes as make the source bytes total
--gib GiB, encoded by Ragged.encode. For each sector size and each checksum
(crc32_iscsi, crc64_rocksoft_refl) three routes over the same shards:

  sector      one isal_amd.Ragged.sector_crc / sector_crc64: a word per sector,
              1 launch
  whole       isal_amd.Ragged.crc / crc64: a word per shard, pass + combine, 2
              launches: the byte-rate yardstick (what the log-step join costs)
  as_shards   what a caller has without sector checksums: a uniform Batch
              whose "shards" are the sectors (len = sector, k = 1, rows = 1, one
              8-byte pointer per sector) through Batch.crc / crc64, 2 launches.
              A uniform batch has one length, so it covers the WHOLE sectors
              only (every shard's short last sector is left out; the row says
              how many words it yields). Its create time is reported apart.

Before anything is timed the sector words are compared with as_shards' on
every whole sector and a sample of sectors, short last ones included, with the
host's crc32_iscsi / crc64. Timing: HIP events around `steps` back-to-back
calls after a warm-up, routes interleaved round by round, each round led by
another route. One JSON line per (sector, checksum, route, round), then one
summary line per pair of routes.

  tools/sector_crc_bench.py --out profiles/sector_crc_ab.jsonl
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "isa-l_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from ragged_bench import Shards, draw_lengths, time_steps  # noqa: E402

INIT32, INIT64 = 0x9E3779B9, 0x9E3779B97F4A7C15
ROCKSOFT_REFL = 6


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
        raise SystemExit("sector_crc_bench: needs the GPU (no timing without one)")
    k, rows = args.k, args.rows
    m = k + rows
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    L = isal_amd.lib()
    tbls = isal_amd.ec_init_tables(k, rows, isal_amd.gf_gen_rs_matrix(m, k)[k * k:])
    one = isal_amd.ec_init_tables(1, 1, np.ones(1, np.uint8))
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

    common = {"tool": "sector_crc_bench", "gen": "rs", "k": k, "rows": rows, "stripes": S,
              "distinct_lengths": len(set(lens)), "min_len": min(lens), "max_len": max(lens)}
    rng = random.Random(args.seed)
    for sector in args.sectors:
        first, total = isal_amd.ragged_sector_offsets(lens, sector)
        # the whole sectors, in the order of the sector words: their addresses and their words
        ptrs, idx = [], []
        for s, n in enumerate(lens):
            ns, nw = -(-n // sector), n // sector
            for j in range(m):
                ptrs.append(shard_ptr[s][j] + sector * np.arange(nw, dtype=np.uint64))
                idx.append(m * int(first[s]) + j * ns + np.arange(nw, dtype=np.int64))
        ptrs, idx = np.concatenate(ptrs), np.concatenate(idx)
        if ptrs.size % 2:  # stripes of k = 1 source and 1 parity row
            ptrs, idx = ptrs[:-1], idx[:-1]
        nstripes = ptrs.size // 2
        data, coding = np.ascontiguousarray(ptrs[0::2]), np.ascontiguousarray(ptrs[1::2])
        u8pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_ubyte))
        for name, variant in (("crc32_iscsi", None), ("crc64_rocksoft_refl", ROCKSOFT_REFL)):
            t32 = variant is None
            dt, npdt = (torch.int32, np.uint32) if t32 else (torch.int64, np.uint64)
            w_sector = torch.zeros(m * total, dtype=dt, device=dev)
            w_whole = torch.zeros(S * m, dtype=dt, device=dev)
            w_shards = torch.zeros(2 * nstripes, dtype=dt, device=dev)
            h = ctypes.c_void_p()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = L.isal_hip_batch_create(ctypes.byref(h), sector, 1, 1,
                                         one.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), nstripes,
                                         data.ctypes.data_as(u8pp), coding.ctypes.data_as(u8pp))
            create_ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise SystemExit(f"sector_crc_bench: isal_hip_batch_create of {nstripes} stripes failed ({rc})")

            def as_shards():
                if t32:
                    rc = L.isal_hip_batch_crc(h, INIT32, ctypes.c_void_p(w_shards.data_ptr()), None)
                else:
                    rc = L.isal_hip_batch_crc64(h, variant, INIT64, ctypes.c_void_p(w_shards.data_ptr()), None)
                return rc

            if t32:
                routes = [("sector", lambda: ragged.sector_crc(sector, INIT32, w_sector, 0)),
                          ("whole", lambda: ragged.crc(INIT32, w_whole, 0)), ("as_shards", as_shards)]
            else:
                routes = [("sector", lambda: ragged.sector_crc64(variant, sector, INIT64, w_sector, 0)),
                          ("whole", lambda: ragged.crc64(variant, INIT64, w_whole, 0)), ("as_shards", as_shards)]
            t0 = time.perf_counter()
            rc = as_shards()  # the first call allocates the partials
            torch.cuda.synchronize()
            first_call_ms = (time.perf_counter() - t0) * 1e3
            case = dict(common, checksum=name, sector=sector)
            if rc != 0:  # said, not hidden: the route then has no timing rows
                emit(dict(case, route="as_shards", failed=rc, create_ms=round(create_ms, 1), pointers=int(2 * nstripes)))
                routes = routes[:2]
            routes[0][1]()
            routes[1][1]()
            torch.cuda.synchronize()
            got = w_sector.cpu().numpy().view(npdt)
            other = w_shards.cpu().numpy().view(npdt)
            if rc == 0 and not np.array_equal(got[idx], other):
                pos = int(np.nonzero(got[idx] != other)[0][0])
                raise SystemExit(f"sector_crc_bench: {name} sector {sector}: word {int(idx[pos])}: sector "
                                 f"{int(got[idx[pos]]):#x}, as_shards {int(other[pos]):#x}")
            for t in range(args.sample):
                s = rng.randrange(S)
                j, ns = rng.randrange(m), -(-lens[s] // sector)
                i = ns - 1 if t % 2 else rng.randrange(ns)  # every other one a last sector
                n = min(sector, lens[s] - i * sector)
                at = shard_ptr[s][j] - base + i * sector
                host = sh.buf[at:at + n].cpu().numpy()
                want = isal_amd.crc32_iscsi(host, n, INIT32) if t32 else isal_amd.crc64(variant, INIT64, host, n)
                word = int(got[m * int(first[s]) + j * ns + i])
                if word != want:
                    raise SystemExit(f"sector_crc_bench: {name} sector {sector}: stripe {s} (len {lens[s]}) shard {j} "
                                     f"sector {i}: {word:#x}, host {want:#x}")
            launches = {}
            for rname, fn in routes:
                for _ in range(args.warmup):
                    fn()
                n0 = isal_amd.kernel_launches()
                fn()
                launches[rname] = isal_amd.kernel_launches() - n0
            torch.cuda.synchronize()
            nbytes = {"sector": m * sum(lens), "whole": m * sum(lens), "as_shards": 2 * nstripes * sector}
            nwords = {"sector": m * total, "whole": S * m, "as_shards": 2 * nstripes}
            if rc == 0:
                emit(dict(case, route="as_shards", create_ms=round(create_ms, 1), first_call_ms=round(first_call_ms, 1),
                          pointers=int(2 * nstripes), pointer_table_bytes=int(16 * nstripes)))
            ms_of = {rname: [] for rname, _ in routes}
            for rnd in range(args.rounds):
                lead = rnd % len(routes)
                for rname, fn in routes[lead:] + routes[:lead]:  # every route leads a round
                    ms = time_steps(torch, fn, args.steps)
                    ms_of[rname].append(ms)
                    emit(dict(case, route=rname, round=rnd, steps=args.steps, launches_per_step=launches[rname],
                              words=int(nwords[rname]), ms_per_step=round(ms, 5), bytes_per_step=int(nbytes[rname]),
                              GBps=round(nbytes[rname] / ms / 1e6, 1)))
            x = ms_of["sector"]
            for o, _ in routes[1:]:
                y = ms_of[o]
                emit(dict(case, summary=f"sector / {o}",
                          ratio_of_medians=round(statistics.median(x) / statistics.median(y), 4),
                          sector_ms_min_max=[round(min(x), 5), round(max(x), 5)],
                          other_ms_min_max=[round(min(y), 5), round(max(y), 5)]))
            L.isal_hip_batch_destroy(h)
            del w_sector, w_whole, w_shards
            torch.cuda.empty_cache()
    ragged.close()


if __name__ == "__main__":
    main()
