"""The checker of the T10 protection information tests: crc16_t10dif restated
from its polynomial (the oracle has no CRC-16), table-driven and vectorised
with numpy over sectors, and the tuples and verify words built from it. It
never sees the engine's output; tests/golden/crc16_t10dif_golden.json, recorded
from the reference's crc16_t10dif_base, anchors it (test_dif_cpu.py)."""
import json
import os
import struct

import numpy as np

POLY = 0x8BB7
GUARD, APP, REF = 1, 2, 4
CLEAN = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crc16_t10dif_golden.json")


def _table():
    t = np.zeros(256, np.uint32)
    for b in range(256):
        c = b << 8
        for _ in range(8):
            c = ((c << 1) ^ (POLY if c & 0x8000 else 0)) & 0xFFFF
        t[b] = c
    return t


TAB = _table()


def sector_guards(shards, S, seed):
    """crc16_t10dif(seed, .) of every S-byte sector (the last of a shard may
    be short) of every shard of the list, in order: a uint16 array."""
    rows, lens = [], []
    for sh in shards:
        n = len(sh)
        ns = -(-n // S)
        if ns:
            pad = np.zeros(ns * S, np.uint8)
            pad[:n] = sh
            rows.append(pad.reshape(ns, S))
            lens += [S] * (ns - 1) + [n - (ns - 1) * S]
    if not rows:
        return np.zeros(0, np.uint16)
    cols = np.ascontiguousarray(np.concatenate(rows).T)
    lens = np.array(lens)
    full = int(lens.min())
    crc = np.full(len(lens), seed & 0xFFFF, np.uint32)
    for c in range(int(lens.max())):
        nxt = ((crc << 8) & 0xFFFF) ^ TAB[(crc >> 8) ^ cols[c]]
        crc = nxt if c < full else np.where(c < lens, nxt, crc)
    return crc.astype(np.uint16)


def crc16(data, seed=0):
    return int(sector_guards([np.frombuffer(bytes(data), np.uint8)], max(1, len(data)), seed)[0]) if len(data) else seed


def golden_input(fill, n):
    """The inputs of the fixture (its driver's header, crc16_t10dif_golden.c)."""
    if fill != "lcg":
        return np.full(n, int(fill, 16), np.uint8)
    out, x = np.zeros(n, np.uint8), 12345
    for i in range(n):
        x = (1103515245 * x + 12345) & 0x7FFFFFFF
        out[i] = (x >> 16) & 0xFF
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def shards_of(st, image):
    """The shards of a test_ragged_gpu.Stripes case in the sector layout's
    order: stripe by stripe, shard by shard."""
    return [image[st.off[s][j]:st.off[s][j] + n] for s, n in enumerate(st.lens) for j in range(st.m)]


def sectors_per_shard(st, S):
    return [-(-n // S) for n in st.lens for _ in range(st.m)]


def ref_tags(st, S, type_, ref0):
    """The reference tag of every sector: ref0 of its shard (None: 0), plus
    the sector's index for type 1, modulo 2^32."""
    out = []
    for row, ns in enumerate(sectors_per_shard(st, S)):
        r0 = 0 if ref0 is None else int(ref0[row])
        out += [(r0 + (i if type_ == 1 else 0)) & 0xFFFFFFFF for i in range(ns)]
    return out


def tuples(guards, app, refs):
    """The 8-byte tuples: guard, application tag, reference tag, big-endian."""
    return np.frombuffer(b"".join(struct.pack(">HHI", int(g), app, r) for g, r in zip(guards, refs)), np.uint8).copy()


def verify_words(st, S, guards, app, refs, stored, type_, flags):
    """What dif_verify must leave in bad: per shard CLEAN or (i << 3) | kinds of
    the first failing sector, from the stored tuples and the escape rule."""
    out, at = [], 0
    for ns in sectors_per_shard(st, S):
        word = CLEAN
        for i in range(ns):
            g, a, r = struct.unpack(">HHI", bytes(stored[8 * (at + i):8 * (at + i) + 8]))
            if a == 0xFFFF and (type_ == 1 or r == 0xFFFFFFFF):
                continue
            kinds = (GUARD * (g != int(guards[at + i])) | APP * (a != app) | REF * (r != refs[at + i])) & flags
            if kinds:
                word = (i << 3) | kinds
                break
        out.append(word)
        at += ns
    return np.array(out, np.uint32)
