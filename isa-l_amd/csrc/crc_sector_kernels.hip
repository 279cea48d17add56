// crc_sector_kernels.hip — sector checksums (isal_hip.h isal_hip_batch_sector_crc,
// isal_hip_ragged_sector_crc and their crc64 forms): the CRC32C or any crc64_*
// flavour of every 512 B .. 4 KiB sector of every shard, in ONE launch and with
// no partials in global memory — a sector never leaves a 4 KiB tile.
//
// A workgroup takes (shard, 4 KiB tile) work items, grid-stride, with the
// tables loaded into LDS once per workgroup. With m = sector / 16 lanes per
// sector, lane L serves sector L / m of the tile at position p = L % m:
//  * the sector's q = n / 16 whole chunks (n = its byte count: the sector size,
//    less for the shard's last sector) are RIGHT-aligned over the m positions —
//    position p holds chunk p - (m - q) — so the last whole chunk always sits at
//    position m - 1 and the positions before the first hold 0, which a raw CRC
//    from register 0 ignores. A full sector is the coalesced layout of the
//    whole-shard kernels (lane L reads bytes [16L, 16L + 16) of the tile);
//  * the start register (init, or ~init for crc64) is XORed into the first
//    bytes of chunk 0 as a CRC register is, so raw(0, .) of the chunks joined
//    is raw(start, whole chunks) with no Z^n(init) term;
//  * lane value h = raw(0, chunk) by the conflict-free 5-bit field tables
//    (crc_host.c / crc64_host.c; the layout and the lookups, crc_device.h, of
//    the whole-shard kernels);
//  * log-step join, crc(A || B) = Z^|B|(crc A) ^ crc B: step d maps h through
//    Z^(16 * 2^d) and XORs the value 2^d lanes up; after log2(min(m, 64))
//    steps position 0 of each sector (or of each wave) holds its bytes' CRC;
//    sectors of 2 or 4 KiB then take the waves' values through LDS (one
//    barrier per tile, two alternating slots) with Z^1024 per wave;
//  * the lane at position 0 runs the last n % 16 bytes through the flavour's
//    bit-serial byte step (the one place that knows the bit order) and stores
//    the word. A sector shorter than 16 bytes starts that loop at the start
//    register itself.
// Tables in LDS: the chunk map and Z^16 .. Z^1024, 9.6 KiB (CRC32C) / 31.5 KiB
// (crc64); they depend on the flavour alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc_device.h"

namespace {

static_assert(kBlock == 256, "four waves of 64 lanes per tile");

// ---- what the one kernel body needs of a checksum family -------------------
// The table lookups are crc_device.h's, shared with the whole-shard kernels:
// lookup7 / chunk_map on CRC32C's dword tables, apply_op / chunk_acc on crc64's
// qword tables.
// start: the register a sector starts from (init; ~init for crc64). poly and
// refl: the byte step's polynomial (x^N implicit, in the register's bit order)
// and direction.
struct Crc32c {
  using reg = uint32_t;
  static constexpr int kImage = ISAL_HIP_SECTOR32_DWORDS, kChunk = ISAL_HIP_CRC_CHUNK_DWORDS, kOp = kF * 32;
  static __device__ __forceinline__ void inject(uint4& x, reg start, int) { x.x ^= start; }
  static __device__ __forceinline__ reg chunk(const reg* lt, const uint4& x) {
    return chunk_map(lt, x.x, x.y, x.z, x.w);
  }
  static __device__ __forceinline__ reg zmap(const reg* lt, int d, reg h) { return lookup7(lt + kChunk + d * kOp, h); }
  static __device__ __forceinline__ reg up(reg h, unsigned by) { return __shfl_down(h, by, 64); }
  static __device__ __forceinline__ reg byte(reg s, uint8_t b, reg poly, int) {
    s ^= b;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = (s >> 1) ^ ((s & 1u) ? poly : 0u);
    return s;
  }
  static __device__ __forceinline__ reg fin(reg s) { return s; }
};

struct Crc64 {
  using reg = uint64_t;
  static constexpr int kImage = ISAL_HIP_SECTOR64_ENTRIES, kChunk = ISAL_HIP_CRC64_CHUNK_ENTRIES,
                       kOp = ISAL_HIP_CRC64_OP_ENTRIES;
  // a refl register meets the data's first byte at its low byte, a norm one at
  // its high byte: as a little-endian word of 8 data bytes, start or its byte swap
  static __device__ __forceinline__ void inject(uint4& x, reg start, int refl) {
    const reg u = refl ? start : __builtin_bswap64(start);
    x.x ^= static_cast<uint32_t>(u);
    x.y ^= static_cast<uint32_t>(u >> 32);
  }
  static __device__ __forceinline__ reg chunk(const reg* lt, const uint4& x) {
    X64 a{0u, 0u};
    chunk_acc(a, lt, x.x, x.y, x.z, x.w);
    return a.get();
  }
  static __device__ __forceinline__ reg zmap(const reg* lt, int d, reg h) { return apply_op(lt + kChunk + d * kOp, h); }
  static __device__ __forceinline__ reg up(reg h, unsigned by) {
    const uint32_t lo = __shfl_down(static_cast<uint32_t>(h), by, 64);
    const uint32_t hi = __shfl_down(static_cast<uint32_t>(h >> 32), by, 64);
    return (static_cast<uint64_t>(hi) << 32) | lo;
  }
  static __device__ __forceinline__ reg byte(reg s, uint8_t b, reg poly, int refl) {
    if (refl) {
      s ^= b;
#pragma unroll
      for (int j = 0; j < 8; ++j) s = (s >> 1) ^ ((s & 1u) ? poly : 0ull);
    } else {
      s ^= static_cast<uint64_t>(b) << 56;
#pragma unroll
      for (int j = 0; j < 8; ++j) s = (s << 1) ^ ((s >> 63) ? poly : 0ull);
    }
    return s;
  }
  static __device__ __forceinline__ reg fin(reg s) { return ~s; }
};

template <class R>
struct SectorArgs {
  const uint64_t* ptrs;             // rows of nsh shard addresses
  const int* lens;                  // ragged: per stripe
  const unsigned* items;            // ragged: {stripe, tile} rows
  const unsigned long long* first;  // ragged: sectors of one shard of the stripes before s
  const R* image;
  R* out;
  R start, poly;
  unsigned nwork, nsh, ntiles;  // ntiles, len: uniform
  int len, refl;
};

// RAG: work item w is (row w / nsh of the item table, shard w % nsh) with the
// stripe's own length; else (shard w / ntiles, tile w % ntiles) of one length.
// LM: log2 of the lanes per sector, 5 (512 B) .. 8 (4 KiB).
template <class C, bool RAG, int LM>
__global__ __launch_bounds__(kBlock) void crc_sectors(const SectorArgs<typename C::reg> a) {
  using R = typename C::reg;
  constexpr int M = 1 << LM, S = M * kVec, SPT = kTile / S, kWaves = kBlock / 64;
  constexpr int kSteps = LM < 6 ? LM : 6;  // joins inside a wave
  __shared__ R lt[C::kImage];
  __shared__ R xw[2][kWaves];
  {
    static_assert(C::kImage * sizeof(R) % 16 == 0, "tables are copied 16 bytes at a time");
    const uint4* src = reinterpret_cast<const uint4*>(a.image);
    uint4* dst = reinterpret_cast<uint4*>(lt);
    for (unsigned i = threadIdx.x; i < C::kImage * sizeof(R) / 16; i += kBlock) dst[i] = src[i];
  }
  __syncthreads();
  const unsigned L = threadIdx.x, sec = L >> LM, p = L & (M - 1);
  unsigned it = 0;
  for (unsigned w = blockIdx.x; w < a.nwork; w += gridDim.x, ++it) {
    uint64_t base;
    size_t out0;  // word of the shard's sector 0
    unsigned tile;
    int len;
    if constexpr (RAG) {
      const unsigned item = w / a.nsh, j = w - item * a.nsh;
      const unsigned stripe = a.items[2 * static_cast<size_t>(item)];
      tile = a.items[2 * static_cast<size_t>(item) + 1];
      len = a.lens[stripe];
      base = a.ptrs[static_cast<size_t>(stripe) * a.nsh + j];
      const size_t ns = (static_cast<size_t>(len) + S - 1) / S;
      out0 = static_cast<size_t>(a.first[stripe]) * a.nsh + j * ns;
    } else {
      const unsigned si = w / a.ntiles;
      tile = w - si * a.ntiles;
      len = a.len;
      base = a.ptrs[si];
      out0 = static_cast<size_t>(si) * ((static_cast<size_t>(len) + S - 1) / S);
    }
    const long long soff = static_cast<long long>(tile) * kTile + sec * S;  // the sector's first byte
    const long long left = len - soff;
    const int n = left >= S ? S : (left > 0 ? static_cast<int>(left) : 0);  // its bytes (0: no such sector)
    const int q = n / kVec;
    const int c = static_cast<int>(p) - (M - q);  // this position's chunk of the sector
    R h = 0;
    if (c >= 0) {
      uint4 x = load16<kBufNT>(base, soff + c * kVec, len);
      if (c == 0) C::inject(x, a.start, a.refl);
      h = C::chunk(lt, x);
    }
#pragma unroll
    for (int d = 0; d < kSteps; ++d) h = C::zmap(lt, d, h) ^ C::up(h, 1u << d);
    if constexpr (LM > 6) {  // the sector spans M / 64 waves
      if ((L & 63) == 0) xw[it & 1][L >> 6] = h;
      __syncthreads();
      if (p == 0) {
#pragma unroll
        for (int i = 1; i < M / 64; ++i) h = C::zmap(lt, 6, h) ^ xw[it & 1][(L >> 6) + i];
      }
    }
    if (p == 0 && n > 0) {
      R s = q ? h : a.start;
      const uint8_t* b = reinterpret_cast<const uint8_t*>(base) + soff + q * kVec;
      for (int i = 0; i < n % kVec; ++i) s = C::byte(s, b[i], a.poly, a.refl);
      a.out[out0 + static_cast<size_t>(tile) * SPT + sec] = C::fin(s);
    }
  }
}

// Workgroups stay resident and stride over the items, so the tables are loaded
// once per workgroup, not per tile: 8 (CRC32C) / 5 (crc64, by its LDS) per CU
// of the 256.
constexpr unsigned kCUs = 256;

template <class C, bool RAG>
int launch_lm(int lm, unsigned grid, hipStream_t s, const SectorArgs<typename C::reg>& a) {
  switch (lm) {
    case 5: ISAL_LAUNCH((crc_sectors<C, RAG, 5>), dim3(grid), dim3(kBlock), 0, s, a); break;
    case 6: ISAL_LAUNCH((crc_sectors<C, RAG, 6>), dim3(grid), dim3(kBlock), 0, s, a); break;
    case 7: ISAL_LAUNCH((crc_sectors<C, RAG, 7>), dim3(grid), dim3(kBlock), 0, s, a); break;
    case 8: ISAL_LAUNCH((crc_sectors<C, RAG, 8>), dim3(grid), dim3(kBlock), 0, s, a); break;
    default: return static_cast<int>(hipErrorInvalidValue);
  }
  isal_hip_count_launch();
  return static_cast<int>(hipGetLastError());
}

template <class C>
int launch(const isal_hip_sector_geom* g, const typename C::reg* image, typename C::reg start,
           typename C::reg poly, int refl, typename C::reg* out, unsigned per_cu, void* stream) {
  int lm = 0;
  while ((kVec << lm) < g->sector) ++lm;
  if ((kVec << lm) != g->sector || g->nwork == 0 || g->nwork > ISAL_HIP_RAGGED_MAX_ITEMS)
    return static_cast<int>(hipErrorInvalidValue);
  SectorArgs<typename C::reg> a{};
  a.ptrs = g->d_ptrs;
  a.lens = g->d_lens;
  a.items = g->d_items;
  a.first = g->d_first;
  a.image = image;
  a.out = out;
  a.start = start;
  a.poly = poly;
  a.nwork = static_cast<unsigned>(g->nwork);
  a.nsh = static_cast<unsigned>(g->nsh);
  a.ntiles = g->ntiles;
  a.len = g->len;
  a.refl = refl;
  const unsigned cap = kCUs * per_cu, grid = a.nwork < cap ? a.nwork : cap;
  return g->d_items ? launch_lm<C, true>(lm, grid, static_cast<hipStream_t>(stream), a)
                    : launch_lm<C, false>(lm, grid, static_cast<hipStream_t>(stream), a);
}

}  // namespace

extern "C" int isal_hip_launch_sector_crc32c(const isal_hip_sector_geom* g, const uint32_t* d_image,
                                             unsigned int init, uint32_t* out, void* stream) {
  return launch<Crc32c>(g, d_image, init, 0x82F63B78u, 1, out, 8, stream);
}

extern "C" int isal_hip_launch_sector_crc64(const isal_hip_sector_geom* g, const uint64_t* d_image, int refl,
                                            uint64_t poly, uint64_t init, uint64_t* out, void* stream) {
  return launch<Crc64>(g, d_image, ~init, poly, refl, out, 5, stream);
}
