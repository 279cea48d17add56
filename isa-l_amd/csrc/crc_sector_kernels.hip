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
//
// A third family, the 16-bit T10 guard crc16_t10dif (7 KiB of tables), runs the
// same body for T10 protection information (isal_hip.h isal_hip_*_sector_t10dif,
// _dif_generate, _dif_verify; isal_hip_dif.c). What the lane at position 0 does
// with its word is an output policy: store it (every family), store the 8-byte
// tuple of guard and tags, or compare with a stored tuple and leave the first
// failing sector of each shard in a per-shard word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc_device.h"
#include "isal_hip.h"

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

// The T10 guard, crc16_t10dif: a normal 16-bit register in the low half of a
// dword, so the chunk map is CRC32C's (lookup7 / chunk_map on another image)
// and a join maps 4 fields, lookup4, where CRC32C maps 7.
struct Crc16T10 {
  using reg = uint32_t;
  static constexpr int kImage = ISAL_HIP_SECTOR16_DWORDS, kChunk = ISAL_HIP_CRC_CHUNK_DWORDS,
                       kOp = ISAL_HIP_CRC16_OP_DWORDS;
  // a norm register meets the data's first byte at its high byte
  static __device__ __forceinline__ void inject(uint4& x, reg start, int) {
    x.x ^= ((start & 0xffu) << 8) | (start >> 8);
  }
  static __device__ __forceinline__ reg chunk(const reg* lt, const uint4& x) {
    return chunk_map(lt, x.x, x.y, x.z, x.w);
  }
  static __device__ __forceinline__ reg zmap(const reg* lt, int d, reg h) { return lookup4(lt + kChunk + d * kOp, h); }
  static __device__ __forceinline__ reg up(reg h, unsigned by) { return __shfl_down(h, by, 64); }
  static __device__ __forceinline__ reg byte(reg s, uint8_t b, reg poly, int) {
    s ^= static_cast<reg>(b) << 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = (s << 1) ^ ((s & 0x8000u) ? poly : 0u);
    return s & 0xffffu;
  }
  static __device__ __forceinline__ reg fin(reg s) { return s; }
};

// ---- what the lane at position 0 does with its sector's word -----------------
// put(n, w, i, v): v is the word of sector i of shard n (row n of the pointer
// table: s*m + j), word w of the sector layout.
template <class R>
struct PutWord {
  R* out;
  __device__ __forceinline__ void put(size_t, size_t w, unsigned, R v) const { out[w] = v; }
};

struct PutGuard {
  uint16_t* out;
  __device__ __forceinline__ void put(size_t, size_t w, unsigned, uint32_t v) const {
    out[w] = static_cast<uint16_t>(v);
  }
};

__device__ __forceinline__ uint32_t swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }

// The 8-byte tuple of a sector as the two little-endian dwords of one 8-byte
// access: guard, application tag, reference tag, each most significant byte first.
struct DifTags {
  const unsigned* ref0;  // per shard; NULL: 0
  unsigned app;
  int type;
  __device__ __forceinline__ uint2 tuple(size_t n, unsigned i, uint32_t guard) const {
    const unsigned r0 = ref0 ? ref0[n] : 0u;
    return make_uint2(swap16(guard) | (swap16(app) << 16),
                      __builtin_bswap32(type == ISAL_HIP_DIF_TYPE1 ? r0 + i : r0));
  }
};

struct PutTuple {
  uint2* pi;
  DifTags t;
  __device__ __forceinline__ void put(size_t n, size_t w, unsigned i, uint32_t v) const { pi[w] = t.tuple(n, i, v); }
};

// Compares under flags (ISAL_HIP_DIF_CHECK_*) unless the stored tags say "not
// checked"; a failing sector leaves the least i << 3 | kinds in bad[n].
struct CheckTuple {
  const uint2* pi;
  unsigned* bad;
  DifTags t;
  unsigned flags;
  __device__ __forceinline__ void put(size_t n, size_t w, unsigned i, uint32_t v) const {
    const uint2 got = pi[w];
    const bool escape = (got.x >> 16) == 0xffffu && (t.type == ISAL_HIP_DIF_TYPE1 || got.y == 0xffffffffu);
    if (escape) return;
    const uint2 want = t.tuple(n, i, v);
    const unsigned dx = got.x ^ want.x;
    const unsigned kinds = ((dx & 0xffffu) ? ISAL_HIP_DIF_CHECK_GUARD : 0u) | ((dx >> 16) ? ISAL_HIP_DIF_CHECK_APP : 0u) |
                           (got.y != want.y ? ISAL_HIP_DIF_CHECK_REF : 0u);
    if (kinds & flags) atomicMin(bad + n, (i << 3) | (kinds & flags));
  }
};

template <class R, class O>
struct SectorArgs {
  const uint64_t* ptrs;             // rows of nsh shard addresses
  const int* lens;                  // ragged: per stripe
  const unsigned* items;            // ragged: {stripe, tile} rows
  const unsigned long long* first;  // ragged: sectors of one shard of the stripes before s
  const R* image;
  O out;
  R start, poly;
  unsigned nwork, nsh, ntiles;  // ntiles, len: uniform
  int len, refl;
};

// RAG: work item w is (row w / nsh of the item table, shard w % nsh) with the
// stripe's own length; else (shard w / ntiles, tile w % ntiles) of one length.
// LM: log2 of the lanes per sector, 5 (512 B) .. 8 (4 KiB). O: the output
// policy above.
template <class C, class O, bool RAG, int LM>
__global__ __launch_bounds__(kBlock) void crc_sectors(const SectorArgs<typename C::reg, O> a) {
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
    size_t out0, row;  // word of the shard's sector 0; the shard's row of the pointer table
    unsigned tile;
    int len;
    if constexpr (RAG) {
      const unsigned item = w / a.nsh, j = w - item * a.nsh;
      const unsigned stripe = a.items[2 * static_cast<size_t>(item)];
      tile = a.items[2 * static_cast<size_t>(item) + 1];
      len = a.lens[stripe];
      row = static_cast<size_t>(stripe) * a.nsh + j;
      base = a.ptrs[row];
      const size_t ns = (static_cast<size_t>(len) + S - 1) / S;
      out0 = static_cast<size_t>(a.first[stripe]) * a.nsh + j * ns;
    } else {
      const unsigned si = w / a.ntiles;
      tile = w - si * a.ntiles;
      len = a.len;
      row = si;
      base = a.ptrs[row];
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
      const unsigned i = tile * SPT + sec;  // the sector of the shard
      a.out.put(row, out0 + i, i, C::fin(s));
    }
  }
}

// Workgroups stay resident and stride over the items, so the tables are loaded
// once per workgroup, not per tile: 8 (CRC32C) / 5 (crc64, by its LDS) per CU
// of the 256.
constexpr unsigned kCUs = 256;

template <class C, bool RAG, class O>
int launch_lm(int lm, unsigned grid, hipStream_t s, const SectorArgs<typename C::reg, O>& a) {
  switch (lm) {
    case 5: ISAL_LAUNCH((crc_sectors<C, O, RAG, 5>), dim3(grid), dim3(kBlock), 0, s, a); break;
    case 6: ISAL_LAUNCH((crc_sectors<C, O, RAG, 6>), dim3(grid), dim3(kBlock), 0, s, a); break;
    case 7: ISAL_LAUNCH((crc_sectors<C, O, RAG, 7>), dim3(grid), dim3(kBlock), 0, s, a); break;
    case 8: ISAL_LAUNCH((crc_sectors<C, O, RAG, 8>), dim3(grid), dim3(kBlock), 0, s, a); break;
    default: return static_cast<int>(hipErrorInvalidValue);
  }
  isal_hip_count_launch();
  return static_cast<int>(hipGetLastError());
}

template <class C, class O>
int launch(const isal_hip_sector_geom* g, const typename C::reg* image, typename C::reg start,
           typename C::reg poly, int refl, const O& out, unsigned per_cu, void* stream) {
  int lm = 0;
  while ((kVec << lm) < g->sector) ++lm;
  if ((kVec << lm) != g->sector || g->nwork == 0 || g->nwork > ISAL_HIP_RAGGED_MAX_ITEMS)
    return static_cast<int>(hipErrorInvalidValue);
  SectorArgs<typename C::reg, O> a{};
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
  return launch<Crc32c>(g, d_image, init, 0x82F63B78u, 1, PutWord<uint32_t>{out}, 8, stream);
}

extern "C" int isal_hip_launch_sector_crc64(const isal_hip_sector_geom* g, const uint64_t* d_image, int refl,
                                            uint64_t poly, uint64_t init, uint64_t* out, void* stream) {
  return launch<Crc64>(g, d_image, ~init, poly, refl, PutWord<uint64_t>{out}, 5, stream);
}

extern "C" int isal_hip_launch_sector_t10dif(const isal_hip_sector_geom* g, const uint32_t* d_image,
                                             const isal_hip_dif_args* d, void* stream) {
  const uint32_t seed = d->seed & 0xffffu;
  const DifTags t{d->ref0, d->app & 0xffffu, d->type};
  switch (d->mode) {
    case ISAL_HIP_DIF_GUARD:
      return launch<Crc16T10>(g, d_image, seed, ISAL_HIP_CRC16_POLY, 0, PutGuard{d->crc}, 8, stream);
    case ISAL_HIP_DIF_GENERATE:
      return launch<Crc16T10>(g, d_image, seed, ISAL_HIP_CRC16_POLY, 0, PutTuple{reinterpret_cast<uint2*>(d->pi), t}, 8,
                              stream);
    case ISAL_HIP_DIF_VERIFY:
      return launch<Crc16T10>(g, d_image, seed, ISAL_HIP_CRC16_POLY, 0,
                              CheckTuple{reinterpret_cast<const uint2*>(d->pi), d->bad, t, d->flags}, 8, stream);
    default: return static_cast<int>(hipErrorInvalidValue);
  }
}
