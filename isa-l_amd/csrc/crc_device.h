// crc_device.h — device-side building blocks shared by the checksum kernels:
// crc_kernels.hip (CRC32C), crc64_kernels.hip (the crc64_* flavours) and
// crc_sector_kernels.hip (both and the 16-bit T10 guard, per sector). One definition each of the chunk
// path of either width — field offsets, the conflict-free table lookups, the
// chunk and chain maps — and of what the kernels of both widths do alike: a
// block's tile range, the byte offsets of the fused kernels' byte tables, the
// fused kernels' load-group rule and the combine launches' grid. Included by
// exactly those translation units (and the probes that include them); as in
// ec_device.h everything lives in an anonymous namespace.
#pragma once
#include "ec_device.h"

namespace {

constexpr int kF = ISAL_HIP_CRC_FIELDS;

static_assert(ISAL_HIP_CRC_TILE == kTile, "CRC tile = encode tile");
static_assert(kF == 7, "field layouts below assume 7 fields per dword");

// One v_bfe_u32. (Through the builtin, LLVM sees that the low bits are zero,
// narrows the mask to a non-contiguous one and emits shift + and.)
template <int OFF, int WIDTH>
__device__ __forceinline__ uint32_t bfe(uint32_t x) {
  uint32_t r;
  asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "n"(OFF), "n"(WIDTH));
  return r;
}

// ---- CRC32C: 32-entry dword tables -----------------------------------------
// Byte offsets (entry index * 4) of the 7 fields of w, bits [0,5) [5,10)
// [10,15) [15,20) [20,25) [25,30) [30,32): 11 VALU ops for 7 lookups. Shifting
// w left by 2 puts every field at its entry's byte offset; masking the even
// and the odd fields into separate words leaves two zero bits below each
// field, so one bit-field extract yields the offset.
__device__ __forceinline__ void field_offsets4(uint32_t w, uint32_t (&o)[kF]) {
  const uint32_t s = w << 2;
  const uint32_t ev = s & 0x07C1F07Cu;  // fields 0, 2, 4 at [2,7) [12,17) [22,27)
  const uint32_t od = s & 0xF83E0F80u;  // fields 1, 3, 5 at [7,12) [17,22) [27,32)
  o[0] = ev & 0x7Cu;
  o[1] = bfe<5, 7>(od);
  o[2] = bfe<10, 7>(ev);
  o[3] = bfe<15, 7>(od);
  o[4] = bfe<20, 7>(ev);
  o[5] = bfe<25, 7>(od);
  o[6] = (w >> 28) & 0xCu;
}

// XOR of the 7 field lookups of w in the 7 consecutive 32-entry tables at t.
__device__ __forceinline__ uint32_t lookup7(const uint32_t* t, uint32_t w) {
  uint32_t o[kF];
  field_offsets4(w, o);
  const char* b = reinterpret_cast<const char*>(t);
  auto at = [&](int f) { return *reinterpret_cast<const uint32_t*>(b + f * 128 + o[f]); };
  return xor3(xor3(at(0), at(1), at(2)), xor3(at(3), at(4), at(5)), at(6));
}

// The chunk map whose 28 field tables start at t, applied to a 16-byte chunk:
// 28 conflict-free lookups.
__device__ __forceinline__ uint32_t chunk_map(const uint32_t* t, uint32_t w0, uint32_t w1,
                                              uint32_t w2, uint32_t w3) {
  constexpr int D = kF * 32;  // tables per dword of the chunk
  return xor3(lookup7(t, w0), lookup7(t + D, w1), lookup7(t + 2 * D, w2)) ^ lookup7(t + 3 * D, w3);
}

// ---- crc16: a 16-bit register through CRC32C's dword tables -------------------
// XOR of the 4 field lookups of the 16-bit w (bits [0,5) [5,10) [10,15)
// [15,16); the bits above are 0) in the 4 consecutive 32-entry tables at t:
// field_offsets4 without the three offsets a 16-bit value does not have.
__device__ __forceinline__ uint32_t lookup4(const uint32_t* t, uint32_t w) {
  const uint32_t s = w << 2;
  const uint32_t ev = s & 0x0001F07Cu;  // fields 0, 2 at [2,7) [12,17)
  const uint32_t od = s & 0x00020F80u;  // fields 1, 3 at [7,12) [17,18)
  const uint32_t o0 = ev & 0x7Cu, o1 = bfe<5, 7>(od), o2 = bfe<10, 7>(ev), o3 = bfe<15, 7>(od);
  const char* b = reinterpret_cast<const char*>(t);
  auto at = [&](int f, uint32_t o) { return *reinterpret_cast<const uint32_t*>(b + f * 128 + o); };
  return xor3(at(0, o0), at(1, o1), at(2, o2)) ^ at(3, o3);
}

// ---- crc64: 32-entry qword tables -------------------------------------------
// Byte offsets (entry index * 8) of the 7 fields of w. w << 3 puts fields 0-4
// at their entry offsets; the even and odd fields are masked into separate
// words so that one bit-field extract per field lands on zeros below it.
// Fields 5 and 6 would leave the dword after the shift and come from w directly.
__device__ __forceinline__ void field_offsets8(uint32_t w, uint32_t (&o)[kF]) {
  const uint32_t s = w << 3;
  const uint32_t ev = s & 0x0F83E0F8u;  // fields 0, 2, 4 at [3,8) [13,18) [23,28)
  const uint32_t od = s & 0x007C1F00u;  // fields 1, 3 at [8,13) [18,23)
  o[0] = ev & 0xF8u;
  o[1] = bfe<5, 8>(od);
  o[2] = bfe<10, 8>(ev);
  o[3] = bfe<15, 8>(od);
  o[4] = bfe<20, 8>(ev);
  o[5] = (w >> 22) & 0xF8u;
  o[6] = (w >> 27) & 0x18u;
}

// 64-bit XOR accumulator kept as two dwords so that every fold is one
// v_bitop3 (3-input XOR) per half: a lookup costs one XOR op instead of two
// (the compiler does not form bitop3 from 64-bit XOR chains by itself).
struct X64 {
  uint32_t lo, hi;
  __device__ __forceinline__ void add2(uint64_t x, uint64_t y) {
    lo = xor3(lo, static_cast<uint32_t>(x), static_cast<uint32_t>(y));
    hi = xor3(hi, static_cast<uint32_t>(x >> 32), static_cast<uint32_t>(y >> 32));
  }
  __device__ __forceinline__ uint64_t get() const { return (static_cast<uint64_t>(hi) << 32) | lo; }
};

// Entry of field f of table set t at byte offset o (field tables are 256 B apart).
__device__ __forceinline__ uint64_t tab_at(const uint64_t* t, int f, uint32_t o) {
  return *reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(t) + f * 256 + o);
}

// acc ^= the 14 field lookups of the two dwords (w0, w1) in the 14 consecutive
// 32-entry tables at t: seven 3-input XORs per half.
__device__ __forceinline__ void lookup14(X64& acc, const uint64_t* t, uint32_t w0, uint32_t w1) {
  uint32_t o[kF], q[kF];
  field_offsets8(w0, o);
  field_offsets8(w1, q);
  const uint64_t* u = t + kF * 32;
  acc.add2(tab_at(t, 0, o[0]), tab_at(t, 1, o[1]));
  acc.add2(tab_at(t, 2, o[2]), tab_at(t, 3, o[3]));
  acc.add2(tab_at(t, 4, o[4]), tab_at(t, 5, o[5]));
  acc.add2(tab_at(t, 6, o[6]), tab_at(u, 0, q[0]));
  acc.add2(tab_at(u, 1, q[1]), tab_at(u, 2, q[2]));
  acc.add2(tab_at(u, 3, q[3]), tab_at(u, 4, q[4]));
  acc.add2(tab_at(u, 5, q[5]), tab_at(u, 6, q[6]));
}

// M(v) for a map stored as 14 field tables.
__device__ __forceinline__ uint64_t apply_op(const uint64_t* op, uint64_t v) {
  X64 a{0u, 0u};
  lookup14(a, op, static_cast<uint32_t>(v), static_cast<uint32_t>(v >> 32));
  return a.get();
}

// acc ^= raw(0, 16-byte chunk) through the chunk map at t, dwords little-endian.
__device__ __forceinline__ void chunk_acc(X64& acc, const uint64_t* t, uint32_t w0, uint32_t w1,
                                          uint32_t w2, uint32_t w3) {
  constexpr int D = kF * 32;
  lookup14(acc, t, w0, w1);
  lookup14(acc, t + 2 * D, w2, w3);
}

// ---- both widths -------------------------------------------------------------
__device__ __forceinline__ uint32_t le32(const uint8_t* p) {
  return p[0] | (p[1] << 8) | (p[2] << 16) | (static_cast<uint32_t>(p[3]) << 24);
}

// Bytes of the 16-byte lane chunk at off that lie below len: 16, or fewer for
// the lane that straddles len, or 0 past it.
__device__ __forceinline__ int lane_bytes(int len, long long off) {
  const long long left = len - off;
  return left >= kVec ? kVec : (left > 0 ? static_cast<int>(left) : 0);
}

// Block blk of tt tiles of a shard's n tiles: tiles [t0, t1).
__device__ __forceinline__ void block_tiles(unsigned blk, unsigned tt, unsigned n, unsigned& t0, unsigned& t1) {
  t0 = blk * tt;
  t1 = t0 + tt < n ? t0 + tt : n;
}

// Byte b of w times 1 << SH (the offset of a 4- or 8-byte entry of the fused
// kernels' 256-entry byte tables) in one VALU op: an SDWA shift with a byte select.
template <int SH>
__device__ __forceinline__ void byte_offs(uint32_t w, uint32_t (&o)[4]) {
  const uint32_t sh = SH;
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
      : "=v"(o[0]) : "v"(sh), "v"(w));
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1"
      : "=v"(o[1]) : "v"(sh), "v"(w));
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2"
      : "=v"(o[2]) : "v"(sh), "v"(w));
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3"
      : "=v"(o[3]) : "v"(sh), "v"(w));
}

// Sources per load group of the fused encode+CRC kernels: the largest
// candidate dividing k, else 4.
inline int fused_group(int k) {
  static const int cand[] = {12, 10, 8, 6, 5, 4};
  for (int u : cand)
    if (k >= u && k % u == 0) return u;
  return 4;
}

// Stripes per launch (for_slices) so that its work items, per_stripe of them
// each, stay within kMaxItems.
inline unsigned crc_stripes_per_launch(unsigned long long per_stripe) {
  return kMaxItems / per_stripe > 0 ? static_cast<unsigned>(kMaxItems / per_stripe) : 1u;
}

// Grid of a combine launch: one wave per shard, four shards per workgroup at
// a time, at most cap workgroups (what stays resident with the tables each
// copies into LDS once).
inline unsigned combine_grid(unsigned long long nshards, unsigned cap) {
  const unsigned long long want = (nshards + 3) / 4;
  return want < cap ? static_cast<unsigned>(want) : cap;
}

}  // namespace
