// What the matrix-core attention kernels share (attn_mfma.hip: forward; attn_mfma_bwd.hip: backward,
// §15; attn_mfma_f32.hip: float32 forward, §16; attn_mfma_f32_bwd.hip: float32 backward, §17): the tile constants, the vector types, the v_mfma_f32_16x16x32 and
// 16x16x4 wrappers, pack2 and the gates.
#pragma once
#include "attn_desc.hpp"

namespace pdt {

constexpr int kMfmaThreads = 256;
constexpr int kMfmaWaveRows = 16;
constexpr int kMfmaRows = 64;    // rows per workgroup
constexpr int kMfmaFrames = 64;  // frames per key block
constexpr int kMfmaPad = 8;      // halves of padding per LDS row
constexpr int kMfmaVtPitch = kMfmaFrames + kMfmaPad;
constexpr int kMfmaMinD = 32, kMfmaMaxD = 128;
constexpr int64_t kMfmaMinRows = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma_16x16x32(f16_t, u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_16x16x32(bf16_t, u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}

// v_mfma_f32_16x16x4_f32 (attn_mfma_f32.hip, §16): lane l gives A[l % 16][l / 16] and B[l / 16][l % 16], products and
// sums in float32; the accumulator layout is that of the 16x16x32 forms
__device__ __forceinline__ f32x4 mfma_16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// two float32 rounded to E (nearest even, elem_store's conversion), packed low element first
template <typename E> __device__ __forceinline__ unsigned pack2(float lo, float hi) {
  E e[2];
  elem_store(&e[0], lo);
  elem_store(&e[1], hi);
  return (unsigned)__builtin_bit_cast(unsigned short, e[0]) | ((unsigned)__builtin_bit_cast(unsigned short, e[1]) << 16);
}

// The gate of the forward: half elements, groups of 64 rows or more, head dims of whole 16-column tiles, 16-byte
// loads of query, key and value rows and 8-byte stores of out rows.
static inline bool attn_mfma_gate(const AttnDesc &d, int elem) {
  if (elem != 2 && elem != 3) return false;
  if (d.R == 0 || d.T < 1 || d.M < kMfmaMinRows) return false;
  if (d.D < kMfmaMinD || d.D > kMfmaMaxD || d.D % 16 || d.Dv < kMfmaMinD || d.Dv > kMfmaMaxD || d.Dv % 16) return false;
  if (d.fs[SQ] != 1 || d.fs[SK] != 1 || d.fs[SV] != 1 || d.fs[SO] != 1) return false;
  if (d.ts[SQ] % 8 || d.ts[SK] % 8 || d.ts[SV] % 8) return false;
  for (int i = 0; i < d.nd; ++i)
    if (d.st[SQ][i] % 8 || d.st[SK][i] % 8 || d.st[SV][i] % 8 || d.st[SO][i] % 4) return false;
  return true;
}

// The gate of the float32 forward (attn_mfma_f32.hip): the same rows and head dims; 16-byte loads of query, key and
// value rows and 16-byte stores of out rows are four elements here.
static inline bool attn_mfma_f32_gate(const AttnDesc &d) {
  if (d.R == 0 || d.T < 1 || d.M < kMfmaMinRows) return false;
  if (d.D < kMfmaMinD || d.D > kMfmaMaxD || d.D % 16 || d.Dv < kMfmaMinD || d.Dv > kMfmaMaxD || d.Dv % 16) return false;
  if (d.fs[SQ] != 1 || d.fs[SK] != 1 || d.fs[SV] != 1 || d.fs[SO] != 1) return false;
  if (d.ts[SQ] % 4 || d.ts[SK] % 4 || d.ts[SV] % 4) return false;
  for (int i = 0; i < d.nd; ++i)
    if (d.st[SQ][i] % 4 || d.st[SK][i] % 4 || d.st[SV][i] % 4 || d.st[SO][i] % 4) return false;
  return true;
}

// The decode kernels (attn_mfma_dec.hip: forward, §18; attn_mfma_dec_bwd.hip: backward, §19)
constexpr int kDecRows = 16;             // the tile's columns: rows of a group, padded
constexpr int kDecMinD = 64, kDecMaxD = 512;
constexpr int64_t kDecFill = 512;        // workgroups wanted before T is split: two per CU
constexpr int kDecQPad = 4;              // floats of padding per query (grad_out) row in LDS
constexpr int kDecPPitch = 20;           // floats per frame of the P (dS) tile
constexpr int kDecPFloats = kMfmaFrames * kDecPPitch;

// The gate of the decode forward: 1 to 16 rows a group, head dims of whole 16-column chunks in [64, 512], 16-byte loads
// of query, key and value rows and 16-byte stores of out rows (four elements each).
static inline bool attn_mfma_dec_gate(const AttnDesc &d) {
  if (d.R == 0 || d.T < 1 || d.M < 1 || d.M > kDecRows) return false;
  if (d.D < kDecMinD || d.D > kDecMaxD || d.D % 16 || d.Dv < kDecMinD || d.Dv > kDecMaxD || d.Dv % 16) return false;
  if (d.fs[SQ] != 1 || d.fs[SK] != 1 || d.fs[SV] != 1 || d.fs[SO] != 1) return false;
  if (d.ts[SQ] % 4 || d.ts[SK] % 4 || d.ts[SV] % 4) return false;
  for (int i = 0; i < d.nd; ++i)
    if (d.st[SQ][i] % 4 || d.st[SK][i] % 4 || d.st[SV][i] % 4 || d.st[SO][i] % 4) return false;
  return true;
}

}  // namespace pdt
