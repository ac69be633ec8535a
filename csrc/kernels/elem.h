// What the row kernels (permute.hip, collate.hip, augment.hip) share: the workgroup size, the 32-bit index
// decompositions, the element codec -- every load, store and conversion of the element types they convert -- and
// the host dispatch from a DType code to the element's storage type.
#pragma once

#include <type_traits>

#include "common.h"

namespace ddl {

constexpr int kThreads = 256;

// a / b for non-negative a < bound: 32-bit unsigned division when the bound fits (a short
// v_rcp_iflag sequence), the 64-bit expansion otherwise. `bound` is a kernel argument, so the
// branch is wave-uniform.
__device__ __forceinline__ int64_t div_small(int64_t a, int64_t b, int64_t bound) {
  if (bound <= static_cast<int64_t>(UINT32_MAX)) return static_cast<uint32_t>(a) / static_cast<uint32_t>(b);
  return a / b;
}

// Tile number -> (row, chunk of the row) for tile < 2^32 (host-checked): 32-bit division, not the 64-bit expansion.
struct RowChunk {
  int64_t row, chunk;
};
__device__ __forceinline__ RowChunk row_chunk(int64_t tile, int64_t chunks_per_row) {
  const uint32_t row = static_cast<uint32_t>(tile) / static_cast<uint32_t>(chunks_per_row);
  return {row, static_cast<uint32_t>(tile) - row * static_cast<uint32_t>(chunks_per_row)};
}

// bf16 helpers: the plain cast lowers to v_cvt_pk_bf16_f32 (RNE, NaN-safe) at
// -O3 on gfx950 (MI355X_MICROARCH "Correctness boundaries").
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
  __bf16 b = static_cast<__bf16>(f);
  return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ float bf16_bits_to_f32(uint16_t u) {
  return __builtin_bit_cast(float, static_cast<uint32_t>(u) << 16);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  return static_cast<uint32_t>(f32_to_bf16_bits(lo)) | (static_cast<uint32_t>(f32_to_bf16_bits(hi)) << 16);
}

// Storage types of the converted elements: uint8_t, float and these 2-byte tags (sizeof must equal the element
// size for pointer math). Elem<T>: load1 / load8 read 1 / 8 consecutive elements as float (load8: from a 16 B
// aligned address, 8 B for uint8), store1 / store<N> write 1 / N = 2, 4 or 8 floats to an address aligned to the
// N elements (f32: at most 16 B). uint8 is never an output: Elem<uint8_t> has no store.
struct BF16Tag { uint16_t bits; };
struct F16Tag { uint16_t bits; };
static_assert(sizeof(BF16Tag) == 2 && sizeof(F16Tag) == 2, "tag size");

// 8 uint8 held in two registers (lo: elements 0 .. 3) -> float
__device__ __forceinline__ void unpack_u8x8(uint32_t lo, uint32_t hi, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = static_cast<float>((lo >> (8 * i)) & 0xffu);
#pragma unroll
  for (int i = 0; i < 4; ++i) f[4 + i] = static_cast<float>((hi >> (8 * i)) & 0xffu);
}

template <typename T>
struct Elem;
template <>
struct Elem<uint8_t> {
  static __device__ __forceinline__ void load8(const uint8_t* p, float (&f)[8]) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    unpack_u8x8(v.x, v.y, f);
  }
  static __device__ __forceinline__ float load1(const uint8_t* p) { return static_cast<float>(*p); }
};
template <>
struct Elem<float> {
  static __device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
  template <int N>
  static __device__ __forceinline__ void store(float* p, const float (&f)[N]) {
    static_assert(N == 2 || N == 4 || N == 8, "store width");
    if constexpr (N == 2) {
      *reinterpret_cast<float2*>(p) = make_float2(f[0], f[1]);
    } else {
      *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
      if constexpr (N == 8) *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
  }
  static __device__ __forceinline__ float load1(const float* p) { return *p; }
  static __device__ __forceinline__ void store1(float* p, float f) { *p = f; }
};
template <>
struct Elem<BF16Tag> {
  static __device__ __forceinline__ void load8(const BF16Tag* p, float (&f)[8]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = bf16_bits_to_f32(static_cast<uint16_t>(w[i] & 0xffffu));
      f[2 * i + 1] = bf16_bits_to_f32(static_cast<uint16_t>(w[i] >> 16));
    }
  }
  template <int N>
  static __device__ __forceinline__ void store(BF16Tag* p, const float (&f)[N]) {
    static_assert(N == 2 || N == 4 || N == 8, "store width");
    if constexpr (N == 2)
      *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(f[0], f[1]);
    else if constexpr (N == 4)
      *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]));
    else
      *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]),
                                                pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
  }
  static __device__ __forceinline__ float load1(const BF16Tag* p) { return bf16_bits_to_f32(p->bits); }
  static __device__ __forceinline__ void store1(BF16Tag* p, float f) { p->bits = f32_to_bf16_bits(f); }
};
template <>
struct Elem<F16Tag> {
  template <int N>
  using HalfN = _Float16 __attribute__((ext_vector_type(N)));
  static __device__ __forceinline__ void load8(const F16Tag* p, float (&f)[8]) {
    const HalfN<8> v = *reinterpret_cast<const HalfN<8>*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = static_cast<float>(v[i]);
  }
  template <int N>
  static __device__ __forceinline__ void store(F16Tag* p, const float (&f)[N]) {
    static_assert(N == 2 || N == 4 || N == 8, "store width");
    HalfN<N> v;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = static_cast<_Float16>(f[i]);
    *reinterpret_cast<HalfN<N>*>(p) = v;
  }
  static __device__ __forceinline__ float load1(const F16Tag* p) {
    return static_cast<float>(*reinterpret_cast<const _Float16*>(p));
  }
  static __device__ __forceinline__ void store1(F16Tag* p, float f) {
    *reinterpret_cast<_Float16*>(p) = static_cast<_Float16>(f);
  }
};

// DType code -> storage type, on the host: with_dtype<codes...>(code, f) returns f(T{}) for the storage type T of
// `code` when it is one of `codes` (only those are instantiated), -1 otherwise.
template <DType D>
struct DTypeStorage;
template <> struct DTypeStorage<kU8> { using type = uint8_t; };
template <> struct DTypeStorage<kF32> { using type = float; };
template <> struct DTypeStorage<kBF16> { using type = BF16Tag; };
template <> struct DTypeStorage<kF16> { using type = F16Tag; };

template <DType... Allowed, typename F>
int with_dtype(int32_t code, F&& f) {
  int rc = -1;
  (void)((code == Allowed && ((rc = f(typename DTypeStorage<Allowed>::type{})), true)) || ...);
  return rc;
}

}  // namespace ddl
