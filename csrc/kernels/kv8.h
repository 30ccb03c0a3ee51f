// kv8: device helpers of the fp8 (OCP e4m3) KV cache rows, shared by decode.hip (append, decode and verify
// attention) and prefill_paged_kv8.hip (paged prefill attention).  Row format: decode.hip's kv8 section and
// mxllm/serve/quant.py kv8_quantize.
#pragma once
#include "common.h"

namespace mx {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kKv8MinExp = -100;

// e of a row's scale 2^e from the largest bf16 magnitude of the row (its bits without the sign):
// amax = m 2^E, 1 <= m < 2: E - 8 if m <= 1.75, else E - 7
__device__ __forceinline__ int kv8_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  return max((int)(amax_bits >> 7) - 135 + ((amax_bits & 0x7Fu) > 0x60u ? 1 : 0), kKv8MinExp);
}
__device__ __forceinline__ float kv8_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
__device__ __forceinline__ uint32_t kv8_amax8(const u16x8& v) {
  uint32_t a = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = max(a, (uint32_t)v[j] & 0x7FFFu);
  return a;
}
// 8 bf16 values times inv (a power of two) -> 8 e4m3 codes
__device__ __forceinline__ uint2 kv8_pack8(const u16x8& v, float inv) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[0]) * inv, bf2f(v[1]) * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[2]) * inv, bf2f(v[3]) * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[4]) * inv, bf2f(v[5]) * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[6]) * inv, bf2f(v[7]) * inv, hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}
// 8 e4m3 codes times sc (a power of two) -> 8 bf16: the hardware conversion is exact for every
// code (subnormals included) and the product has 4 significant bits, so the bf16 is the upper
// half of the f32
__device__ __forceinline__ uint32_t kv8_hi2(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ u16x8 kv8_dec8(uint32_t lo, uint32_t hi, float sc) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return __builtin_bit_cast(u16x8, u32x4{kv8_hi2(a[0] * sc, a[1] * sc), kv8_hi2(b[0] * sc, b[1] * sc),
                                         kv8_hi2(c[0] * sc, c[1] * sc), kv8_hi2(d[0] * sc, d[1] * sc)});
}
__device__ __forceinline__ u16x8 kv8_dec8(uint32_t lo, uint32_t hi) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return __builtin_bit_cast(u16x8, u32x4{kv8_hi2(a[0], a[1]), kv8_hi2(b[0], b[1]), kv8_hi2(c[0], c[1]),
                                         kv8_hi2(d[0], d[1])});
}

}  // namespace mx
