// maxk_types.h -- feature storage types of the *_t entry points (MAXK_F32 /
// MAXK_F16 / MAXK_BF16): fp16 and bf16 live in HBM as 2-byte elements, every
// product and sum is fp32.  Loads up-cast (exact); a store rounds to nearest
// even, once per element (include/maxk_spgemm.h).
#ifndef MAXK_TYPES_H
#define MAXK_TYPES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/maxk_spgemm.h"

namespace maxk {

struct f16_t { uint16_t u; };
struct bf16_t { uint16_t u; };

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct DType;
template <> struct DType<float> { static constexpr int id = MAXK_F32; };
template <> struct DType<f16_t> { static constexpr int id = MAXK_F16; };
template <> struct DType<bf16_t> { static constexpr int id = MAXK_BF16; };

inline bool dtype_ok(int dt) { return dt == MAXK_F32 || dt == MAXK_F16 || dt == MAXK_BF16; }
__host__ __device__ inline int dtype_bytes(int dt) { return dt == MAXK_F32 ? 4 : 2; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 16 raw bits -> fp32 (DT: MAXK_F16 or MAXK_BF16), exact
template <int DT>
__device__ __forceinline__ float half_bits_to_f32(uint32_t lo16)
{
    if constexpr (DT == MAXK_F16)
        return (float)__builtin_bit_cast(_Float16, (uint16_t)lo16);
    else
        return __builtin_bit_cast(float, lo16 << 16);
}
// the two elements of one 4-byte word
template <int DT>
__device__ __forceinline__ float word_lo(uint32_t w)
{
    return half_bits_to_f32<DT>(w & 0xffffu);
}
template <int DT>
__device__ __forceinline__ float word_hi(uint32_t w)
{
    if constexpr (DT == MAXK_F16) return half_bits_to_f32<DT>(w >> 16);
    else return __builtin_bit_cast(float, w & 0xffff0000u);
}

__device__ __forceinline__ float load_f32(const float *p) { return *p; }
__device__ __forceinline__ float load_f32(const f16_t *p) { return half_bits_to_f32<MAXK_F16>(p->u); }
__device__ __forceinline__ float load_f32(const bf16_t *p) { return half_bits_to_f32<MAXK_BF16>(p->u); }

// fp32 -> 16 raw bits, round to nearest even (NaN stays NaN, overflow -> inf)
__device__ __forceinline__ uint32_t f32_to_f16_bits(float x)
{
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);  // v_cvt_f16_f32, RNE mode
}
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float x)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (x != x) return (u >> 16) | 0x40u;  // quiet NaN, sign and high payload kept
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// run-time storage type dt (MAXK_F16 / MAXK_BF16; wave-uniform)
__device__ __forceinline__ uint32_t f32_to_half_bits(float x, int dt)
{
    return dt == MAXK_F16 ? f32_to_f16_bits(x) : f32_to_bf16_bits(x);
}

}  // namespace maxk
#endif  // MAXK_TYPES_H
