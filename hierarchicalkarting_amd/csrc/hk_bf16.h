// hk_bf16.h — the ONE fp32 -> bf16 rounding of the library: the PPO trainer's operands (hk_ppo.h) and the bf16 inference chain
// (hk_policy_bf16.h) round with it, so a weight or an activation is the same 16 bits on both sides.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace hk {

// fp32 -> bf16, to nearest even; Inf stays Inf, every NaN becomes the quiet NaN 0x7FC0 (torch's conversion; host twin ppo.bf16_round)
__device__ __forceinline__ uint16_t ppo_bf16_rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)0x7FC0u;
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float ppo_bf16_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

}  // namespace hk
