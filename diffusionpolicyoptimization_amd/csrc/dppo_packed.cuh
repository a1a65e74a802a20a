// dppo_packed.cuh — device helpers that read one element of a packed weight image, shared by the
// backward tail (backward_tail.hip) and the optimizer's virtual l2 gradient (optimizer.hip).
#pragma once
#include "dppo_common.cuh"

// element (k, n) of a packed [K][N] weight image (dppo_layout.h; pack_all_kernel's slot order)
__device__ inline float packed_elem(const uint8_t* img, int K, int k, int n, int prec) {
    const bool two = prec == DPPO_BF16 || prec == DPPO_F16;
    const int KG = two ? 32 : 16, EPL = two ? 8 : 4;
    const int lane = (n & 15) + 16 * ((k % KG) / EPL);
    const size_t slot = ((size_t)(n >> 4) * packed_ksteps(K, KG) + k / KG) * 64 + lane;
    const uint8_t* e = img + slot * 16 + (size_t)(k % EPL) * (two ? 2 : 4);
    if (prec == DPPO_BF16) return (float)*(const __bf16*)e;
    if (prec == DPPO_F16) return (float)*(const _Float16*)e;
    return *(const float*)e;
}
// the same with the precision a compile-time constant: no branch between the loads (a per-element
// precision switch made hipcc wait vmcnt(0) after every 2-byte load)
template <int PREC>
__device__ inline float packed_elem_t(const uint8_t* img, int K, int k, int n) {
    constexpr bool two = PREC == DPPO_BF16 || PREC == DPPO_F16;
    constexpr int KG = two ? 32 : 16, EPL = two ? 8 : 4;
    const int lane = (n & 15) + 16 * ((k % KG) / EPL);
    const size_t slot = ((size_t)(n >> 4) * packed_ksteps(K, KG) + k / KG) * 64 + lane;
    const uint8_t* e = img + slot * 16 + (size_t)(k % EPL) * (two ? 2 : 4);
    if constexpr (PREC == DPPO_BF16) return (float)*(const __bf16*)e;
    else if constexpr (PREC == DPPO_F16) return (float)*(const _Float16*)e;
    else return *(const float*)e;
}
// x rounded to the operand precision
template <int PREC>
__device__ inline float round_prec(float x) {
    if constexpr (PREC == DPPO_BF16) return (float)(__bf16)x;
    else if constexpr (PREC == DPPO_F16) return (float)(_Float16)x;
    else return x;
}
