// What the lock-step rollout kernels share (rubiks_egvm.hip, rubiks_rollout.hip): how a row of the engines' 13-column head is
// read, np.argmax's order, and the host's MT19937.
#pragma once
#include "rubiks_common.h"

namespace rubiks {

__device__ __forceinline__ float egvm_head_elem(const void *head, size_t i, bool bf16) {
    return bf16 ? __uint_as_float((u32) reinterpret_cast<const u16 *>(head)[i] << 16) : reinterpret_cast<const float *>(head)[i];
}

// "v replaces the best b" in a scan by ascending index that must end where np.argmax ends: on the first NaN if there is one,
// else on the first maximum.
__device__ __forceinline__ bool egvm_better(float v, float b) { return !isnan(b) && (isnan(v) || v > b); }

// np.argmax of the 12 numbers x[i0], x[i0 + step], ...: the first maximum, a NaN being the maximum
__device__ __forceinline__ u32 egvm_argmax12(const void *x, size_t i0, size_t step, bool bf16) {
    float best = egvm_head_elem(x, i0, bf16);
    u32 a = 0;
#pragma unroll
    for (u32 k = 1; k < (u32)kActions; ++k) {
        const float v = egvm_head_elem(x, i0 + k * step, bf16);
        if (egvm_better(v, best)) { best = v; a = k; }
    }
    return a;
}

// ---- the host's draws: MT19937 as np.random.RandomState runs it (Matsumoto & Nishimura 1998) ------------------------------------
struct Mt19937 {
    u32 *key;
    int pos;
    u32 next() {
        constexpr int N = 624, M = 397;
        if (pos >= N) {
            for (int k = 0; k < N; ++k) {
                const u32 y = (key[k] & 0x80000000u) | (key[(k + 1) % N] & 0x7fffffffu);
                key[k] = key[(k + M) % N] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            pos = 0;
        }
        u32 y = key[pos++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
};

}  // namespace rubiks
