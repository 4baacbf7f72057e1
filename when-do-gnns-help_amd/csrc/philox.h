// Philox4x32-10, the counter-based generator of the device-drawn random objects: the node sets of the kernel-regression epochs
// (kr_sets.hip) and the synthetic graphs and feature rows (synth.hip).  Counter {c0, c1, 0, 0}, key {k0, k1}; include/wdg.h
// documents which output words each caller consumes, and the tests restate the generator in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace wdg {

struct philox_words {
    unsigned w[4];
};

__device__ __forceinline__ void philox_round(unsigned &c0, unsigned &c1, unsigned &c2, unsigned &c3, unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<unsigned>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<unsigned>(p1);
    c3 = static_cast<unsigned>(p0);
    c0 = n0;
    c2 = n2;
}
// all four output words
__device__ __forceinline__ philox_words philox4x32_10_words(unsigned c0, unsigned c1, unsigned k0, unsigned k1) {
    unsigned c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return philox_words{{c0, c1, c2, c3}};
}
// the first output word
__device__ __forceinline__ unsigned philox4x32_10(unsigned c0, unsigned c1, unsigned k0, unsigned k1) {
    return philox4x32_10_words(c0, c1, k0, k1).w[0];
}

}  // namespace wdg
