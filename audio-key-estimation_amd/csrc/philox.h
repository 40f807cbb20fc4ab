// Philox4x32-10, the counter-based generator of the synthesiser's noise (synth.hip) and of the training-window draw (track.hip).
#pragma once

namespace ake {

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c[1] ^ k0, n2 = static_cast<unsigned>(p0 >> 32) ^ c[3] ^ k1;
    c[1] = static_cast<unsigned>(p1); c[3] = static_cast<unsigned>(p0);
    c[0] = n0; c[2] = n2;
}

// Philox4x32-10 (Salmon et al., SC 2011): 10 rounds, the key bumped by the Weyl constants between them
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

}  // namespace ake
