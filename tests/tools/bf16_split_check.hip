// Stand-alone check of csrc/bf16_split.h, built and run by tests/test_gpu_bf16_split.py: the packed split (bf16_split2: v_cvt_pk_bf16_f32)
// against the integer one (bf16_bits, twice per value) on all 2^32 float bit patterns, in the low and in the high half of the pack.
// Thread i walks patterns i, i + 2^24, ...: pattern u goes into the low half, pattern u * 2654435761 (odd: a bijection of the 2^32
// patterns) into the high half.  Prints how many non-NaN patterns differ in hi or lo (the test asserts 0) and, for the record, how many
// NaN patterns do.
#include <cstdio>

#include "bf16_split.h"

__global__ void bf16_split_check_kernel(unsigned long long* counts) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;              // 2^24 threads
    unsigned int differ = 0, nan_differ = 0, nans = 0;
    for (unsigned int k = 0; k < 256; ++k) {
        const unsigned int u[2] = {i + (k << 24), (i + (k << 24)) * 2654435761u};
        unsigned int hi, lo;
        ake_k::bf16_split2(__uint_as_float(u[0]), __uint_as_float(u[1]), hi, lo);
        for (int h = 0; h < 2; ++h) {
            const float v = __uint_as_float(u[h]);
            const unsigned int hb = ake_k::bf16_bits(v) & 0xFFFFu;
            const unsigned int lb = ake_k::bf16_bits(v - __uint_as_float(hb << 16)) & 0xFFFFu;
            const bool same = hb == ((hi >> (16 * h)) & 0xFFFFu) && lb == ((lo >> (16 * h)) & 0xFFFFu);
            const bool is_nan = (u[h] & 0x7FFFFFFFu) > 0x7F800000u;
            nans += is_nan;
            if (!same) (is_nan ? nan_differ : differ) += 1;
        }
    }
    if (differ) atomicAdd(&counts[0], static_cast<unsigned long long>(differ));
    if (nan_differ) atomicAdd(&counts[1], static_cast<unsigned long long>(nan_differ));
    atomicAdd(&counts[2], static_cast<unsigned long long>(nans));
}

int main() {
    unsigned long long* dev = nullptr;
    unsigned long long host[3] = {0, 0, 0};
    if (hipMalloc(&dev, sizeof(host)) != hipSuccess || hipMemset(dev, 0, sizeof(host)) != hipSuccess) { std::printf("error no device memory\n"); return 1; }
    bf16_split_check_kernel<<<dim3(1u << 16), dim3(256)>>>(dev);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, dev, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) {
        std::printf("error the kernel did not run\n");
        return 1;
    }
    (void)hipFree(dev);
    // every pattern is seen twice (once per half of the pack)
    std::printf("patterns %llu\ndiffer %llu\nnan_patterns %llu\nnan_differ %llu\n", 2ull << 32, host[0], host[2], host[1]);
    return 0;
}
