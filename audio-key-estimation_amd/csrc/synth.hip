// Additive synthesiser: R recordings from lists of enveloped sinusoidal partials plus Gaussian noise, peak-normalised, float32, ragged.
// It makes the long modulating recordings (synthetic.make_modulating_batch_device) that key tracks are scored on; semantics in
// include/ake_hip.h, host model synthetic.synth_partials_reference.
//
//   y[t] = sum_p amp_p * g_in * g_out * sin(2 pi frac(cps_p t + phase_p)) + noise_sigma * z_r[t]        t < n_r, start_p <= t < end_p
//
// synth_kernel: one thread per 4 consecutive samples (one 16-byte store, and one Philox4x32-10 block: it yields exactly 4 normals), a
// block of 256 per tile of 1024 samples of one recording.  The block first compacts the recording's partials that overlap its tile into
// LDS -- kSynthBatch candidates at a time, in their own order (ballot + prefix count, no atomics), so a sample's sum is added in one fixed
// order and two runs agree to the bit -- and every thread then walks the compacted list.  The phase is one float64 fma and a floor per
// (sample, partial): only the fraction (a turn in [0, 1), folded to [-1/2, 1/2)) is rounded to float32, so the error does not grow with t.
// The block's max |y| goes through a wave butterfly and LDS into one integer atomicMax on the float's bit pattern per block (the maximum
// does not depend on the order).  synth_scale_kernel is the second pass: y *= peak / max.
#include "common.h"
#include "philox.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kSynthBlock = 256;
constexpr int kSynthTile = 4 * kSynthBlock;          // samples per block
constexpr int kSynthBatch = kSynthBlock;             // partials the LDS list holds: one candidate per thread and round
constexpr float kTwoPi = 6.2831853071795864769f;

struct SynthArgs {
    const int* offsets;        // [R + 1]
    const double* cps;         // per partial: cycles per sample
    const double* phase;       // turns
    const float* amp;
    const long long* start;
    const long long* end;
    const long long* n;        // [R]
    const long long* seed;     // [R], nullable when sigma == 0
    float* out;                // [R][stride]
    unsigned* peak_bits;       // [R], zeroed before the launch; null: no normalisation
    long long stride;
    int fade;
    float sigma;
};

// ((x >> 9) + 0.5) 2^-23: an odd multiple of 2^-24 in (0, 1), exact in float32
__device__ __forceinline__ float philox_uniform(unsigned x) { return (static_cast<float>(x >> 9) + 0.5f) * 0x1p-23f; }

// a turn in [0, 1] -> the same angle in [-1/2, 1/2] (exact: Sterbenz), which halves the rounding error of the product with 2 pi
__device__ __forceinline__ float fold_turn(float f) { return f >= 0.5f ? f - 1.0f : f; }

// a raised-cosine ramp: 0.5 - 0.5 cos(pi (k + 0.5) / fade), k = 0..fade-1 samples into the fade
__device__ __forceinline__ float fade_gain(long long k, int fade) {
    const float x = static_cast<float>((static_cast<double>(k) + 0.5) / static_cast<double>(fade));
    return 0.5f - 0.5f * cosf(3.14159265358979323846f * x);
}

__global__ __launch_bounds__(kSynthBlock) void synth_kernel(SynthArgs a) {
    __shared__ double s_cps[kSynthBatch], s_phase[kSynthBatch];
    __shared__ long long s_start[kSynthBatch], s_end[kSynthBatch];
    __shared__ float s_amp[kSynthBatch];
    __shared__ int s_wave[kSynthBlock / 64];
    __shared__ unsigned s_max[kSynthBlock / 64];
    const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long tile0 = static_cast<long long>(blockIdx.x) * kSynthTile, t0 = tile0 + 4 * tid;
    long long n = a.n[r];
    n = n < 0 ? 0 : n > a.stride ? a.stride : n;                         // (host-checked against n_max <= stride; the clamp bounds the stores)
    float4* const dst = reinterpret_cast<float4*>(a.out + static_cast<long long>(r) * a.stride + t0);
    const bool stores = t0 < a.stride;                                   // stride is a multiple of 4: all 4 samples or none
    if (tile0 >= n) {                                                    // block-uniform: nothing sounds here
        if (stores) *dst = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const long long tile1 = tile0 + kSynthTile < n ? tile0 + kSynthTile : n;     // the tile's samples that exist: [tile0, tile1)
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    const int p0 = a.offsets[r], p1 = a.offsets[r + 1];
    for (int base = p0; base < p1; base += kSynthBatch) {                // (block-uniform loop: every thread meets every barrier)
        const int p = base + tid;
        long long ps = 0, pe = 0;
        if (p < p1) { ps = a.start[p]; pe = a.end[p]; }
        const bool hit = p < p1 && ps < tile1 && pe > tile0 && ps < pe;
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();                                                 // also: the round before has been read by everyone
        int slot = __popcll(mask & ((1ull << lane) - 1)), count = 0;
#pragma unroll
        for (int v = 0; v < kSynthBlock / 64; ++v) {
            slot += v < wave ? s_wave[v] : 0;
            count += s_wave[v];
        }
        if (hit) {                                                       // slot < kSynthBatch: at most one hit per thread
            s_cps[slot] = a.cps[p]; s_phase[slot] = a.phase[p]; s_amp[slot] = a.amp[p];
            s_start[slot] = ps; s_end[slot] = pe;
        }
        __syncthreads();
        for (int q = 0; q < count; ++q) {
            const long long qs = s_start[q], qe = s_end[q];
            if (qs >= t0 + 4 || qe <= t0) continue;
            const double cps = s_cps[q], ph = s_phase[q];
            const float amp = s_amp[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long t = t0 + k;
                if (t < qs || t >= qe || t >= n) continue;
                const double turns = fma(cps, static_cast<double>(t), ph);
                float v = amp * sinf(kTwoPi * fold_turn(static_cast<float>(turns - floor(turns))));
                if (a.fade > 0) {
                    if (t - qs < a.fade) v *= fade_gain(t - qs, a.fade);
                    if (qe - 1 - t < a.fade) v *= fade_gain(qe - 1 - t, a.fade);
                }
                y[k] += v;
            }
        }
        __syncthreads();                                                 // the list and s_wave are rewritten by the next round
    }
    if (a.sigma != 0.f) {
        const unsigned long long b = static_cast<unsigned long long>(t0) >> 2, sd = static_cast<unsigned long long>(a.seed[r]);
        unsigned c[4] = {static_cast<unsigned>(b), static_cast<unsigned>(b >> 32), static_cast<unsigned>(r), 0u};
        ake::philox4x32_10(c, static_cast<unsigned>(sd), static_cast<unsigned>(sd >> 32));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float rad = a.sigma * sqrtf(-2.0f * logf(philox_uniform(c[2 * h])));
            float sn, cs;
            sincosf(kTwoPi * fold_turn(philox_uniform(c[2 * h + 1])), &sn, &cs);
            y[2 * h] += rad * cs;
            y[2 * h + 1] += rad * sn;
        }
    }
    unsigned m = 0;                                                      // bits of max |y|: for floats >= 0 the bit patterns order as the values
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (t0 + k >= n) y[k] = 0.f;
        const unsigned bits = __float_as_uint(fabsf(y[k]));
        m = bits > m ? bits : m;
    }
    if (stores) *dst = make_float4(y[0], y[1], y[2], y[3]);
    if (!a.peak_bits) return;                                            // (kernel-uniform)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned o = static_cast<unsigned>(__shfl_xor(static_cast<int>(m), s));
        m = o > m ? o : m;
    }
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < kSynthBlock / 64; ++v) m = s_max[v] > m ? s_max[v] : m;
        if (m) atomicMax(a.peak_bits + r, m);
    }
}

// y *= peak / max |y| of the recording; an all-zero recording stays as it is.  One float4 per thread, grid-stride along the row.
__global__ __launch_bounds__(256) void synth_scale_kernel(float* out, const unsigned* __restrict__ peak_bits, const long long* __restrict__ n,
                                                          long long stride, float peak) {
    const int r = blockIdx.y;
    const float mx = __uint_as_float(peak_bits[r]);
    if (!(mx > 0.f)) return;
    const double s = static_cast<double>(peak) / static_cast<double>(mx);      // (in float64: one rounding per sample, the last)
    long long quads = n[r];
    quads = quads < 0 ? 0 : quads > stride ? stride : quads;
    quads = (quads + 3) >> 2;                                            // (the samples behind n in the last quad are zeros and stay zeros)
    float4* const row = reinterpret_cast<float4*>(out + static_cast<long long>(r) * stride);
    for (long long q = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; q < quads; q += static_cast<long long>(gridDim.x) * blockDim.x) {
        float4 v = row[q];
        v.x = static_cast<float>(v.x * s); v.y = static_cast<float>(v.y * s); v.z = static_cast<float>(v.z * s); v.w = static_cast<float>(v.w * s);
        row[q] = v;
    }
}

}  // namespace

extern "C" {

int ake_synth_batch_partials(void) { return kSynthBatch; }

size_t ake_synth_partials_workspace_bytes(int recordings) {
    return recordings > 0 ? ake::align_up(static_cast<size_t>(recordings) * sizeof(unsigned), 256) : 0;
}

int ake_synth_partials_f32(const int32_t* offsets_dev, const double* cps_dev, const double* phase_dev, const float* amp_dev,
                           const int64_t* start_dev, const int64_t* end_dev, int fade, int recordings, const int64_t* n_dev, int64_t n_max,
                           int64_t stride, float noise_sigma, const int64_t* seed_dev, float peak, float* out_dev, void* workspace,
                           size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(offsets_dev && n_dev && out_dev, AKE_ERR_INVALID, "synth_partials: null argument");
    AKE_REQUIRE(recordings > 0 && recordings <= 65535, AKE_ERR_INVALID, "synth_partials: %d recordings (1..65535)", recordings);
    AKE_REQUIRE(n_max >= 0 && stride >= 4 && stride % 4 == 0 && stride >= n_max, AKE_ERR_INVALID,
                "synth_partials: stride %lld must be a multiple of 4, at least 4 and at least n_max = %lld", static_cast<long long>(stride),
                static_cast<long long>(n_max));
    const long long tiles = (stride + kSynthTile - 1) / kSynthTile;
    AKE_REQUIRE(tiles < (1ll << 31), AKE_ERR_INVALID, "synth_partials: stride %lld is too long", static_cast<long long>(stride));
    AKE_REQUIRE(fade >= 0, AKE_ERR_INVALID, "synth_partials: fade %d is negative", fade);
    AKE_REQUIRE(std::isfinite(noise_sigma) && std::isfinite(peak) && peak >= 0.f, AKE_ERR_INVALID, "synth_partials: noise_sigma and peak must be finite, peak not negative");
    AKE_REQUIRE(noise_sigma == 0.f || seed_dev, AKE_ERR_INVALID, "synth_partials: noise needs seed_dev");
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 15) == 0, AKE_ERR_INVALID, "synth_partials: out_dev must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* peak_bits = nullptr;
    if (peak > 0.f) {
        const size_t need = ake_synth_partials_workspace_bytes(recordings);
        AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "synth_partials: workspace %zu < %zu bytes", workspace_bytes, need);
        peak_bits = static_cast<unsigned*>(workspace);
        AKE_HIP_CHECK(hipMemsetAsync(peak_bits, 0, static_cast<size_t>(recordings) * sizeof(unsigned), s));
    }
    SynthArgs a{offsets_dev, cps_dev, phase_dev, amp_dev, reinterpret_cast<const long long*>(start_dev), reinterpret_cast<const long long*>(end_dev),
                reinterpret_cast<const long long*>(n_dev), reinterpret_cast<const long long*>(seed_dev), out_dev, peak_bits, stride, fade, noise_sigma};
    const int rc = ake::launch("synth_kernel", synth_kernel, dim3(static_cast<unsigned>(tiles), recordings), dim3(kSynthBlock), 0, s, a);
    if (rc || !peak_bits) return rc;
    const long long quads = stride / 4;
    const unsigned blocks = static_cast<unsigned>(std::min<long long>((quads + 255) / 256, 1024));
    return ake::launch("synth_scale_kernel", synth_scale_kernel, dim3(blocks, recordings), dim3(256), 0, s, out_dev, peak_bits,
                       reinterpret_cast<const long long*>(n_dev), stride, peak);
}

}  // extern "C"
