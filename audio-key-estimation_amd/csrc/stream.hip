// The front end of a stream of audio (KeyEstimator.stream; semantics in include/ake_hip.h): what a push does to the two buffers a
// stream keeps on the device between calls, one launch each.
//   - the audio history [recordings][stride] float32: the samples the next transform still needs slide to the front, the chunk (float32
//     or 16-bit PCM) follows them;
//   - the frame cache: the frames later windows still need, then the newly final frames out of the transform's output, written into the
//     other of two buffers (the cache is compact, [recordings][frames][pitches] or [recordings][pitches][frames] with `frames` what it
//     holds now, because ake_pcnet_forward_windows_f32 takes a recording's stride from the frame count).
// All recordings advance in lockstep, so every count is a host integer.  Plain loads and stores, no atomics.
#include "common.h"

#include <cstdint>

namespace {

constexpr int kHistThreads = 1024;
constexpr int kHistPer = 4;                                   // samples per thread and tile
constexpr int kHistTile = kHistThreads * kHistPer;

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(short v) { return static_cast<float>(v) * (1.f / 32768.f); }      // exact: pcm16_to_float

template <typename T>
struct HistArgs {
    float* hist;               // [recordings][stride]
    const T* chunk;            // [recordings][chunk_stride]
    long long stride, chunk_stride, drop, keep, m;
};

// One workgroup per recording: it moves its row's kept samples `drop` to the front, then appends the chunk behind them.  The move's
// destination lies in front of its source and may overlap it, so the workgroup takes the tiles in ascending order, loads a whole tile
// into registers, meets at a barrier and only then stores it: a tile's stores reach no sample a later tile still has to load (those
// start at or behind this tile's end), and none of its own before every lane has loaded.  The chunk lands on [keep, keep + m), which
// overlaps the move's source [drop, drop + keep): it follows the move in the same workgroup, behind the last tile's barrier.
template <typename T>
__global__ __launch_bounds__(kHistThreads) void stream_history_kernel(HistArgs<T> a) {
    float* const row = a.hist + static_cast<long long>(blockIdx.x) * a.stride;
    if (a.drop > 0) {
        for (long long t0 = 0; t0 < a.keep; t0 += kHistTile) {
            float v[kHistPer];
#pragma unroll
            for (int q = 0; q < kHistPer; ++q) {
                const long long i = t0 + q * kHistThreads + threadIdx.x;
                v[q] = i < a.keep ? row[i + a.drop] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kHistPer; ++q) {
                const long long i = t0 + q * kHistThreads + threadIdx.x;
                if (i < a.keep) row[i] = v[q];
            }
            __syncthreads();                                  // this tile's stores, before the next tile's loads and the chunk's stores
        }
    }
    const T* const src = a.chunk + static_cast<long long>(blockIdx.x) * a.chunk_stride;
    for (long long i = threadIdx.x; i < a.m; i += kHistThreads) row[a.keep + i] = to_float(src[i]);
}

struct FrameArgs {
    float* dst;                // keep + n_new frames
    const float* old;          // old_frames frames
    const float* mel;          // mel_frames frames
    int P, old_frames, drop, keep, mel_frames, first, n_new;
    long long quads;           // frames-major: 16-byte pieces of dst per recording
};

// Frames-major: a frame is P contiguous floats (P % 4 == 0), so a recording of the cache is two straight copies in 16-byte pieces.
__global__ __launch_bounds__(256) void stream_frames_fm_kernel(FrameArgs a) {
    const long long x = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= a.quads) return;
    const int r = blockIdx.y, pq = a.P / 4;
    const long long kept = static_cast<long long>(a.keep) * pq;
    const float4 v = x < kept
        ? reinterpret_cast<const float4*>(a.old + (static_cast<long long>(r) * a.old_frames + a.drop) * a.P)[x]
        : reinterpret_cast<const float4*>(a.mel + (static_cast<long long>(r) * a.mel_frames + a.first) * a.P)[x - kept];
    reinterpret_cast<float4*>(a.dst + static_cast<long long>(r) * (a.keep + a.n_new) * a.P)[x] = v;
}

// Pitch-major ([recording][pitch][frame]): both copies run along the frames, the fast axis of source and destination alike.  grid
// (frame tiles, P, recordings).
__global__ __launch_bounds__(256) void stream_frames_pm_kernel(FrameArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y, r = blockIdx.z, cf = a.keep + a.n_new;
    if (f >= cf) return;
    const long long line = static_cast<long long>(r) * a.P + p;
    a.dst[line * cf + f] = f < a.keep ? a.old[line * a.old_frames + a.drop + f] : a.mel[line * a.mel_frames + a.first + (f - a.keep)];
}

template <typename T>
int stream_history(float* hist, int recordings, int64_t stride, int64_t drop, int64_t keep, const T* chunk, int64_t chunk_stride, int64_t m,
                   ake_stream_t stream) {
    AKE_REQUIRE(hist && recordings > 0 && stride > 0, AKE_ERR_INVALID, "stream_history: null history or bad shape");
    AKE_REQUIRE(drop >= 0 && keep >= 0 && m >= 0 && (m == 0 || (chunk && chunk_stride >= m)), AKE_ERR_INVALID, "stream_history: bad chunk");
    AKE_REQUIRE(keep + m <= stride && drop + keep <= stride, AKE_ERR_INVALID,
                "stream_history: keep %lld + chunk %lld or drop %lld + keep exceed the history's %lld samples", static_cast<long long>(keep),
                static_cast<long long>(m), static_cast<long long>(drop), static_cast<long long>(stride));
    if (m == 0 && (keep == 0 || drop == 0)) return AKE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HistArgs<T> a{hist, chunk, stride, chunk_stride, drop, keep, m};
    return ake::launch("stream_history_kernel", stream_history_kernel<T>, dim3(recordings), dim3(kHistThreads), 0, s, a);
}

}  // namespace

extern "C" {

int ake_stream_history_f32(float* history_dev, int recordings, int64_t history_stride, int64_t drop, int64_t keep, const float* chunk_dev,
                           int64_t chunk_stride, int64_t m, ake_stream_t stream) {
    return stream_history<float>(history_dev, recordings, history_stride, drop, keep, chunk_dev, chunk_stride, m, stream);
}

int ake_stream_history_pcm16(float* history_dev, int recordings, int64_t history_stride, int64_t drop, int64_t keep,
                             const int16_t* chunk_dev, int64_t chunk_stride, int64_t m, ake_stream_t stream) {
    return stream_history<short>(history_dev, recordings, history_stride, drop, keep, reinterpret_cast<const short*>(chunk_dev), chunk_stride, m,
                                 stream);
}

int ake_stream_frames_f32(float* dst_dev, const float* old_dev, const float* mel_dev, int frames_major, int recordings, int pitches,
                          int old_frames, int drop, int keep, int mel_frames, int first, int n_new, ake_stream_t stream) {
    AKE_REQUIRE(dst_dev && recordings > 0 && recordings <= 65535 && pitches > 0 && pitches <= 65535 && keep >= 0 && n_new >= 0 && drop >= 0 && first >= 0, AKE_ERR_INVALID,
                "stream_frames: null destination or bad shape");
    AKE_REQUIRE(keep == 0 || (old_dev && drop + keep <= old_frames), AKE_ERR_INVALID, "stream_frames: frames %d..%d of a cache of %d", drop,
                drop + keep, old_frames);
    AKE_REQUIRE(n_new == 0 || (mel_dev && first + n_new <= mel_frames), AKE_ERR_INVALID, "stream_frames: frames %d..%d of a transform of %d",
                first, first + n_new, mel_frames);
    AKE_REQUIRE(dst_dev != old_dev && dst_dev != mel_dev, AKE_ERR_INVALID, "stream_frames: the destination must not be a source");
    const long long cf = static_cast<long long>(keep) + n_new;
    AKE_REQUIRE(cf * pitches < (1ll << 31), AKE_ERR_INVALID, "stream_frames: %lld frames are too many", cf);
    if (cf == 0) return AKE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameArgs a{dst_dev, old_dev, mel_dev, pitches, old_frames, drop, keep, mel_frames, first, n_new, cf * (pitches / 4)};
    if (frames_major) {
        AKE_REQUIRE(pitches % 4 == 0 && ((reinterpret_cast<uintptr_t>(dst_dev) | reinterpret_cast<uintptr_t>(old_dev) | reinterpret_cast<uintptr_t>(mel_dev)) & 15) == 0,
                    AKE_ERR_INVALID, "stream_frames: frames-major needs pitches %% 4 == 0 and 16-byte aligned buffers");
        return ake::launch("stream_frames_fm_kernel", stream_frames_fm_kernel, dim3(static_cast<unsigned>((a.quads + 255) / 256), recordings), dim3(256), 0, s, a);
    }
    return ake::launch("stream_frames_pm_kernel", stream_frames_pm_kernel, dim3(static_cast<unsigned>((cf + 255) / 256), pitches, recordings), dim3(256), 0, s, a);
}

}  // extern "C"
