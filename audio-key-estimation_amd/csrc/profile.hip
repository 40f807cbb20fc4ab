// Key-profile emissions: a key track without a trained net (Krumhansl-Schmuckler; not part of the reference, which has no method that
// runs without a checkpoint).  Every window's chroma is correlated with the 24 rotations of a minor and a major key profile; the result
// is an (R, W, 24) emission tensor that the Viterbi smoother, the posteriors and the scorer take as they take the net's.
//
// The transform has 3 bins per semitone from C with in-tune notes on the bins k = 0 (mod 3), so bin k belongs to semitone (k + 1) / 3
// and pitch class ((k + 1) / 3) % 12 (metrics.profile_emissions is the float64 model).  Two launches: profile_chroma_kernel reduces a
// tile of kProfChunk frames of one recording to its per-frame chroma c[r][t][12] in double, each sum in ascending bin order;
// profile_score_kernel adds one window's frames in ascending order, forms the 24 Pearson correlations in double and writes the float32
// outputs.  No floating-point atomics, every sum in a fixed order: two runs give the same bits.  expm1 is the double library form.
#include "common.h"
#include "profile.h"

#include <cmath>

namespace {

using namespace ake_profile;                                      // the arithmetic itself: shared with the streamed kernels

// 256 threads on a tile of 64 frames x 12 pitch classes: 768 sums of pitches / 12 bins each, three per thread.  Pitch-major input:
// lanes run along the frames, which are contiguous; frames-major: lanes run along the pitch classes, whose three-bin groups are 12
// bytes apart.  Left as it is until the two launches have been timed (tools/profile_baseline.py).
constexpr int kProfChunk = 64;       // frames per block
constexpr int kProfThreads = 256;

struct ProfChromaArgs {
    const float* mel;           // [recordings][pitches][frames], or [recordings][frames][pitches] (frames_major)
    const int* counts;          // frames of each recording (clamped to 0..frames), or null
    double* chroma;             // [recordings][frames][12]
    int pitches, frames, compression;
};

__device__ __forceinline__ int prof_count(const int* counts, int rec, int frames) {
    if (!counts) return frames;
    const int c = counts[rec];
    return c < 0 ? 0 : (c < frames ? c : frames);
}

template <bool kFramesMajor>
__global__ __launch_bounds__(kProfThreads) void profile_chroma_kernel(ProfChromaArgs a) {
    const int rec = blockIdx.y, t0 = blockIdx.x * kProfChunk;
    const int T = prof_count(a.counts, rec, a.frames);
    const float* mel = a.mel + static_cast<long long>(rec) * a.pitches * a.frames;
    for (int item = threadIdx.x; item < kProfChunk * kProfClasses; item += kProfThreads) {
        const int j = kFramesMajor ? item % kProfClasses : item / kProfChunk;
        const int t = t0 + (kFramesMajor ? item / kProfClasses : item % kProfChunk);
        if (t >= a.frames) continue;
        double s = 0.0;
        if (t < T)                                                // frames at or behind the count are written as zeros
            s = prof_class_sum(j, a.pitches, a.compression, [&](int k) {
                return kFramesMajor ? mel[static_cast<long long>(t) * a.pitches + k] : mel[static_cast<long long>(k) * a.frames + t];
            });
        a.chroma[(static_cast<long long>(rec) * a.frames + t) * kProfClasses + j] = s;
    }
}

struct ProfScoreArgs {
    const double* frame_chroma; // [recordings][frames][12]
    const int* counts;
    const float* profiles;      // [2][12]: minor, major, tonic first
    ProfScoreOut out;           // [recordings][windows] cells
    int frames, window_frames, stride_frames, windows;
    double sharpness;
};

__global__ __launch_bounds__(kProfScoreThreads) void profile_score_kernel(ProfScoreArgs a) {
    __shared__ ProfScoreLds lds;
    const int rec = blockIdx.y, w = blockIdx.x;
    const int T = prof_count(a.counts, rec, a.frames);
    int n_win, first, len;
    if (a.window_frames == 0) { n_win = T > 0 ? 1 : 0; first = 0; len = T; }                 // the whole clip
    else { n_win = T < a.window_frames ? 0 : (T - a.window_frames) / a.stride_frames + 1; first = w * a.stride_frames; len = a.window_frames; }
    prof_score_block(lds, w < n_win, [&](int j) {
        const double* c = a.frame_chroma + (static_cast<long long>(rec) * a.frames + first) * kProfClasses + j;
        double s = 0.0;
        for (int t = 0; t < len; ++t) s += c[static_cast<long long>(t) * kProfClasses];      // ascending t
        return s;
    }, a.profiles, a.sharpness, static_cast<long long>(rec) * a.windows + w, a.out);
}

bool prof_shape_ok(int recordings, int frames) { return recordings > 0 && recordings <= 65535 && frames > 0; }

}  // namespace

extern "C" {

size_t ake_profile_workspace_bytes(int recordings, int frames) {
    if (!prof_shape_ok(recordings, frames)) return 0;
    return ake::align_up(static_cast<size_t>(recordings) * static_cast<size_t>(frames) * kProfClasses * sizeof(double), 256);
}

int ake_profile_windows(int frames, int window_frames, int stride_frames) {
    if (frames < 1 || window_frames < 0 || stride_frames < 1) return -1;
    if (window_frames == 0) return 1;
    return frames < window_frames ? 0 : (frames - window_frames) / stride_frames + 1;
}

int ake_profile_emissions_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int frames, const int32_t* counts_dev,
                              int window_frames, int stride_frames, int windows, const float* profiles_dev, int compression,
                              float sharpness, float* chroma_out, float* emissions_out, int32_t* key_id_out, float* confidence_out,
                              void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(mel_dev && profiles_dev && chroma_out && emissions_out && key_id_out && confidence_out, AKE_ERR_INVALID,
                "profile_emissions: null argument");
    AKE_REQUIRE(prof_shape_ok(recordings, frames) && pitches > 0, AKE_ERR_INVALID,
                "profile_emissions: bad shape (%d recordings, %d pitches, %d frames)", recordings, pitches, frames);
    AKE_REQUIRE(pitches % 3 == 0, AKE_ERR_UNSUPPORTED, "profile_emissions: %d bins are no multiple of 3 (3 bins per semitone)", pitches);
    AKE_REQUIRE(static_cast<long long>(pitches) * frames <= (1ll << 31) - 1, AKE_ERR_INVALID, "profile_emissions: %d x %d is too large", pitches, frames);
    AKE_REQUIRE(compression >= 0 && compression <= 2, AKE_ERR_INVALID, "profile_emissions: compression %d is none of 0 (log), 1 (magnitude), 2 (power)", compression);
    AKE_REQUIRE(sharpness > 0.0f, AKE_ERR_INVALID, "profile_emissions: sharpness must be positive (and not NaN)");
    AKE_REQUIRE(window_frames >= 0 && stride_frames >= 1, AKE_ERR_INVALID, "profile_emissions: window_frames %d (>= 0), stride_frames %d (>= 1)",
                window_frames, stride_frames);
    const int want = ake_profile_windows(frames, window_frames, stride_frames);
    AKE_REQUIRE(windows == want, AKE_ERR_INVALID, "profile_emissions: %d windows given, ake_profile_windows says %d", windows, want);
    const size_t need = ake_profile_workspace_bytes(recordings, frames);
    AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "profile_emissions: workspace %zu < %zu bytes", workspace_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AKE_ERR_INVALID, "profile_emissions: the workspace must be 8-byte aligned");
    if (windows == 0) return AKE_OK;                              // no recording can hold a window: the outputs have no elements
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = (frames + kProfChunk - 1) / kProfChunk;
    ProfChromaArgs c{mel_dev, counts_dev, static_cast<double*>(workspace), pitches, frames, compression};
    const int rc = frames_major ? ake::launch("profile_chroma_kernel", profile_chroma_kernel<true>, dim3(chunks, recordings), dim3(kProfThreads), 0, s, c)
                                : ake::launch("profile_chroma_kernel", profile_chroma_kernel<false>, dim3(chunks, recordings), dim3(kProfThreads), 0, s, c);
    if (rc) return rc;
    ProfScoreArgs f{static_cast<const double*>(workspace), counts_dev, profiles_dev, {chroma_out, emissions_out, key_id_out, confidence_out},
                    frames, window_frames, stride_frames, windows, static_cast<double>(sharpness)};
    return ake::launch("profile_score_kernel", profile_score_kernel, dim3(windows, recordings), dim3(kProfScoreThreads), 0, s, f);
}

}  // extern "C"
