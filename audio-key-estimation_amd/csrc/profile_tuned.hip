// Tuned chroma: key-profile emissions of a detuned recording from its one transform, without retuning the audio (not part of the
// reference).  The profile method only sums bins, so a detuning of c cents is met by moving the pitch classes' boundaries by
// 3 c / 100 bins and splitting the one bin every boundary crosses (metrics.profile_emissions(cents=...) is the float64 model).
//
// Two launches: profile_fold_kernel reduces a tile of kFoldChunk frames of one recording to its 36 octave-folded sums per frame,
// F[r][t][p] in double, each sum in ascending octave; profile_tuned_score_kernel adds one window's frames in ascending order, cuts the
// 36 sums into 12 class sums by the window's cents and hands them to prof_score_block, the scoring of profile.hip.  The weights enter
// behind the frame sums, so a window's cents may change while its frames are summed once.  No atomics, every sum in a fixed order: two
// runs give the same bits.
#include "common.h"
#include "profile.h"

#include <cmath>

namespace {

using namespace ake_profile;

constexpr int kFoldChunk = 64;       // frames per block
constexpr int kFoldThreads = 256;
constexpr int kWinBatch = 8;         // frames of a window whose loads go out together

struct ProfFoldArgs {
    const float* mel;           // [recordings][pitches][frames], or [recordings][frames][pitches] (frames_major)
    const int* counts;          // frames of each recording (clamped to 0..frames), or null
    double* folded;             // [recordings][frames][36]
    int pitches, frames, compression;
};

__device__ __forceinline__ int tuned_count(const int* counts, int rec, int frames) {
    if (!counts) return frames;
    const int c = counts[rec];
    return c < 0 ? 0 : (c < frames ? c : frames);
}

// 256 threads on a tile of 64 frames x 36 folded positions: 2304 sums of pitches / 36 bins each, nine per thread.  Pitch-major input:
// lanes run along the frames, which are contiguous; frames-major: lanes run along the 36 positions, 144 contiguous bytes per octave.
template <bool kFramesMajor>
__global__ __launch_bounds__(kFoldThreads) void profile_fold_kernel(ProfFoldArgs a) {
    const int rec = blockIdx.y, t0 = blockIdx.x * kFoldChunk;
    const int T = tuned_count(a.counts, rec, a.frames);
    const float* mel = a.mel + static_cast<long long>(rec) * a.pitches * a.frames;
    for (int item = threadIdx.x; item < kFoldChunk * kProfFolded; item += kFoldThreads) {
        const int p = kFramesMajor ? item % kProfFolded : item / kFoldChunk;
        const int t = t0 + (kFramesMajor ? item / kProfFolded : item % kFoldChunk);
        if (t >= a.frames) continue;
        double s = 0.0;
        if (t < T)                                                // frames at or behind the count are written as zeros
            s = prof_fold_sum(p, a.pitches, a.compression, [&](int k) {
                return kFramesMajor ? mel[static_cast<long long>(t) * a.pitches + k] : mel[static_cast<long long>(k) * a.frames + t];
            });
        a.folded[(static_cast<long long>(rec) * a.frames + t) * kProfFolded + p] = s;
    }
}

struct ProfTunedScoreArgs {
    const double* folded;       // [recordings][frames][36]
    const int* counts;
    const float* profiles;      // [2][12]: minor, major, tonic first
    const float* cents;         // window (r, w) reads cents[r * cents_rec_stride + w * cents_win_stride]
    long long cents_rec_stride, cents_win_stride;
    ProfScoreOut out;           // [recordings][windows] cells
    int frames, window_frames, stride_frames, windows;
    double sharpness;
};

__global__ __launch_bounds__(kProfScoreThreads) void profile_tuned_score_kernel(ProfTunedScoreArgs a) {
    __shared__ ProfScoreLds lds;
    __shared__ double fw[kProfFolded];
    const int rec = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const int T = tuned_count(a.counts, rec, a.frames);
    int n_win, first, len;
    if (a.window_frames == 0) { n_win = T > 0 ? 1 : 0; first = 0; len = T; }                 // the whole clip
    else { n_win = T < a.window_frames ? 0 : (T - a.window_frames) / a.stride_frames + 1; first = w * a.stride_frames; len = a.window_frames; }
    const bool live = w < n_win;                                  // a live window's frames lie below T <= frames
    if (live && tid < kProfFolded) {
        const double* f = a.folded + (static_cast<long long>(rec) * a.frames + first) * kProfFolded + tid;
        double s = 0.0;
        for (int t = 0; t < len; t += kWinBatch) {                // ascending t, the loads of kWinBatch frames ahead of their adds
            double v[kWinBatch];
#pragma unroll
            for (int q = 0; q < kWinBatch; ++q) v[q] = t + q < len ? f[static_cast<long long>(t + q) * kProfFolded] : 0.0;
#pragma unroll
            for (int q = 0; q < kWinBatch; ++q)
                if (t + q < len) s += v[q];
        }
        fw[tid] = s;
    }
    __syncthreads();
    ProfTunedCut cut{-1, 1.0, 0.0};
    if (live && tid < kProfClasses) cut = prof_tuned_cut(a.cents[rec * a.cents_rec_stride + w * a.cents_win_stride]);
    prof_score_block(lds, live, [&](int j) { return prof_tuned_class(j, cut, fw); }, a.profiles, a.sharpness,
                     static_cast<long long>(rec) * a.windows + w, a.out);
}

bool tuned_shape_ok(int recordings, int frames) { return recordings > 0 && recordings <= 65535 && frames > 0; }

}  // namespace

extern "C" {

size_t ake_profile_tuned_workspace_bytes(int recordings, int frames) {
    if (!tuned_shape_ok(recordings, frames)) return 0;
    return ake::align_up(static_cast<size_t>(recordings) * static_cast<size_t>(frames) * kProfFolded * sizeof(double), 256);
}

int ake_profile_emissions_tuned_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int frames, const int32_t* counts_dev,
                                    int window_frames, int stride_frames, int windows, const float* profiles_dev, int compression,
                                    float sharpness, const float* cents_dev, int64_t cents_rec_stride, int64_t cents_win_stride,
                                    float* chroma_out, float* emissions_out, int32_t* key_id_out, float* confidence_out, void* workspace,
                                    size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(mel_dev && profiles_dev && chroma_out && emissions_out && key_id_out && confidence_out, AKE_ERR_INVALID,
                "profile_emissions_tuned: null argument");
    AKE_REQUIRE(cents_dev, AKE_ERR_UNSUPPORTED, "profile_emissions_tuned: no cents given (ake_profile_emissions_f32 is the entry without them)");
    AKE_REQUIRE(cents_rec_stride >= 0 && cents_win_stride >= 0, AKE_ERR_INVALID, "profile_emissions_tuned: the cents' strides must not be negative");
    AKE_REQUIRE(tuned_shape_ok(recordings, frames) && pitches > 0, AKE_ERR_INVALID,
                "profile_emissions_tuned: bad shape (%d recordings, %d pitches, %d frames)", recordings, pitches, frames);
    AKE_REQUIRE(pitches % kProfFolded == 0, AKE_ERR_UNSUPPORTED, "profile_emissions_tuned: %d bins are no multiple of 36 (whole octaves of 3 bins per semitone)", pitches);
    AKE_REQUIRE(static_cast<long long>(pitches) * frames <= (1ll << 31) - 1, AKE_ERR_INVALID, "profile_emissions_tuned: %d x %d is too large", pitches, frames);
    AKE_REQUIRE(compression >= 0 && compression <= 2, AKE_ERR_INVALID, "profile_emissions_tuned: compression %d is none of 0 (log), 1 (magnitude), 2 (power)", compression);
    AKE_REQUIRE(sharpness > 0.0f, AKE_ERR_INVALID, "profile_emissions_tuned: sharpness must be positive (and not NaN)");
    AKE_REQUIRE(window_frames >= 0 && stride_frames >= 1, AKE_ERR_INVALID, "profile_emissions_tuned: window_frames %d (>= 0), stride_frames %d (>= 1)",
                window_frames, stride_frames);
    const int want = ake_profile_windows(frames, window_frames, stride_frames);
    AKE_REQUIRE(windows == want, AKE_ERR_INVALID, "profile_emissions_tuned: %d windows given, ake_profile_windows says %d", windows, want);
    const size_t need = ake_profile_tuned_workspace_bytes(recordings, frames);
    AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "profile_emissions_tuned: workspace %zu < %zu bytes", workspace_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AKE_ERR_INVALID, "profile_emissions_tuned: the workspace must be 8-byte aligned");
    if (windows == 0) return AKE_OK;                              // no recording can hold a window: the outputs have no elements
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = (frames + kFoldChunk - 1) / kFoldChunk;
    ProfFoldArgs c{mel_dev, counts_dev, static_cast<double*>(workspace), pitches, frames, compression};
    const int rc = frames_major ? ake::launch("profile_fold_kernel", profile_fold_kernel<true>, dim3(chunks, recordings), dim3(kFoldThreads), 0, s, c)
                                : ake::launch("profile_fold_kernel", profile_fold_kernel<false>, dim3(chunks, recordings), dim3(kFoldThreads), 0, s, c);
    if (rc) return rc;
    ProfTunedScoreArgs f{static_cast<const double*>(workspace), counts_dev, profiles_dev, cents_dev, cents_rec_stride, cents_win_stride,
                         {chroma_out, emissions_out, key_id_out, confidence_out}, frames, window_frames, stride_frames, windows,
                         static_cast<double>(sharpness)};
    return ake::launch("profile_tuned_score_kernel", profile_tuned_score_kernel, dim3(windows, recordings), dim3(kProfScoreThreads), 0, s, f);
}

}  // extern "C"
