// Key changes to the frame: where, between the centres of two windows of a key track that carry different keys, the key changes
// (not part of the reference, which names one key per clip).  metrics.key_changes is the float64 model and the definition.
//
// One workgroup per possible boundary (window w and w + 1 of one recording).  The span's frames are scored tile by tile: 256 threads
// add the 12 pitch-class sums of 64 frames with profile.h's prof_class_sum (the bits of the offline and the streamed chroma), then a
// thread per frame forms that frame's Pearson correlation with the two keys in question, in double and unfused, and leaves their
// difference d_i in the LDS.  One thread then adds C_{i+1} = C_i + d_i in ascending i and keeps the first maximum: the definition fixes
// that order, and the span has at most kMaxSpan frames.  No atomics, no workspace: two runs give the same bits.  The span, the
// per-frame arithmetic and the scan are changes.h's, which the streamed kernel (stream_changes.hip) calls too.
#include "common.h"
#include "changes.h"

#include <cmath>

namespace {

using namespace ake_changes;

constexpr int kChgTile = 64;         // frames scored at a time

struct KeyChangesArgs {
    const float* mel;           // [recordings][pitches][frames], or [recordings][frames][pitches] (frames_major)
    const int* frame_counts;    // frames of each recording (clamped to 0..frames), or null
    const int* labels;          // [recordings][windows]
    const int* window_counts;   // windows of each recording (clamped to 0..windows and to what its frames hold), or null
    const float* profiles;      // [2][12]: minor, major, tonic first
    int* change_frame;          // [recordings][windows - 1]
    float* gain;
    float* contrast;
    int pitches, frames, windows, window_frames, stride_frames, slack_frames, compression;
};

__device__ __forceinline__ int chg_count(const int* counts, int rec, int limit) {      // profile.hip's prof_count
    if (!counts) return limit;
    const int c = counts[rec];
    return c < 0 ? 0 : (c < limit ? c : limit);
}

struct KeyChangesLds {
    double d[kMaxSpan];
    double x[kProfClasses][kChgTile];
    ChgProfileLds prof;
};

template <bool kFramesMajor>
__global__ __launch_bounds__(kChgThreads) void key_changes_kernel(KeyChangesArgs a) {
#pragma clang fp contract(off)
    __shared__ KeyChangesLds lds;
    const int rec = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const long long cell = static_cast<long long>(rec) * (a.windows - 1) + w;
    const int T = chg_count(a.frame_counts, rec, a.frames);
    const int fits = T < a.window_frames ? 0 : (T - a.window_frames) / a.stride_frames + 1;
    int n_win = chg_count(a.window_counts, rec, a.windows);
    n_win = n_win < fits ? n_win : fits;
    const int* lab = a.labels + static_cast<long long>(rec) * a.windows;
    ChgSpan span;
    if (w + 1 >= n_win || !chg_span(span, w, n_win, T, a.window_frames, a.stride_frames, a.slack_frames, [&](int v) { return lab[v]; })) {
        if (tid == 0) { a.change_frame[cell] = -1; a.gain[cell] = 0.f; a.contrast[cell] = 0.f; }      // no boundary here (the same for every thread)
        return;
    }
    const int lo = span.lo, n = span.hi - span.lo;                    // 1 .. stride_frames + 2 * slack_frames <= kMaxSpan
    if (tid < 2) chg_profile_stats(lds.prof, a.profiles, tid);        // the two profile rows' statistics, once per block
    const float* mel = a.mel + static_cast<long long>(rec) * a.pitches * a.frames;
    for (int t0 = 0; t0 < n; t0 += kChgTile) {
        // pitch-major: lanes run along the frames, which are contiguous; frames-major: along the pitch classes (profile_chroma_kernel)
        for (int item = tid; item < kChgTile * kProfClasses; item += kChgThreads) {
            const int j = kFramesMajor ? item % kProfClasses : item / kChgTile;
            const int i = kFramesMajor ? item / kProfClasses : item % kChgTile;
            const int t = lo + t0 + i;
            if (t0 + i < n)
                lds.x[j][i] = prof_class_sum(j, a.pitches, a.compression, [&](int k) {
                    return kFramesMajor ? mel[static_cast<long long>(t) * a.pitches + k] : mel[static_cast<long long>(k) * a.frames + t];
                });
        }
        __syncthreads();                                              // (the first one also publishes e and see)
        if (tid < kChgTile && t0 + tid < n) {                         // one frame's scores of the two keys
            double x[kProfClasses];
#pragma unroll
            for (int j = 0; j < kProfClasses; ++j) x[j] = lds.x[j][tid];
            lds.d[t0 + tid] = chg_frame_diff(x, span.ka, span.kb, lds.prof);
        }
        __syncthreads();
    }
    if (tid == 0) chg_scan(lds.d, span, a.stride_frames, &a.change_frame[cell], &a.gain[cell], &a.contrast[cell]);
}

}  // namespace

extern "C" {

int ake_key_changes_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int frames, const int32_t* frame_counts_dev,
                        const int32_t* labels_dev, int windows, const int32_t* window_counts_dev, int window_frames, int stride_frames,
                        int slack_frames, const float* profiles_dev, int compression, int32_t* change_frame_out, float* gain_out,
                        float* contrast_out, ake_stream_t stream) {
    AKE_REQUIRE(mel_dev && labels_dev && profiles_dev && change_frame_out && gain_out && contrast_out, AKE_ERR_INVALID,
                "key_changes: null argument");
    AKE_REQUIRE(recordings > 0 && recordings <= 65535 && pitches > 0 && frames > 0 && windows >= 0, AKE_ERR_INVALID,
                "key_changes: bad shape (%d recordings, %d pitches, %d frames, %d windows)", recordings, pitches, frames, windows);
    AKE_REQUIRE(pitches % 3 == 0, AKE_ERR_UNSUPPORTED, "key_changes: %d bins are no multiple of 3 (3 bins per semitone)", pitches);
    AKE_REQUIRE(static_cast<long long>(pitches) * frames <= (1ll << 31) - 1, AKE_ERR_INVALID, "key_changes: %d x %d is too large", pitches, frames);
    AKE_REQUIRE(compression >= 0 && compression <= 2, AKE_ERR_INVALID, "key_changes: compression %d is none of 0 (log), 1 (magnitude), 2 (power)", compression);
    AKE_REQUIRE(window_frames >= 1 && stride_frames >= 1 && slack_frames >= 0, AKE_ERR_INVALID,
                "key_changes: window_frames %d (>= 1), stride_frames %d (>= 1), slack_frames %d (>= 0)", window_frames, stride_frames, slack_frames);
    AKE_REQUIRE(static_cast<long long>(stride_frames) + 2ll * slack_frames <= kMaxSpan, AKE_ERR_UNSUPPORTED,
                "key_changes: a span of stride_frames %d + 2 * slack_frames %d frames exceeds %d", stride_frames, slack_frames, kMaxSpan);
    if (windows < 2) return AKE_OK;                                   // no pair of windows: the outputs have no elements
    KeyChangesArgs a{mel_dev, frame_counts_dev, labels_dev, window_counts_dev, profiles_dev, change_frame_out, gain_out, contrast_out,
                     pitches, frames, windows, window_frames, stride_frames, slack_frames, compression};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(windows - 1, recordings);
    return frames_major ? ake::launch("key_changes_kernel", key_changes_kernel<true>, grid, dim3(kChgThreads), 0, s, a)
                        : ake::launch("key_changes_kernel", key_changes_kernel<false>, grid, dim3(kChgThreads), 0, s, a);
}

}  // extern "C"
