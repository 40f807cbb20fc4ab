// Tuning estimate: how far a recording sits from A4 = 440 Hz, read off its log-CQT (not part of the reference, whose librosa 0.9.2
// transform runs at tuning = 0.0 and whose net collapses each semitone's three bins as they come).
//
// The transform has 3 bins per semitone with in-tune notes on the bins k = 0 (mod 3).  With m = expm1(L) the magnitudes and P_j the sum
// of m^2 over the bins k = j (mod 3) and a recording's frames:
//     z = P_0 + P_1 e^{2 pi i / 3} + P_2 e^{4 pi i / 3},   cents = 100 arg(z) / (2 pi) in (-50, 50],   strength = |z| / (P_0 + P_1 + P_2)
// (metrics.estimate_tuning is the float64 model).  Two launches: tuning_sums_kernel reduces a tile of kTuneChunk frames of one recording
// to its three sums in double, in a fixed order; tuning_finish_kernel adds the chunks of a recording in chunk order and writes the two
// floats.  No floating-point atomics anywhere, so two runs give the same bits.  expm1 and atan2 are the double library forms: the
// estimate is a few million elements, and in double its rounding disappears beside the method's own error of about a cent.
// ake_tuning_track_f32, further down, is the same estimate over sliding windows of frames, for a tuning that drifts.
#include "common.h"

#include <cmath>

namespace {

// 256 threads on a tile of 64 frames x all bins.  Frames-major: lanes run along the bins, so 288 bins take two passes and the second
// keeps 32 of 256 lanes busy; pitch-major: lanes run along the frames, so a 76-frame clip's second chunk keeps 12 of 64.  Both are
// left as they are until the two launches have been timed (tools/tuning_bench.py): the tile is 74 KB of loads against a double expm1
// per element, and a 96-thread-multiple tiling would change the order of the sums that the tests pin.
constexpr int kTuneChunk = 64;       // frames per block
constexpr int kTuneThreads = 256;
constexpr int kTuneBinsPerSemitone = 3;

struct TuneArgs {
    const float* mel;           // [batch][pitches][frames], or [batch][frames][pitches] (frames_major)
    const int* counts;          // frames of each recording (clamped to 0..frames), or null
    double* partial;            // [batch][chunks][3]
    int pitches, frames, chunks;
};

template <bool kFramesMajor>
__global__ __launch_bounds__(kTuneThreads) void tuning_sums_kernel(TuneArgs a) {
    __shared__ double red[kTuneThreads][3];
    const int rec = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    int T = a.frames;
    if (a.counts) { const int c = a.counts[rec]; T = c < 0 ? 0 : (c < T ? c : T); }
    const int t0 = chunk * kTuneChunk;
    const int t1 = t0 + kTuneChunk < T ? t0 + kTuneChunk : T;
    const float* mel = a.mel + static_cast<long long>(rec) * a.pitches * a.frames;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (kFramesMajor) {                                           // lanes along the bins, which are contiguous
        for (int t = t0; t < t1; ++t)
            for (int k = tid; k < a.pitches; k += kTuneThreads) {
                const double m = expm1(static_cast<double>(mel[static_cast<long long>(t) * a.pitches + k])), v = m * m;
                const int j = k % kTuneBinsPerSemitone;
                s0 += j == 0 ? v : 0.0; s1 += j == 1 ? v : 0.0; s2 += j == 2 ? v : 0.0;
            }
    } else {                                                      // lanes along the frames, one wave per bin row
        const int t = t0 + (tid & 63);
        if (t < t1)
            for (int k = tid >> 6; k < a.pitches; k += kTuneThreads / 64) {
                const double m = expm1(static_cast<double>(mel[static_cast<long long>(k) * a.frames + t])), v = m * m;
                const int j = k % kTuneBinsPerSemitone;
                s0 += j == 0 ? v : 0.0; s1 += j == 1 ? v : 0.0; s2 += j == 2 ? v : 0.0;
            }
    }
    red[tid][0] = s0; red[tid][1] = s1; red[tid][2] = s2;
    __syncthreads();
    for (int half = kTuneThreads / 2; half > 0; half >>= 1) {     // a fixed tree: the same order of additions every run
        if (tid < half)
            for (int j = 0; j < 3; ++j) red[tid][j] += red[tid + half][j];
        __syncthreads();
    }
    if (tid < 3) a.partial[(static_cast<long long>(rec) * a.chunks + chunk) * 3 + tid] = red[0][tid];
}

struct TuneFinishArgs {
    const double* partial;
    float* cents;
    float* strength;
    int batch, chunks;
    float min_strength;
};

__global__ __launch_bounds__(64) void tuning_finish_kernel(TuneFinishArgs a) {
    const int rec = blockIdx.x * 64 + threadIdx.x;
    if (rec >= a.batch) return;
    double P[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < a.chunks; ++c)                            // chunk order
        for (int j = 0; j < 3; ++j) P[j] += a.partial[(static_cast<long long>(rec) * a.chunks + c) * 3 + j];
    const double total = P[0] + P[1] + P[2];
    double cents = 0.0, strength = 0.0;
    if (total > 0.0) {
        const double re = P[0] - 0.5 * (P[1] + P[2]), im = 0.86602540378443865 * (P[1] - P[2]);      // sqrt(3) / 2
        cents = 100.0 * atan2(im, re) / (2.0 * M_PI);
        strength = fmin(sqrt(re * re + im * im) / total, 1.0);
    }
    if (strength < static_cast<double>(a.min_strength)) cents = 0.0;
    a.cents[rec] = static_cast<float>(cents);
    a.strength[rec] = static_cast<float>(strength);
}

bool tune_shape_ok(int batch, int frames) { return batch > 0 && batch <= 65535 && frames > 0; }
int tune_chunks(int frames) { return (frames + kTuneChunk - 1) / kTuneChunk; }

// ---- the tuning track: the same estimate over sliding windows of frames, and the curve a retuner follows (ake_tuning_track_f32) ----
// Three launches.  tuning_frame_sums_kernel writes every frame's three sums p_j(t) once, in double (zeros at and behind a recording's
// count), whatever number of windows overlap it.  tuning_windows_kernel gives a thread to every (recording, window): it adds the
// window's frames in ascending order and evaluates tuning_finish_kernel's formulas.  tuning_curve_kernel gives a thread to every
// recording and walks its windows in order: hold over weak windows, unwrap, clamp.  Fixed orders everywhere, no atomics.
// Workspace: double [batch][frames][3], then double [batch][windows][2] (cents and strength before they are rounded: the curve's
// decisions are made on the doubles).
struct TrackSumsArgs {
    const float* mel;
    const int* counts;
    double* frame_sums;         // [batch][frames][3]
    int pitches, frames;
};

template <bool kFramesMajor>
__global__ __launch_bounds__(kTuneThreads) void tuning_frame_sums_kernel(TrackSumsArgs a) {
    __shared__ double red[kTuneThreads / 64][64][3];
    const int rec = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int T = a.frames;
    if (a.counts) { const int c = a.counts[rec]; T = c < 0 ? 0 : (c < T ? c : T); }
    const int t0 = blockIdx.x * kTuneChunk;
    const float* mel = a.mel + static_cast<long long>(rec) * a.pitches * a.frames;
    double* out = a.frame_sums + static_cast<long long>(rec) * a.frames * 3;
    if (kFramesMajor) {                                           // a wave per frame, lanes along the bins, which are contiguous
        for (int f = wave; f < kTuneChunk; f += kTuneThreads / 64) {
            const int t = t0 + f;
            if (t >= a.frames) break;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            if (t < T)
                for (int k = lane; k < a.pitches; k += 64) {
                    const double m = expm1(static_cast<double>(mel[static_cast<long long>(t) * a.pitches + k])), v = m * m;
                    const int j = k % kTuneBinsPerSemitone;
                    s0 += j == 0 ? v : 0.0; s1 += j == 1 ? v : 0.0; s2 += j == 2 ? v : 0.0;
                }
            for (int d = 32; d > 0; d >>= 1) {                    // a fixed tree over the wave
                s0 += __shfl_down(s0, d, 64); s1 += __shfl_down(s1, d, 64); s2 += __shfl_down(s2, d, 64);
            }
            if (lane == 0) { out[t * 3ll + 0] = s0; out[t * 3ll + 1] = s1; out[t * 3ll + 2] = s2; }
        }
    } else {                                                      // lanes along the frames, the four waves share the bin rows
        const int t = t0 + lane;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (t < T)
            for (int k = wave; k < a.pitches; k += kTuneThreads / 64) {
                const double m = expm1(static_cast<double>(mel[static_cast<long long>(k) * a.frames + t])), v = m * m;
                const int j = k % kTuneBinsPerSemitone;
                s0 += j == 0 ? v : 0.0; s1 += j == 1 ? v : 0.0; s2 += j == 2 ? v : 0.0;
            }
        red[wave][lane][0] = s0; red[wave][lane][1] = s1; red[wave][lane][2] = s2;
        __syncthreads();
        if (tid < 64 * 3) {
            const int f = tid / 3, j = tid % 3;
            if (t0 + f < a.frames) {
                double s = 0.0;
                for (int w = 0; w < kTuneThreads / 64; ++w) s += red[w][f][j];      // wave order
                out[(t0 + f) * 3ll + j] = s;
            }
        }
    }
}

struct TrackWindowsArgs {
    const double* frame_sums;   // [batch][frames][3]
    const int* counts;
    double* window_vals;        // [batch][windows][2]: cents, strength
    float* cents_raw;           // [batch][windows]
    float* strength;
    float* curve;
    int* window_counts;         // [batch]
    int batch, frames, windows, window_frames, stride_frames;
    float min_strength;
};

__device__ __forceinline__ int track_window_count(int T, int wf, int sf) { return T <= 0 ? 0 : (T < wf ? 1 : 1 + (T - wf) / sf); }

__global__ __launch_bounds__(64) void tuning_windows_kernel(TrackWindowsArgs a) {
    const int rec = blockIdx.y, w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.windows) return;
    int T = a.frames;
    if (a.counts) { const int c = a.counts[rec]; T = c < 0 ? 0 : (c < T ? c : T); }
    double cents = 0.0, strength = 0.0;
    if (w < track_window_count(T, a.window_frames, a.stride_frames)) {
        const long long f0 = static_cast<long long>(w) * a.stride_frames;
        const long long f1 = f0 + a.window_frames < T ? f0 + a.window_frames : T;
        const double* p = a.frame_sums + static_cast<long long>(rec) * a.frames * 3;
        double P[3] = {0.0, 0.0, 0.0};
        for (long long t = f0; t < f1; ++t)                       // frame order
            for (int j = 0; j < 3; ++j) P[j] += p[t * 3 + j];
        const double total = P[0] + P[1] + P[2];
        if (total > 0.0) {
            const double re = P[0] - 0.5 * (P[1] + P[2]), im = 0.86602540378443865 * (P[1] - P[2]);
            cents = 100.0 * atan2(im, re) / (2.0 * M_PI);
            strength = fmin(sqrt(re * re + im * im) / total, 1.0);
        }
    }
    const long long at = static_cast<long long>(rec) * a.windows + w;
    a.window_vals[at * 2] = cents; a.window_vals[at * 2 + 1] = strength;
    a.cents_raw[at] = static_cast<float>(cents);
    a.strength[at] = static_cast<float>(strength);
}

__global__ __launch_bounds__(64) void tuning_curve_kernel(TrackWindowsArgs a) {
    const int rec = blockIdx.x * 64 + threadIdx.x;
    if (rec >= a.batch) return;
    int T = a.frames;
    if (a.counts) { const int c = a.counts[rec]; T = c < 0 ? 0 : (c < T ? c : T); }
    const int n = track_window_count(T, a.window_frames, a.stride_frames);
    a.window_counts[rec] = n;
    const double* v = a.window_vals + static_cast<long long>(rec) * a.windows * 2;
    float* curve = a.curve + static_cast<long long>(rec) * a.windows;
    const double floor_strength = static_cast<double>(a.min_strength);
    int first = 0;
    while (first < n && v[first * 2ll + 1] < floor_strength) ++first;
    double held = first < n ? v[first * 2ll] : 0.0, unwrapped = held, last = 0.0;
    for (int w = 0; w < a.windows; ++w) {
        if (w < n && first < n) {
            if (v[w * 2ll + 1] >= floor_strength) held = v[w * 2ll];
            unwrapped = held + 100.0 * floor((unwrapped - held) / 100.0 + 0.5);       // within 50 of the value before it
            last = fmin(fmax(unwrapped, -50.0), 50.0);
        }
        curve[w] = static_cast<float>(last);                      // behind the count: the last valid value
    }
}

bool track_geometry_ok(int wf, int sf) { return wf >= 1 && sf >= 1; }
size_t track_sums_bytes(int batch, int frames) { return ake::align_up(static_cast<size_t>(batch) * frames * 3 * sizeof(double), 256); }

}  // namespace

extern "C" {

size_t ake_tuning_workspace_bytes(int batch, int frames) {
    if (!tune_shape_ok(batch, frames)) return 0;
    return ake::align_up(static_cast<size_t>(batch) * tune_chunks(frames) * 3 * sizeof(double), 256);
}

int ake_tuning_estimate_f32(const float* mel_dev, int frames_major, int batch, int pitches, int frames, const int32_t* counts_dev,
                            float min_strength, float* cents_dev, float* strength_dev, void* workspace, size_t workspace_bytes,
                            ake_stream_t stream) {
    AKE_REQUIRE(mel_dev && cents_dev && strength_dev, AKE_ERR_INVALID, "tuning_estimate: null argument");
    AKE_REQUIRE(tune_shape_ok(batch, frames) && pitches > 0, AKE_ERR_INVALID, "tuning_estimate: bad shape (%d recordings, %d pitches, %d frames)",
                batch, pitches, frames);
    AKE_REQUIRE(pitches % kTuneBinsPerSemitone == 0, AKE_ERR_UNSUPPORTED, "tuning_estimate: %d bins are no multiple of 3 (3 bins per semitone)", pitches);
    AKE_REQUIRE(static_cast<long long>(pitches) * frames <= (1ll << 31) - 1, AKE_ERR_INVALID, "tuning_estimate: %d x %d is too large", pitches, frames);
    AKE_REQUIRE(min_strength == min_strength, AKE_ERR_INVALID, "tuning_estimate: min_strength is NaN");
    const size_t need = ake_tuning_workspace_bytes(batch, frames);
    AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "tuning_estimate: workspace %zu < %zu bytes", workspace_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AKE_ERR_INVALID, "tuning_estimate: the workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = tune_chunks(frames);
    TuneArgs a{mel_dev, counts_dev, static_cast<double*>(workspace), pitches, frames, chunks};
    const int rc = frames_major ? ake::launch("tuning_sums_kernel", tuning_sums_kernel<true>, dim3(chunks, batch), dim3(kTuneThreads), 0, s, a)
                                : ake::launch("tuning_sums_kernel", tuning_sums_kernel<false>, dim3(chunks, batch), dim3(kTuneThreads), 0, s, a);
    if (rc) return rc;
    TuneFinishArgs f{static_cast<const double*>(workspace), cents_dev, strength_dev, batch, chunks, min_strength};
    return ake::launch("tuning_finish_kernel", tuning_finish_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, f);
}

int ake_tuning_track_windows(int frames, int window_frames, int stride_frames) {
    if (frames < 0 || !track_geometry_ok(window_frames, stride_frames)) return -1;
    return frames == 0 ? 0 : (frames < window_frames ? 1 : 1 + (frames - window_frames) / stride_frames);
}

size_t ake_tuning_track_workspace_bytes(int batch, int frames, int window_frames, int stride_frames) {
    if (!tune_shape_ok(batch, frames) || !track_geometry_ok(window_frames, stride_frames)) return 0;
    const size_t windows = static_cast<size_t>(ake_tuning_track_windows(frames, window_frames, stride_frames));
    return track_sums_bytes(batch, frames) + ake::align_up(static_cast<size_t>(batch) * windows * 2 * sizeof(double), 256);
}

int ake_tuning_track_f32(const float* mel_dev, int frames_major, int batch, int pitches, int frames, const int32_t* counts_dev,
                         int window_frames, int stride_frames, float min_strength, float* cents_raw_dev, float* strength_dev,
                         float* curve_dev, int32_t* window_counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(mel_dev && cents_raw_dev && strength_dev && curve_dev && window_counts_dev, AKE_ERR_INVALID, "tuning_track: null argument");
    AKE_REQUIRE(tune_shape_ok(batch, frames) && pitches > 0, AKE_ERR_INVALID, "tuning_track: bad shape (%d recordings, %d pitches, %d frames)",
                batch, pitches, frames);
    AKE_REQUIRE(pitches % kTuneBinsPerSemitone == 0, AKE_ERR_UNSUPPORTED, "tuning_track: %d bins are no multiple of 3 (3 bins per semitone)", pitches);
    AKE_REQUIRE(static_cast<long long>(pitches) * frames <= (1ll << 31) - 1, AKE_ERR_INVALID, "tuning_track: %d x %d is too large", pitches, frames);
    AKE_REQUIRE(track_geometry_ok(window_frames, stride_frames), AKE_ERR_INVALID, "tuning_track: bad geometry (windows of %d frames, %d apart)",
                window_frames, stride_frames);
    AKE_REQUIRE(min_strength == min_strength, AKE_ERR_INVALID, "tuning_track: min_strength is NaN");
    const size_t need = ake_tuning_track_workspace_bytes(batch, frames, window_frames, stride_frames);
    AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "tuning_track: workspace %zu < %zu bytes", workspace_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AKE_ERR_INVALID, "tuning_track: the workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int windows = ake_tuning_track_windows(frames, window_frames, stride_frames);
    double* frame_sums = static_cast<double*>(workspace);
    double* window_vals = reinterpret_cast<double*>(static_cast<char*>(workspace) + track_sums_bytes(batch, frames));
    TrackSumsArgs a{mel_dev, counts_dev, frame_sums, pitches, frames};
    const dim3 grid(tune_chunks(frames), batch);
    int rc = frames_major ? ake::launch("tuning_frame_sums_kernel", tuning_frame_sums_kernel<true>, grid, dim3(kTuneThreads), 0, s, a)
                          : ake::launch("tuning_frame_sums_kernel", tuning_frame_sums_kernel<false>, grid, dim3(kTuneThreads), 0, s, a);
    if (rc) return rc;
    TrackWindowsArgs w{frame_sums, counts_dev, window_vals, cents_raw_dev, strength_dev, curve_dev, window_counts_dev, batch, frames, windows,
                       window_frames, stride_frames, min_strength};
    rc = ake::launch("tuning_windows_kernel", tuning_windows_kernel, dim3((windows + 63) / 64, batch), dim3(64), 0, s, w);
    if (rc) return rc;
    return ake::launch("tuning_curve_kernel", tuning_curve_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, w);
}

}  // extern "C"
