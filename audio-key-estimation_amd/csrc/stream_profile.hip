// The profile method and a tuning meter on a stream of audio (KeyEstimator.stream(method="profile", tuning_meter=True); semantics in
// include/ake_hip.h): what a stream without a net keeps on the device between pushes, and the two launches that use it.
//   - per recording a ring of per-frame chroma, double [ring_frames][12], the stream's frame t in row t % ring_frames: 96 bytes a frame
//     where the net's frame cache holds 4 * pitches, and every frame's chroma is computed once, not once per window that covers it;
//   - per recording the three running sums P_0, P_1, P_2 of the tuning estimate (tuning.hip) as doubles.
// stream_frame_stats_kernel reads a push's new frames out of the transform's output once and feeds both; stream_profile_score_kernel
// scores the windows a push completed from the ring.  The arithmetic is profile.h's, which the offline kernels call too, so a stream's
// chroma and scores are ake_profile_emissions_f32's on the same frames to the bit, however the audio is cut.  All recordings advance
// in lockstep, so every count is a host integer; the device keeps none.  No atomics: every sum has one fixed order.
#include "common.h"
#include "profile.h"

#include <cmath>

namespace {

using namespace ake_profile;

constexpr int kStatsTile = 64;       // frames per tile
constexpr int kStatsThreads = 256;
constexpr int kStatsChroma = 1, kStatsTuning = 2;
constexpr int kStatsStage = 4624;    // doubles of LDS for a round's squared magnitudes: 16 frames of 288 bins, a double of padding each

__host__ __device__ inline size_t state_ring_doubles(int recordings, int ring_frames) {
    return static_cast<size_t>(recordings) * static_cast<size_t>(ring_frames) * kProfClasses;
}

struct StatsArgs {
    const float* mel;           // [recordings][pitches][mel_frames], or [recordings][mel_frames][pitches] (frames_major)
    double* ring;               // [recordings][ring_frames][12], or null: no chroma
    double* sums;               // [recordings][3], or null: no tuning
    float* cents;               // [recordings]
    float* strength;            // [recordings]
    long long frames_before;
    int pitches, mel_frames, first, n_new, ring_frames, compression;
    float min_strength;
};

// One workgroup per recording walks its new frames in tiles of kStatsTile.  A tile's chroma sums are independent and go straight to
// their ring rows; its tuning sums p_j(t) go to the LDS, and behind a barrier thread j < 3 adds them to P_j in frame order.
// A push brings two or three frames, so a p_j(t) per thread would keep nine lanes of one wave busy with 96 double expm1 each: the
// squared magnitudes are computed an element per thread instead, into the LDS, a round of kStatsStage / (pitches + 1) frames at a
// time, and the ascending-k chain of a p_j(t) then only adds.  More bins than a round holds: the chain computes them itself.  Both ways
// add the same doubles in the same order.
template <bool kFramesMajor>
__global__ __launch_bounds__(kStatsThreads) void stream_frame_stats_kernel(StatsArgs a) {
    __shared__ double p[kStatsTile][3];
    __shared__ double stage[kStatsStage];
    __shared__ double total[3];
    const int rec = blockIdx.x, tid = threadIdx.x;
    const float* mel = a.mel + static_cast<long long>(rec) * a.pitches * a.mel_frames;
    auto load = [&](int t, int k) {
        return kFramesMajor ? mel[static_cast<long long>(a.first + t) * a.pitches + k] : mel[static_cast<long long>(k) * a.mel_frames + a.first + t];
    };
    double* ring = a.ring ? a.ring + static_cast<long long>(rec) * a.ring_frames * kProfClasses : nullptr;
    // more new frames than rows: only the last ring_frames of them survive, and each row is written once
    const int ring_from = a.n_new > a.ring_frames ? a.n_new - a.ring_frames : 0;
    if (ring && a.frames_before == 0)                             // a fresh stream: the rows no frame has reached yet
        for (int i = a.n_new * kProfClasses + tid; i < a.ring_frames * kProfClasses; i += kStatsThreads) ring[i] = 0.0;
    double P = 0.0;                                               // P_tid, on the threads tid < 3
    if (a.sums && tid < 3 && a.frames_before > 0) P = a.sums[rec * 3 + tid];
    for (int t0 = 0; t0 < a.n_new; t0 += kStatsTile) {
        const int nt = a.n_new - t0 < kStatsTile ? a.n_new - t0 : kStatsTile;
        if (ring)
            for (int item = tid; item < kStatsTile * kProfClasses; item += kStatsThreads) {
                const int j = kFramesMajor ? item % kProfClasses : item / kStatsTile;
                const int t = t0 + (kFramesMajor ? item / kProfClasses : item % kStatsTile);
                if (t >= t0 + nt || t < ring_from) continue;
                const double c = prof_class_sum(j, a.pitches, a.compression, [&](int k) { return load(t, k); });
                ring[((a.frames_before + t) % a.ring_frames) * kProfClasses + j] = c;
            }
        if (a.sums) {
            const int row = a.pitches + 1;                        // (a row of the stage: odd in doubles, so frames fall on different banks)
            if (row <= kStatsStage) {
                const int per = kStatsStage / row;
                for (int r0 = 0; r0 < nt; r0 += per) {
                    const int nr = nt - r0 < per ? nt - r0 : per;
                    for (int e = tid; e < nr * a.pitches; e += kStatsThreads) {
                        const int tt = kFramesMajor ? e / a.pitches : e % nr, k = kFramesMajor ? e % a.pitches : e / nr;
                        stage[tt * row + k] = prof_add(0.0, load(t0 + r0 + tt, k), 2);
                    }
                    __syncthreads();
                    for (int item = tid; item < nr * 3; item += kStatsThreads) {
                        const int tt = item / 3, j = item % 3;
                        double s = 0.0;
                        for (int k = j; k < a.pitches; k += 3) s += stage[tt * row + k];      // ascending k
                        p[r0 + tt][j] = s;
                    }
                    __syncthreads();                              // before the next round's squares land in the stage
                }
            } else {
                for (int item = tid; item < kStatsTile * 3; item += kStatsThreads) {
                    const int j = kFramesMajor ? item % 3 : item / kStatsTile;
                    const int tt = kFramesMajor ? item / 3 : item % kStatsTile;
                    if (tt < nt) p[tt][j] = prof_power_sum(j, 3, a.pitches, [&](int k) { return load(t0 + tt, k); });
                }
                __syncthreads();
            }
            if (tid < 3)
                for (int tt = 0; tt < nt; ++tt) P += p[tt][tid];  // ascending frames
            __syncthreads();                                      // before the next tile's sums land in p
        }
    }
    if (!a.sums) return;
    if (tid < 3) { a.sums[rec * 3 + tid] = P; total[tid] = P; }
    __syncthreads();
    if (tid == 0) {                                               // tuning_finish_kernel's formulas
        const double P0 = total[0], P1 = total[1], P2 = total[2];
        const double sum = P0 + P1 + P2;
        double cents = 0.0, strength = 0.0;
        if (sum > 0.0) {
            const double re = P0 - 0.5 * (P1 + P2), im = 0.86602540378443865 * (P1 - P2);             // sqrt(3) / 2
            cents = 100.0 * atan2(im, re) / (2.0 * M_PI);
            strength = fmin(sqrt(re * re + im * im) / sum, 1.0);
        }
        if (strength < static_cast<double>(a.min_strength)) cents = 0.0;
        a.cents[rec] = static_cast<float>(cents);
        a.strength[rec] = static_cast<float>(strength);
    }
}

struct StreamScoreArgs {
    const double* ring;         // [recordings][ring_frames][12]
    const float* profiles;      // [2][12]: minor, major, tonic first
    const int* key_sig;         // [24]: the signature of every key
    ProfScoreOut out;           // [recordings][k] cells
    float* tonic;               // [recordings][k][12]
    int* tonic_id;              // [recordings][k]
    int* signature_id;          // [recordings][k]
    long long first_window;
    int k, ring_frames, window_frames, stride_frames;
    double sharpness;
};

// One block per (new window, recording): the window's frames out of the ring in ascending t, then profile_score_kernel's scoring.
__global__ __launch_bounds__(kProfScoreThreads) void stream_profile_score_kernel(StreamScoreArgs a) {
    __shared__ ProfScoreLds lds;
    const int rec = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const long long cell = static_cast<long long>(rec) * a.k + w;
    const double* ring = a.ring + static_cast<long long>(rec) * a.ring_frames * kProfClasses;
    const int key = prof_score_block(lds, true, [&](int j) {
        int row = static_cast<int>(((a.first_window + w) * a.stride_frames) % a.ring_frames);
        double s = 0.0;
        for (int t = 0; t < a.window_frames; ++t) {               // ascending t: the row index wraps
            s += ring[row * kProfClasses + j];
            if (++row == a.ring_frames) row = 0;
        }
        return s;
    }, a.profiles, a.sharpness, cell, a.out);
    if (tid < kProfClasses)
        a.tonic[cell * kProfClasses + tid] = fmaxf(static_cast<float>(a.sharpness * lds.r[tid]), static_cast<float>(a.sharpness * lds.r[kProfClasses + tid]));
    if (tid == 0) {
        a.tonic_id[cell] = key < 0 ? -1 : key % kProfClasses;
        a.signature_id[cell] = key < 0 ? -1 : a.key_sig[key];
    }
}

bool state_shape_ok(int recordings, int ring_frames) { return recordings > 0 && recordings <= 65535 && ring_frames > 0; }

}  // namespace

extern "C" {

size_t ake_stream_profile_state_bytes(int recordings, int ring_frames) {
    if (!state_shape_ok(recordings, ring_frames)) return 0;
    return ake::align_up((state_ring_doubles(recordings, ring_frames) + static_cast<size_t>(recordings) * 3) * sizeof(double), 16);
}

int ake_stream_frame_stats_f32(const float* mel_dev, int frames_major, int recordings, int pitches, int mel_frames, int first, int n_new,
                               int64_t frames_before, int ring_frames, int parts, int compression, float min_strength, void* state_dev,
                               size_t state_bytes, float* cents_out, float* strength_out, ake_stream_t stream) {
    AKE_REQUIRE(parts >= 1 && parts <= (kStatsChroma | kStatsTuning), AKE_ERR_INVALID, "stream_frame_stats: parts %d is none of 1 (chroma), 2 (tuning), 3 (both)", parts);
    const bool chroma = parts & kStatsChroma, tuning = parts & kStatsTuning;
    AKE_REQUIRE(mel_dev && state_dev && (!tuning || (cents_out && strength_out)), AKE_ERR_INVALID, "stream_frame_stats: null argument");
    AKE_REQUIRE(state_shape_ok(recordings, ring_frames) && pitches > 0 && mel_frames > 0, AKE_ERR_INVALID,
                "stream_frame_stats: bad shape (%d recordings, %d pitches, %d frames, a ring of %d)", recordings, pitches, mel_frames, ring_frames);
    AKE_REQUIRE(pitches % 3 == 0, AKE_ERR_UNSUPPORTED, "stream_frame_stats: %d bins are no multiple of 3 (3 bins per semitone)", pitches);
    AKE_REQUIRE(static_cast<long long>(pitches) * mel_frames <= (1ll << 31) - 1, AKE_ERR_INVALID, "stream_frame_stats: %d x %d is too large", pitches, mel_frames);
    AKE_REQUIRE(first >= 0 && n_new >= 0 && static_cast<long long>(first) + n_new <= mel_frames, AKE_ERR_INVALID,
                "stream_frame_stats: frames %d..%lld of a transform of %d", first, static_cast<long long>(first) + n_new, mel_frames);
    AKE_REQUIRE(frames_before >= 0 && frames_before <= (1ll << 62), AKE_ERR_INVALID, "stream_frame_stats: frames_before %lld", static_cast<long long>(frames_before));
    AKE_REQUIRE(!chroma || (compression >= 0 && compression <= 2), AKE_ERR_INVALID,
                "stream_frame_stats: compression %d is none of 0 (log), 1 (magnitude), 2 (power)", compression);
    AKE_REQUIRE(!tuning || min_strength == min_strength, AKE_ERR_INVALID, "stream_frame_stats: min_strength is NaN");
    const size_t need = ake_stream_profile_state_bytes(recordings, ring_frames);
    AKE_REQUIRE(state_bytes >= need, AKE_ERR_WORKSPACE, "stream_frame_stats: state %zu < %zu bytes", state_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 15) == 0, AKE_ERR_INVALID, "stream_frame_stats: the state must be 16-byte aligned");
    if (n_new == 0) return AKE_OK;                                // nothing is launched; the state and the two outputs stand
    double* ring = static_cast<double*>(state_dev);
    StatsArgs a{mel_dev, chroma ? ring : nullptr, tuning ? ring + state_ring_doubles(recordings, ring_frames) : nullptr, cents_out, strength_out,
                static_cast<long long>(frames_before), pitches, mel_frames, first, n_new, ring_frames, compression, min_strength};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return frames_major ? ake::launch("stream_frame_stats_kernel", stream_frame_stats_kernel<true>, dim3(recordings), dim3(kStatsThreads), 0, s, a)
                        : ake::launch("stream_frame_stats_kernel", stream_frame_stats_kernel<false>, dim3(recordings), dim3(kStatsThreads), 0, s, a);
}

int ake_stream_profile_emissions_f32(const void* state_dev, size_t state_bytes, int recordings, int ring_frames, int64_t frames,
                                     int window_frames, int stride_frames, int64_t first_window, int k, const float* profiles_dev,
                                     float sharpness, const int32_t* key_signature_dev, float* chroma_out, float* emissions_out,
                                     int32_t* key_id_out, float* confidence_out, float* tonic_out, int32_t* tonic_id_out,
                                     int32_t* signature_id_out, ake_stream_t stream) {
    AKE_REQUIRE(state_dev && profiles_dev && key_signature_dev, AKE_ERR_INVALID, "stream_profile_emissions: null argument");
    AKE_REQUIRE(state_shape_ok(recordings, ring_frames), AKE_ERR_INVALID, "stream_profile_emissions: bad shape (%d recordings, a ring of %d frames)",
                recordings, ring_frames);
    AKE_REQUIRE(window_frames >= 1 && stride_frames >= 1 && ring_frames >= window_frames, AKE_ERR_INVALID,
                "stream_profile_emissions: window_frames %d (>= 1), stride_frames %d (>= 1), ring_frames %d (>= window_frames)", window_frames,
                stride_frames, ring_frames);
    AKE_REQUIRE(k >= 0 && k <= 65535 && first_window >= 0 && frames >= 0 && frames <= (1ll << 62) && first_window <= (1ll << 31), AKE_ERR_INVALID,
                "stream_profile_emissions: %d windows from %lld on, %lld frames", k, static_cast<long long>(first_window), static_cast<long long>(frames));
    AKE_REQUIRE(sharpness > 0.0f, AKE_ERR_INVALID, "stream_profile_emissions: sharpness must be positive (and not NaN)");
    const size_t need = ake_stream_profile_state_bytes(recordings, ring_frames);
    AKE_REQUIRE(state_bytes >= need, AKE_ERR_WORKSPACE, "stream_profile_emissions: state %zu < %zu bytes", state_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 15) == 0, AKE_ERR_INVALID, "stream_profile_emissions: the state must be 16-byte aligned");
    if (k == 0) return AKE_OK;                                    // nothing is launched
    AKE_REQUIRE(chroma_out && emissions_out && key_id_out && confidence_out && tonic_out && tonic_id_out && signature_id_out, AKE_ERR_INVALID,
                "stream_profile_emissions: null output");
    // the ring holds the frames [frames - ring_frames, frames): the first window must begin in it and the last must end in it
    const long long begin = static_cast<long long>(first_window) * stride_frames;
    const long long end = (static_cast<long long>(first_window) + k - 1) * stride_frames + window_frames;
    AKE_REQUIRE(end <= frames, AKE_ERR_INVALID, "stream_profile_emissions: window %lld ends at frame %lld, the stream has %lld",
                static_cast<long long>(first_window) + k - 1, end, static_cast<long long>(frames));
    AKE_REQUIRE(begin >= frames - ring_frames, AKE_ERR_INVALID, "stream_profile_emissions: window %lld begins at frame %lld, the ring of %d holds %lld on",
                static_cast<long long>(first_window), begin, ring_frames, static_cast<long long>(frames) - ring_frames);
    StreamScoreArgs a{static_cast<const double*>(state_dev), profiles_dev, key_signature_dev, {chroma_out, emissions_out, key_id_out, confidence_out},
                      tonic_out, tonic_id_out, signature_id_out, static_cast<long long>(first_window), k, ring_frames, window_frames, stride_frames,
                      static_cast<double>(sharpness)};
    return ake::launch("stream_profile_score_kernel", stream_profile_score_kernel, dim3(k, recordings), dim3(kProfScoreThreads), 0,
                       static_cast<hipStream_t>(stream), a);
}

}  // extern "C"
