// Key changes to the frame inside a key stream (KeyEstimator.stream(refine=True); semantics in include/ake_hip.h): the streamed twin of
// changes.hip's key_changes_kernel.  metrics.stream_key_changes is the float64 model; joined over a stream's calls the outputs are
// ake_key_changes_f32's on the joined frames and labels, to the bit.
//
// The frames come out of the chroma ring that stream_frame_stats_kernel (stream_profile.hip) keeps: 12 doubles a frame, the very class
// sums key_changes_kernel forms from the log-CQT, since both go through profile.h's prof_class_sum.  So this kernel does not touch the
// transform: 96 bytes a frame instead of 4 * pitches.  The labels of the windows decided in earlier calls come out of a carried ring of
// its own, int32 [recordings][label_ring], window v in slot v % label_ring.  All recordings advance in lockstep, so every count is a
// host integer; the device keeps none.
//
// One launch, stream_key_changes_kernel, a workgroup per (new boundary, recording).  The span, a frame's score difference and the
// ordered scan are changes.h's, which key_changes_kernel calls too.  The span has at most kMaxSpan = 1024 frames and no class sums are
// left to compute, so all of it is scored in one pass, a frame per thread in at most four rounds, a thread's six 16-byte loads of its
// ring row issued together; one thread then adds C_{i+1} = C_i + d_i in ascending i.
//
// The label ring is written in the same launch, by the first workgroup of every recording (alone where a call brings labels but
// completes no boundary), and it is sized so that the slots cannot meet: the entry refuses a call whose new labels would land in a slot
// that one of its boundaries still reads from the ring (label_ring >= the labels carried + the call's new ones,
// metrics.stream_changes_labels_carried), so no workgroup reads what another writes and no second launch is needed.  No atomics, no
// workspace: reruns are bit-identical.
#include "common.h"
#include "changes.h"

#include <cmath>

namespace {

using namespace ake_changes;

struct StreamChangesArgs {
    const double* ring;         // [recordings][ring_frames][12]: the chroma state of ake_stream_frame_stats_f32, read only
    const int* new_labels;      // [recordings][k]: the windows labels_before .. labels_before + k - 1
    const float* profiles;      // [2][12]: minor, major, tonic first
    int* label_state;           // [recordings][label_ring]
    int* change_frame;          // [recordings][n_boundaries]
    float* gain;
    float* contrast;
    int frames, ring_frames, k, labels_before, label_ring, first_boundary, n_boundaries;
    int window_frames, stride_frames, slack_frames;
};

struct StreamChangesLds {
    double d[kMaxSpan];
    ChgProfileLds prof;
};

__global__ __launch_bounds__(kChgThreads) void stream_key_changes_kernel(StreamChangesArgs a) {
#pragma clang fp contract(off)
    __shared__ StreamChangesLds lds;
    const int rec = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    int* state = a.label_state + static_cast<long long>(rec) * a.label_ring;
    const int* fresh = a.new_labels + static_cast<long long>(rec) * a.k;
    if (b == 0) {
        // the call's labels into their slots (k <= label_ring, and none of them a slot this launch reads: the entry's checks); a fresh
        // stream writes every slot, so what the state held before never matters
        if (a.labels_before == 0)
            for (int slot = tid; slot < a.label_ring; slot += kChgThreads) state[slot] = slot < a.k ? fresh[slot] : -1;
        else
            for (int i = tid; i < a.k; i += kChgThreads) state[(a.labels_before + i) % a.label_ring] = fresh[i];
    }
    if (b >= a.n_boundaries) return;                                  // (a call without a boundary: the one workgroup that wrote the labels)
    const long long cell = static_cast<long long>(rec) * a.n_boundaries + b;
    const int w = a.first_boundary + b;
    // every window decided so far lies inside the frames so far (the entry's check), and where the stream goes on, window w + 2 is
    // decided and frame m_{w+1} + slack has arrived: the span is the one the whole recording's counts give
    const int n_win = a.labels_before + a.k;
    ChgSpan span;
    const bool there = chg_span(span, w, n_win, a.frames, a.window_frames, a.stride_frames, a.slack_frames,
                                [&](int v) { return v >= a.labels_before ? fresh[v - a.labels_before] : state[v % a.label_ring]; });
    if (!there) {                                                     // no boundary here (the same for every thread)
        if (tid == 0) { a.change_frame[cell] = -1; a.gain[cell] = 0.f; a.contrast[cell] = 0.f; }
        return;
    }
    const int n = span.hi - span.lo;                                  // 1 .. stride_frames + 2 * slack_frames <= kMaxSpan
    if (tid < 2) chg_profile_stats(lds.prof, a.profiles, tid);        // the two profile rows' statistics, once per block
    __syncthreads();
    const double2* ring = reinterpret_cast<const double2*>(a.ring + static_cast<long long>(rec) * a.ring_frames * kProfClasses);
    for (int i = tid; i < n; i += kChgThreads) {                      // a frame per thread; a row is 96 bytes, 16-byte aligned
        const double2* row = ring + static_cast<long long>((span.lo + i) % a.ring_frames) * (kProfClasses / 2);
        double2 v[kProfClasses / 2];
#pragma unroll
        for (int q = 0; q < kProfClasses / 2; ++q) v[q] = row[q];     // the six loads go out before the first is used
        double x[kProfClasses];
#pragma unroll
        for (int q = 0; q < kProfClasses / 2; ++q) { x[2 * q] = v[q].x; x[2 * q + 1] = v[q].y; }
        lds.d[i] = chg_frame_diff(x, span.ka, span.kb, lds.prof);
    }
    __syncthreads();
    if (tid == 0) chg_scan(lds.d, span, a.stride_frames, &a.change_frame[cell], &a.gain[cell], &a.contrast[cell]);
}

bool label_shape_ok(int recordings, int label_ring) { return recordings > 0 && recordings <= 65535 && label_ring > 0; }

}  // namespace

extern "C" {

size_t ake_stream_key_changes_state_bytes(int recordings, int label_ring) {
    if (!label_shape_ok(recordings, label_ring)) return 0;
    return ake::align_up(static_cast<size_t>(recordings) * static_cast<size_t>(label_ring) * sizeof(int32_t), 16);
}

int ake_stream_key_changes_f32(const void* chroma_state_dev, size_t chroma_state_bytes, int recordings, int ring_frames, int64_t frames,
                               const int32_t* labels_dev, int k, int64_t labels_before, int flush, int window_frames, int stride_frames,
                               int slack_frames, const float* profiles_dev, void* label_state_dev, size_t label_state_bytes, int label_ring,
                               int64_t first_boundary, int n_boundaries, int32_t* change_frame_out, float* gain_out, float* contrast_out,
                               ake_stream_t stream) {
    AKE_REQUIRE(chroma_state_dev && profiles_dev && label_state_dev, AKE_ERR_INVALID, "stream_key_changes: null argument");
    AKE_REQUIRE(label_shape_ok(recordings, label_ring) && ring_frames > 0, AKE_ERR_INVALID,
                "stream_key_changes: bad shape (%d recordings, a ring of %d frames, a ring of %d labels)", recordings, ring_frames, label_ring);
    AKE_REQUIRE(window_frames >= 1 && stride_frames >= 1 && slack_frames >= 0, AKE_ERR_INVALID,
                "stream_key_changes: window_frames %d (>= 1), stride_frames %d (>= 1), slack_frames %d (>= 0)", window_frames, stride_frames, slack_frames);
    AKE_REQUIRE(k >= 0 && k <= 65535 && n_boundaries >= 0 && n_boundaries <= 65535 && first_boundary >= 0 && labels_before >= 0 && frames >= 0 &&
                    frames <= (1ll << 30) && labels_before <= (1ll << 30) && first_boundary <= (1ll << 30),
                AKE_ERR_INVALID, "stream_key_changes: %d labels behind %lld, %d boundaries from %lld on, %lld frames", k,
                static_cast<long long>(labels_before), n_boundaries, static_cast<long long>(first_boundary), static_cast<long long>(frames));
    AKE_REQUIRE(static_cast<long long>(stride_frames) + 2ll * slack_frames <= kMaxSpan, AKE_ERR_UNSUPPORTED,
                "stream_key_changes: a span of stride_frames %d + 2 * slack_frames %d frames exceeds %d", stride_frames, slack_frames, kMaxSpan);
    const size_t need_chroma = ake_stream_profile_state_bytes(recordings, ring_frames), need = ake_stream_key_changes_state_bytes(recordings, label_ring);
    AKE_REQUIRE(chroma_state_bytes >= need_chroma, AKE_ERR_WORKSPACE, "stream_key_changes: chroma state %zu < %zu bytes", chroma_state_bytes, need_chroma);
    AKE_REQUIRE(label_state_bytes >= need, AKE_ERR_WORKSPACE, "stream_key_changes: label state %zu < %zu bytes", label_state_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(chroma_state_dev) & 15) == 0, AKE_ERR_INVALID, "stream_key_changes: the chroma state must be 16-byte aligned");
    if (k == 0 && n_boundaries == 0) return AKE_OK;                   // nothing is launched; the state stands
    AKE_REQUIRE(k == 0 || labels_dev, AKE_ERR_INVALID, "stream_key_changes: null labels");
    AKE_REQUIRE(n_boundaries == 0 || (change_frame_out && gain_out && contrast_out), AKE_ERR_INVALID, "stream_key_changes: null output");
    // ---- the readiness rule (metrics.stream_changes_ready) on the host's counts ----
    const long long L = labels_before + k, sf = stride_frames, wf = window_frames, half = window_frames / 2;
    AKE_REQUIRE(L == 0 || (L - 1) * sf + wf <= frames, AKE_ERR_INVALID, "stream_key_changes: window %lld ends at frame %lld, the stream has %lld",
                L - 1, (L - 1) * sf + wf, static_cast<long long>(frames));
    AKE_REQUIRE(k <= label_ring, AKE_ERR_INVALID, "stream_key_changes: %d new labels into a ring of %d", k, label_ring);
    if (n_boundaries > 0) {
        const long long last = first_boundary + n_boundaries - 1;
        AKE_REQUIRE(flush ? last + 1 < L : last + 2 < L, AKE_ERR_INVALID,
                    "stream_key_changes: boundary %lld needs the label of window %lld, and %lld windows are decided", last, last + (flush ? 1 : 2), L);
        AKE_REQUIRE(flush || (last + 1) * sf + half + slack_frames <= frames, AKE_ERR_INVALID,
                    "stream_key_changes: boundary %lld reads up to frame %lld, the stream has %lld", last, (last + 1) * sf + half + slack_frames,
                    static_cast<long long>(frames));
        const long long oldest_frame = first_boundary * sf + half - slack_frames;
        AKE_REQUIRE((oldest_frame > 0 ? oldest_frame : 0) >= frames - ring_frames, AKE_ERR_INVALID,
                    "stream_key_changes: boundary %lld reads from frame %lld on, the ring of %d holds %lld on", static_cast<long long>(first_boundary),
                    oldest_frame > 0 ? oldest_frame : 0, ring_frames, static_cast<long long>(frames) - ring_frames);
        // the oldest window whose label comes out of the ring: still there, and in no slot that this call's labels go to
        const long long oldest = first_boundary > 0 ? first_boundary - 1 : 0;
        AKE_REQUIRE(oldest >= labels_before || L - oldest <= label_ring, AKE_ERR_INVALID,
                    "stream_key_changes: boundary %lld reads the label of window %lld, and a ring of %d labels cannot hold it beside the windows up to %lld",
                    static_cast<long long>(first_boundary), oldest, label_ring, L - 1);
    }
    StreamChangesArgs a{static_cast<const double*>(chroma_state_dev), labels_dev, profiles_dev, static_cast<int*>(label_state_dev), change_frame_out,
                        gain_out, contrast_out, static_cast<int>(frames), ring_frames, k, static_cast<int>(labels_before), label_ring,
                        static_cast<int>(first_boundary), n_boundaries, window_frames, stride_frames, slack_frames};
    return ake::launch("stream_key_changes_kernel", stream_key_changes_kernel, dim3(n_boundaries > 0 ? n_boundaries : 1, recordings),
                       dim3(kChgThreads), 0, static_cast<hipStream_t>(stream), a);
}

}  // extern "C"
