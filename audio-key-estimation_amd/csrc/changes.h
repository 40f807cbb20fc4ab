// The arithmetic of a key change's placement, shared by the offline kernel (changes.hip) and the streamed one (stream_changes.hip): the
// span of a boundary, a frame's score difference between the two keys in question, and the ordered scan that picks the change frame.
// Both kernels call these functions instead of restating them, so that a boundary comes out with the same bits whether its frames are
// read from a whole recording's log-CQT or from a stream's chroma ring.  metrics.key_changes is the float64 model and the definition.
#pragma once

#include "profile.h"

#include <cmath>

namespace ake_changes {

using namespace ake_profile;

constexpr int kMaxSpan = 1024;       // stride_frames + 2 * slack_frames at most: the d_i of one span, 8 KB of the LDS
constexpr int kChgThreads = 256;

// The two profile rows, centred, and their squared norms: what every frame of a span is correlated with.
struct ChgProfileLds {
    double e[2][kProfClasses], see[2];
};

// Called by the threads mode = 0, 1 of a block, once; a barrier stands between this and the first chg_frame_diff.
__device__ __forceinline__ void chg_profile_stats(ChgProfileLds& s, const float* profiles, int mode) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int i = 0; i < kProfClasses; ++i) sum += static_cast<double>(profiles[mode * kProfClasses + i]);
    const double mean = sum / 12.0;
    double ss = 0.0;
    for (int i = 0; i < kProfClasses; ++i) {
        const double v = static_cast<double>(profiles[mode * kProfClasses + i]) - mean;
        s.e[mode][i] = v;
        ss += v * v;
    }
    s.see[mode] = ss;
}

struct ChgSpan {
    int ka, kb;                 // the keys of the windows w and w + 1
    int m0, lo, hi;             // window w's centre frame; the span's frames lo .. hi - 1
};

// Boundary w of a recording with T frames and n_win windows (w + 1 < n_win, and window w + 1 lies inside the T frames, so
// lo < hi <= T), lab(v) the label of window v: false where the two windows do not carry two different keys.  The span: the slack on
// either side of the two centres, clipped where the neighbouring window ends another run.
template <typename Label>
__device__ __forceinline__ bool chg_span(ChgSpan& s, int w, int n_win, int T, int window_frames, int stride_frames, int slack_frames, Label lab) {
    s.ka = lab(w);
    s.kb = lab(w + 1);
    if (s.ka < 0 || s.kb < 0 || s.ka >= kProfKeys || s.kb >= kProfKeys || s.ka == s.kb) return false;
    s.m0 = w * stride_frames + window_frames / 2;
    const int m1 = s.m0 + stride_frames;
    s.lo = s.m0 - slack_frames > 0 ? s.m0 - slack_frames : 0;
    s.hi = m1 + slack_frames < T ? m1 + slack_frames : T;
    if (w >= 1 && lab(w - 1) != s.ka && s.lo < s.m0) s.lo = s.m0;
    if (w + 2 < n_win && lab(w + 2) != s.kb && s.hi > m1) s.hi = m1;
    return true;                                                      // hi - lo in 1 .. stride_frames + 2 * slack_frames <= kMaxSpan
}

// One frame's d = r_a - r_b from its 12 class sums x (overwritten): prof_score_block's arithmetic for the two keys, in double and
// unfused.  A silent frame scores 0 for every key.
__device__ __forceinline__ double chg_frame_diff(double (&x)[kProfClasses], int ka, int kb, const ChgProfileLds& s) {
#pragma clang fp contract(off)
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kProfClasses; ++j) sum += x[j];
    const double mean = sum / 12.0;
    double sxx = 0.0;
#pragma unroll
    for (int j = 0; j < kProfClasses; ++j) { x[j] = x[j] - mean; sxx += x[j] * x[j]; }
    double diff = 0.0;
    if (!(sxx <= kProfSilence * 12.0 * mean * mean)) {
        double r[2];
        for (int side = 0; side < 2; ++side) {
            const int key = side == 0 ? ka : kb, mode = key / kProfClasses, tonic = key % kProfClasses;
            double num = 0.0;
#pragma unroll
            for (int j = 0; j < kProfClasses; ++j) num += x[j] * s.e[mode][(j - tonic + kProfClasses) % kProfClasses];
            const double den = sqrt(sxx * s.see[mode]);
            r[side] = den > 0.0 ? num / den : 0.0;
        }
        diff = r[0] - r[1];
    }
    return diff;
}

// One thread: C_{i+1} = C_i + d_i in ascending i over the span's n = hi - lo differences, the first maximum, and the three outputs.
// g is where the grid puts this boundary (KeyTrack.segments without refinement), inside the span.
__device__ __forceinline__ void chg_scan(const double* d, const ChgSpan& s, int stride_frames, int* change_frame, float* gain, float* contrast) {
#pragma clang fp contract(off)
    const int n = s.hi - s.lo;
    int g = s.m0 + (stride_frames + 1) / 2;
    g = g < s.lo ? s.lo : (g > s.hi ? s.hi : g);
    double c = 0.0, best = 0.0, at_g = 0.0;
    int j_best = 0;
    for (int i = 0; i < n; ++i) {
        c += d[i];
        if (c > best) { best = c; j_best = i + 1; }
        if (i + 1 == g - s.lo) at_g = c;
    }
    *change_frame = s.lo + j_best;
    *gain = static_cast<float>(best - at_g);
    *contrast = static_cast<float>((2.0 * best - c) / static_cast<double>(n));
}

}  // namespace ake_changes
