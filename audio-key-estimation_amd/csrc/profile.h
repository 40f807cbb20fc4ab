// The arithmetic of the key-profile method, shared by the offline kernels (profile.hip) and the streamed ones (stream_profile.hip): a
// frame's chroma sum and a window's scoring.  Both sides call these functions instead of restating them, so that a frame's chroma and a
// window's scores come out with the same bits whether the frames arrive as a whole recording or push by push.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace ake_profile {

constexpr int kProfClasses = 12;
constexpr int kProfKeys = 24;
constexpr int kProfScoreThreads = 64;
constexpr double kProfSilence = 1e-12;
constexpr int kProfBatch = 4;        // semitones (of 3 bins each) whose loads go out together

// s + v(L): v = L (compression 0), expm1(L) (1) or expm1(L)^2 (2), expm1 in its double library form.  The square is rounded before it is
// added: a multiply and an add, never a fused multiply-add, whatever loop the caller's compiler has made of the call.
__device__ __forceinline__ double prof_add(double s, float Lf, int compression) {
#pragma clang fp contract(off)
    const double L = static_cast<double>(Lf);
    double v = L;
    if (compression != 0) {
        v = expm1(L);
        if (compression == 2) v = v * v;
    }
    return s + v;
}

// The sum of v over the bins of pitch class j, in ascending k: bin k belongs to semitone (k + 1) / 3, so class j holds the bins
// 3 sem - 1 .. 3 sem + 1 of the semitones sem = j, j + 12, ... (semitone 0 lacks its flat-side bin, and the top bin is the flat side of
// a semitone above the range).  load(k) gives L[k] of the frame; the loads of kProfBatch semitones are issued before the first is used.
template <typename Load>
__device__ __forceinline__ double prof_class_sum(int j, int pitches, int compression, Load load) {
    double s = 0.0;
    for (int sem = j; 3 * sem - 1 < pitches; sem += kProfClasses * kProfBatch) {
        float L[kProfBatch][3];
#pragma unroll
        for (int g = 0; g < kProfBatch; ++g)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int k = 3 * (sem + kProfClasses * g) - 1 + q;
                L[g][q] = (k >= 0 && k < pitches) ? load(k) : 0.f;
            }
#pragma unroll
        for (int g = 0; g < kProfBatch; ++g)
#pragma unroll
            for (int q = 0; q < 3; ++q) {                         // ascending k
                const int k = 3 * (sem + kProfClasses * g) - 1 + q;
                if (k >= 0 && k < pitches) s = prof_add(s, L[g][q], compression);
            }
    }
    return s;
}

// The sum of expm1(L)^2 over the bins k = k0, k0 + step, ... below pitches, in ascending k, its loads in batches likewise.
template <typename Load>
__device__ __forceinline__ double prof_power_sum(int k0, int step, int pitches, Load load) {
    constexpr int kBatch = 3 * kProfBatch;
    double s = 0.0;
    for (int k = k0; k < pitches; k += step * kBatch) {
        float L[kBatch];
#pragma unroll
        for (int q = 0; q < kBatch; ++q) L[q] = k + q * step < pitches ? load(k + q * step) : 0.f;
#pragma unroll
        for (int q = 0; q < kBatch; ++q)
            if (k + q * step < pitches) s = prof_add(s, L[q], 2);
    }
    return s;
}

// What a scoring block keeps in the LDS.
struct ProfScoreLds {
    double x[kProfClasses], d[kProfClasses], e[2][kProfClasses], see[2], r[kProfKeys];
    double sxx, total;
    int best_k;                                                   // -1: silent, or behind the recording's windows
};

struct ProfScoreOut {
    float* chroma;              // [cells][12]
    float* emissions;           // [cells][24]
    int* key_id;                // [cells]
    float* confidence;          // [cells]
};

// One window's scoring by a block of kProfScoreThreads threads: frame_sum(j) is the window's chroma x_j (called by the threads
// j < 12 of a live window), profiles [2][12] minor and major, tonic first.  Means first, the 24 Pearson correlations in double, the
// silence rule, the first maximum on the doubles; writes the four outputs of `cell`.  Behind its last barrier s.r holds the
// correlations (zeros for a silent window); returns the key, or -1 (valid on thread 0).
template <typename FrameSum>
__device__ __forceinline__ int prof_score_block(ProfScoreLds& s, bool live, FrameSum frame_sum, const float* profiles, double sharpness,
                                                long long cell, const ProfScoreOut& out) {
    const int tid = threadIdx.x;
    if (tid < kProfClasses) {
        s.x[tid] = live ? frame_sum(tid) : 0.0;
    } else if (tid >= 32 && tid < 34) {                           // the two profile rows' statistics, once per block
        const int mode = tid - 32;
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
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int j = 0; j < kProfClasses; ++j) sum += s.x[j];
        const double mean = sum / 12.0;
        double ss = 0.0;
        for (int j = 0; j < kProfClasses; ++j) { const double v = s.x[j] - mean; s.d[j] = v; ss += v * v; }
        s.sxx = ss;
        s.total = sum;
        s.best_k = (!live || ss <= kProfSilence * 12.0 * mean * mean) ? -1 : 0;
    }
    __syncthreads();
    const bool silent = s.best_k < 0;
    if (tid < kProfKeys) {
        double rk = 0.0;
        if (!silent) {
            const int mode = tid / kProfClasses, tonic = tid % kProfClasses;
            double num = 0.0;
            for (int j = 0; j < kProfClasses; ++j) num += s.d[j] * s.e[mode][(j - tonic + kProfClasses) % kProfClasses];
            const double den = sqrt(s.sxx * s.see[mode]);
            rk = den > 0.0 ? num / den : 0.0;
        }
        s.r[tid] = rk;
    }
    __syncthreads();
    int k = -1;
    if (tid == 0) {
        double best = 0.0;
        if (!silent) {
            best = s.r[0]; k = 0;
            for (int i = 1; i < kProfKeys; ++i)
                if (s.r[i] > best) { best = s.r[i]; k = i; }      // the first maximum, on the double values
        }
        out.key_id[cell] = k;
        out.confidence[cell] = static_cast<float>(best);
    }
    if (tid < kProfKeys) out.emissions[cell * kProfKeys + tid] = static_cast<float>(sharpness * s.r[tid]);
    if (tid < kProfClasses) out.chroma[cell * kProfClasses + tid] = silent ? 0.0f : static_cast<float>(s.x[tid] / s.total);
    return k;
}

// ---- the tuned chroma (profile_tuned.hip): 36 octave-folded sums per frame, cut into 12 classes at boundaries that follow the tuning ----

constexpr int kProfFolded = 36;      // folded positions: bin k sits at k % 36
constexpr int kProfFoldBatch = 12;   // octaves whose loads go out together (12 octaves from C1 lie beyond any audio rate's range)

// The sum of v over the bins p, p + 36, ... below pitches, in ascending octave.  load(k) gives L[k] of the frame; the loads of
// kProfFoldBatch octaves are issued before the first is used.
template <typename Load>
__device__ __forceinline__ double prof_fold_sum(int p, int pitches, int compression, Load load) {
    double s = 0.0;
    for (int k = p; k < pitches; k += kProfFolded * kProfFoldBatch) {
        float L[kProfFoldBatch];
#pragma unroll
        for (int q = 0; q < kProfFoldBatch; ++q) L[q] = k + kProfFolded * q < pitches ? load(k + kProfFolded * q) : 0.f;
#pragma unroll
        for (int q = 0; q < kProfFoldBatch; ++q)
            if (k + kProfFolded * q < pitches) s = prof_add(s, L[q], compression);
    }
    return s;
}

// Where a window's cents put the class boundaries: class j holds the folded bins 3 j + n .. 3 j + n + 3 (mod 36), the first weighted
// by w0 = 1 - g, the last by w3 = g, the two between whole.  cents as the kernel receives it: NaN reads as 0, beyond +-50 as +-50.
struct ProfTunedCut {
    int n;                      // -3 .. 0
    double w0, w3;              // w0 in (0, 1], w3 in [0, 1)
};

__device__ __forceinline__ ProfTunedCut prof_tuned_cut(float cents) {
#pragma clang fp contract(off)
    double c = cents != cents ? 0.0 : static_cast<double>(cents);
    c = c < -50.0 ? -50.0 : (c > 50.0 ? 50.0 : c);
    const double u = 3.0 * c / 100.0 - 1.0;                       // delta - 1, in [-2.5, 0.5]
    const double fl = floor(u);
    const double g = u - fl;                                      // exact
    return ProfTunedCut{static_cast<int>(fl), 1.0 - g, g};
}

// x_j = ((w0 FW[b0] + FW[b1]) + FW[b2]) + w3 FW[b3], every product rounded before it is added; a term of weight 0 is not added.
__device__ __forceinline__ double prof_tuned_class(int j, const ProfTunedCut& cut, const double* fw) {
#pragma clang fp contract(off)
    const int b = 3 * j + cut.n + kProfFolded;                    // >= 33: the remainders below are those of a positive number
    const double head = cut.w0 * fw[b % kProfFolded];
    double x = head + fw[(b + 1) % kProfFolded];
    x = x + fw[(b + 2) % kProfFolded];
    if (cut.w3 != 0.0) {
        const double tail = cut.w3 * fw[(b + 3) % kProfFolded];
        x = x + tail;
    }
    return x;
}

}  // namespace ake_profile
