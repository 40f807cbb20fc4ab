// Everything PitchClassNet.general_step computes behind the forward, in ONE launch (reference: models.py:826-905 -- label
// preparation, BCE / cross-entropy losses with the genre mask and the optional cosine term -- and models.py:1065-1116, the MIREX
// categories over the 21-row key-signature table of utils/key_signatures.py:19-42), plus the gradient of the loss with respect to
// the three network outputs.  With torch ops this is ~110 tiny kernels forward and ~50 in autograd's backward per step: at the
// reference's batch size (8 clips) that was a quarter of the step, at 256 clips the host could not issue them as fast as the GPU
// finished them.  One workgroup; a thread owns whole rows (a clip's 12 + 12 + 11 outputs), sums in double, block reduction in a
// fixed order (bit-reproducible).
#include "common.h"

#include <cstdint>

namespace {

struct StepLossArgs {
    const float* key;          // [B][12] sigmoid outputs
    const float* tonic;        // [B][12] logits
    const float* genre;        // [B][11] logits, nullable
    const float* key_labels;   // [B][12]
    const void* tonic_lab;     // [B][12] one-hot, float32 or int64
    const void* genre_lab;     // [B][11] one-hot (rows that do not sum to 1 carry no genre label), nullable
    const void* sig_lab;       // [B][24] one-hot key-signature id
    int tonic_i64, genre_i64, sig_i64;
    int B;
    float key_w, tonic_w, genre_w;
    int use_cos;
    const float* weight;       // [B] sample weights >= 0, nullable (ake_general_step_weighted_f32)
    float* scalars;            // [10]: loss, accuracy, mirex, correct, fifths, relative, parallel, other, accuracy_tonic, accuracy_genre
    float* d_key;              // nullable (all three or none)
    float* d_tonic;
    float* d_genre;
};

// label element; float32 tonic / genre labels go through the reference's .long() (models.py:826, 831: truncation toward zero)
__device__ __forceinline__ double lab(const void* p, int is_i64, long long i, bool as_long = true) {
    if (is_i64) return static_cast<double>(static_cast<const long long*>(p)[i]);
    const double v = static_cast<double>(static_cast<const float*>(p)[i]);
    return as_long ? trunc(v) : v;
}

// first maximum of a one-hot row (torch.argmax on the labels, models.py:832 / :840 / :1090)
__device__ __forceinline__ int lab_argmax(const void* p, int is_i64, long long base, int n, bool as_long = true) {
    int best = 0;
    double bv = lab(p, is_i64, base, as_long);
    for (int j = 1; j < n; ++j) {
        const double v = lab(p, is_i64, base + j, as_long);
        if (v > bv) { bv = v; best = j; }
    }
    return best;
}

// tonic (pitch class of the major scale's first degree) of row k of the key-signature table: circle of fifths Cb .. C# (15 rows),
// then the six enharmonic duplicates (utils/key_signatures.py:19-42)
__device__ __forceinline__ int table_tonic(int k) {
    const int dup[6] = {9, 11, 10, 4, 3, 5};
    const int i = k < 15 ? k : dup[k - 15];
    return ((7 * (i - 7)) % 12 + 12) % 12;
}
__device__ __forceinline__ bool in_major_scale(int pc, int tonic) {
    const int d = ((pc - tonic) % 12 + 12) % 12;
    return d == 0 || d == 2 || d == 4 || d == 5 || d == 7 || d == 9 || d == 11;
}

// MIREX categories of one prediction, models.py:1065-1116: first-maximum cosine match over the 21 table rows, then the reference's
// if-chain ('fifths' first).  p: sigmoid outputs, y: key labels, pn = max(|p|, 1e-8), tok: the predicted tonic is the labelled one,
// label_id: first maximum of the 24-way key-signature row.  Adds 1 to cat[0] (all 12 key bits right) and to at most one of
// cat[1..4] = correct, fifths, relative, parallel.
__device__ __forceinline__ void mirex_row(const double* p, const double* y, double pn, bool tok, int label_id, double* cat) {
    int pred = 0;
    double best = -1e300;
    for (int k = 0; k < 21; ++k) {
        const int tk = table_tonic(k);
        double dot = 0.0;
        for (int j = 0; j < 12; ++j) dot += in_major_scale(j, tk) ? p[j] : 0.0;
        const double sim = dot / (pn * fmax(sqrt(7.0), 1e-8));
        if (sim > best) { best = sim; pred = k; }
    }
    const int tp = table_tonic(pred);
    bool full = true;
    for (int j = 0; j < 12; ++j) full = full && ((in_major_scale(j, tp) ? 1.0 : 0.0) == y[j]);
    const int diff = pred > label_id ? pred - label_id : label_id - pred;
    const bool fifths = diff == 1 && !(tok && full);
    const bool correct = tok && full && !fifths;
    const bool relative = full && !tok && !fifths;
    const bool parallel = tok && !full && !fifths;
    cat[0] += full ? 1.0 : 0.0;
    cat[1] += correct ? 1.0 : 0.0;
    cat[2] += fifths ? 1.0 : 0.0;
    cat[3] += relative ? 1.0 : 0.0;
    cat[4] += parallel ? 1.0 : 0.0;
}

constexpr int kNS = 12;        // per-thread sums: bce, ce_tonic, ce_genre (masked), genre count, genre correct, cos, tonic ok, full, correct, fifths, relative, parallel

// kWeighted: row r counts w_r = sample_weight[r] times in every sum, and the means divide by Wsum = sum_r w_r (a thirteenth sum)
// instead of B; the genre term by sum_r w_r m_r.  A row's terms are collected on their own and enter the sums as w_r * term; a row with
// w_r = 0 is not read at all.  The gradients are written as w_r * (the row's derivative) and scaled by 1 / Wsum (the genre's by its own
// denominator) after the reduction, the way the unweighted genre gradient always was.  !kWeighted is the arithmetic it always was.
template <bool kWeighted>
__global__ __launch_bounds__(256) void general_step_kernel(StepLossArgs a) {
    constexpr int NS = kWeighted ? kNS + 1 : kNS;
    __shared__ double red[NS][256];
    const int B = a.B;
    double sum[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sum[k] = 0.0;
    for (int r = threadIdx.x; r < B; r += blockDim.x) {
        double row[NS];
        double* const acc = kWeighted ? row : sum;                                 // where this row's terms are added
        double w = 1.0;
        if (kWeighted) {
            w = static_cast<double>(a.weight[r]);
            if (!(w > 0.0)) {                                                      // exact zeros, whatever the row holds
                if (a.d_key)
                    for (int j = 0; j < 12; ++j) { a.d_key[r * 12 + j] = 0.0f; a.d_tonic[r * 12 + j] = 0.0f; }
                if (a.genre && a.d_genre)
                    for (int j = 0; j < 11; ++j) a.d_genre[r * 11 + j] = 0.0f;
                continue;
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) row[k] = 0.0;
            row[kNS] = 1.0;
        }
        const double rows = kWeighted ? 1.0 / w : static_cast<double>(B);          // a gradient's divisor before the reduction
        // ---- key: BCE (log clamped at -100 as torch does), models.py:855, 878 ----
        double p[12], y[12];
        double pp = 0.0, yy = 0.0, py = 0.0;
        for (int j = 0; j < 12; ++j) {
            p[j] = static_cast<double>(a.key[r * 12 + j]);
            y[j] = static_cast<double>(a.key_labels[r * 12 + j]);
            const double lp = fmax(log(p[j]), -100.0), l1p = fmax(log1p(-p[j]), -100.0);
            acc[0] -= y[j] * lp + (1.0 - y[j]) * l1p;
            pp += p[j] * p[j]; yy += y[j] * y[j]; py += p[j] * y[j];
        }
        const double pn = fmax(sqrt(pp), 1e-8), yn = fmax(sqrt(yy), 1e-8);
        if (a.use_cos) acc[5] += py / (pn * yn);                                   // models.py:885-887
        if (a.d_key) {
            for (int j = 0; j < 12; ++j) {
                double g = a.key_w * (p[j] - y[j]) / fmax((1.0 - p[j]) * p[j], 1e-12) / (12.0 * rows);      // torch's binary_cross_entropy_backward
                if (a.use_cos) g -= (y[j] / (pn * yn) - py * p[j] / (pn * pn * pn * yn)) / rows;
                a.d_key[r * 12 + j] = static_cast<float>(g);
            }
        }
        // ---- tonic: cross entropy on the logits, models.py:856, 879 ----
        const int t_idx = lab_argmax(a.tonic_lab, a.tonic_i64, static_cast<long long>(r) * 12, 12);
        bool tok;                                                                  // the predicted tonic is the labelled one
        {
            double z[12], zmax = -1e300;
            int zarg = 0;
            for (int j = 0; j < 12; ++j) {
                z[j] = static_cast<double>(a.tonic[r * 12 + j]);
                if (z[j] > zmax) { zmax = z[j]; zarg = j; }
            }
            double se = 0.0;
            for (int j = 0; j < 12; ++j) se += exp(z[j] - zmax);
            acc[1] -= z[t_idx] - zmax - log(se);
            if (a.d_tonic)
                for (int j = 0; j < 12; ++j) a.d_tonic[r * 12 + j] = static_cast<float>(a.tonic_w * (exp(z[j] - zmax) / se - (j == t_idx ? 1.0 : 0.0)) / rows);
            tok = zarg == t_idx;
            acc[6] += tok ? 1.0 : 0.0;
        }
        // ---- genre: cross entropy over the rows that carry a label, models.py:839-840, 881-883, 892-893 ----
        if (a.genre) {
            double ls = 0.0;
            for (int j = 0; j < 11; ++j) ls += lab(a.genre_lab, a.genre_i64, static_cast<long long>(r) * 11 + j);
            const double m = ls == 1.0 ? 1.0 : 0.0;
            const int g_idx = lab_argmax(a.genre_lab, a.genre_i64, static_cast<long long>(r) * 11, 11);
            double z[11], zmax = -1e300;
            int zarg = 0;
            for (int j = 0; j < 11; ++j) {
                z[j] = static_cast<double>(a.genre[r * 11 + j]);
                if (z[j] > zmax) { zmax = z[j]; zarg = j; }
            }
            double se = 0.0;
            for (int j = 0; j < 11; ++j) se += exp(z[j] - zmax);
            acc[2] -= m * (z[g_idx] - zmax - log(se));
            acc[3] += m;
            acc[4] += m * (zarg == g_idx ? 1.0 : 0.0);
            if (a.d_genre)   // scaled by 1 / (number of labelled rows) after the reduction
                for (int j = 0; j < 11; ++j)
                    a.d_genre[r * 11 + j] = static_cast<float>(a.genre_w * (kWeighted ? w * m : m) * (exp(z[j] - zmax) / se - (j == g_idx ? 1.0 : 0.0)));
        }
        // ---- MIREX categories, models.py:1065-1116 ----
        mirex_row(p, y, pn, tok, lab_argmax(a.sig_lab, a.sig_i64, static_cast<long long>(r) * 24, 24, false), acc + 7);   // (models.py:1090: no .long())
        if (kWeighted) {
#pragma unroll
            for (int k = 0; k < NS; ++k) sum[k] += w * row[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][threadIdx.x] = sum[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w)
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
    const double cnt = red[3][0];
    const double inv_cnt = kWeighted ? (cnt > 0.0 ? 1.0 / cnt : 0.0) : 1.0 / fmax(cnt, 1.0);
    const double n = kWeighted ? red[NS - 1][0] : static_cast<double>(B);          // Wsum, or the batch
    const double inv_n = kWeighted ? (n > 0.0 ? 1.0 / n : 0.0) : 0.0;
    if (a.genre && a.d_genre)
        for (int r = threadIdx.x; r < B; r += blockDim.x)          // the rows this thread wrote above
            for (int j = 0; j < 11; ++j) a.d_genre[r * 11 + j] = static_cast<float>(static_cast<double>(a.d_genre[r * 11 + j]) * inv_cnt);
    if (kWeighted && a.d_key)
        for (int r = threadIdx.x; r < B; r += blockDim.x)
            for (int j = 0; j < 12; ++j) {
                a.d_key[r * 12 + j] = static_cast<float>(static_cast<double>(a.d_key[r * 12 + j]) * inv_n);
                a.d_tonic[r * 12 + j] = static_cast<float>(static_cast<double>(a.d_tonic[r * 12 + j]) * inv_n);
            }
    if (threadIdx.x == 0) {
        if (kWeighted && !(n > 0.0)) {                                                              // no row counts: zeros
            for (int k = 0; k < 10; ++k) a.scalars[k] = 0.0f;
            return;
        }
        double loss = a.key_w * red[0][0] / (12.0 * n) + a.tonic_w * red[1][0] / n;                 // models.py:889
        if (a.genre) loss += a.genre_w * red[2][0] * inv_cnt;                                       // an exact zero when no row carries a label (:892)
        if (a.use_cos) loss += 1.0 - red[5][0] / n;
        const double correct = red[8][0], fifths = red[9][0], relative = red[10][0], parallel = red[11][0];
        a.scalars[0] = static_cast<float>(loss);
        a.scalars[1] = static_cast<float>(red[7][0] / n);                                           // accuracy = all 12 key bits right
        a.scalars[2] = static_cast<float>((1.0 * correct + 0.5 * fifths + 0.3 * relative + 0.2 * parallel) / n);
        a.scalars[3] = static_cast<float>(correct / n);
        a.scalars[4] = static_cast<float>(fifths / n);
        a.scalars[5] = static_cast<float>(relative / n);
        a.scalars[6] = static_cast<float>(parallel / n);
        a.scalars[7] = static_cast<float>((n - correct - fifths - relative - parallel) / n);
        a.scalars[8] = static_cast<float>(red[6][0] / n);
        a.scalars[9] = static_cast<float>(a.genre ? red[4][0] * inv_cnt : 0.0);
    }
}

// ---- --local: general_step over per-frame outputs (models.py:861-876, 898-909) ----------------------------------------------------
// Clip i has T' output rows of which the first n_i are scored; its labels have R >= n_i rows.  A (chunk, clip) grid: a thread owns one
// output row, a workgroup kLocRows rows of one clip and writes its kLocNS sums (double, fixed-order LDS tree) to its own slot of the
// workspace; general_step_local_finish_kernel adds them per clip in chunk order, then over the clips in clip order.  No atomics, so the
// results are bit-reproducible.

constexpr int kLocRows = 64;   // rows (threads) per workgroup: one wave
constexpr int kLocNS = 8;      // per-clip sums: bce, ce_tonic, tonic ok (first n - 2 rows), full, correct, fifths, relative, parallel

struct StepLocalArgs {
    const float* key;          // [B][T'][12] sigmoid outputs
    const float* tonic;        // [B][T'][12] logits
    const float* key_labels;   // [B][R][12]
    const void* tonic_lab;     // [B][R][12] one-hot, float32 or int64
    const void* sig_lab;       // [B][R][24] one-hot key-signature id, float32 or int64
    const int* valid;          // [B] n_i
    int tonic_i64, sig_i64;
    int B, T, R, chunks;
    float key_w, tonic_w;
    double* part;              // [B][chunks][kLocNS] (workspace)
    float* scalars;            // [10]
    float* d_key;              // [B][T'][12], nullable (both or none)
    float* d_tonic;
};

// n_i as the kernels read it: within [0, min(T', R)] whatever the caller passed (the contract is 1 <= n_i <= min(T', R))
__device__ __forceinline__ int local_valid(const StepLocalArgs& a, int clip) {
    const int n = a.valid[clip];
    const int lim = a.T < a.R ? a.T : a.R;
    return n < 0 ? 0 : (n > lim ? lim : n);
}

__global__ __launch_bounds__(kLocRows) void general_step_local_kernel(StepLocalArgs a) {
    __shared__ double red[kLocNS][kLocRows];
    const int clip = blockIdx.y, t = blockIdx.x * kLocRows + threadIdx.x;
    const int n = local_valid(a, clip);
    double sum[kLocNS];
#pragma unroll
    for (int k = 0; k < kLocNS; ++k) sum[k] = 0.0;
    const long long o = (static_cast<long long>(clip) * a.T + t) * 12;       // output row
    const long long l = static_cast<long long>(clip) * a.R + t;             // label row
    if (t < n) {
        // ---- key: BCE over the clip's n * 12 elements (log clamped at -100 as torch does) ----
        double p[12], y[12], pp = 0.0;
        for (int j = 0; j < 12; ++j) {
            p[j] = static_cast<double>(a.key[o + j]);
            y[j] = static_cast<double>(a.key_labels[l * 12 + j]);
            const double lp = fmax(log(p[j]), -100.0), l1p = fmax(log1p(-p[j]), -100.0);
            sum[0] -= y[j] * lp + (1.0 - y[j]) * l1p;
            pp += p[j] * p[j];
        }
        if (a.d_key)
            for (int j = 0; j < 12; ++j)
                a.d_key[o + j] = static_cast<float>(a.key_w * (p[j] - y[j]) / fmax((1.0 - p[j]) * p[j], 1e-12) / (12.0 * n * a.B));
        // ---- tonic: cross entropy over the clip's n frames ----
        const int t_idx = lab_argmax(a.tonic_lab, a.tonic_i64, l * 12, 12);
        double z[12], zmax = -1e300;
        int zarg = 0;
        for (int j = 0; j < 12; ++j) {
            z[j] = static_cast<double>(a.tonic[o + j]);
            if (z[j] > zmax) { zmax = z[j]; zarg = j; }
        }
        double se = 0.0;
        for (int j = 0; j < 12; ++j) se += exp(z[j] - zmax);
        sum[1] -= z[t_idx] - zmax - log(se);
        if (a.d_tonic)
            for (int j = 0; j < 12; ++j)
                a.d_tonic[o + j] = static_cast<float>(a.tonic_w * (exp(z[j] - zmax) / se - (j == t_idx ? 1.0 : 0.0)) / (static_cast<double>(n) * a.B));
        const bool tok = zarg == t_idx;
        if (t < n - 2) sum[2] += tok ? 1.0 : 0.0;                            // the reference's seq_length - (span + 1) rows (:906)
        mirex_row(p, y, fmax(sqrt(pp), 1e-8), tok, lab_argmax(a.sig_lab, a.sig_i64, l * 24, 24, false), sum + 3);
    } else if (t < a.T && a.d_key) {
        for (int j = 0; j < 12; ++j) { a.d_key[o + j] = 0.0f; a.d_tonic[o + j] = 0.0f; }
    }
#pragma unroll
    for (int k = 0; k < kLocNS; ++k) red[k][threadIdx.x] = sum[k];
    __syncthreads();
    for (int w = kLocRows / 2; w > 0; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w)
#pragma unroll
            for (int k = 0; k < kLocNS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < kLocNS) a.part[(static_cast<long long>(clip) * a.chunks + blockIdx.x) * kLocNS + threadIdx.x] = red[threadIdx.x][0];
}

constexpr int kLocFinish = 256;

// per clip: sums over its chunks in chunk order, divided by n_i (n_i - 2 for the tonic accuracy); then the mean over the clips in clip order
__global__ __launch_bounds__(kLocFinish) void general_step_local_finish_kernel(StepLocalArgs a) {
    __shared__ double clip_val[9][kLocFinish];   // bce / (12 n), ce / n, tonic acc, accuracy, correct, fifths, relative, parallel, other
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int base = 0; base < a.B; base += kLocFinish) {
        const int clip = base + threadIdx.x;
        if (clip < a.B) {
            double s[kLocNS];
#pragma unroll
            for (int k = 0; k < kLocNS; ++k) s[k] = 0.0;
            for (int c = 0; c < a.chunks; ++c)
#pragma unroll
                for (int k = 0; k < kLocNS; ++k) s[k] += a.part[(static_cast<long long>(clip) * a.chunks + c) * kLocNS + k];
            const double n = fmax(static_cast<double>(local_valid(a, clip)), 1.0);
            const double m = static_cast<double>(local_valid(a, clip) - 2);
            clip_val[0][threadIdx.x] = s[0] / (12.0 * n);
            clip_val[1][threadIdx.x] = s[1] / n;
            clip_val[2][threadIdx.x] = m > 0.0 ? s[2] / m : 0.0;
            for (int k = 3; k < kLocNS; ++k) clip_val[k][threadIdx.x] = s[k] / n;
            clip_val[8][threadIdx.x] = (n - s[4] - s[5] - s[6] - s[7]) / n;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = a.B - base < kLocFinish ? a.B - base : kLocFinish;
            for (int c = 0; c < cnt; ++c)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[k] += clip_val[k][c];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double B = a.B;
        const double correct = acc[4] / B, fifths = acc[5] / B, relative = acc[6] / B, parallel = acc[7] / B;
        a.scalars[0] = static_cast<float>(a.key_w * (acc[0] / B) + a.tonic_w * (acc[1] / B));
        a.scalars[1] = static_cast<float>(acc[3] / B);
        a.scalars[2] = static_cast<float>((acc[4] + 0.5 * acc[5] + 0.3 * acc[6] + 0.2 * acc[7]) / B);
        a.scalars[3] = static_cast<float>(correct);
        a.scalars[4] = static_cast<float>(fifths);
        a.scalars[5] = static_cast<float>(relative);
        a.scalars[6] = static_cast<float>(parallel);
        a.scalars[7] = static_cast<float>(acc[8] / B);
        a.scalars[8] = static_cast<float>(acc[2] / B);
        a.scalars[9] = 0.0f;
    }
}

}  // namespace

namespace {

int general_step_launch(const float* key_out, const float* tonic_out, const float* genre_out, const float* key_labels, const void* tonic_labels,
                        int tonic_labels_i64, const void* genre_labels, int genre_labels_i64, const void* key_signature_id, int key_signature_i64,
                        int batch, float key_weight, float tonic_weight, float genre_weight, int use_cos, const float* sample_weight,
                        float* scalars_out, float* d_key, float* d_tonic, float* d_genre, ake_stream_t stream) {
    AKE_REQUIRE(key_out && tonic_out && key_labels && tonic_labels && key_signature_id && scalars_out, AKE_ERR_INVALID, "general_step: null argument");
    AKE_REQUIRE(batch >= 1, AKE_ERR_INVALID, "general_step: batch %d", batch);
    AKE_REQUIRE(!genre_out || genre_labels, AKE_ERR_INVALID, "general_step: genre outputs without genre labels");
    const bool grads = d_key || d_tonic || d_genre;
    AKE_REQUIRE(!grads || (d_key && d_tonic && (d_genre || !genre_out)), AKE_ERR_INVALID, "general_step: pass every gradient buffer or none");
    StepLossArgs a;
    a.key = key_out; a.tonic = tonic_out; a.genre = genre_out; a.key_labels = key_labels;
    a.tonic_lab = tonic_labels; a.genre_lab = genre_labels; a.sig_lab = key_signature_id;
    a.tonic_i64 = tonic_labels_i64; a.genre_i64 = genre_labels_i64; a.sig_i64 = key_signature_i64;
    a.B = batch; a.key_w = key_weight; a.tonic_w = tonic_weight; a.genre_w = genre_weight; a.use_cos = use_cos; a.weight = sample_weight;
    a.scalars = scalars_out; a.d_key = d_key; a.d_tonic = d_tonic; a.d_genre = genre_out ? d_genre : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return sample_weight ? ake::launch("general_step_kernel", general_step_kernel<true>, dim3(1), dim3(256), 0, s, a)
                         : ake::launch("general_step_kernel", general_step_kernel<false>, dim3(1), dim3(256), 0, s, a);
}

}  // namespace

extern "C" int ake_general_step_f32(const float* key_out, const float* tonic_out, const float* genre_out, const float* key_labels,
                                    const void* tonic_labels, int tonic_labels_i64, const void* genre_labels, int genre_labels_i64,
                                    const void* key_signature_id, int key_signature_i64, int batch, float key_weight, float tonic_weight,
                                    float genre_weight, int use_cos, float* scalars_out, float* d_key, float* d_tonic, float* d_genre,
                                    ake_stream_t stream) {
    return general_step_launch(key_out, tonic_out, genre_out, key_labels, tonic_labels, tonic_labels_i64, genre_labels, genre_labels_i64,
                               key_signature_id, key_signature_i64, batch, key_weight, tonic_weight, genre_weight, use_cos, nullptr, scalars_out,
                               d_key, d_tonic, d_genre, stream);
}

extern "C" int ake_general_step_weighted_f32(const float* key_out, const float* tonic_out, const float* genre_out, const float* key_labels,
                                             const void* tonic_labels, int tonic_labels_i64, const void* genre_labels, int genre_labels_i64,
                                             const void* key_signature_id, int key_signature_i64, int batch, float key_weight,
                                             float tonic_weight, float genre_weight, int use_cos, const float* sample_weight_dev,
                                             float* scalars_out, float* d_key, float* d_tonic, float* d_genre, ake_stream_t stream) {
    return general_step_launch(key_out, tonic_out, genre_out, key_labels, tonic_labels, tonic_labels_i64, genre_labels, genre_labels_i64,
                               key_signature_id, key_signature_i64, batch, key_weight, tonic_weight, genre_weight, use_cos, sample_weight_dev,
                               scalars_out, d_key, d_tonic, d_genre, stream);
}

extern "C" size_t ake_general_step_local_workspace_bytes(int batch, int out_frames) {
    if (batch < 1 || out_frames < 1) return 0;
    const size_t chunks = (static_cast<size_t>(out_frames) + kLocRows - 1) / kLocRows;
    return ake::align_up(static_cast<size_t>(batch) * chunks * kLocNS * sizeof(double), 256);
}

extern "C" int ake_general_step_local_f32(const float* key_out, const float* tonic_out, const float* key_labels, const void* tonic_labels,
                                          int tonic_labels_i64, const void* key_signature_id, int key_signature_i64, const int* valid_frames,
                                          int batch, int out_frames, int label_frames, float key_weight, float tonic_weight,
                                          float* scalars_out, float* d_key, float* d_tonic, void* workspace, size_t workspace_bytes,
                                          ake_stream_t stream) {
    AKE_REQUIRE(key_out && tonic_out && key_labels && tonic_labels && key_signature_id && valid_frames && scalars_out, AKE_ERR_INVALID,
                "general_step_local: null argument");
    AKE_REQUIRE(batch >= 1 && batch <= 65535 && out_frames >= 1 && label_frames >= 1, AKE_ERR_INVALID,
                "general_step_local: batch %d, out_frames %d, label_frames %d", batch, out_frames, label_frames);   // (grid y <= 65535)
    AKE_REQUIRE(!d_key == !d_tonic, AKE_ERR_INVALID, "general_step_local: pass both gradient buffers or none");
    const size_t need = ake_general_step_local_workspace_bytes(batch, out_frames);
    AKE_REQUIRE(workspace, AKE_ERR_INVALID, "general_step_local: null workspace");
    AKE_REQUIRE(workspace_bytes >= need, AKE_ERR_WORKSPACE, "general_step_local: workspace %zu < %zu bytes", workspace_bytes, need);
    StepLocalArgs a;
    a.key = key_out; a.tonic = tonic_out; a.key_labels = key_labels; a.tonic_lab = tonic_labels; a.sig_lab = key_signature_id;
    a.valid = valid_frames; a.tonic_i64 = tonic_labels_i64; a.sig_i64 = key_signature_i64;
    a.B = batch; a.T = out_frames; a.R = label_frames; a.chunks = (out_frames + kLocRows - 1) / kLocRows;
    a.key_w = key_weight; a.tonic_w = tonic_weight;
    a.part = static_cast<double*>(workspace); a.scalars = scalars_out; a.d_key = d_key; a.d_tonic = d_tonic;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ake::launch("general_step_local_kernel", general_step_local_kernel, dim3(a.chunks, batch), dim3(kLocRows), 0, s, a);
    if (rc) return rc;
    return ake::launch("general_step_local_finish_kernel", general_step_local_finish_kernel, dim3(1), dim3(kLocFinish), 0, s, a);
}
