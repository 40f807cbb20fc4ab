// Smoothing a key track (csrc/track.hip makes one): everything that is done with the windows' (key, tonic) outputs once they exist.
// Semantics: include/ake_hip.h; host models: metrics.py.
//
// A smooth track is two launches on the track's outputs: key_emissions_kernel (every window's log-score of the 24 keys) and
// viterbi_keys_kernel (the most likely path through them).  Posterior key probabilities are a forward-backward pass over the same
// emissions: key_forward_backward_kernel (the two serial chains, side by side) and key_posteriors_kernel (everything per window), below
// the Viterbi kernel.
//
// A stream of audio is smoothed a call at a time by key_stream_step_kernel (ake_key_stream_step_f32): the Viterbi step and the forward
// step on every new window, with d, a and a ring of the last `lag` back-pointer rows carried in device memory between calls, and a
// fixed-lag path out of the ring.  The stream's front end is csrc/stream.hip.  Fixed-lag posteriors and a running log-likelihood come
// from two launches behind the step (ake_key_stream_posteriors_f32): key_stream_sweep_kernel, a backward sweep of at most `lag` steps
// per written window, and key_stream_loglik_kernel, which adds the new windows' c and keeps a second state -- the last `lag` rows of e
// and of a -- for the sweeps of later calls.
//
// These five chain kernels are one wave per chain and give the same bits however a stream is cut, because they share their parts: the
// wave's layout (ChainLane), the loop that prefetches a step's inputs (chain_steps; the sweep kernel has a copy, see there) and the
// steps themselves (viterbi_step, lse_step, states_lse, first_best_state).
//
// Training for the smoothed track adds a loss over sequences of consecutive windows (ake_key_sequence_loss_f32): the emission formula and
// the forward-backward recurrences above, in double, run on the free and on the label-clamped scores side by side, and a gradient kernel
// per window; below the posterior kernels.
#include "common.h"
#include "keys.h"

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

namespace {

// ---- a smooth track: key emissions and a Viterbi decode over them (semantics: include/ake_hip.h; host restatement: metrics.py) ----
constexpr int kVitBatch = 8;          // emission rows in flight ahead of the recurrence (a multiple of 4: one back-pointer word is 4 steps)
constexpr int kVitChunk = 256;        // windows of back-pointers the backtrace stages into LDS at a time (a multiple of 4)

struct EmisArgs {
    const float* key;          // [rows][12]
    const float* tonic;        // [rows][12]
    const int* counts;         // nullable, as DecodeArgs
    int rows, windows;
    float scale;               // signature_weight / 12
    float* emis;               // [rows][24]
};

// One row's 24 scores from its 12 memberships and 12 tonic logits (96 bytes in, moved as float4s): the arithmetic of every kernel that
// needs the emissions, in the precision T it needs them in (float for the tracker, whose bits this is; double for the sequence loss).
// Only 12 distinct signature sums exist (key k's scale is that of its relative major), so 12 are computed and the 24 outputs index them.
template <typename T>
__device__ __forceinline__ void emission_row(const float* key, const float* tonic, size_t r, T scale, T (&e)[kKeys]) {
    T p[12], t[12];
    for (int q = 0; q < 3; ++q) {
        const float4 pv = reinterpret_cast<const float4*>(key + r * 12)[q];
        const float4 tv = reinterpret_cast<const float4*>(tonic + r * 12)[q];
        p[4 * q] = pv.x; p[4 * q + 1] = pv.y; p[4 * q + 2] = pv.z; p[4 * q + 3] = pv.w;
        t[4 * q] = tv.x; t[4 * q + 1] = tv.y; t[4 * q + 2] = tv.z; t[4 * q + 3] = tv.w;
    }
    T in[12], outside[12];                                               // the two Bernoulli terms, clamped as nn.BCELoss clamps them
    for (int j = 0; j < 12; ++j) {
        in[j] = fmax(log(p[j]), T(-100));                                // (the overloads of T: logf, log1pf, expf, fmaxf for float)
        outside[j] = fmax(log1p(-p[j]), T(-100));
    }
    T tmax = t[0];
    for (int j = 1; j < 12; ++j) tmax = fmax(tmax, t[j]);
    T se = T(0);
    for (int j = 0; j < 12; ++j) se += exp(t[j] - tmax);
    const T lse = tmax + log(se);
    T sig[12];                                                           // by major tonic
    for (int m = 0; m < 12; ++m) {
        T s = T(0);
        for (int j = 0; j < 12; ++j) s += (kMajorScale >> ((j - m + 12) % 12)) & 1 ? in[j] : outside[j];
        sig[m] = s;
    }
    for (int k = 0; k < kKeys; ++k) e[k] = (t[k % 12] - lse) + scale * sig[k >= 12 ? k - 12 : (k + 3) % 12];
}

// window r of a [recordings][windows] layout lies at or behind its recording's count (counts null: never)
__device__ __forceinline__ bool behind_count(const int* counts, int windows, int r) {
    if (!counts) return false;
    const int rec = r / windows;
    return r - rec * windows >= counts[rec];
}

// One thread per row, as decode_keys_kernel: 96 bytes in and 96 out, moved as float4s.
__global__ __launch_bounds__(256) void key_emissions_kernel(EmisArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    float4* const out = reinterpret_cast<float4*>(a.emis + static_cast<size_t>(r) * kKeys);
    if (behind_count(a.counts, a.windows, r)) {
        for (int q = 0; q < 6; ++q) out[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float e[kKeys];
    emission_row<float>(a.key, a.tonic, static_cast<size_t>(r), a.scale, e);
    for (int q = 0; q < 6; ++q) out[q] = make_float4(e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]);
}

struct VitArgs {
    const float* emis;         // [recordings][windows][24]
    const int* counts;         // nullable
    const float* trans;        // [24][24], from i (row) to j
    const float* prior;        // [24], nullable = zeros
    int* path;                 // [recordings][windows]
    unsigned* bp;              // [recordings][groups][24] words: byte b of word [g][j] = bp_{4g+b}[j]
    int windows, groups;       // groups = ceil(windows / 4)
};

// f32 bits <-> a signed integer with the same order (its own inverse): the normalising maximum runs on these, because an integer
// maximum folds into its DPP operand (v_max_i32_dpp) where a float one costs a move and a canonicalisation beside it.
__device__ __forceinline__ int order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

template <int kCtrl>
__device__ __forceinline__ int dpp_max(int x) {
    const int y = __builtin_amdgcn_update_dpp(0, x, kCtrl, 0xf, 0xf, true);
    return x > y ? x : y;
}

// max over the states of a wave whose 64 lanes are all active; `valid` marks the lanes that hold one (lanes 0..23 must).  Four
// in-register butterfly steps inside each row of 16 lanes (xor 1, xor 2, half-row mirror, row mirror), then the two rows that hold
// states meet through two v_readlane and scalar arithmetic: no LDS round trip.
__device__ __forceinline__ float states_max(float x, bool valid) {
    int k = valid ? order_key(__float_as_int(x)) : INT_MIN;
    k = dpp_max<0xB1>(k);      // quad_perm [1,0,3,2]
    k = dpp_max<0x4E>(k);      // quad_perm [2,3,0,1]
    k = dpp_max<0x141>(k);     // row_half_mirror
    k = dpp_max<0x140>(k);     // row_mirror
    const int k0 = __builtin_amdgcn_readlane(k, 0), k1 = __builtin_amdgcn_readlane(k, 16);
    return __int_as_float(order_key(k0 > k1 ? k0 : k1));
}

// The layout of a chain kernel's one wave.  A step is a latency chain on that wave, so what counts is its number of instructions:
//   - lanes j and 32 + j (j < 24) share state j: the first takes the predecessors i = 0..11, the second i = 12..23, each with its half
//     of the 24 transition terms of j in registers (a column half of A where the chain runs forward, a row half where it runs
//     backward), so a lane adds, maximises (v_max3) and compare-selects over 12 candidates, not 24; the halves meet through two
//     v_permlane32_swap (a tie goes to the lower half: the smallest i);
//   - the step's 24 scores reach the lanes through a 96-byte LDS row, 48 bytes of it per lane as three 16-byte broadcast reads;
//   - the normalising maximum is the butterfly above;
//   - nothing else on the chain touches memory: chain_steps loads the steps' inputs ahead of them.
struct ChainLane {
    int half, j;               // which 12 predecessors, which state (the lanes without one run along on state 0; their scores are never read)
    bool own, writer;          // the lane holds a state; it is the one of the state's two lanes that writes it
    float A[kKeys / 2];
    // this half's 48 bytes of an LDS row of 24 scores
    __device__ __forceinline__ const float4* half_of(const float4* row) const { return row + half * (kKeys / 8); }
};

// kRows false: A[i] = trans[half * 12 + i][j], into state j (forward, Viterbi); true: A[i] = trans[j][half * 12 + i], out of it (backward)
template <bool kRows>
__device__ __forceinline__ ChainLane chain_lane(const float* trans, int lane) {
    constexpr int kHalf = kKeys / 2;
    ChainLane c;
    c.half = lane >> 5;
    c.own = (lane & 31) < kKeys;
    c.writer = lane < kKeys;
    c.j = c.own ? lane & 31 : 0;
#pragma unroll
    for (int i = 0; i < kHalf; ++i) c.A[i] = kRows ? trans[c.j * kKeys + c.half * kHalf + i] : trans[(c.half * kHalf + i) * kKeys + c.j];
    return c;
}

// A lane's 12 candidates of a step, c[i] = score[i] + A[i] for its half of the predecessors (the scores: three 16-byte broadcast reads
// of the LDS row), and their maximum.  Shared by the Viterbi step and the forward-backward step.
__device__ __forceinline__ float half_candidates(const float4* dsrc, const float (&A)[12], float (&c)[12]) {
    const float4 q0 = dsrc[0], q1 = dsrc[1], q2 = dsrc[2];
    c[0] = q0.x + A[0]; c[1] = q0.y + A[1]; c[2] = q0.z + A[2];  c[3] = q0.w + A[3];
    c[4] = q1.x + A[4]; c[5] = q1.y + A[5]; c[6] = q1.z + A[6];  c[7] = q1.w + A[7];
    c[8] = q2.x + A[8]; c[9] = q2.y + A[9]; c[10] = q2.z + A[10]; c[11] = q2.w + A[11];
    return fmaxf(fmaxf(fmaxf(fmaxf(c[0], c[1]), c[2]), fmaxf(fmaxf(c[3], c[4]), c[5])),
                 fmaxf(fmaxf(fmaxf(c[6], c[7]), c[8]), fmaxf(fmaxf(c[9], c[10]), c[11])));
}

// The Viterbi step of one wave: this lane's score d of the step before goes into the LDS row, the lane's half of
// max_i (d[i] + A[i][j]) comes back and meets the other half.  Returns the maximum, `arg` the smallest i attaining it.  Shared by
// viterbi_keys_kernel and key_stream_step_kernel.
__device__ __forceinline__ float viterbi_step(const ChainLane& cl, float d, float4* d_lds, unsigned& arg) {
    constexpr int kHalf = 12;
    if (cl.writer) reinterpret_cast<float*>(d_lds)[threadIdx.x] = d;    // (a writer's lane is its j)
    __syncthreads();                                                     // (one wave: the wait for the LDS write, no more)
    float c[kHalf];
    const float mh = half_candidates(cl.half_of(d_lds), cl.A, c);
    unsigned ah = 0;
#pragma unroll
    for (int i = kHalf - 1; i >= 0; --i) ah = c[i] == mh ? static_cast<unsigned>(i) : ah;        // ends on the smallest i
    // v_permlane32_swap(x, x): the lower half's x in every lane of the first result, the upper half's in the second
    const auto ms = __builtin_amdgcn_permlane32_swap(__float_as_uint(mh), __float_as_uint(mh), false, false);
    const auto as = __builtin_amdgcn_permlane32_swap(ah, ah, false, false);
    const float m_lo = __uint_as_float(ms[0]), m_hi = __uint_as_float(ms[1]);
    const bool upper = m_hi > m_lo;                                      // strict: a tie goes to the smaller i
    const float m = upper ? m_hi : m_lo;
    arg = upper ? as[1] + kHalf : as[0];
    return m;
}

// the smallest state attaining the maximum of the wave's scores (wave-uniform)
__device__ __forceinline__ int first_best_state(float d, bool own, bool writer) {
    const float mx = states_max(d, own);
    return __ffsll(static_cast<unsigned long long>(__ballot(writer && d == mx))) - 1;
}

// Steps 0..n-1 of a chain, step(t, k, v) on v = load(t), with the loads kVitBatch steps ahead of the chain: a batch is in flight while
// the one before is consumed.  load(t) is also called for t behind the last step and clamps its own index (clamped, not branched
// around: the loads stay one straight batch).  k = t % kVitBatch is a constant once the loop is unrolled.
template <typename V = float, typename Load, typename Step>
__device__ __forceinline__ void chain_steps(int n, Load load, Step step) {
    V eb[kVitBatch];
#pragma unroll
    for (int k = 0; k < kVitBatch; ++k) eb[k] = load(k);
    for (int t0 = 0; t0 < n; t0 += kVitBatch) {
        V en[kVitBatch];
#pragma unroll
        for (int k = 0; k < kVitBatch; ++k) en[k] = load(t0 + kVitBatch + k);
#pragma unroll
        for (int k = 0; k < kVitBatch; ++k) {
            if (t0 + k >= n) break;                                      // wave-uniform: all 64 lanes stay active for the cross-lane steps
            step(t0 + k, k, eb[k]);
        }
#pragma unroll
        for (int k = 0; k < kVitBatch; ++k) eb[k] = en[k];
    }
}

// One wave per recording (layout: ChainLane); the back-pointers leave as one word per state every 4 steps.  The backtrace then walks
// the back-pointers in LDS, kVitChunk windows at a time, staged in and written out by all lanes.
__global__ __launch_bounds__(64) void viterbi_keys_kernel(VitArgs a) {
    __shared__ uint4 bp_lds[kVitChunk / 4 * kKeys / 4];
    __shared__ int path_lds[kVitChunk];
    __shared__ float4 d_lds[kKeys / 4];
    const int r = blockIdx.x, lane = threadIdx.x, W = a.windows;
    const int n = clamped_count(a.counts, r, W);
    const ChainLane cl = chain_lane<false>(a.trans, lane);
    const bool own = cl.own, writer = cl.writer;
    const int j = cl.j;
    const float* const e = a.emis + static_cast<size_t>(r) * W * kKeys + j;
    unsigned* const bp = a.bp + static_cast<size_t>(r) * a.groups * kKeys + j;
    float d = a.prior ? a.prior[j] : 0.f;
    const int wl = n > 0 ? n - 1 : 0;                                    // the last row that is read (W >= 1)
    unsigned word = 0;
    chain_steps(
        n, [&](int w) { return e[static_cast<size_t>(w < wl ? w : wl) * kKeys]; },
        [&](int w, int k, float ew) {
            float m = d;                                                 // w == 0: the prior
            unsigned arg = 0;
            if (w > 0) m = viterbi_step(cl, d, d_lds, arg);
            const float raw = m + ew;
            d = raw - states_max(raw, own);
            word |= arg << (8 * (k & 3));                                // (a batch is whole words, so w & 3 == k & 3: a constant shift)
            if ((k & 3) == 3) {
                if (writer) bp[static_cast<size_t>(w >> 2) * kKeys] = word;
                word = 0;
            }
        });
    if ((n & 3) && writer) bp[static_cast<size_t>((n - 1) >> 2) * kKeys] = word;  // the last, partial word
    __syncthreads();                                                     // the wave's own stores, before other lanes load them

    // the last state: the smallest j attaining the maximum (0 after the normalisation, found the same way all the same)
    int cur = 0;
    if (n > 0) cur = first_best_state(d, own, writer);
    int* const path = a.path + static_cast<size_t>(r) * W;
    const unsigned char* const bytes = reinterpret_cast<const unsigned char*>(bp_lds);
    for (int c0 = (W - 1) / kVitChunk * kVitChunk; c0 >= 0; c0 -= kVitChunk) {
        const int len = W - c0 < kVitChunk ? W - c0 : kVitChunk;         // windows of this chunk
        const int nv = n - c0 < len ? n - c0 : len;                      // of which decoded (<= 0: none)
        if (nv > 0) {
            const uint4* const src = reinterpret_cast<const uint4*>(a.bp + (static_cast<size_t>(r) * a.groups + c0 / 4) * kKeys);
            const int quads = (nv + 3) / 4 * (kKeys / 4);                // 16-byte pieces: 6 per group of 4 windows
            for (int x = lane; x < quads; x += 64) bp_lds[x] = src[x];
            __syncthreads();
            for (int w = nv - 1; w >= 0; --w) {                          // a chain of LDS reads, one per window; cur is wave-uniform
                path_lds[w] = cur;
                cur = bytes[(w >> 2) * (4 * kKeys) + cur * 4 + (w & 3)];
            }
            __syncthreads();
        }
        for (int x = lane; x < len; x += 64) path[c0 + x] = x < nv ? path_lds[x] : -1;
        __syncthreads();                                                 // path_lds and bp_lds are reused by the chunk before
    }
}

// ---- posterior key probabilities: forward-backward over the same emissions (semantics: include/ake_hip.h; host model: metrics.key_posteriors) ----
constexpr int kPostChunk = 64;        // windows per block of key_posteriors_kernel: 16 per wave for the transition sums (a multiple of 4)
constexpr int kCells = kKeys * kKeys; // 576 = 9 per lane of a wave

struct FbArgs {
    const float* emis;         // [recordings][windows][24]
    const int* counts;         // nullable
    const float* trans;        // [24][24], from i (row) to j
    const float* prior;        // [24], nullable = zeros
    float* a;                  // [recordings][windows][24] normalised forward scores (rows behind the count are not written)
    float* b;                  // the same, backward
    float* loglik;             // [recordings]
    int windows;
};

template <int kCtrl>
__device__ __forceinline__ float dpp_add(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xf, 0xf, true));
}

// sum over the states, laid out and joined as states_max: every stage adds a lane's value and its partner's, which is the same sum in
// both (x + y == y + x), so all 16 lanes of a row end on the same bits, and the order is fixed.
__device__ __forceinline__ float states_sum(float x, bool valid) {
    float s = valid ? x : 0.f;
    s = dpp_add<0xB1>(s);
    s = dpp_add<0x4E>(s);
    s = dpp_add<0x141>(s);
    s = dpp_add<0x140>(s);
    const int bits = __float_as_int(s);                                  // (v_readlane is typed int: the bits, not the value)
    return __int_as_float(__builtin_amdgcn_readlane(bits, 0)) + __int_as_float(__builtin_amdgcn_readlane(bits, 16));
}

// The forward-backward step of one wave (layout: ChainLane): this lane's score x (kAdd: x + e) goes into the
// LDS row, the lane's half of LSE_i (row[i] + A[i]) comes back and meets the other half at their common maximum.  Shared by the two chains and
// key_stream_step_kernel.
template <bool kAdd>
__device__ __forceinline__ float lse_step(const ChainLane& cl, float x, float e, float4* d_lds) {
    constexpr int kHalf = 12;
    if (cl.writer) reinterpret_cast<float*>(d_lds)[threadIdx.x] = kAdd ? x + e : x;
    __syncthreads();                                                     // (one wave: the wait for the LDS write, no more)
    float c[kHalf];
    const float mh = half_candidates(cl.half_of(d_lds), cl.A, c);
    float sh = 0.f;
#pragma unroll
    for (int i = 0; i < kHalf; ++i) sh += __expf(c[i] - mh);
    const auto ms = __builtin_amdgcn_permlane32_swap(__float_as_uint(mh), __float_as_uint(mh), false, false);
    const auto ss = __builtin_amdgcn_permlane32_swap(__float_as_uint(sh), __float_as_uint(sh), false, false);
    const float m_lo = __uint_as_float(ms[0]), m_hi = __uint_as_float(ms[1]);
    const float m = fmaxf(m_lo, m_hi);
    const float s = __uint_as_float(ss[0]) * __expf(m_lo - m) + __uint_as_float(ss[1]) * __expf(m_hi - m);
    return m + __logf(s);
}

// c = LSE over the states of a step's raw scores (what the step subtracts)
__device__ __forceinline__ float states_lse(float raw, bool own) {
    const float mx = states_max(raw, own);
    return mx + __logf(states_sum(__expf(raw - mx), own));
}

// One direction of one recording on one wave (layout: ChainLane), with log-sum-exp in the place of the Viterbi step's max: the halves'
// two partial sums meet at their common maximum.
//   forward  (kBack = false), step t = window t:         the row holds a_{t-1},               the lane a column half of A, raw = e[t] + LSE
//   backward (kBack = true),  step t = window n - 1 - t: the row holds b_{w+1} + e[w+1],      the lane a row half of A,    raw = LSE
// Every exponential's argument is <= 0 and the largest is 0, so a sum lies in [1, 24]: the fast v_exp_f32 / v_log_f32 forms are exact
// to an ulp of the sum (a term's error is |x| e^x 2^-24 <= 0.37 * 2^-24), and no range handling is needed.  loglik adds the c_w in a
// double beside the chain: a float32 running sum would lose sqrt(n) ulps.
template <bool kBack>
__device__ __forceinline__ void forward_backward_chain(const FbArgs& a, float4* d_lds) {
    const int r = blockIdx.x, lane = threadIdx.x, W = a.windows;
    const int n = clamped_count(a.counts, r, W);
    const ChainLane cl = chain_lane<kBack>(a.trans, lane);
    const bool own = cl.own, writer = cl.writer;
    const int j = cl.j;
    const float* const e = a.emis + static_cast<size_t>(r) * W * kKeys + j;
    float* const out = (kBack ? a.b : a.a) + static_cast<size_t>(r) * W * kKeys + j;
    const int wl = n > 0 ? n - 1 : 0;                                    // the last row that is read (W >= 1)
    float d = kBack ? 0.f : (a.prior ? a.prior[j] : 0.f);
    double ll = 0.0;
    chain_steps(n,
        // the emission row of step t: window t forward, window n - t backward (step 0 reads none there), clamped into 0..wl
        [&](int t) { const int w = kBack ? n - t : t; return e[static_cast<size_t>(w < 0 ? 0 : w < wl ? w : wl) * kKeys]; },
        [&](int t, int, float et) {
            float raw = kBack ? 0.f : d + et;                            // t == 0: b_{n-1} = 0, a_0 = prior + e[0]
            if (t > 0) {
                const float lse = lse_step<kBack>(cl, d, et, d_lds);
                raw = kBack ? lse : lse + et;
            }
            if (!kBack || t > 0) {                                       // b_{n-1} stays 0, unnormalised
                const float cw = states_lse(raw, own);
                d = raw - cw;
                ll += static_cast<double>(cw);
            } else {
                d = raw;
            }
            if (writer) out[static_cast<size_t>(kBack ? n - 1 - t : t) * kKeys] = d;
        });
    if (!kBack && lane == 0) a.loglik[r] = static_cast<float>(ll);
}

// grid (recordings, 2): blockIdx.y picks the direction, so the two chains of a recording run at the same time on two CUs.
__global__ __launch_bounds__(64) void key_forward_backward_kernel(FbArgs a) {
    __shared__ float4 d_lds[kKeys / 4];
    if (blockIdx.y == 0) forward_backward_chain<false>(a, d_lds);
    else forward_backward_chain<true>(a, d_lds);
}

// ---- the smoother with carried state: a stream's new windows, a call at a time (semantics: include/ake_hip.h; host model: metrics.key_stream) ----
constexpr int kStreamMaxLag = 255;
constexpr int kStreamScores = 2 * kKeys * static_cast<int>(sizeof(float));    // bytes of d[24], a[24] in front of a recording's ring

// bytes of one recording's state: d[24], a[24], then the ring of the last `lag` back-pointer rows (24 bytes each), in 16-byte pieces
constexpr size_t stream_state_stride(int lag) { return static_cast<size_t>(kStreamScores + (kKeys * lag + 15) / 16 * 16); }

struct StreamStepArgs {
    const float* emis;         // [recordings][k][24]
    const float* trans;        // [24][24], from i (row) to j
    const float* prior;        // [24], nullable = zeros
    unsigned char* state;      // [recordings][stream_state_stride(lag)]
    float* filtered;           // [recordings][k][24], nullable
    int* path;                 // [recordings][k_out]
    long long before;          // windows of the stream before this call
    int k, lag, flush, k_out;
    int slot0;                 // before % lag (0 for lag 0): the ring row of the call's first window
};

// One wave per recording (layout: ChainLane), both recurrences side by side on every new window: the Viterbi step
// (viterbi_step; its back-pointers go into a ring of `lag` rows in LDS, row w % lag for window w) and the forward step (lse_step,
// states_lse; the normalised row is `filtered`).  After the step of window w >= lag the wave follows `lag` back-pointers from the first
// maximum of d_w and writes the label of window w - lag; a flush writes the windows still inside the lag from the last best state.
// d, a and the ring come from `state` once, in front of the first step (not at all on a fresh stream, before == 0), and go back once,
// behind the last.
__global__ __launch_bounds__(64) void key_stream_step_kernel(StreamStepArgs a) {
    __shared__ uint4 ring_lds[(kStreamMaxLag * kKeys + 15) / 16];
    __shared__ float4 d_lds[kKeys / 4], f_lds[kKeys / 4];
    const int r = blockIdx.x, lane = threadIdx.x, k = a.k, lag = a.lag;
    const ChainLane cl = chain_lane<false>(a.trans, lane);
    const bool own = cl.own, writer = cl.writer;
    const int j = cl.j;
    unsigned char* const ring = reinterpret_cast<unsigned char*>(ring_lds);
    unsigned char* const st = a.state + static_cast<size_t>(r) * stream_state_stride(lag);
    const int ring_quads = (kKeys * lag + 15) / 16;
    const float prior = a.prior ? a.prior[j] : 0.f;
    float d = prior, f = prior;                                          // window 0 adds its emissions to the prior
    if (a.before > 0) {
        d = reinterpret_cast<const float*>(st)[j];
        f = reinterpret_cast<const float*>(st)[kKeys + j];
        for (int x = lane; x < ring_quads; x += 64) ring_lds[x] = reinterpret_cast<const uint4*>(st + kStreamScores)[x];
    } else {
        for (int x = lane; x < ring_quads; x += 64) ring_lds[x] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const long long first_out = a.before > lag ? a.before - lag : 0;    // the window path[0] belongs to
    int* const path = a.path + static_cast<size_t>(r) * a.k_out;
    int slot = a.slot0;                                                  // ring row of the window being stepped
    if (k > 0) {
        const float* const e = a.emis + static_cast<size_t>(r) * k * kKeys + j;
        float* const out = a.filtered ? a.filtered + static_cast<size_t>(r) * k * kKeys + j : nullptr;
        const int wl = k - 1;
        chain_steps(
            k, [&](int i) { return e[static_cast<size_t>(i < wl ? i : wl) * kKeys]; },
            [&](int i, int, float ei) {
                const long long w = a.before + i;
                float m = d, fr = f;
                unsigned arg = 0;
                if (w > 0) {
                    m = viterbi_step(cl, d, d_lds, arg);
                    fr = lse_step<false>(cl, f, 0.f, f_lds);
                }
                const float raw = m + ei;
                d = raw - states_max(raw, own);
                const float fraw = fr + ei;
                f = fraw - states_lse(fraw, own);
                if (out && writer) out[static_cast<size_t>(i) * kKeys] = f;
                if (lag > 0 && writer) ring[slot * kKeys + lane] = static_cast<unsigned char>(arg);
                if (w >= lag) {
                    int cur = first_best_state(d, own, writer);
                    if (lag > 0) {
                        __syncthreads();                                 // the row just written, before any lane reads it
                        int s = slot;
                        for (int b = 0; b < lag; ++b) {                  // a chain of LDS reads; cur is wave-uniform
                            cur = ring[s * kKeys + cur];
                            s = s == 0 ? lag - 1 : s - 1;
                        }
                    }
                    if (lane == 0) path[w - lag - first_out] = cur;
                }
                slot = slot + 1 == lag ? 0 : slot + 1;
            });
    }
    const long long total = a.before + k;
    if (a.flush && total > 0) {                                          // the windows still inside the lag, from the last best state
        int cur = first_best_state(d, own, writer);
        __syncthreads();
        const long long v_min = total > lag ? total - lag : 0;
        int s = slot == 0 ? (lag > 0 ? lag - 1 : 0) : slot - 1;          // the ring row of window total - 1
        for (long long v = total - 1; v >= v_min; --v) {
            if (lane == 0) path[v - first_out] = cur;
            if (v > v_min) {
                cur = ring[s * kKeys + cur];
                s = s == 0 ? lag - 1 : s - 1;
            }
        }
    }
    __syncthreads();
    if (writer) {
        reinterpret_cast<float*>(st)[lane] = d;
        reinterpret_cast<float*>(st)[kKeys + lane] = f;
    }
    for (int x = lane; x < ring_quads; x += 64) reinterpret_cast<uint4*>(st + kStreamScores)[x] = ring_lds[x];
}

// ---- fixed-lag posteriors and the running log-likelihood of a stream (semantics: include/ake_hip.h; host model:
// metrics.key_stream_posteriors) ----
// A second state beside the step kernel's, per recording: the double sum of c (in a 16-byte piece of its own), then a ring of the last
// `lag` emission rows and a ring of the last `lag` filtered rows, row w % lag for window w (one row each for lag 0: the forward step of
// a call's first window needs a_{w-1} whatever the lag).
constexpr int kStreamPostHead = 16;
constexpr int stream_post_rows(int lag) { return lag > 0 ? lag : 1; }
constexpr size_t stream_post_stride(int lag) {
    return static_cast<size_t>(kStreamPostHead) + 2 * static_cast<size_t>(stream_post_rows(lag)) * kKeys * sizeof(float);
}

struct StreamPostArgs {
    const float* emis;         // [recordings][k][24]: the new windows
    const float* filtered;     // [recordings][k][24]: key_stream_step_kernel's a rows of the same windows
    const float* trans;        // [24][24], from i (row) to j
    const float* prior;        // [24], nullable = zeros
    const int* path;           // [recordings][k_out], nullable
    unsigned char* state;      // [recordings][stream_post_stride(lag)]
    float* post;               // [recordings][k_out][24]
    float* path_post;          // [recordings][k_out], nullable
    float* loglik;             // [recordings][k], nullable
    long long before;          // windows of the stream before this call
    int k, lag, k_out;         // (a flush shows in k_out alone: its windows end at the last one, total - 1)
};

// One wave per (recording, written window v), in the backward chain's layout (ChainLane): the backward sweep from the end window
// s = min(v + lag, total - 1) down to v, at most `lag` steps of lse_step<true> / states_lse with b_s = 0, then softmax(a_v + b_v) over the
// wave's 24 states.  A row of window u comes from the call's inputs (u >= before) or from the state's rings (u < before; never on a fresh
// stream): the choice moves a pointer and nothing else, so a sweep's operations do not depend on how the stream was cut into calls.
// The kernel only reads the state.
// It keeps chain_steps' loop as a copy of its own: its load chooses between two row pointers, and through the helper that choice costs
// either stack slots and flat loads or, with the pointers taken ahead of it, 1-3 % of the launch (profiles/track_chain_helpers.md).
__global__ __launch_bounds__(64) void key_stream_sweep_kernel(StreamPostArgs a) {
    __shared__ float4 d_lds[kKeys / 4];
    const int r = blockIdx.x / a.k_out, x = blockIdx.x - r * a.k_out, lane = threadIdx.x, k = a.k, lag = a.lag;
    const ChainLane cl = chain_lane<true>(a.trans, lane);
    const bool own = cl.own, writer = cl.writer;
    const int j = cl.j;
    const int rows = stream_post_rows(lag);
    const float* const e_ring = reinterpret_cast<const float*>(a.state + static_cast<size_t>(r) * stream_post_stride(lag) + kStreamPostHead);
    const float* const a_ring = e_ring + static_cast<size_t>(rows) * kKeys;
    const long long before = a.before, total = before + k;
    const long long v = (before > lag ? before - lag : 0) + x;           // the window this wave writes
    const long long s = v + lag < total - 1 ? v + lag : total - 1;       // its end window (without a flush v + lag <= total - 1 anyway)
    const int steps = static_cast<int>(s - v);                           // 0..lag
    const size_t in0 = static_cast<size_t>(r) * k;
    const float av = (v >= before ? a.filtered + (in0 + static_cast<size_t>(v - before)) * kKeys : a_ring + static_cast<size_t>(v % rows) * kKeys)[j];
    float d = 0.f;                                                       // b_s = 0
    // the emission row step t = 1..steps adds: window s - t + 1, in v + 1..s (clamped into it; window s itself where there is no step)
    auto step_e = [&](int t) {
        const long long u = s + 1 - (t < 1 ? 1 : t > steps ? (steps > 0 ? steps : 1) : t);
        const float* const row = u >= before ? a.emis + (in0 + static_cast<size_t>(u - before)) * kKeys : e_ring + static_cast<size_t>(u % rows) * kKeys;
        return row[j];
    };
    float eb[kVitBatch];
#pragma unroll
    for (int q = 0; q < kVitBatch; ++q) eb[q] = step_e(1 + q);
    for (int t0 = 0; t0 < steps; t0 += kVitBatch) {
        float en[kVitBatch];
#pragma unroll
        for (int q = 0; q < kVitBatch; ++q) en[q] = step_e(t0 + kVitBatch + 1 + q);
#pragma unroll
        for (int q = 0; q < kVitBatch; ++q) {
            if (t0 + q >= steps) break;                                  // wave-uniform
            const float raw = lse_step<true>(cl, d, eb[q], d_lds);
            d = raw - states_lse(raw, own);
        }
#pragma unroll
        for (int q = 0; q < kVitBatch; ++q) eb[q] = en[q];
    }
    const float xv = av + d;
    const float ex = __expf(xv - states_max(xv, own));
    const float p = ex / states_sum(ex, own);
    const size_t out = static_cast<size_t>(r) * a.k_out + x;
    if (writer) a.post[out * kKeys + lane] = p;
    if (a.path_post) {
        const int k0 = a.path[out];                                      // wave-uniform; -1 (or anything that is no key) gives 0
        const float pp = __shfl(p, k0 >= 0 && k0 < kKeys ? k0 : 0);
        if (lane == 0) a.path_post[out] = k0 >= 0 && k0 < kKeys ? pp : 0.f;
    }
}

// One wave per recording, after the sweeps on the same stream: the only kernel that writes the state.  It recomputes c_w of every new
// window through the step kernel's own forward step (lse_step<false> on a_{w-1}, + e_w, states_lse) -- the steps do not chain: a_{w-1}
// is the filtered row the step kernel wrote, or the state's last one in front of the call's first window --, adds them in window order
// to the double that forward_backward_chain keeps, writes the running sums, and moves the call's last rows into the rings.  A fresh
// stream (before == 0) reads nothing from the state and writes all of it, zeros where no window has been.
__global__ __launch_bounds__(64) void key_stream_loglik_kernel(StreamPostArgs a) {
    __shared__ float4 f_lds[kKeys / 4];
    const int r = blockIdx.x, lane = threadIdx.x, k = a.k, lag = a.lag;
    const ChainLane cl = chain_lane<false>(a.trans, lane);
    const bool own = cl.own;
    const int j = cl.j;
    const int rows = stream_post_rows(lag);
    unsigned char* const st = a.state + static_cast<size_t>(r) * stream_post_stride(lag);
    float* const e_ring = reinterpret_cast<float*>(st + kStreamPostHead);
    float* const a_ring = e_ring + static_cast<size_t>(rows) * kKeys;
    const long long before = a.before;
    double ll = 0.0;
    float f = a.prior ? a.prior[j] : 0.f;                                // window 0 adds its emissions to the prior
    if (before > 0) {
        ll = *reinterpret_cast<const double*>(st);
        f = a_ring[static_cast<size_t>((before - 1) % rows) * kKeys + j];
    }
    const float* const e = a.emis + static_cast<size_t>(r) * k * kKeys;
    const float* const fl = a.filtered + static_cast<size_t>(r) * k * kKeys;
    float* const out = a.loglik ? a.loglik + static_cast<size_t>(r) * k : nullptr;
    const int wl = k - 1;                                                // (k >= 1: the host launches nothing for k == 0)
    struct Window { float e, a; };                                       // a window's emission and its filtered score, of this lane's state
    chain_steps<Window>(
        k,
        [&](int i) {
            const size_t at = static_cast<size_t>(i < wl ? i : wl) * kKeys + j;
            return Window{e[at], fl[at]};
        },
        [&](int i, int, Window w) {
            float fr = f;
            if (before + i > 0) fr = lse_step<false>(cl, f, 0.f, f_lds);
            ll += static_cast<double>(states_lse(fr + w.e, own));
            if (out && lane == 0) out[i] = static_cast<float>(ll);
            f = w.a;                                                     // a_w, the bits the step kernel went on with
        });
    // the state: every read of it lies above
    if (lane == 0) {
        reinterpret_cast<double*>(st)[0] = ll;
        if (before == 0) reinterpret_cast<double*>(st)[1] = 0.0;
    }
    const int m = k < rows ? k : rows;                                   // the call's last m windows are the ring's newest
    for (int c = lane; c < m * kKeys; c += 64) {
        const int i = k - m + c / kKeys, key = c - c / kKeys * kKeys;
        const size_t to = static_cast<size_t>((before + i) % rows) * kKeys + key;
        e_ring[to] = e[static_cast<size_t>(i) * kKeys + key];
        a_ring[to] = fl[static_cast<size_t>(i) * kKeys + key];
    }
    if (before == 0)                                                     // rows 0..m-1 were just written: the rest has seen no window yet
        for (int c = m * kKeys + lane; c < rows * kKeys; c += 64) e_ring[c] = a_ring[c] = 0.f;
}

struct PostArgs {
    const float* emis;         // [recordings][windows][24]
    const int* counts;         // nullable
    const float* trans;        // [24][24]
    const int* path;           // [recordings][windows], nullable
    const float* a;            // [recordings][windows][24]
    const float* b;
    float* post;               // [recordings][windows][24], nullable: the transition sums alone
    float* path_post;          // [recordings][windows], nullable
    float* xi_part;            // [recordings][chunks][576], nullable: no transition sums
    int windows, chunks;       // chunks = ceil(windows / kPostChunk)
};

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m));
    return x;
}
__device__ __forceinline__ float wave_sum(float x) {                     // (x + y == y + x: every lane ends on the same bits)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// One block of 4 waves per (recording, chunk of kPostChunk windows).
//   - post / path_post: one thread per window (a row is 2 x 96 bytes in and 96 out, moved as float4s, as key_emissions_kernel's);
//   - the transition sums: wave v takes windows c0 + v, c0 + v + 4, ... of the chunk in turn, a lane 9 of the 576 cells of each (a
//     softmax over the wave: one maximum, one sum), and keeps its cells' running sums in registers.  The four waves' sums meet in LDS
//     and leave as one partial per chunk, added in wave order; key_xi_reduce_kernel adds the chunks in chunk order.  No atomics: the
//     order of every addition is fixed by the shape alone.
__device__ __forceinline__ void key_posteriors_block(const PostArgs& p, float (&part)[4][kCells]) {
    const int r = blockIdx.x / p.chunks, chunk = blockIdx.x - r * p.chunks, c0 = chunk * kPostChunk;
    const int W = p.windows, tid = threadIdx.x;
    const int n = clamped_count(p.counts, r, W);
    const size_t row0 = static_cast<size_t>(r) * W;
    if (p.post && tid < kPostChunk && c0 + tid < W) {
        const int w = c0 + tid;
        float4* const out = reinterpret_cast<float4*>(p.post + (row0 + w) * kKeys);
        float pp = 0.f;
        if (w < n) {
            const float4* const av = reinterpret_cast<const float4*>(p.a + (row0 + w) * kKeys);
            const float4* const bv = reinterpret_cast<const float4*>(p.b + (row0 + w) * kKeys);
            float s[kKeys];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const float4 x = av[q], y = bv[q];
                s[4 * q] = x.x + y.x; s[4 * q + 1] = x.y + y.y; s[4 * q + 2] = x.z + y.z; s[4 * q + 3] = x.w + y.w;
            }
            float mx = s[0];
#pragma unroll
            for (int k = 1; k < kKeys; ++k) mx = fmaxf(mx, s[k]);
            float z = 0.f;
#pragma unroll
            for (int k = 0; k < kKeys; ++k) { s[k] = __expf(s[k] - mx); z += s[k]; }
#pragma unroll
            for (int k = 0; k < kKeys; ++k) s[k] = s[k] / z;
#pragma unroll
            for (int q = 0; q < 6; ++q) out[q] = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
            if (p.path_post) {
                const int k0 = p.path[row0 + w];
#pragma unroll
                for (int k = 0; k < kKeys; ++k) pp = k == k0 ? s[k] : pp;   // (selects, not an indexed register array; -1 matches none)
            }
        } else {
#pragma unroll
            for (int q = 0; q < 6; ++q) out[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (p.path_post) p.path_post[row0 + w] = pp;
    }
    if (!p.xi_part) return;
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int kPer = kCells / 64;
    float A[kPer], acc[kPer];
    int ci[kPer], cj[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int cell = lane + 64 * q;
        ci[q] = cell / kKeys; cj[q] = cell - ci[q] * kKeys;
        A[q] = p.trans[cell];
        acc[q] = 0.f;
    }
    for (int k = 0; k < kPostChunk / 4; ++k) {
        const int w = c0 + wave + 4 * k;
        if (w < 1 || w >= n) continue;                                   // wave-uniform
        const float* const ap = p.a + (row0 + w - 1) * kKeys;
        const float* const bw = p.b + (row0 + w) * kKeys;
        const float* const ew = p.emis + (row0 + w) * kKeys;
        float x[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) x[q] = ((ap[ci[q]] + A[q]) + ew[cj[q]]) + bw[cj[q]];
        float mx = x[0];
#pragma unroll
        for (int q = 1; q < kPer; ++q) mx = fmaxf(mx, x[q]);
        mx = wave_max(mx);
        float z = 0.f;
#pragma unroll
        for (int q = 0; q < kPer; ++q) { x[q] = __expf(x[q] - mx); z += x[q]; }
        z = wave_sum(z);
#pragma unroll
        for (int q = 0; q < kPer; ++q) acc[q] += x[q] / z;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) part[wave][lane + 64 * q] = acc[q];
    __syncthreads();
    float* const dst = p.xi_part + static_cast<size_t>(blockIdx.x) * kCells;
    for (int cell = tid; cell < kCells; cell += 256) dst[cell] = ((part[0][cell] + part[1][cell]) + part[2][cell]) + part[3][cell];
}

__global__ __launch_bounds__(256) void key_posteriors_kernel(PostArgs p) {
    __shared__ float part[4][kCells];
    key_posteriors_block(p, part);
}

// xi_sum[r] = the chunks' partial sums, added in chunk order.
__global__ __launch_bounds__(192) void key_xi_reduce_kernel(const float* __restrict__ part, float* __restrict__ xi, int chunks) {
    const int r = blockIdx.x;
    for (int cell = threadIdx.x; cell < kCells; cell += 192) {
        float s = 0.f;
        for (int c = 0; c < chunks; ++c) s += part[(static_cast<size_t>(r) * chunks + c) * kCells + cell];
        xi[static_cast<size_t>(r) * kCells + cell] = s;
    }
}

// ---- a sequence loss for training: the conditional log-likelihood of the labelled windows under the tracker's own chain ----
// (semantics and formulas: include/ake_hip.h; host model: metrics.key_sequence_loss)
// Everything exists twice, as set 0 (the free emissions e) and set 1 (the clamped ones e~), laid out [set][recordings][windows][...], so
// that one launch covers both.  Launches: the emissions of both sets; the four chains of every recording side by side; the scalars
// (one block); the gradient per window; with d_trans two more (the per-chunk transition sums of both sets, then their ordered
// difference).  No float atomics and no sum whose order depends on anything but the shape.
// The emissions, the chains and the gradient are in DOUBLE.  The gradient is a difference of two posteriors that are nearly equal
// wherever the net is already right, and a posterior whose log-odds against its row's largest is L carries, out of float32 log-scores,
// a relative error of |L| * 2^-24 -- 1e-6 at |L| = 16, the float32 tracker's own (profiles/track_sequence.md has what the float32
// chains measured).  A training sequence is a handful of windows, so the slower step (48 double exponentials per lane) costs nothing
// that shows; the transition sums take float32 copies of the same scores through key_posteriors_kernel's own code.
constexpr double kSequenceClamp = -1e4;   // AKE_SEQUENCE_CLAMP: an off-label key of a labelled window

struct SeqArgs {
    const float* key;          // [rows][12]
    const float* tonic;        // [rows][12]
    const int* labels;         // [rows]; outside 0..23 = unlabelled
    const int* counts;         // nullable
    const float* trans;        // [24][24]
    const float* prior;        // [24], nullable = zeros
    int rows, windows, recordings;
    double scale;              // signature_weight / 12
    double* emis;              // [2][rows][24]
    double* a;                 // [2][rows][24] (rows behind the count are not written)
    double* b;
    float* emis32;             // the same three rounded to float32, for the transition sums
    float* a32;
    float* b32;
    double* loglik;            // [2][recordings]
    double* inv_n;             // [1]: 1 / N, 0 for N == 0
    float* scalars;            // [4]
    float* d_key;              // [rows][12]
    float* d_tonic;            // [rows][12]
    float* d_emis;             // [rows][24], nullable
};

// One thread per row: e by key_emissions_kernel's own arithmetic (emission_row) in double, and e~ beside it.
__global__ __launch_bounds__(256) void sequence_emissions_kernel(SeqArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    const size_t at = static_cast<size_t>(r) * kKeys, set = static_cast<size_t>(a.rows) * kKeys;
    double e[kKeys], ec[kKeys];
    if (behind_count(a.counts, a.windows, r)) {
        for (int k = 0; k < kKeys; ++k) e[k] = ec[k] = 0.0;
    } else {
        emission_row<double>(a.key, a.tonic, static_cast<size_t>(r), a.scale, e);
        const int label = a.labels[r];
        const bool labelled = static_cast<unsigned>(label) < static_cast<unsigned>(kKeys);
        for (int k = 0; k < kKeys; ++k) ec[k] = !labelled || k == label ? e[k] : kSequenceClamp;
    }
    for (int k = 0; k < kKeys; ++k) {
        a.emis[at + k] = e[k]; a.emis[set + at + k] = ec[k];
        a.emis32[at + k] = static_cast<float>(e[k]); a.emis32[set + at + k] = static_cast<float>(ec[k]);
    }
}

// log-sum-exp of 24 doubles about their largest
__device__ __forceinline__ double lse24(const double (&x)[kKeys]) {
    double mx = x[0];
    for (int k = 1; k < kKeys; ++k) mx = fmax(mx, x[k]);
    double z = 0.0;
    for (int k = 0; k < kKeys; ++k) z += exp(x[k] - mx);
    return mx + log(z);
}

// grid (recordings, 4): blockIdx.y = 2 * set + direction, one wave each, so the four chains of a recording run at the same time.  The
// recurrences of forward_backward_chain (include/ake_hip.h) in double and in the plainest layout: lane j < 24 holds state j and takes
// all 24 terms of its log-sum-exp; a step's scores travel through two LDS rows (the scores the recurrence reads, then the raw results
// the normaliser reads), each written, then read, between two barriers of the one wave.
__global__ __launch_bounds__(64) void key_sequence_chains_kernel(SeqArgs a) {
    __shared__ double row_lds[kKeys], raw_lds[kKeys];
    const int r = blockIdx.x, lane = threadIdx.x, W = a.windows;
    const bool back = blockIdx.y & 1, own = lane < kKeys;
    const int j = own ? lane : 0;                                        // (the other lanes run along on state 0 and write nothing)
    const size_t base = (static_cast<size_t>(blockIdx.y >> 1) * a.recordings + r) * W * kKeys;
    const double* const e = a.emis + base;
    double* const out = (back ? a.b : a.a) + base;
    float* const out32 = (back ? a.b32 : a.a32) + base;
    const int n = clamped_count(a.counts, r, W);
    double A[kKeys];                                                     // forward: column j of the transition; backward: row j
    for (int i = 0; i < kKeys; ++i) A[i] = back ? a.trans[j * kKeys + i] : a.trans[i * kKeys + j];
    double d = back ? 0.0 : (a.prior ? static_cast<double>(a.prior[j]) : 0.0), ll = 0.0;
    for (int t = 0; t < n; ++t) {                                        // n is wave-uniform: every lane meets every barrier
        const int w = back ? n - 1 - t : t;
        double raw;
        if (t == 0) {
            raw = back ? 0.0 : d + e[static_cast<size_t>(w) * kKeys + j];      // b_{n-1} = 0, a_0 = prior + e[0]
        } else {
            if (own) row_lds[lane] = back ? d + e[static_cast<size_t>(w + 1) * kKeys + j] : d;
            __syncthreads();
            double x[kKeys];
            for (int i = 0; i < kKeys; ++i) x[i] = row_lds[i] + A[i];
            raw = lse24(x);
            if (!back) raw += e[static_cast<size_t>(w) * kKeys + j];
        }
        if (!back || t > 0) {                                            // b_{n-1} stays 0, unnormalised
            if (own) raw_lds[lane] = raw;
            __syncthreads();
            double x[kKeys];
            for (int i = 0; i < kKeys; ++i) x[i] = raw_lds[i];
            const double cw = lse24(x);
            d = raw - cw;
            ll += cw;
        } else {
            d = raw;
        }
        if (own) {
            out[static_cast<size_t>(w) * kKeys + j] = d;
            out32[static_cast<size_t>(w) * kKeys + j] = static_cast<float>(d);
        }
    }
    if (!back && lane == 0) a.loglik[(blockIdx.y >> 1) * a.recordings + r] = ll;
}

// One block.  N = the labelled windows below their counts (an integer sum: any order gives the same), then thread 0 adds the chains'
// doubles in recording order: the loss is the difference of two large, nearly equal sums, so it is taken per recording and in double.
__global__ __launch_bounds__(256) void sequence_scalars_kernel(SeqArgs a) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int r = threadIdx.x; r < a.rows; r += blockDim.x)
        mine += !behind_count(a.counts, a.windows, r) && static_cast<unsigned>(a.labels[r]) < static_cast<unsigned>(kKeys);
    atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int N = s_n;
    double diff = 0.0, ll = 0.0, llc = 0.0;
    for (int r = 0; r < a.recordings; ++r) {
        const double x = a.loglik[r], y = a.loglik[a.recordings + r];
        diff += x - y; ll += x; llc += y;
    }
    const double inv = N > 0 ? 1.0 / N : 0.0;
    a.inv_n[0] = inv;
    a.scalars[0] = static_cast<float>(diff * inv);
    a.scalars[1] = static_cast<float>(ll * inv);
    a.scalars[2] = static_cast<float>(llc * inv);
    a.scalars[3] = static_cast<float>(N);
}

// softmax of a row of a + b
__device__ __forceinline__ void posterior_row(const double* a, const double* b, double (&s)[kKeys]) {
    for (int k = 0; k < kKeys; ++k) s[k] = a[k] + b[k];
    double mx = s[0];
    for (int k = 1; k < kKeys; ++k) mx = fmax(mx, s[k]);
    double z = 0.0;
    for (int k = 0; k < kKeys; ++k) { s[k] = exp(s[k] - mx); z += s[k]; }
    for (int k = 0; k < kKeys; ++k) s[k] = s[k] / z;
}

// One thread per window: g = (post - post~) / N, then its way back through the emission formula to the two heads' outputs.
__global__ __launch_bounds__(256) void sequence_grad_kernel(SeqArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    const size_t row = static_cast<size_t>(r);
    float4* const dk = reinterpret_cast<float4*>(a.d_key + row * 12);
    float4* const dt = reinterpret_cast<float4*>(a.d_tonic + row * 12);
    float4* const de = a.d_emis ? reinterpret_cast<float4*>(a.d_emis + row * kKeys) : nullptr;
    if (behind_count(a.counts, a.windows, r)) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = 0; q < 3; ++q) dk[q] = dt[q] = zero;
        if (de) for (int q = 0; q < 6; ++q) de[q] = zero;
        return;
    }
    const size_t set = static_cast<size_t>(a.rows) * kKeys;
    double g[kKeys], pc[kKeys];
    posterior_row(a.a + row * kKeys, a.b + row * kKeys, g);
    posterior_row(a.a + set + row * kKeys, a.b + set + row * kKeys, pc);
    const double inv = a.inv_n[0];
    double gsum = 0.0;
    for (int k = 0; k < kKeys; ++k) { g[k] = (g[k] - pc[k]) * inv; gsum += g[k]; }
    if (de)
        for (int q = 0; q < 6; ++q)
            de[q] = make_float4(static_cast<float>(g[4 * q]), static_cast<float>(g[4 * q + 1]), static_cast<float>(g[4 * q + 2]), static_cast<float>(g[4 * q + 3]));
    float p[12], t[12];
    for (int q = 0; q < 3; ++q) {
        const float4 pv = reinterpret_cast<const float4*>(a.key + row * 12)[q];
        const float4 tv = reinterpret_cast<const float4*>(a.tonic + row * 12)[q];
        p[4 * q] = pv.x; p[4 * q + 1] = pv.y; p[4 * q + 2] = pv.z; p[4 * q + 3] = pv.w;
        t[4 * q] = tv.x; t[4 * q + 1] = tv.y; t[4 * q + 2] = tv.z; t[4 * q + 3] = tv.w;
    }
    // the tonic head: e[k] holds log_softmax(tonic)[k mod 12]
    float tmax = t[0];
    for (int j = 1; j < 12; ++j) tmax = fmaxf(tmax, t[j]);
    double sm[12], se = 0.0;
    for (int j = 0; j < 12; ++j) { sm[j] = exp(static_cast<double>(t[j]) - tmax); se += sm[j]; }
    float out[12];
    for (int j = 0; j < 12; ++j) out[j] = static_cast<float>((g[j] + g[j + 12]) - (sm[j] / se) * gsum);
    for (int q = 0; q < 3; ++q) dt[q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    // the key head: the keys that share a scale share its sum (major m and minor m + 9); pitch class j lies inside the scales whose
    // major tonic m has bit (j - m) mod 12 of kMajorScale, and outside the others (the two sums are taken apart: they nearly cancel).
    // The derivative of a clamped or subnormal logarithm is 0: log p > -100 holds for every normal float32, so the comparison with
    // FLT_MIN decides alone.
    double G[12];
    for (int m = 0; m < 12; ++m) G[m] = g[12 + m] + g[(m + 9) % 12];
    for (int j = 0; j < 12; ++j) {
        double inside = 0.0, outside = 0.0;
        for (int m = 0; m < 12; ++m) {
            if ((kMajorScale >> ((j - m + 12) % 12)) & 1) inside += G[m];
            else outside += G[m];
        }
        const float q = 1.f - p[j];
        const double u = p[j] >= FLT_MIN ? 1.0 / p[j] : 0.0, v = q >= FLT_MIN ? 1.0 / q : 0.0;
        out[j] = static_cast<float>(a.scale * (inside * u - outside * v));
    }
    for (int q = 0; q < 3; ++q) dk[q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
}

// key_posteriors_kernel's transition sums for both sets: grid (recordings * chunks, 2), blockIdx.y = the set.
__global__ __launch_bounds__(256) void key_sequence_xi_kernel(PostArgs p, int recordings) {
    __shared__ float part[4][kCells];
    const size_t set = blockIdx.y, floats = static_cast<size_t>(recordings) * p.windows * kKeys;
    p.emis += set * floats; p.a += set * floats; p.b += set * floats;
    p.xi_part += set * recordings * p.chunks * kCells;
    key_posteriors_block(p, part);
}

// d_trans = sum_r (xi_sum[r] - xi~_sum[r]) / N: the chunks in chunk order, the recordings in recording order, in double.
__global__ __launch_bounds__(192) void sequence_trans_kernel(const float* __restrict__ part, const double* __restrict__ inv_n,
                                                             float* __restrict__ d_trans, int recordings, int chunks) {
    const size_t set = static_cast<size_t>(recordings) * chunks * kCells;
    for (int cell = threadIdx.x; cell < kCells; cell += 192) {
        double s = 0.0;
        for (int r = 0; r < recordings; ++r) {
            double x = 0.0, y = 0.0;
            for (int c = 0; c < chunks; ++c) {
                const size_t at = (static_cast<size_t>(r) * chunks + c) * kCells + cell;
                x += part[at]; y += part[set + at];
            }
            s += x - y;
        }
        d_trans[cell] = static_cast<float>(s * inv_n[0]);
    }
}

struct PostCarve {
    float* a;
    float* b;
    float* part;
    size_t total;
    int chunks;
};

bool carve_posteriors(int recordings, int windows, void* ws, PostCarve* pc) {
    if (recordings <= 0 || windows <= 0 || static_cast<long long>(recordings) * windows > (1ll << 30)) return false;
    pc->chunks = (windows + kPostChunk - 1) / kPostChunk;
    const size_t rows = static_cast<size_t>(recordings) * windows;
    ake::Carver c(ws, 0);
    pc->a = c.take<float>(rows * kKeys);
    pc->b = c.take<float>(rows * kKeys);
    pc->part = c.take<float>(static_cast<size_t>(recordings) * pc->chunks * kCells);
    pc->total = ake::align_up(c.off, 256);
    return true;
}

struct SeqCarve {
    double* emis;              // [2][rows][24]
    double* a;
    double* b;
    float* emis32;             // the same three in float32
    float* a32;
    float* b32;
    double* loglik;            // [2][recordings]
    double* inv_n;             // [1]
    float* part;               // [2][recordings][chunks][576]
    size_t total;
    int chunks;
};

bool carve_sequence(int recordings, int windows, void* ws, SeqCarve* sc) {
    if (recordings <= 0 || windows <= 0 || static_cast<long long>(recordings) * windows > (1ll << 28)) return false;
    sc->chunks = (windows + kPostChunk - 1) / kPostChunk;
    const size_t rows = static_cast<size_t>(recordings) * windows;
    ake::Carver c(ws, 0);
    sc->emis = c.take<double>(2 * rows * kKeys);
    sc->a = c.take<double>(2 * rows * kKeys);
    sc->b = c.take<double>(2 * rows * kKeys);
    sc->emis32 = c.take<float>(2 * rows * kKeys);
    sc->a32 = c.take<float>(2 * rows * kKeys);
    sc->b32 = c.take<float>(2 * rows * kKeys);
    sc->loglik = c.take<double>(2 * static_cast<size_t>(recordings));
    sc->inv_n = c.take<double>(1);
    sc->part = c.take<float>(2 * static_cast<size_t>(recordings) * sc->chunks * kCells);
    sc->total = ake::align_up(c.off, 256);
    return true;
}

// What the two stream entries (`name`, for the messages) check and count alike.  `fixed`: the pointers every call needs are there;
// `inputs` / `outputs`: those that a new / a written window needs; `need`: the entry's state size; `most`: the bound on *k_out.
// The count, on the host: window v leaves the lag once window v + lag has been stepped, a flush writes every window that is left.
int stream_call(const char* name, int recordings, int k, int64_t windows_before, int lag, int flush, bool fixed, bool inputs, bool outputs,
                const void* state_dev, size_t state_bytes, size_t need, int64_t most, int* k_out) {
    AKE_REQUIRE(lag >= 0 && lag <= kStreamMaxLag, AKE_ERR_INVALID, "%s: lag %d outside 0..%d", name, lag, kStreamMaxLag);
    AKE_REQUIRE(recordings > 0 && k >= 0 && windows_before >= 0 && static_cast<long long>(recordings) * k <= (1ll << 30), AKE_ERR_INVALID,
                "%s: bad shape (%d recordings, %d windows after %lld)", name, recordings, k, static_cast<long long>(windows_before));
    AKE_REQUIRE(fixed, AKE_ERR_INVALID, "%s: null argument", name);
    const int64_t first = windows_before > lag ? windows_before - lag : 0, total = windows_before + k;
    const int64_t n_out = (flush ? total : (total > lag ? total - lag : 0)) - first;
    AKE_REQUIRE(n_out <= most, AKE_ERR_INVALID, "%s: %lld windows to write", name, static_cast<long long>(n_out));
    AKE_REQUIRE((k == 0 || inputs) && (n_out == 0 || outputs), AKE_ERR_INVALID, "%s: null argument", name);
    AKE_REQUIRE(state_bytes >= need, AKE_ERR_WORKSPACE, "%s: state %zu < %zu bytes", name, state_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 15) == 0, AKE_ERR_INVALID, "%s: the state must be 16-byte aligned", name);
    *k_out = static_cast<int>(n_out);
    return AKE_OK;
}

}  // namespace

extern "C" {

int ake_key_emissions_f32(const float* key_dev, const float* tonic_dev, int rows, const int32_t* counts_dev, int windows_per_recording,
                          float signature_weight, float* emis_dev, ake_stream_t stream) {
    AKE_REQUIRE(key_dev && tonic_dev && emis_dev, AKE_ERR_INVALID, "key_emissions: null argument");
    AKE_REQUIRE(rows >= 0 && (!counts_dev || (windows_per_recording > 0 && rows % windows_per_recording == 0)), AKE_ERR_INVALID,
                "key_emissions: %d rows do not divide into recordings of %d windows", rows, windows_per_recording);
    AKE_REQUIRE(((reinterpret_cast<uintptr_t>(key_dev) | reinterpret_cast<uintptr_t>(tonic_dev) | reinterpret_cast<uintptr_t>(emis_dev)) & 15) == 0,
                AKE_ERR_INVALID, "key_emissions: the buffers must be 16-byte aligned");
    AKE_REQUIRE(std::isfinite(signature_weight), AKE_ERR_INVALID, "key_emissions: signature_weight is not finite");
    if (rows == 0) return AKE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    EmisArgs a{key_dev, tonic_dev, counts_dev, rows, counts_dev ? windows_per_recording : 1, signature_weight / 12.f, emis_dev};
    return ake::launch_flat("key_emissions_kernel", key_emissions_kernel, s, rows, a);
}

int ake_viterbi_chunk_windows(void) { return kVitChunk; }

size_t ake_viterbi_keys_workspace_bytes(int recordings, int windows) {
    if (recordings <= 0 || windows <= 0 || static_cast<long long>(recordings) * windows > (1ll << 30)) return 0;
    return ake::align_up(static_cast<size_t>(recordings) * ((windows + 3) / 4) * kKeys * sizeof(unsigned), 256);
}

int ake_viterbi_keys_f32(const float* emis_dev, int recordings, int windows, const int32_t* counts_dev, const float* log_trans_dev,
                         const float* log_prior_dev, int32_t* path_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(emis_dev && log_trans_dev && path_dev, AKE_ERR_INVALID, "viterbi_keys: null argument");
    const size_t need = ake_viterbi_keys_workspace_bytes(recordings, windows);
    AKE_REQUIRE(need > 0, AKE_ERR_INVALID, "viterbi_keys: bad shape (%d recordings, %d windows)", recordings, windows);
    AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "viterbi_keys: workspace %zu < %zu bytes", workspace_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, AKE_ERR_INVALID, "viterbi_keys: the workspace must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    VitArgs a{emis_dev, counts_dev, log_trans_dev, log_prior_dev, path_dev, static_cast<unsigned*>(workspace), windows, (windows + 3) / 4};
    return ake::launch("viterbi_keys_kernel", viterbi_keys_kernel, dim3(recordings), dim3(64), 0, s, a);
}

int ake_key_posteriors_chunk_windows(void) { return kPostChunk; }

size_t ake_key_posteriors_workspace_bytes(int recordings, int windows) {
    PostCarve pc;
    return carve_posteriors(recordings, windows, nullptr, &pc) ? pc.total : 0;
}

int ake_key_posteriors_f32(const float* emis_dev, int recordings, int windows, const int32_t* counts_dev, const float* log_trans_dev,
                           const float* log_prior_dev, const int32_t* path_dev, float* post_dev, float* loglik_dev, float* xi_sum_dev,
                           float* path_post_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(emis_dev && log_trans_dev && post_dev && loglik_dev, AKE_ERR_INVALID, "key_posteriors: null argument");
    AKE_REQUIRE(!path_post_dev || path_dev, AKE_ERR_INVALID, "key_posteriors: path_post_dev needs the path it reads (path_dev)");
    PostCarve pc;
    AKE_REQUIRE(carve_posteriors(recordings, windows, workspace, &pc), AKE_ERR_INVALID, "key_posteriors: bad shape (%d recordings, %d windows)",
                recordings, windows);
    AKE_REQUIRE(workspace && workspace_bytes >= pc.total, AKE_ERR_WORKSPACE, "key_posteriors: workspace %zu < %zu bytes", workspace_bytes, pc.total);
    AKE_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(post_dev)) & 15) == 0, AKE_ERR_INVALID,
                "key_posteriors: the workspace and post_dev must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FbArgs fa{emis_dev, counts_dev, log_trans_dev, log_prior_dev, pc.a, pc.b, loglik_dev, windows};
    int rc = ake::launch("key_forward_backward_kernel", key_forward_backward_kernel, dim3(recordings, 2), dim3(64), 0, s, fa);
    if (rc) return rc;
    PostArgs pa{emis_dev, counts_dev, log_trans_dev, path_post_dev ? path_dev : nullptr, pc.a, pc.b, post_dev, path_post_dev,
                xi_sum_dev ? pc.part : nullptr, windows, pc.chunks};
    rc = ake::launch("key_posteriors_kernel", key_posteriors_kernel, dim3(recordings * pc.chunks), dim3(256), 0, s, pa);
    if (rc || !xi_sum_dev) return rc;
    return ake::launch("key_xi_reduce_kernel", key_xi_reduce_kernel, dim3(recordings), dim3(192), 0, s, pc.part, xi_sum_dev, pc.chunks);
}

size_t ake_key_stream_state_bytes(int recordings, int lag) {
    if (recordings <= 0 || lag < 0 || lag > kStreamMaxLag) return 0;
    return static_cast<size_t>(recordings) * stream_state_stride(lag);
}

int ake_key_stream_step_f32(const float* emis_dev, int recordings, int k, int64_t windows_before, int lag, int flush,
                            const float* log_trans_dev, const float* log_prior_dev, void* state_dev, size_t state_bytes, float* filtered_dev,
                            int32_t* path_dev, int* k_out, ake_stream_t stream) {
    const int rc = stream_call("key_stream_step", recordings, k, windows_before, lag, flush, log_trans_dev && state_dev && k_out, emis_dev, path_dev,
                               state_dev, state_bytes, ake_key_stream_state_bytes(recordings, lag), INT_MAX, k_out);
    if (rc) return rc;
    const int n_out = *k_out;
    if (k == 0 && n_out == 0) return AKE_OK;                             // nothing to step and nothing to flush
    hipStream_t s = static_cast<hipStream_t>(stream);
    StreamStepArgs a{emis_dev, log_trans_dev, log_prior_dev, static_cast<unsigned char*>(state_dev), filtered_dev, path_dev,
                     static_cast<long long>(windows_before), k, lag, flush ? 1 : 0, n_out,
                     lag > 0 ? static_cast<int>(windows_before % lag) : 0};
    return ake::launch("key_stream_step_kernel", key_stream_step_kernel, dim3(recordings), dim3(64), 0, s, a);
}

size_t ake_key_stream_posteriors_state_bytes(int recordings, int lag) {
    if (recordings <= 0 || lag < 0 || lag > kStreamMaxLag) return 0;
    return static_cast<size_t>(recordings) * stream_post_stride(lag);
}

int ake_key_stream_posteriors_f32(const float* emis_dev, const float* filtered_dev, int recordings, int k, int64_t windows_before, int lag,
                                  int flush, const float* log_trans_dev, const float* log_prior_dev, const int32_t* path_dev, void* state_dev,
                                  size_t state_bytes, float* post_dev, float* path_post_dev, float* loglik_dev, int* k_out,
                                  ake_stream_t stream) {
    AKE_REQUIRE(!path_post_dev || path_dev, AKE_ERR_INVALID, "key_stream_posteriors: path_post_dev needs the path it reads (path_dev)");
    // the step entry's count, and a grid of one block per written row
    int rc = stream_call("key_stream_posteriors", recordings, k, windows_before, lag, flush, log_trans_dev && state_dev && k_out,
                               emis_dev && filtered_dev, post_dev, state_dev, state_bytes, ake_key_stream_posteriors_state_bytes(recordings, lag),
                               recordings > 0 ? INT_MAX / recordings : 0, k_out);
    if (rc) return rc;
    const int n_out = *k_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    StreamPostArgs a{emis_dev, filtered_dev, log_trans_dev, log_prior_dev, path_post_dev ? path_dev : nullptr,
                     static_cast<unsigned char*>(state_dev), post_dev, path_post_dev, loglik_dev, static_cast<long long>(windows_before), k, lag,
                     n_out};
    if (n_out > 0) {                                                     // the sweeps read the state of the calls before
        rc = ake::launch("key_stream_sweep_kernel", key_stream_sweep_kernel, dim3(static_cast<unsigned>(recordings * n_out)), dim3(64), 0, s, a);
        if (rc) return rc;
    }
    if (k == 0) return AKE_OK;                                           // no new window: the state stands
    return ake::launch("key_stream_loglik_kernel", key_stream_loglik_kernel, dim3(recordings), dim3(64), 0, s, a);
}

size_t ake_key_sequence_loss_workspace_bytes(int recordings, int windows) {
    SeqCarve sc;
    return carve_sequence(recordings, windows, nullptr, &sc) ? sc.total : 0;
}

int ake_key_sequence_loss_f32(const float* key_dev, const float* tonic_dev, const int32_t* labels_dev, int recordings, int windows,
                              const int32_t* counts_dev, const float* log_trans_dev, const float* log_prior_dev, float signature_weight,
                              float* scalars_dev, float* d_key_dev, float* d_tonic_dev, float* d_trans_dev, float* d_emis_dev, void* workspace,
                              size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(key_dev && tonic_dev && labels_dev && log_trans_dev && scalars_dev && d_key_dev && d_tonic_dev, AKE_ERR_INVALID,
                "key_sequence_loss: null argument");
    SeqCarve sc;
    AKE_REQUIRE(carve_sequence(recordings, windows, workspace, &sc), AKE_ERR_INVALID, "key_sequence_loss: bad shape (%d recordings, %d windows)",
                recordings, windows);
    AKE_REQUIRE(workspace && workspace_bytes >= sc.total, AKE_ERR_WORKSPACE, "key_sequence_loss: workspace %zu < %zu bytes", workspace_bytes, sc.total);
    AKE_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(key_dev) | reinterpret_cast<uintptr_t>(tonic_dev) |
                  reinterpret_cast<uintptr_t>(d_key_dev) | reinterpret_cast<uintptr_t>(d_tonic_dev) | reinterpret_cast<uintptr_t>(d_emis_dev)) & 15) == 0,
                AKE_ERR_INVALID, "key_sequence_loss: the workspace, the heads' outputs and their gradients must be 16-byte aligned");
    AKE_REQUIRE(std::isfinite(signature_weight), AKE_ERR_INVALID, "key_sequence_loss: signature_weight is not finite");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rows = recordings * windows;
    SeqArgs a{key_dev, tonic_dev, labels_dev, counts_dev, log_trans_dev, log_prior_dev, rows, windows, recordings,
              static_cast<double>(signature_weight) / 12.0, sc.emis, sc.a, sc.b, sc.emis32, sc.a32, sc.b32, sc.loglik, sc.inv_n, scalars_dev,
              d_key_dev, d_tonic_dev, d_emis_dev};
    int rc;
    if ((rc = ake::launch_flat("sequence_emissions_kernel", sequence_emissions_kernel, s, rows, a))) return rc;
    if ((rc = ake::launch("key_sequence_chains_kernel", key_sequence_chains_kernel, dim3(recordings, 4), dim3(64), 0, s, a))) return rc;
    if ((rc = ake::launch("sequence_scalars_kernel", sequence_scalars_kernel, dim3(1), dim3(256), 0, s, a))) return rc;
    rc = ake::launch_flat("sequence_grad_kernel", sequence_grad_kernel, s, rows, a);
    if (rc || !d_trans_dev) return rc;
    PostArgs pa{sc.emis32, counts_dev, log_trans_dev, nullptr, sc.a32, sc.b32, nullptr, nullptr, sc.part, windows, sc.chunks};
    if ((rc = ake::launch("key_sequence_xi_kernel", key_sequence_xi_kernel, dim3(recordings * sc.chunks, 2), dim3(256), 0, s, pa, recordings))) return rc;
    return ake::launch("sequence_trans_kernel", sequence_trans_kernel, dim3(1), dim3(192), 0, s, sc.part, sc.inv_n, d_trans_dev, recordings, sc.chunks);
}

}  // extern "C"
