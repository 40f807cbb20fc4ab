// Device-side audio preparation in front of the CQT: channel selection / mono mix-down and
// polyphase resampling, for ragged batches.
//
// The reference does neither: it takes channel 0 of whatever torchaudio.load returns, at the file's own sample rate, and sets
// hop = round(rate / frames) (KeyDataset.py:479-485).  With channel = 0 and rate_in == rate_out this stage is the identity on
// channel 0, i.e. the reference's behaviour; everything else is opt-in, for serving pipelines that hold decoded multi-channel
// audio of mixed rates on the GPU and want ONE CQT plan (one hop, one set of filter tables) for all of it.
//
// Resampling = scipy.signal.resample_poly(x, up, down) with its default filter (the checker, oracle/resample_oracle.py, is pinned
// on scipy itself):  up, down = rate_out, rate_in reduced by their gcd;  h = firwin(2 * half + 1, 1 / max(up, down),
// window = ("kaiser", 5.0)) * up  with  half = 10 * max(up, down);  y[k] = sum_i x[i] h[k * down - i * up + half],
// k < ceil(n * up / down).  One thread per output sample: ~20 * max(up, down) / up + 1 taps (41 for 44.1 -> 22.05 kHz, 44 for
// 48 -> 22.05 kHz), input and filter served from L1/L2 -- a streaming kernel, bound by HBM (4 B read per input sample and channel,
// 4 B written per output sample).
//
// Retuning (ake_retune_f32, not in the reference either) is the same stage with a ratio per row that is no fraction of small integers:
// rho = 2^(cents / 1200) undoes a detuning of `cents` (ake_tuning_estimate_f32 measures it).  Definition, table and order of the sums:
// metrics.retune_reference, the float64 model of retune_kernel.
//
// Both stages also run on audio that arrives in chunks (ake_stream_resample_*, ake_stream_retune_*): the offline kernel's sums over a
// short carried ring of inputs and the chunk, bit-identical to the offline call on the joined audio however it is cut.
#include "common.h"

#include <cmath>
#include <cstdint>
#include <numeric>

struct ake_resampler {
    int rate_in, rate_out, up, down, half;
    float* h_dev = nullptr;     // [2 * half + 1]
};

namespace {

double bessel_i0d(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / (static_cast<double>(k) * k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

struct ResampleArgs {
    const float* in;            // [batch][channels][n_in] by strides
    long long clip_stride, channel_stride;
    int channels, channel;      // channel >= 0: that channel; -1: mean over the channels
    long long n_in;
    const long long* n_in_clip; // ragged: samples of each clip (<= n_in), or null
    float* out;                 // [batch][out_stride]
    long long out_stride, n_out_max;
    long long* n_out_clip;      // per-clip output length written here (or null)
    const float* h;
    int up, down, half;
};

__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
    const int clip = blockIdx.y;
    long long n = a.n_in;
    if (a.n_in_clip) { const long long nc = a.n_in_clip[clip]; n = nc < 0 ? 0 : (nc < n ? nc : n); }
    const long long n_out = (n * a.up + a.down - 1) / a.down;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.n_out_clip) a.n_out_clip[clip] = n_out;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= a.n_out_max) return;
    float* o = a.out + clip * a.out_stride + k;
    if (k >= n_out) { *o = 0.f; return; }                         // zero padding behind a shorter clip
    const float* x = a.in + clip * a.clip_stride;
    const int nch = a.channel >= 0 ? 1 : a.channels;
    const long long c0 = a.channel >= 0 ? a.channel : 0;
    const float scale = a.channel >= 0 ? 1.f : 1.f / a.channels;
    float acc = 0.f;
    if (a.up == a.down) {                                         // same rate: channel selection / mix only
        for (int c = 0; c < nch; ++c) acc += x[(c0 + c) * a.channel_stride + k];
        *o = acc * scale;
        return;
    }
    const long long t = k * a.down;
    long long i_lo = t - a.half <= 0 ? 0 : (t - a.half + a.up - 1) / a.up;
    long long i_hi = (t + a.half) / a.up;
    i_hi = i_hi < n - 1 ? i_hi : n - 1;
    int j = static_cast<int>(t - i_lo * a.up + a.half);           // tap of input sample i_lo; the next sample's is up less
    for (long long i = i_lo; i <= i_hi; ++i, j -= a.up) {
        float v = 0.f;
        for (int c = 0; c < nch; ++c) v += x[(c0 + c) * a.channel_stride + i];
        acc = fmaf(v, a.h[j], acc);
    }
    *o = acc * scale;
}

// 16-bit PCM in place: sample s stands for float(s) * 2^-15 (exact), read at x[c * channel_stride + i * sample_stride] -- planar
// (B, C, n) and interleaved (B, n, C) storage alike.  Same order of additions and the same fmaf chain as resample_kernel, so the output
// is bit-identical to resample_kernel on the converted planar tensor.
struct ResamplePcmArgs {
    const short* in;
    long long clip_stride, channel_stride, sample_stride;
    int channels, channel;
    long long n_in;
    const long long* n_in_clip;
    float* out;
    long long out_stride, n_out_max;
    long long* n_out_clip;
    const float* h;
    int up, down, half;
};

__global__ __launch_bounds__(256) void resample_pcm16_kernel(ResamplePcmArgs a) {
    constexpr float kScale = 1.f / 32768.f;
    const int clip = blockIdx.y;
    long long n = a.n_in;
    if (a.n_in_clip) { const long long nc = a.n_in_clip[clip]; n = nc < 0 ? 0 : (nc < n ? nc : n); }
    const long long n_out = (n * a.up + a.down - 1) / a.down;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.n_out_clip) a.n_out_clip[clip] = n_out;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= a.n_out_max) return;
    float* o = a.out + clip * a.out_stride + k;
    if (k >= n_out) { *o = 0.f; return; }                         // zero padding behind a shorter clip
    const short* x = a.in + clip * a.clip_stride;
    const int nch = a.channel >= 0 ? 1 : a.channels;
    const long long c0 = a.channel >= 0 ? a.channel : 0;
    const float scale = a.channel >= 0 ? 1.f : 1.f / a.channels;
    float acc = 0.f;
    if (a.up == a.down) {                                         // same rate: channel selection / mix only
        for (int c = 0; c < nch; ++c) acc += static_cast<float>(x[(c0 + c) * a.channel_stride + k * a.sample_stride]) * kScale;
        *o = acc * scale;
        return;
    }
    const long long t = k * a.down;
    long long i_lo = t - a.half <= 0 ? 0 : (t - a.half + a.up - 1) / a.up;
    long long i_hi = (t + a.half) / a.up;
    i_hi = i_hi < n - 1 ? i_hi : n - 1;
    int j = static_cast<int>(t - i_lo * a.up + a.half);           // tap of input sample i_lo; the next sample's is up less
    for (long long i = i_lo; i <= i_hi; ++i, j -= a.up) {
        float v = 0.f;
        for (int c = 0; c < nch; ++c) v += static_cast<float>(x[(c0 + c) * a.channel_stride + i * a.sample_stride]) * kScale;
        acc = fmaf(v, a.h[j], acc);
    }
    *o = acc * scale;
}

// ---- retuning: varispeed resampling by a ratio per row ----
// y[k] = sum_j x[j] h(k / rho - j), h(d) = c sinc(c d) kaiser_beta(d / Z) on |d| < Z: 2 Z = 64 taps of a contiguous input stretch per
// output sample, and a filter phase of its own for every sample (rho is irrational), so there is no polyphase table to index.  h is
// held one-sided at kRetuneRes entries per sample, G[q] = h(q / kRetuneRes), and blended linearly between neighbours: 32 KiB of LDS.
// A workgroup loads it once and then makes kRetuneTiles tiles of kRetuneTile consecutive samples of one row; the input stretch of a
// tile (at most kRetuneTile * 2^(50/1200) + 2 Z + 1 samples) is staged in LDS as float32 -- the PCM form converts there, and nowhere
// else, so both forms run the same sums on the same values.  41 KiB per workgroup: three fit a CU.
constexpr int kRetuneZeros = 32;
constexpr int kRetuneRes = 256;
constexpr int kRetuneTable = kRetuneZeros * kRetuneRes + 1;       // G[Z * res] = h(Z) is stored as 0: the taps are |d| < Z
constexpr double kRetuneBeta = 9.0, kRetuneCutoff = 0.94, kRetuneMaxCents = 50.0;
constexpr double kRetuneMaxRatio = 1.029302236643492;            // 2^(50/1200) as one double: metrics.RETUNE_MAX_RATIO, host and device
constexpr int kRetuneTile = 2048, kRetuneTiles = 8, kRetuneThreads = 256;
constexpr int kRetuneStretch = 2240;                              // >= ceil(2047 * 1.02931) + 1 + 2 Z = 2173
static_assert(kRetuneTile % kRetuneThreads == 0 && (kRetuneRes & (kRetuneRes - 1)) == 0, "retune tiling");

__device__ float g_retune_table[kRetuneTable + 1];
ake::DeviceOnce g_retune_table_once;

template <typename T> __device__ __forceinline__ float retune_sample(T v);
template <> __device__ __forceinline__ float retune_sample<float>(float v) { return v; }
template <> __device__ __forceinline__ float retune_sample<short>(short v) { return static_cast<float>(v) * (1.f / 32768.f); }

// `cents` as a caller gives them -> what the retuner reads: NaN as 0, beyond +-50 as +-50.  Host and device.
__host__ __device__ __forceinline__ float retune_clamped(float cents) {
    return cents != cents ? 0.f : fminf(fmaxf(cents, -static_cast<float>(kRetuneMaxCents)), static_cast<float>(kRetuneMaxCents));
}

// clamped cents -> rho.  Device only: the host's exp2 may round the last place another way, and every count and every read position
// hangs on this double (ake_retune_ratio hands it to the host).
__device__ __forceinline__ double retune_ratio(float cents) {
    // at the clamp the ratio is the literal the buffer's width was sized with, so n_out < width whatever exp2 rounds to
    return cents >= static_cast<float>(kRetuneMaxCents) ? kRetuneMaxRatio
         : cents <= -static_cast<float>(kRetuneMaxCents) ? 1.0 / kRetuneMaxRatio : exp2(static_cast<double>(cents) / 1200.0);
}

// The 64 taps of one output sample: xs[m] = x[j0 + m], m = -Z + 1 .. Z, in LDS, and `fraction` in [0, 1) the read position behind j0.
// Shared by every retuner here (one ratio per row, a curve, chunks).
__device__ __forceinline__ float retune_taps(const float* xs, float fraction, const float* G) {
    const float fr = fraction * kRetuneRes;
    int r = static_cast<int>(fr);
    r = r < kRetuneRes - 1 ? r : kRetuneRes - 1;
    const float t = fr - static_cast<float>(r);
    float acc = 0.f;
    int q = r + (kRetuneZeros - 1) * kRetuneRes;
#pragma unroll 8
    for (int m = -kRetuneZeros + 1; m <= 0; ++m, q -= kRetuneRes)    // d = fraction - m >= 0
        acc = fmaf(xs[m], fmaf(t, G[q + 1] - G[q], G[q]), acc);
    q = kRetuneRes - r - 1;
#pragma unroll 8
    for (int m = 1; m <= kRetuneZeros; ++m, q += kRetuneRes)         // d < 0: h(-d), read downwards
        acc = fmaf(xs[m], fmaf(t, G[q] - G[q + 1], G[q + 1]), acc);
    return acc;
}

// Output sample k of a row: G the filter table and X the staged input stretch, both in LDS, X[j - j_base] = x[j] (zeros outside the row).
__device__ __forceinline__ float retune_output(long long k, double inv, const float* G, const float* X, long long j_base) {
    // the read position in double; only its fraction is rounded to float32, so the error does not grow with k
    const double pos = static_cast<double>(k) * inv, j0d = floor(pos);
    return retune_taps(X + (static_cast<long long>(j0d) - j_base), static_cast<float>(pos - j0d), G);
}

template <typename T>
struct RetuneArgs {
    const T* in;                // [batch][in_stride]
    long long in_stride, n_max;
    const long long* n_in;      // samples of each row (clamped to 0..n_max), or null
    const float* cents;         // [batch]
    float* out;                 // [batch][out_stride]; columns [0, width) are written
    long long out_stride, width;
    long long* n_out;           // [batch], or null
};

template <typename T>
__global__ __launch_bounds__(kRetuneThreads) void retune_kernel(RetuneArgs<T> a) {
    __shared__ float G[kRetuneTable + 1];
    __shared__ float X[kRetuneStretch];
    const int row = blockIdx.y, tid = threadIdx.x;
    long long n = a.n_max;
    if (a.n_in) { const long long nc = a.n_in[row]; n = nc < 0 ? 0 : (nc < n ? nc : n); }
    const float cents = retune_clamped(a.cents[row]);
    const bool copy = cents == 0.f;
    const double rho = retune_ratio(cents);
    const double inv = 1.0 / rho;
    long long n_out = copy ? n : static_cast<long long>(floor(static_cast<double>(n) * rho));
    n_out = n_out < a.width ? n_out : a.width - 1;                // (|cents| < 50: rho < the literal by far more than an ulp; a guard all the same)
    if (blockIdx.x == 0 && tid == 0 && a.n_out) a.n_out[row] = n_out;
    const T* x = a.in + row * a.in_stride;
    float* y = a.out + row * a.out_stride;
    const long long k_first = static_cast<long long>(blockIdx.x) * (kRetuneTile * kRetuneTiles);
    const bool filter = !copy && k_first < n_out;                 // (uniform over the workgroup)
    if (filter)
        for (int i = tid; i < kRetuneTable + 1; i += kRetuneThreads) G[i] = g_retune_table[i];
    for (int tile = 0; tile < kRetuneTiles; ++tile) {
        const long long k0 = k_first + static_cast<long long>(tile) * kRetuneTile;
        if (k0 >= a.width) break;
        if (copy || k0 >= n_out) {                                // a row that is not retuned, or the zeros behind a row's end
            for (int i = tid; i < kRetuneTile; i += kRetuneThreads) {
                const long long k = k0 + i;
                if (k < a.width) y[k] = k < n_out ? retune_sample<T>(x[k]) : 0.f;
            }
            continue;
        }
        // the tile's input stretch: sample j of the row at X[j - j_base], zeros outside [0, n)
        const long long j_base = static_cast<long long>(floor(static_cast<double>(k0) * inv)) - kRetuneZeros + 1;
        __syncthreads();                                          // (the last tile's reads of X are done)
        for (int i = tid; i < kRetuneStretch; i += kRetuneThreads) {
            const long long j = j_base + i;
            X[i] = (j >= 0 && j < n) ? retune_sample<T>(x[j]) : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < kRetuneTile; i += kRetuneThreads) {
            const long long k = k0 + i;
            if (k >= a.width) break;
            if (k >= n_out) { y[k] = 0.f; continue; }
            y[k] = retune_output(k, inv, G, X, j_base);
        }
    }
}

int retune_table_upload() {
    if (!g_retune_table_once.need()) return AKE_OK;
    std::vector<float> h(kRetuneTable + 1, 0.f);
    const double i0b = bessel_i0d(kRetuneBeta);
    for (int q = 0; q < kRetuneTable - 1; ++q) {
        const double d = static_cast<double>(q) / kRetuneRes, u = d / kRetuneZeros, a = M_PI * kRetuneCutoff * d;
        const double sinc = q == 0 ? 1.0 : std::sin(a) / a;
        h[q] = static_cast<float>(kRetuneCutoff * sinc * bessel_i0d(kRetuneBeta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b);
    }
    AKE_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_retune_table), h.data(), h.size() * sizeof(float)));
    g_retune_table_once.mark();
    return AKE_OK;
}

template <typename T>
int retune_launch(const char* name, const T* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* n_in_dev, const float* cents_dev,
                  float* out_dev, int64_t out_stride, int64_t* n_out_dev, ake_stream_t stream) {
    AKE_REQUIRE(in_dev && cents_dev && out_dev, AKE_ERR_INVALID, "%s: null argument", name);
    AKE_REQUIRE(batch > 0 && batch <= 65535 && n_max >= 0 && n_max <= (1ll << 40), AKE_ERR_INVALID, "%s: bad batch %d / n_max %lld", name, batch,
                static_cast<long long>(n_max));
    const int64_t width = ake_retune_out_len(n_max);
    AKE_REQUIRE(in_stride >= n_max && out_stride >= width, AKE_ERR_INVALID, "%s: row strides %lld, %lld < %lld input, %lld output samples", name,
                static_cast<long long>(in_stride), static_cast<long long>(out_stride), static_cast<long long>(n_max), static_cast<long long>(width));
    const int rc = retune_table_upload();
    if (rc) return rc;
    RetuneArgs<T> a{in_dev, in_stride, n_max, reinterpret_cast<const long long*>(n_in_dev), cents_dev, out_dev, out_stride, width,
                    reinterpret_cast<long long*>(n_out_dev)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr int per_block = kRetuneTile * kRetuneTiles;
    return ake::launch(name, retune_kernel<T>, dim3(static_cast<unsigned>((width + per_block - 1) / per_block), batch), dim3(kRetuneThreads), 0, s, a);
}

// ---- retuning along a curve: a ratio that is piecewise linear in the input position (ake_retune_curve_*) ----
// Knot i of a row sits at input sample p_i = knot_first + i knot_step and carries rho_i = retune_ratio(retune_clamped(cents[i])); rho is
// rho_0 in front of the first knot, rho_{K-1} behind the last and linear in p between two.  The output index of input position p is
// K(p) = integral of rho, piecewise quadratic: K_0 = rho_0 p_0, K_{i+1} = K_i + knot_step (rho_i + rho_{i+1}) / 2, and inside segment i
// K(p) = K_i + rho_i u + (rho_{i+1} - rho_i) u^2 / (2 knot_step), u = p - p_i.  Output k reads the position K^{-1}(k).
//   retune_curve_prefix_kernel: a workgroup per row writes rho_i, then one thread adds K_i in ascending i (double), the row's
//     n_out = floor(K(n)) and whether all its cents are 0 (such a row is copied) into the workspace.
//   retune_curve_kernel: retune_kernel's tiling, staging and taps (retune_taps).  How a tile finds its segments: every thread runs
//     the same binary search of the workspace for the segment of the tile's first output (uniform addresses, one search a tile), the
//     knots from there on are staged in LDS -- a tile of kRetuneTile outputs spans at most kRetuneTile / (64 / kRetuneMaxRatio) + 2 =
//     35 of them since knot_step >= 64 -- and every output searches those (six LDS reads).  The inverse inside a segment is the root
//     form u = 2 c / (rho_s + sqrt(rho_s^2 + 4 a c)), stable at a = 0; a sqrt and a division in double per output are the new work.
// The read position stays the integer p_s + floor(u) and the fraction u - floor(u): only the fraction is rounded to float32.
constexpr int kCurveKnots = 40;                                   // knots a tile stages
constexpr int kCurveMinStep = 64;
static_assert(kRetuneTile * kRetuneMaxRatio / kCurveMinStep + 3 <= kCurveKnots, "curve knots per tile");

// Where output k reads: -> the integer sample j0 and the fraction behind it.  kp / rh: K_i and rho_i of the `cnt` knots from knot
// `s_lo` on (LDS, or the workspace itself with s_lo = 0), kp[0] <= k unless s_lo == 0; rho_row: all the row's ratios (global).
__device__ __forceinline__ void retune_curve_read(long long k, const double* kp, const double* rh, int cnt, int s_lo, int knots,
                                                  long long knot_first, long long knot_step, const double* rho_row, long long* j0,
                                                  double* fraction) {
    const double kd = static_cast<double>(k);
    double u;
    long long base = 0;
    if (kd < kp[0]) {                                             // in front of the first knot
        u = kd / rh[0];
    } else {
        int lo = 0, hi = cnt;                                     // the last e with kp[e] <= k
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (kp[mid] <= kd) lo = mid; else hi = mid;
        }
        const int s = s_lo + lo;
        const double c = kd - kp[lo], r0 = rh[lo];
        base = knot_first + s * knot_step;
        if (s == knots - 1) {                                     // behind the last knot
            u = c / r0;
        } else {
            const double r1 = lo + 1 < cnt ? rh[lo + 1] : rho_row[s + 1];
            const double a = (r1 - r0) / (2.0 * static_cast<double>(knot_step));
            u = 2.0 * c / (r0 + sqrt(r0 * r0 + 4.0 * a * c));
        }
    }
    const double fl = floor(u);
    *j0 = base + static_cast<long long>(fl);
    *fraction = u - fl;
}

struct RetuneCurveKnots {
    const float* cents;         // [batch][cents_stride]
    long long cents_stride;
    int knots;
    long long knot_first, knot_step;
    double* rho;                // workspace: [batch][knots]
    double* kpos;               // workspace: [batch][knots]
    long long* meta;            // workspace: [batch][2]: n_out, copy
};

struct RetuneCurvePrefixArgs {
    RetuneCurveKnots c;
    long long n_max, width;
    const long long* n_in;      // or null
    long long* n_out;           // [batch], or null
};

__global__ __launch_bounds__(64) void retune_curve_prefix_kernel(RetuneCurvePrefixArgs a) {
    __shared__ int any_shared;
    const int row = blockIdx.x, tid = threadIdx.x, K = a.c.knots;
    const float* cents = a.c.cents + row * a.c.cents_stride;
    double* rho = a.c.rho + static_cast<long long>(row) * K;
    double* kpos = a.c.kpos + static_cast<long long>(row) * K;
    if (tid == 0) any_shared = 0;
    __syncthreads();
    int any = 0;
    for (int i = tid; i < K; i += 64) {
        const float c = retune_clamped(cents[i]);
        any |= c != 0.f;
        rho[i] = retune_ratio(c);
    }
    if (any) any_shared = 1;                                      // (every writer writes the same value)
    __syncthreads();
    if (tid != 0) return;
    const double step = static_cast<double>(a.c.knot_step);
    double acc = rho[0] * static_cast<double>(a.c.knot_first);
    kpos[0] = acc;
    for (int i = 1; i < K; ++i) {                                 // ascending i
        acc += step * (rho[i - 1] + rho[i]) / 2.0;
        kpos[i] = acc;
    }
    long long n = a.n_max;
    if (a.n_in) { const long long nc = a.n_in[row]; n = nc < 0 ? 0 : (nc < n ? nc : n); }
    const bool copy = !any_shared;
    long long n_out = n;
    if (!copy) {                                                  // floor(K(n))
        double kn;
        if (n <= a.c.knot_first) {
            kn = rho[0] * static_cast<double>(n);
        } else {
            long long i = (n - a.c.knot_first) / a.c.knot_step;
            i = i < K - 1 ? i : K - 1;
            const double u = static_cast<double>(n - (a.c.knot_first + i * a.c.knot_step));
            kn = i == K - 1 ? kpos[i] + rho[i] * u : kpos[i] + rho[i] * u + (rho[i + 1] - rho[i]) * u * u / (2.0 * step);
        }
        n_out = static_cast<long long>(floor(kn));
    }
    n_out = n_out < a.width ? n_out : a.width - 1;                // (rho <= the literal everywhere; a guard all the same, as in retune_kernel)
    a.c.meta[row * 2ll] = n_out;
    a.c.meta[row * 2ll + 1] = copy ? 1 : 0;
    if (a.n_out) a.n_out[row] = n_out;
}

template <typename T>
struct RetuneCurveArgs {
    const T* in;
    long long in_stride, n_max;
    const long long* n_in;
    RetuneCurveKnots c;
    float* out;
    long long out_stride, width;
};

template <typename T>
__global__ __launch_bounds__(kRetuneThreads) void retune_curve_kernel(RetuneCurveArgs<T> a) {
    __shared__ float G[kRetuneTable + 1];
    __shared__ float X[kRetuneStretch];
    __shared__ double SK[kCurveKnots], SR[kCurveKnots];
    const int row = blockIdx.y, tid = threadIdx.x, K = a.c.knots;
    long long n = a.n_max;
    if (a.n_in) { const long long nc = a.n_in[row]; n = nc < 0 ? 0 : (nc < n ? nc : n); }
    const long long n_out = a.c.meta[row * 2ll];
    const bool copy = a.c.meta[row * 2ll + 1] != 0;
    const double* rho = a.c.rho + static_cast<long long>(row) * K;
    const double* kpos = a.c.kpos + static_cast<long long>(row) * K;
    const T* x = a.in + row * a.in_stride;
    float* y = a.out + row * a.out_stride;
    const long long k_first = static_cast<long long>(blockIdx.x) * (kRetuneTile * kRetuneTiles);
    const bool filter = !copy && k_first < n_out;                 // (uniform over the workgroup)
    if (filter)
        for (int i = tid; i < kRetuneTable + 1; i += kRetuneThreads) G[i] = g_retune_table[i];
    for (int tile = 0; tile < kRetuneTiles; ++tile) {
        const long long k0 = k_first + static_cast<long long>(tile) * kRetuneTile;
        if (k0 >= a.width) break;
        if (copy || k0 >= n_out) {                                // a row that is not retuned, or the zeros behind a row's end
            for (int i = tid; i < kRetuneTile; i += kRetuneThreads) {
                const long long k = k0 + i;
                if (k < a.width) y[k] = k < n_out ? retune_sample<T>(x[k]) : 0.f;
            }
            continue;
        }
        // the tile's knots: from the last one at or in front of its first output (from knot 0 in front of them all)
        int lo = 0, hi = K;
        const double kd0 = static_cast<double>(k0);
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (kpos[mid] <= kd0) lo = mid; else hi = mid;
        }
        const int s_lo = lo, cnt = K - s_lo < kCurveKnots ? K - s_lo : kCurveKnots;
        __syncthreads();                                          // (the last tile's reads of X, SK and SR are done)
        if (tid < cnt) { SK[tid] = kpos[s_lo + tid]; SR[tid] = rho[s_lo + tid]; }
        __syncthreads();
        // the tile's input stretch: sample j of the row at X[j - j_base], zeros outside [0, n)
        long long j_first;
        double fraction;
        retune_curve_read(k0, SK, SR, cnt, s_lo, K, a.c.knot_first, a.c.knot_step, rho, &j_first, &fraction);
        const long long j_base = j_first - kRetuneZeros + 1;
        for (int i = tid; i < kRetuneStretch; i += kRetuneThreads) {
            const long long j = j_base + i;
            X[i] = (j >= 0 && j < n) ? retune_sample<T>(x[j]) : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < kRetuneTile; i += kRetuneThreads) {
            const long long k = k0 + i;
            if (k >= a.width) break;
            if (k >= n_out) { y[k] = 0.f; continue; }
            long long j0;
            retune_curve_read(k, SK, SR, cnt, s_lo, K, a.c.knot_first, a.c.knot_step, rho, &j0, &fraction);
            long long off = j0 - j_base;                          // Z - 1 .. kRetuneStretch - Z - 1 by the bound on rho; held there all the same
            off = off < kRetuneZeros - 1 ? kRetuneZeros - 1 : (off > kRetuneStretch - kRetuneZeros - 1 ? kRetuneStretch - kRetuneZeros - 1 : off);
            y[k] = retune_taps(X + off, static_cast<float>(fraction), G);
        }
    }
}

struct RetuneCurvePositionsArgs {
    RetuneCurveKnots c;
    const long long* index;     // [batch][m]
    double* positions;          // [batch][m]
    long long m;
};

__global__ __launch_bounds__(256) void retune_curve_positions_kernel(RetuneCurvePositionsArgs a) {
    const int row = blockIdx.y, K = a.c.knots;
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.m) return;
    const double* rho = a.c.rho + static_cast<long long>(row) * K;
    const double* kpos = a.c.kpos + static_cast<long long>(row) * K;
    long long j0;
    double fraction;
    retune_curve_read(a.index[row * a.m + i], kpos, rho, K, 0, K, a.c.knot_first, a.c.knot_step, rho, &j0, &fraction);
    a.positions[row * a.m + i] = static_cast<double>(j0) + fraction;
}

constexpr int kCurveMaxKnots = 1 << 22;
constexpr long long kCurveMaxStep = 1ll << 32;

bool retune_curve_shape_ok(int batch, int knots) { return batch > 0 && batch <= 65535 && knots >= 1 && knots <= kCurveMaxKnots; }

// The checks every curve entry point shares, and the carve-up of the workspace.
int retune_curve_knots(const char* name, const float* cents_dev, int batch, int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step,
                       void* workspace, size_t workspace_bytes, RetuneCurveKnots* c) {
    AKE_REQUIRE(cents_dev, AKE_ERR_INVALID, "%s: null argument", name);
    AKE_REQUIRE(batch > 0 && batch <= 65535, AKE_ERR_INVALID, "%s: bad batch %d", name, batch);
    AKE_REQUIRE(knots >= 1 && knots <= kCurveMaxKnots, AKE_ERR_INVALID, "%s: %d knots; a curve has 1..%d", name, knots, kCurveMaxKnots);
    AKE_REQUIRE(knot_step >= kCurveMinStep && knot_step <= kCurveMaxStep, AKE_ERR_INVALID, "%s: knot_step %lld; the knots lie %d..2^32 samples apart",
                name, static_cast<long long>(knot_step), kCurveMinStep);
    AKE_REQUIRE(knot_first >= 0 && knot_first <= (1ll << 40), AKE_ERR_INVALID, "%s: knot_first %lld lies outside 0..2^40", name,
                static_cast<long long>(knot_first));
    AKE_REQUIRE(cents_stride >= knots, AKE_ERR_INVALID, "%s: row stride %lld < %d knots", name, static_cast<long long>(cents_stride), knots);
    const size_t need = ake_retune_curve_workspace_bytes(batch, knots);
    AKE_REQUIRE(workspace && workspace_bytes >= need, AKE_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AKE_ERR_INVALID, "%s: the workspace must be 8-byte aligned", name);
    double* rho = static_cast<double*>(workspace);
    double* kpos = rho + static_cast<size_t>(batch) * knots;
    *c = RetuneCurveKnots{cents_dev, cents_stride, knots, knot_first, knot_step, rho, kpos,
                          reinterpret_cast<long long*>(kpos + static_cast<size_t>(batch) * knots)};
    return AKE_OK;
}

template <typename T>
int retune_curve_launch(const char* name, const T* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* n_in_dev, const float* cents_dev,
                        int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step, float* out_dev, int64_t out_stride,
                        int64_t* n_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(in_dev && cents_dev && out_dev, AKE_ERR_INVALID, "%s: null argument", name);
    AKE_REQUIRE(batch > 0 && batch <= 65535 && n_max >= 0 && n_max <= (1ll << 40), AKE_ERR_INVALID, "%s: bad batch %d / n_max %lld", name, batch,
                static_cast<long long>(n_max));
    const int64_t width = ake_retune_out_len(n_max);
    AKE_REQUIRE(in_stride >= n_max && out_stride >= width, AKE_ERR_INVALID, "%s: row strides %lld, %lld < %lld input, %lld output samples", name,
                static_cast<long long>(in_stride), static_cast<long long>(out_stride), static_cast<long long>(n_max), static_cast<long long>(width));
    RetuneCurveKnots c;
    int rc = retune_curve_knots(name, cents_dev, batch, knots, cents_stride, knot_first, knot_step, workspace, workspace_bytes, &c);
    if (rc) return rc;
    rc = retune_table_upload();
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RetuneCurvePrefixArgs p{c, n_max, width, reinterpret_cast<const long long*>(n_in_dev), reinterpret_cast<long long*>(n_out_dev)};
    rc = ake::launch("retune_curve_prefix_kernel", retune_curve_prefix_kernel, dim3(batch), dim3(64), 0, s, p);
    if (rc) return rc;
    RetuneCurveArgs<T> a{in_dev, in_stride, n_max, reinterpret_cast<const long long*>(n_in_dev), c, out_dev, out_stride, width};
    constexpr int per_block = kRetuneTile * kRetuneTiles;
    return ake::launch(name, retune_curve_kernel<T>, dim3(static_cast<unsigned>((width + per_block - 1) / per_block), batch), dim3(kRetuneThreads), 0, s, a);
}

// ---- the polyphase resampler on audio that arrives in chunks (ake_stream_resample_*) ----
// resample_kernel's sum over "what came before, then the chunk".  Input i of the stream is final output k's as soon as
// floor((k down + half) / up) <= i, and output k needs no input in front of ceil((k down - half) / up): with n_before inputs seen, the
// first output still to come reaches back at most floor(2 half / up) inputs.  Those are carried per recording as a ring of `tail`
// float32, input i at slot i % tail, holding the channel SUM (the 1 / channels scale comes last, as in resample_kernel), so a float32
// and a 16-bit stream carry the same values.
//   stream_resample_kernel: a workgroup makes kSrTile consecutive outputs of one recording.  It first stages the tile's input stretch in
//     LDS, every sample mixed once (ring slot for i < n_before, the chunk behind it), then runs resample_kernel's ascending fmaf chain on
//     it with the same i_lo / i_hi clamps: the output is bit-identical to the offline kernel's on the concatenated audio.
//   stream_resample_tail_kernel: the last `tail` inputs of the chunk go into their ring slots.
// Two launches, not one: the slots the chunk's end lands on are the slots the tile at the chunk's front still reads (whenever the chunk
// is longer than the ring), and those are different workgroups as soon as there is more than one tile.  The stream orders the launches;
// the first only reads the ring, the second only writes it, so no workgroup reads what another writes.  (One workgroup per recording
// with load - barrier - store, stream_history_kernel's way, would put a 10 s chunk of one recording on a single CU.)
constexpr int kSrThreads = 256, kSrTile = 512;
constexpr size_t kSrMaxLds = 64 * 1024;

template <typename T>
struct StreamResampleArgs {
    const T* chunk;             // [recordings][channels][m] by strides
    long long rec_stride, channel_stride, sample_stride;
    int channels, channel;
    long long n_before, n_total;       // inputs in front of this chunk, and with it
    long long k_first, k_count;        // outputs [k_first, k_first + k_count) are written
    float* state;               // [recordings][tail]
    int tail;
    float* out;                 // [recordings][out_stride]
    long long out_stride;
    const float* h;
    int up, down, half;
};

// sample i of the chunk, channels summed in channel order from 0.f as resample_kernel sums them
template <typename T>
__device__ __forceinline__ float stream_mixed(const StreamResampleArgs<T>& a, const T* x, long long i) {
    const int nch = a.channel >= 0 ? 1 : a.channels;
    const long long c0 = a.channel >= 0 ? a.channel : 0;
    float v = 0.f;
    for (int c = 0; c < nch; ++c) v += retune_sample<T>(x[(c0 + c) * a.channel_stride + i * a.sample_stride]);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kSrThreads) void stream_resample_kernel(StreamResampleArgs<T> a) {
    extern __shared__ float sr_stretch[];
    const int rec = blockIdx.y, tid = threadIdx.x;
    const long long q0 = static_cast<long long>(blockIdx.x) * kSrTile;               // the tile, counted from k_first
    const long long q1 = q0 + kSrTile < a.k_count ? q0 + kSrTile : a.k_count;
    const T* x = a.chunk + rec * a.rec_stride;
    float* y = a.out + rec * a.out_stride;
    const float scale = a.channel >= 0 ? 1.f : 1.f / a.channels;
    if (a.up == a.down) {                                         // same rate: output k is input k, out of the chunk; no state
        for (long long q = q0 + tid; q < q1; q += kSrThreads) y[q] = stream_mixed(a, x, a.k_first + q - a.n_before) * scale;
        return;
    }
    // the stretch: from the first output's i_lo to the last output's i_hi (both monotone in k)
    const long long ta = (a.k_first + q0) * a.down;
    const long long i_base = ta - a.half <= 0 ? 0 : (ta - a.half + a.up - 1) / a.up;
    long long i_end = ((a.k_first + q1 - 1) * a.down + a.half) / a.up;
    i_end = i_end < a.n_total - 1 ? i_end : a.n_total - 1;
    const float* ring = a.state + static_cast<long long>(rec) * a.tail;
    for (long long i = i_base + tid; i <= i_end; i += kSrThreads)
        sr_stretch[i - i_base] = i < a.n_before ? ring[i % a.tail] : stream_mixed(a, x, i - a.n_before);
    __syncthreads();
    for (long long q = q0 + tid; q < q1; q += kSrThreads) {
        const long long t = (a.k_first + q) * a.down;
        const long long i_lo = t - a.half <= 0 ? 0 : (t - a.half + a.up - 1) / a.up;
        long long i_hi = (t + a.half) / a.up;
        i_hi = i_hi < a.n_total - 1 ? i_hi : a.n_total - 1;       // (binds only under flush: an output is final once its i_hi has arrived)
        int j = static_cast<int>(t - i_lo * a.up + a.half);
        const float* xs = sr_stretch + (i_lo - i_base);
        float acc = 0.f;
        for (long long i = i_lo; i <= i_hi; ++i, j -= a.up) acc = fmaf(*xs++, a.h[j], acc);
        y[q] = acc * scale;
    }
}

template <typename T>
__global__ __launch_bounds__(kSrThreads) void stream_resample_tail_kernel(StreamResampleArgs<T> a) {
    const int rec = blockIdx.x;
    const T* x = a.chunk + rec * a.rec_stride;
    float* ring = a.state + static_cast<long long>(rec) * a.tail;
    const long long first = a.n_total - a.tail > a.n_before ? a.n_total - a.tail : a.n_before;
    for (long long i = first + threadIdx.x; i < a.n_total; i += kSrThreads) ring[i % a.tail] = stream_mixed(a, x, i - a.n_before);
}

int stream_resample_tail(const ake_resampler* r) { return (2 * r->half / r->up + 1 + 3) / 4 * 4; }

int64_t stream_resample_count(const ake_resampler* r, int64_t n, int flush) {
    if (r->up == r->down) return n;
    if (flush) return (n * r->up + r->down - 1) / r->down;
    const int64_t a = n * r->up - r->half - 1;                    // k is final iff k * down + half < n * up
    return a < 0 ? 0 : a / r->down + 1;
}

template <typename T>
int stream_resample(const char* name, const ake_resampler* r, const T* chunk_dev, int recordings, int channels, int64_t m, int64_t rec_stride,
                    int64_t channel_stride, int64_t sample_stride, int channel, int64_t n_before, int flush, void* state_dev, size_t state_bytes,
                    float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream) {
    AKE_REQUIRE(r && state_dev && k_out, AKE_ERR_INVALID, "%s: null resampler, state or k_out", name);
    AKE_REQUIRE(recordings >= 1 && recordings <= 65535 && channels >= 1 && channel >= -1 && channel < channels, AKE_ERR_INVALID,
                "%s: bad recordings %d / channels %d / channel %d", name, recordings, channels, channel);
    AKE_REQUIRE(m >= 0 && n_before >= 0 && m <= (1ll << 40) && n_before <= (1ll << 40), AKE_ERR_INVALID, "%s: bad m %lld / n_before %lld", name,
                static_cast<long long>(m), static_cast<long long>(n_before));
    AKE_REQUIRE(m == 0 || (chunk_dev && rec_stride >= 0 && channel_stride >= 0 && sample_stride >= 1), AKE_ERR_INVALID,
                "%s: null chunk or bad strides (%lld, %lld, %lld)", name, static_cast<long long>(rec_stride), static_cast<long long>(channel_stride),
                static_cast<long long>(sample_stride));
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 15) == 0, AKE_ERR_INVALID, "%s: the state must be 16-byte aligned", name);
    const size_t need = ake_stream_resample_state_bytes(r, recordings);
    AKE_REQUIRE(state_bytes >= need, AKE_ERR_WORKSPACE, "%s: state of %zu bytes, %zu needed", name, state_bytes, need);
    const int64_t k_first = stream_resample_count(r, n_before, 0), k_count = stream_resample_count(r, n_before + m, flush) - k_first;
    AKE_REQUIRE(k_count == 0 || (out_dev && out_stride >= k_count), AKE_ERR_INVALID, "%s: null output or out_stride %lld < %lld output samples",
                name, static_cast<long long>(out_stride), static_cast<long long>(k_count));
    const bool same = r->up == r->down;
    const size_t lds = same ? 0 : ((static_cast<size_t>(kSrTile - 1) * r->down + 2 * static_cast<size_t>(r->half)) / r->up + 2) * sizeof(float);
    AKE_REQUIRE(lds <= kSrMaxLds, AKE_ERR_UNSUPPORTED, "%s: %d -> %d Hz needs %zu bytes of LDS for a tile's input", name, r->rate_in, r->rate_out, lds);
    *k_out = k_count;
    StreamResampleArgs<T> a{chunk_dev, rec_stride, channel_stride, sample_stride, channels, channel, n_before, n_before + m, k_first, k_count,
                            static_cast<float*>(state_dev), stream_resample_tail(r), out_dev, out_stride, r->h_dev, r->up, r->down, r->half};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (k_count > 0) {
        const int rc = ake::launch("stream_resample_kernel", stream_resample_kernel<T>,
                                   dim3(static_cast<unsigned>((k_count + kSrTile - 1) / kSrTile), recordings), dim3(kSrThreads), lds, s, a);
        if (rc) return rc;
    }
    if (m > 0 && !same)
        return ake::launch("stream_resample_tail_kernel", stream_resample_tail_kernel<T>, dim3(recordings), dim3(kSrThreads), 0, s, a);
    return AKE_OK;
}

// ---- the retuner on audio that arrives in chunks (ake_stream_retune_*) ----
// retune_kernel's sum over "what came before, then the chunk", as stream_resample_kernel is resample_kernel's.  With inv = 1 / rho output k
// reads the inputs floor(k inv) - Z + 1 .. floor(k inv) + Z, so it is final once floor(double(k) inv) + Z <= N - 1 (N inputs so far; a
// prefix of the outputs, the product being monotone in k), and the first output still to come reaches back at most 2 Z - 1 = 63 inputs
// (floor(k inv) + Z > N - 1 for it).  Those are carried per recording as a ring of 2 Z float32, input i at slot i % 64, converted from PCM
// before they are stored.  Every count is the host's (stream_retune_count), from the rho that ake_retune_ratio read off the device once.
//   stream_retune_kernel: a workgroup loads the table and makes kSrtTiles tiles of kSrtTile consecutive outputs of one recording; a
//     tile's input stretch is staged in LDS (ring slot for i < n_before, the chunk behind it, zeros below 0 and -- under flush only -- at
//     and behind n_total), then every thread runs retune_output, retune_kernel's own per-sample code.
//   stream_retune_tail_kernel: the last 64 inputs of the chunk go into their ring slots.  A second launch for stream_resample_tail_kernel's
//     reason: the first only reads the ring, the second only writes it.
// Tiling: a push is 0.1 to 10 s, 2205 to 220500 outputs a recording.  The offline 2048 x 8 would put anything under 0.74 s on one workgroup
// a recording.  256 x 4: one output a thread and tile, 1024 a workgroup, so a 0.1 s push of one recording runs on 3 workgroups and a 10 s
// push on 216, one per CU; the 32 KiB table load (32 loads a thread) stands against 4 x 64 taps a thread, and 34 KiB of LDS let four
// workgroups share a CU.  Smaller tiles pay the table more often than they gain: a 0.1 s push is bound by its launches either way.
constexpr int kSrtThreads = 256, kSrtTile = 256, kSrtTiles = 4, kSrtRing = 2 * kRetuneZeros;
constexpr int kSrtStretch = 336;                                  // >= floor(255 * 1.02931) + 2 + 2 Z = 328
static_assert(kSrtTile == kSrtThreads && kSrtStretch >= static_cast<int>((kSrtTile - 1) * kRetuneMaxRatio) + 2 + 2 * kRetuneZeros, "stream retune tiling");

template <typename T>
struct StreamRetuneArgs {
    const T* chunk;             // [recordings][rec_stride]: m = n_total - n_before samples each
    long long rec_stride;
    long long n_before, n_total;       // inputs in front of this chunk, and with it
    long long k_first, k_count;        // outputs [k_first, k_first + k_count) are written
    double rho;
    int copy;                   // cents == 0: output k is input k, no state
    float* state;               // [recordings][kSrtRing]
    float* out;                 // [recordings][out_stride]
    long long out_stride;
};

template <typename T>
__global__ __launch_bounds__(kSrtThreads) void stream_retune_kernel(StreamRetuneArgs<T> a) {
    __shared__ float G[kRetuneTable + 1];
    __shared__ float X[kSrtStretch];
    const int rec = blockIdx.y, tid = threadIdx.x;
    const T* x = a.chunk + rec * a.rec_stride;
    float* y = a.out + rec * a.out_stride;
    const long long q_first = static_cast<long long>(blockIdx.x) * (kSrtTile * kSrtTiles);       // counted from k_first
    if (a.copy) {                                                 // k_first == n_before: output q of the call is sample q of the chunk
        const long long q_end = q_first + kSrtTile * kSrtTiles < a.k_count ? q_first + kSrtTile * kSrtTiles : a.k_count;
        for (long long q = q_first + tid; q < q_end; q += kSrtThreads) y[q] = retune_sample<T>(x[q]);
        return;
    }
    for (int i = tid; i < kRetuneTable + 1; i += kSrtThreads) G[i] = g_retune_table[i];
    const double inv = 1.0 / a.rho;
    const float* ring = a.state + static_cast<long long>(rec) * kSrtRing;
    for (int tile = 0; tile < kSrtTiles; ++tile) {
        const long long q0 = q_first + static_cast<long long>(tile) * kSrtTile;
        if (q0 >= a.k_count) break;                               // (uniform over the workgroup)
        // the tile's input stretch: input j of the stream at X[j - j_base]; j >= n_before - 63 for the first tile, so the ring holds it
        const long long j_base = static_cast<long long>(floor(static_cast<double>(a.k_first + q0) * inv)) - kRetuneZeros + 1;
        __syncthreads();                                          // (the last tile's reads of X are done)
        for (int i = tid; i < kSrtStretch; i += kSrtThreads) {
            const long long j = j_base + i;
            float v = 0.f;
            if (j >= 0 && j < a.n_total) v = j < a.n_before ? ring[j % kSrtRing] : retune_sample<T>(x[j - a.n_before]);
            X[i] = v;
        }
        __syncthreads();
        const long long q = q0 + tid;
        if (q < a.k_count) y[q] = retune_output(a.k_first + q, inv, G, X, j_base);
    }
}

template <typename T>
__global__ __launch_bounds__(kSrtRing) void stream_retune_tail_kernel(StreamRetuneArgs<T> a) {
    const int rec = blockIdx.x;
    const T* x = a.chunk + rec * a.rec_stride;
    float* ring = a.state + static_cast<long long>(rec) * kSrtRing;
    const long long first = a.n_total - kSrtRing > a.n_before ? a.n_total - kSrtRing : a.n_before;
    const long long i = first + threadIdx.x;
    if (i < a.n_total) ring[i % kSrtRing] = retune_sample<T>(x[i - a.n_before]);
}

__global__ void retune_ratio_kernel(float cents, double* rho) { *rho = retune_ratio(retune_clamped(cents)); }

bool retune_ratio_ok(double rho) { return rho >= 1.0 / kRetuneMaxRatio && rho <= kRetuneMaxRatio; }      // (false for NaN)

// `cents` clamped.  The predicate is evaluated in the double expression the kernel's read position is, never in a closed form.
int64_t stream_retune_count(float cents, double rho, int64_t n, int flush) {
    if (cents == 0.f) return n;
    if (flush) {                                                  // the offline count, under retune_kernel's width guard
        const int64_t n_out = static_cast<int64_t>(std::floor(static_cast<double>(n) * rho)), width = ake_retune_out_len(n);
        return n_out < width ? n_out : width - 1;
    }
    const double inv = 1.0 / rho;
    auto is_final = [&](int64_t k) { return static_cast<int64_t>(std::floor(static_cast<double>(k) * inv)) + kRetuneZeros <= n - 1; };
    int64_t k = n > kRetuneZeros ? static_cast<int64_t>(std::floor(static_cast<double>(n - kRetuneZeros) * rho)) : 0;
    while (k > 0 && !is_final(k - 1)) --k;                           // (a step or two: the guess is off by the roundings alone)
    while (is_final(k)) ++k;
    return k;
}

template <typename T>
int stream_retune(const char* name, const T* chunk_dev, int recordings, int64_t m, int64_t rec_stride, float cents, double rho, int64_t n_before,
                  int flush, void* state_dev, size_t state_bytes, float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream) {
    AKE_REQUIRE(state_dev && k_out, AKE_ERR_INVALID, "%s: null state or k_out", name);
    AKE_REQUIRE(recordings >= 1 && recordings <= 65535, AKE_ERR_INVALID, "%s: bad recordings %d", name, recordings);
    AKE_REQUIRE(m >= 0 && n_before >= 0 && m <= (1ll << 40) && n_before <= (1ll << 40), AKE_ERR_INVALID, "%s: bad m %lld / n_before %lld", name,
                static_cast<long long>(m), static_cast<long long>(n_before));
    AKE_REQUIRE(m == 0 || (chunk_dev && rec_stride >= 0), AKE_ERR_INVALID, "%s: null chunk or bad row stride %lld", name,
                static_cast<long long>(rec_stride));
    AKE_REQUIRE(retune_ratio_ok(rho), AKE_ERR_INVALID, "%s: rho %g is no ratio of the retuner (ake_retune_ratio gives it)", name, rho);
    AKE_REQUIRE((reinterpret_cast<uintptr_t>(state_dev) & 15) == 0, AKE_ERR_INVALID, "%s: the state must be 16-byte aligned", name);
    const size_t need = ake_stream_retune_state_bytes(recordings);
    AKE_REQUIRE(state_bytes >= need, AKE_ERR_WORKSPACE, "%s: state of %zu bytes, %zu needed", name, state_bytes, need);
    cents = retune_clamped(cents);
    const bool copy = cents == 0.f;
    const int64_t k_first = stream_retune_count(cents, rho, n_before, 0), k_count = stream_retune_count(cents, rho, n_before + m, flush) - k_first;
    AKE_REQUIRE(k_count >= 0 && (k_count == 0 || (out_dev && out_stride >= k_count)), AKE_ERR_INVALID,
                "%s: null output or out_stride %lld < %lld output samples", name, static_cast<long long>(out_stride), static_cast<long long>(k_count));
    if (k_count > 0 && !copy) {
        const int rc = retune_table_upload();
        if (rc) return rc;
    }
    *k_out = k_count;
    StreamRetuneArgs<T> a{chunk_dev, rec_stride, n_before, n_before + m, k_first, k_count, rho, copy ? 1 : 0, static_cast<float*>(state_dev), out_dev,
                          out_stride};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (k_count > 0) {
        constexpr int per_block = kSrtTile * kSrtTiles;
        const int rc = ake::launch("stream_retune_kernel", stream_retune_kernel<T>, dim3(static_cast<unsigned>((k_count + per_block - 1) / per_block), recordings),
                                   dim3(kSrtThreads), 0, s, a);
        if (rc) return rc;
    }
    if (m > 0 && !copy && !flush)                                 // (behind a flush nothing is carried)
        return ake::launch("stream_retune_tail_kernel", stream_retune_tail_kernel<T>, dim3(recordings), dim3(kSrtRing), 0, s, a);
    return AKE_OK;
}

}  // namespace

extern "C" {

int ake_resampler_create(int rate_in, int rate_out, ake_resampler** out) {
    AKE_REQUIRE(out && rate_in > 0 && rate_out > 0, AKE_ERR_INVALID, "ake_resampler_create: bad argument");
    auto* r = new ake_resampler();
    r->rate_in = rate_in; r->rate_out = rate_out;
    const int g = std::gcd(rate_in, rate_out);
    r->up = rate_out / g; r->down = rate_in / g;
    const int mr = std::max(r->up, r->down);
    r->half = 10 * mr;
    AKE_REQUIRE(r->half <= (1 << 22), AKE_ERR_UNSUPPORTED, "resampler: %d -> %d Hz needs a %d-tap filter", rate_in, rate_out, 2 * r->half + 1);
    // scipy.signal.firwin(2 * half + 1, 1 / mr, window = ("kaiser", 5.0)), scaled by `up` (resample_poly)
    const int N = 2 * r->half + 1;
    std::vector<double> h(N);
    const double fc = 1.0 / mr, beta = 5.0, i0b = bessel_i0d(beta);
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
        const double m = i - r->half;
        const double sinc = m == 0 ? 1.0 : std::sin(M_PI * fc * m) / (M_PI * fc * m);
        const double rr = 2.0 * i / (N - 1) - 1.0;
        const double win = bessel_i0d(beta * std::sqrt(std::max(0.0, 1.0 - rr * rr))) / i0b;
        h[i] = fc * sinc * win;
        sum += h[i];
    }
    std::vector<float> hf(N);
    for (int i = 0; i < N; ++i) hf[i] = static_cast<float>(h[i] / sum * r->up);
    hipError_t e = hipMalloc(&r->h_dev, N * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(r->h_dev, hf.data(), N * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ake::set_error("resampler: filter upload failed: %s", hipGetErrorString(e));
        ake_resampler_destroy(r);
        return AKE_ERR_HIP;
    }
    *out = r;
    return AKE_OK;
}

void ake_resampler_destroy(ake_resampler* r) {
    if (!r) return;
    if (r->h_dev) (void)hipFree(r->h_dev);
    delete r;
}

int64_t ake_resampler_out_len(const ake_resampler* r, int64_t n_in) {
    if (!r || n_in < 0) return -1;
    return (n_in * r->up + r->down - 1) / r->down;
}

int ake_resample_f32(const ake_resampler* r, const float* in_dev, int batch, int channels, int64_t n_in, int64_t clip_stride,
                     int64_t channel_stride, int channel, const int64_t* n_in_clip_dev, float* out_dev, int64_t out_stride,
                     int64_t* n_out_clip_dev, ake_stream_t stream) {
    AKE_REQUIRE(r && in_dev && out_dev, AKE_ERR_INVALID, "ake_resample_f32: null argument");
    AKE_REQUIRE(batch > 0 && channels > 0 && n_in > 0 && channel >= -1 && channel < channels, AKE_ERR_INVALID, "resample: bad batch / channels / channel");
    const int64_t n_out = ake_resampler_out_len(r, n_in);
    AKE_REQUIRE(out_stride >= n_out, AKE_ERR_INVALID, "resample: out_stride %lld < %lld output samples", static_cast<long long>(out_stride), static_cast<long long>(n_out));
    ResampleArgs a;
    a.in = in_dev; a.clip_stride = clip_stride; a.channel_stride = channel_stride; a.channels = channels; a.channel = channel;
    a.n_in = n_in; a.n_in_clip = reinterpret_cast<const long long*>(n_in_clip_dev);
    a.out = out_dev; a.out_stride = out_stride; a.n_out_max = n_out; a.n_out_clip = reinterpret_cast<long long*>(n_out_clip_dev);
    a.h = r->h_dev; a.up = r->up; a.down = r->down; a.half = r->half;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return ake::launch("resample_kernel", resample_kernel, dim3(static_cast<unsigned>((n_out + 255) / 256), batch), dim3(256), 0, s, a);
}

int ake_resample_pcm16_f32(const ake_resampler* r, const int16_t* in_dev, int batch, int channels, int64_t n_in, int64_t clip_stride,
                           int64_t channel_stride, int64_t sample_stride, int channel, const int64_t* n_in_clip_dev, float* out_dev,
                           int64_t out_stride, int64_t* n_out_clip_dev, ake_stream_t stream) {
    AKE_REQUIRE(r && in_dev && out_dev, AKE_ERR_INVALID, "ake_resample_pcm16_f32: null argument");
    AKE_REQUIRE(batch > 0 && channels > 0 && n_in > 0 && channel >= -1 && channel < channels, AKE_ERR_INVALID, "resample: bad batch / channels / channel");
    AKE_REQUIRE(clip_stride >= 0 && channel_stride >= 0 && sample_stride >= 1, AKE_ERR_INVALID, "resample: bad strides (%lld, %lld, %lld)",
                static_cast<long long>(clip_stride), static_cast<long long>(channel_stride), static_cast<long long>(sample_stride));
    const int64_t n_out = ake_resampler_out_len(r, n_in);
    AKE_REQUIRE(out_stride >= n_out, AKE_ERR_INVALID, "resample: out_stride %lld < %lld output samples", static_cast<long long>(out_stride), static_cast<long long>(n_out));
    ResamplePcmArgs a;
    a.in = in_dev; a.clip_stride = clip_stride; a.channel_stride = channel_stride; a.sample_stride = sample_stride; a.channels = channels;
    a.channel = channel; a.n_in = n_in; a.n_in_clip = reinterpret_cast<const long long*>(n_in_clip_dev);
    a.out = out_dev; a.out_stride = out_stride; a.n_out_max = n_out; a.n_out_clip = reinterpret_cast<long long*>(n_out_clip_dev);
    a.h = r->h_dev; a.up = r->up; a.down = r->down; a.half = r->half;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return ake::launch("resample_pcm16_kernel", resample_pcm16_kernel, dim3(static_cast<unsigned>((n_out + 255) / 256), batch), dim3(256), 0, s, a);
}

int64_t ake_stream_resample_out_count(const ake_resampler* r, int64_t n_in, int flush) {
    if (!r || n_in < 0 || n_in > (1ll << 40)) return -1;
    return stream_resample_count(r, n_in, flush);
}

size_t ake_stream_resample_state_bytes(const ake_resampler* r, int recordings) {
    if (!r || recordings < 1 || recordings > 65535) return 0;
    return static_cast<size_t>(recordings) * stream_resample_tail(r) * sizeof(float);
}

int ake_stream_resample_f32(const ake_resampler* r, const float* chunk_dev, int recordings, int channels, int64_t m, int64_t rec_stride,
                            int64_t channel_stride, int channel, int64_t n_before, int flush, void* state_dev, size_t state_bytes,
                            float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream) {
    return stream_resample<float>("ake_stream_resample_f32", r, chunk_dev, recordings, channels, m, rec_stride, channel_stride, 1, channel, n_before,
                                  flush, state_dev, state_bytes, out_dev, out_stride, k_out, stream);
}

int ake_stream_resample_pcm16_f32(const ake_resampler* r, const int16_t* chunk_dev, int recordings, int channels, int64_t m, int64_t rec_stride,
                                  int64_t channel_stride, int64_t sample_stride, int channel, int64_t n_before, int flush, void* state_dev,
                                  size_t state_bytes, float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream) {
    return stream_resample<short>("ake_stream_resample_pcm16_f32", r, reinterpret_cast<const short*>(chunk_dev), recordings, channels, m, rec_stride,
                                  channel_stride, sample_stride, channel, n_before, flush, state_dev, state_bytes, out_dev, out_stride, k_out,
                                  stream);
}

int64_t ake_retune_out_len(int64_t n) {
    if (n < 0 || n > (1ll << 40)) return -1;
    return static_cast<int64_t>(std::floor(static_cast<double>(n) * kRetuneMaxRatio)) + 1;
}

int ake_retune_f32(const float* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev, const float* cents_dev,
                   float* out_dev, int64_t out_stride, int64_t* lengths_out_dev, ake_stream_t stream) {
    return retune_launch<float>("retune_kernel", in_dev, batch, n_max, in_stride, lengths_dev, cents_dev, out_dev, out_stride, lengths_out_dev, stream);
}

int ake_retune_pcm16_f32(const int16_t* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev, const float* cents_dev,
                         float* out_dev, int64_t out_stride, int64_t* lengths_out_dev, ake_stream_t stream) {
    return retune_launch<short>("retune_pcm16_kernel", reinterpret_cast<const short*>(in_dev), batch, n_max, in_stride, lengths_dev, cents_dev,
                                out_dev, out_stride, lengths_out_dev, stream);
}

size_t ake_retune_curve_workspace_bytes(int batch, int knots) {
    if (!retune_curve_shape_ok(batch, knots)) return 0;
    return ake::align_up((static_cast<size_t>(batch) * knots * 2 + static_cast<size_t>(batch) * 2) * sizeof(double), 256);
}

int ake_retune_curve_f32(const float* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev, const float* cents_dev,
                         int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step, float* out_dev, int64_t out_stride,
                         int64_t* lengths_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    return retune_curve_launch<float>("retune_curve_kernel", in_dev, batch, n_max, in_stride, lengths_dev, cents_dev, knots, cents_stride, knot_first,
                                      knot_step, out_dev, out_stride, lengths_out_dev, workspace, workspace_bytes, stream);
}

int ake_retune_curve_pcm16_f32(const int16_t* in_dev, int batch, int64_t n_max, int64_t in_stride, const int64_t* lengths_dev,
                               const float* cents_dev, int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step, float* out_dev,
                               int64_t out_stride, int64_t* lengths_out_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    return retune_curve_launch<short>("retune_curve_pcm16_kernel", reinterpret_cast<const short*>(in_dev), batch, n_max, in_stride, lengths_dev,
                                      cents_dev, knots, cents_stride, knot_first, knot_step, out_dev, out_stride, lengths_out_dev, workspace,
                                      workspace_bytes, stream);
}

int ake_retune_curve_positions(const float* cents_dev, int batch, int knots, int64_t cents_stride, int64_t knot_first, int64_t knot_step,
                               const int64_t* out_index_dev, int64_t m, double* positions_dev, void* workspace, size_t workspace_bytes,
                               ake_stream_t stream) {
    const char* name = "ake_retune_curve_positions";
    AKE_REQUIRE(out_index_dev && positions_dev, AKE_ERR_INVALID, "%s: null argument", name);
    AKE_REQUIRE(m >= 1 && m <= (1ll << 31), AKE_ERR_INVALID, "%s: %lld indices a row; 1..2^31", name, static_cast<long long>(m));
    RetuneCurveKnots c;
    int rc = retune_curve_knots(name, cents_dev, batch, knots, cents_stride, knot_first, knot_step, workspace, workspace_bytes, &c);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RetuneCurvePrefixArgs p{c, 0, 1, nullptr, nullptr};
    rc = ake::launch("retune_curve_prefix_kernel", retune_curve_prefix_kernel, dim3(batch), dim3(64), 0, s, p);
    if (rc) return rc;
    RetuneCurvePositionsArgs a{c, reinterpret_cast<const long long*>(out_index_dev), positions_dev, m};
    return ake::launch("retune_curve_positions_kernel", retune_curve_positions_kernel, dim3(static_cast<unsigned>((m + 255) / 256), batch), dim3(256), 0,
                       s, a);
}

int ake_retune_ratio(float cents, double* rho_out, ake_stream_t stream) {
    AKE_REQUIRE(rho_out, AKE_ERR_INVALID, "ake_retune_ratio: null rho_out");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* rho_dev = nullptr;
    AKE_HIP_CHECK(hipMalloc(&rho_dev, sizeof(double)));
    int rc = ake::launch("retune_ratio_kernel", retune_ratio_kernel, dim3(1), dim3(1), 0, s, cents, rho_dev);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(rho_out, rho_dev, sizeof(double), hipMemcpyDeviceToHost, s);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(rho_dev);
    if (e != hipSuccess) {
        ake::set_error("ake_retune_ratio: reading the ratio back failed: %s", hipGetErrorString(e));
        return AKE_ERR_HIP;
    }
    return rc;
}

int64_t ake_stream_retune_out_count(float cents, double rho, int64_t n_in, int flush) {
    if (n_in < 0 || n_in > (1ll << 40) || !retune_ratio_ok(rho)) return -1;
    return stream_retune_count(retune_clamped(cents), rho, n_in, flush);
}

size_t ake_stream_retune_state_bytes(int recordings) {
    if (recordings < 1 || recordings > 65535) return 0;
    return static_cast<size_t>(recordings) * kSrtRing * sizeof(float);
}

int ake_stream_retune_f32(const float* chunk_dev, int recordings, int64_t m, int64_t rec_stride, float cents, double rho, int64_t n_before, int flush,
                          void* state_dev, size_t state_bytes, float* out_dev, int64_t out_stride, int64_t* k_out, ake_stream_t stream) {
    return stream_retune<float>("ake_stream_retune_f32", chunk_dev, recordings, m, rec_stride, cents, rho, n_before, flush, state_dev, state_bytes,
                                out_dev, out_stride, k_out, stream);
}

int ake_stream_retune_pcm16_f32(const int16_t* chunk_dev, int recordings, int64_t m, int64_t rec_stride, float cents, double rho, int64_t n_before,
                                int flush, void* state_dev, size_t state_bytes, float* out_dev, int64_t out_stride, int64_t* k_out,
                                ake_stream_t stream) {
    return stream_retune<short>("ake_stream_retune_pcm16_f32", reinterpret_cast<const short*>(chunk_dev), recordings, m, rec_stride, cents, rho,
                                n_before, flush, state_dev, state_bytes, out_dev, out_stride, k_out, stream);
}

}  // extern "C"
