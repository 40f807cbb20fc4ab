// Key tracking over long recordings: ONE CQT per recording, then the clip-level net on sliding windows of its frames, then a decode of
// every window's (key, tonic) outputs to a key label -- all on one stream, no host round trip.
//
// Semantics (also include/ake_hip.h and INTEGRATION.md):
//   - a recording of n samples is transformed once at the plan's hop: T = 1 + n / hop frames (ake_cqt_num_frames);
//   - window w of a recording is frames [w * stride_frames, w * stride_frames + window_frames) of the recording's OWN transform; the net
//     runs on it exactly as on a clip of window_frames frames with seq_length = window_frames (time-circular convolutions wrap at the
//     window's ends).  A frame near a window edge therefore sees the recording's real neighbouring audio where a separately transformed
//     clip sees zero padding: the one intended difference from clip-wise results;
//   - recording i has count_i = (T_i - window_frames) / stride_frames + 1 windows (0 if T_i < window_frames);
//   - decode per window: sig = first-maximum cosine match of the key output over the 21-row key-signature table (the arithmetic and tie
//     rule of metrics.mirex_score / models.py:1065-1083, eps 1e-8), tonic = first maximum of the tonic logits, confidence = that cosine,
//     key_id in the project's 24-way label order (0-11 minor, 12-23 major, tonic = id mod 12; KeyDataset.py:524-527): 12 + tonic if tonic
//     is the table row's major tonic, tonic if it is that tonic + 9 (the relative minor), -1 otherwise (signature and tonic disagree).
//
// The windows reach the net through window_gather_kernel, which copies them out of either CQT layout into the [B][1][P][window_frames]
// tensor ake_pcnet_forward_f32 takes, a chunk of kTrackChunk windows at a time (the chunk bounds the workspace and is the net's own
// pitch-stream chunk, so nothing is chunked twice).
//
// What is done with a track's outputs -- key emissions, the Viterbi decode, posteriors, the streaming smoother, the sequence loss -- is
// csrc/smooth.hip; the two files share csrc/keys.h.
//
// A track is scored against key annotations by track_score_kernel (one launch, integers only), below the decode.
//
// Training on annotated recordings assembles its batches from the same cached transform: draw_windows_kernel (window positions from a
// counter-based generator) and window_batch_kernel (the gather, from a list in device memory, with every window's labels and weight).
#include "common.h"
#include "keys.h"
#include "philox.h"

#include <algorithm>
#include <climits>
#include <cstdint>

namespace {

constexpr int kTrackChunk = 256;      // windows per forward call = ake_pcnet's pitch-stream chunk
constexpr int kTile = 32;

struct GatherArgs {
    const float* src;          // FM: [recording][total_frames][P]; else [recording][P][total_frames]
    float* dst;                // [clip][P][window_frames]
    int P, total_frames, window_frames, stride_frames;
    int windows;               // per recording
    int clip0;                 // global window index of dst's clip 0
};

// One 32 x 32 tile of one window per block of 32 x 8 threads: frames [t0, t0 + window_frames) of `src` (one recording's transform) to
// `dst` ([P][window_frames]).  FM source: the loads run along the bins (the source's fast axis), the stores along the frames (the
// destination's), a padded LDS tile turns the one into the other.  Row-major source: both fast axes are the frames, a straight copy.
template <bool FM>
__device__ __forceinline__ void gather_tile(const float* src, float* dst, int P, int total_frames, int window_frames, int t0,
                                            float (&tile)[kTile][kTile + 1]) {
    const int p0 = blockIdx.x * kTile, f0 = blockIdx.y * kTile;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (FM) {
        for (int j = ty; j < kTile; j += 8) {
            const int f = f0 + j, p = p0 + tx;
            if (f < window_frames && p < P) tile[j][tx] = src[static_cast<long long>(t0 + f) * P + p];
        }
        __syncthreads();
        for (int j = ty; j < kTile; j += 8) {
            const int p = p0 + j, f = f0 + tx;
            if (p < P && f < window_frames) dst[p * window_frames + f] = tile[tx][j];
        }
    } else {
        for (int j = ty; j < kTile; j += 8) {
            const int p = p0 + j, f = f0 + tx;
            if (p < P && f < window_frames) dst[p * window_frames + f] = src[static_cast<long long>(p) * total_frames + t0 + f];
        }
    }
}

// Windows at a fixed stride: global window g is window g % windows of recording g / windows.
template <bool FM>
__global__ __launch_bounds__(256) void window_gather_kernel(GatherArgs a) {
    __shared__ float tile[kTile][kTile + 1];
    const int g = a.clip0 + blockIdx.z;
    const int rec = g / a.windows, t0 = (g - rec * a.windows) * a.stride_frames;      // t0 + window_frames <= total_frames (host-checked)
    gather_tile<FM>(a.src + static_cast<long long>(rec) * a.P * a.total_frames, a.dst + static_cast<long long>(blockIdx.z) * a.P * a.window_frames,
                    a.P, a.total_frames, a.window_frames, t0, tile);
}

__global__ void fill_i64_kernel(long long* dst, long long v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}

// counts of the track: recording i has T_i = min(1 + n_i / hop, total_frames) frames (n_clip null: every recording has total_frames)
__global__ void track_counts_kernel(int* counts, const long long* __restrict__ n_clip, int hop, int total_frames, int window_frames,
                                    int stride_frames, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long t = total_frames;
    if (n_clip) {
        const long long nc = n_clip[i];
        t = nc < 0 ? 0 : 1 + nc / hop;                                   // librosa center=True framing, as ake_cqt_num_frames
        t = t < total_frames ? t : total_frames;
    }
    counts[i] = t < window_frames ? 0 : static_cast<int>((t - window_frames) / stride_frames + 1);
}

// The key-signature table (utils/key_signatures.py:19-42, metrics.KEY_SIGNATURE_MAP): circle of fifths Cb .. C# (15 rows), then six
// enharmonic duplicates; major_tonic[k] is the pitch class of row k's major scale.
struct KeyTable {
    float row[21][12];
    int major_tonic[21];
};
constexpr KeyTable make_key_table() {
    KeyTable t{};
    const int dup[6] = {9, 11, 10, 4, 3, 5};
    for (int k = 0; k < 21; ++k) {
        const int i = k < 15 ? k : dup[k - 15];
        const int tonic = ((7 * (i - 7)) % 12 + 12) % 12;
        t.major_tonic[k] = tonic;
        for (int pc = 0; pc < 12; ++pc) {
            const int d = ((pc - tonic) % 12 + 12) % 12;
            t.row[k][pc] = (d == 0 || d == 2 || d == 4 || d == 5 || d == 7 || d == 9 || d == 11) ? 1.f : 0.f;
        }
    }
    return t;
}
__constant__ const KeyTable kKeyTable = make_key_table();

struct DecodeArgs {
    const float* key;          // [rows][12]
    const float* tonic;        // [rows][12]
    const int* counts;         // [rows / windows] valid windows per recording, nullable (all valid)
    int rows, windows;
    int* key_id;
    int* sig;
    int* tonic_id;
    float* confidence;
};

// One thread per row (a row is 24 floats in, 4 words out).
__global__ __launch_bounds__(256) void decode_keys_kernel(DecodeArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.rows) return;
    if (a.counts) {
        const int rec = r / a.windows;
        if (r - rec * a.windows >= a.counts[rec]) {
            a.key_id[r] = -1; a.sig[r] = -1; a.tonic_id[r] = -1; a.confidence[r] = 0.f;
            return;
        }
    }
    float p[12], pp = 0.f;
    for (int j = 0; j < 12; ++j) { p[j] = a.key[r * 12 + j]; pp += p[j] * p[j]; }
    const float pn = fmaxf(sqrtf(pp), 1e-8f), tn = fmaxf(sqrtf(7.f), 1e-8f);
    int sig = 0;
    float best = -INFINITY;
    for (int k = 0; k < 21; ++k) {
        float dot = 0.f;
        for (int j = 0; j < 12; ++j) dot += p[j] * kKeyTable.row[k][j];
        const float sim = dot / (pn * tn);
        if (sim > best) { best = sim; sig = k; }                          // strict: the first maximum
    }
    int tonic = 0;
    float tb = a.tonic[r * 12];
    for (int j = 1; j < 12; ++j) {
        const float v = a.tonic[r * 12 + j];
        if (v > tb) { tb = v; tonic = j; }
    }
    const int maj = kKeyTable.major_tonic[sig];
    a.key_id[r] = tonic == maj ? 12 + tonic : tonic == (maj + 9) % 12 ? tonic : -1;
    a.sig[r] = sig;
    a.tonic_id[r] = tonic;
    a.confidence[r] = best;
}

// ---- a track against key annotations (semantics: include/ake_hip.h; host restatement: metrics.window_truth / metrics.track_score) ----
struct ScoreArgs {
    const int* pred;           // [recordings][windows], -1..23
    const int* counts;         // nullable
    const long long* seg_start;   // [recordings][max_segments], ascending below seg_count
    const int* seg_key;        // [recordings][max_segments], -1 = unlabelled
    const int* seg_count;      // [recordings]
    int* truth;                // [recordings][windows], nullable
    int* category;             // [recordings][windows], nullable
    int* tally;                // [recordings][2][6]
    int* changes;              // [recordings][2]
    int windows, max_segments;
    long long hop;
    int window_frames, stride_frames;
};

// the relation of a decoded key to the true one: 0 correct, 1 fifth, 2 relative, 3 parallel, 4 other, 5 undecoded (truth in 0..23)
__device__ __forceinline__ int key_relation(int pred, int truth) {
    if (pred < 0) return 5;
    if (pred == truth) return 0;
    if (pred >= kKeys) return 4;
    const int pm = pred >= 12, tm = truth >= 12, pt = pred - 12 * pm, tt = truth - 12 * tm;
    if (pm == tm) {
        const int d = (pt - tt + 12) % 12;
        return d == 5 || d == 7 ? 1 : 4;
    }
    const int pmaj = pm ? pt : (pt + 3) % 12, tmaj = tm ? tt : (tt + 3) % 12;      // the major tonic of the key's scale
    return pmaj == tmaj ? 2 : pt == tt ? 3 : 4;
}

// truth and purity of window w: the key of the last segment that starts at or before the centre sample; pure when every segment that
// overlaps the window's samples [lo, hi] carries that key.  A linear walk over the recording's segments (a handful per recording).
__device__ __forceinline__ int window_truth(const ScoreArgs& a, const long long* start, const int* key, int ns, int w, bool* pure) {
    const long long f0 = static_cast<long long>(w) * a.stride_frames;
    const long long lo = f0 * a.hop, hi = (f0 + a.window_frames - 1) * a.hop, centre = (2 * f0 + a.window_frames - 1) * a.hop / 2;
    int truth = -1;
    for (int s = 0; s < ns; ++s) truth = start[s] <= centre ? key[s] : truth;
    bool all = truth >= 0;
    for (int s = 0; s < ns; ++s) {
        const bool overlaps = start[s] <= hi && (s + 1 >= ns || start[s + 1] > lo);
        all = all && (!overlaps || key[s] == truth);
    }
    *pure = all;
    return truth;
}

// One block per recording, a thread per window in turn.  Integers only: the tallies meet in LDS through integer atomics, whose result
// does not depend on the order, so every run gives the same bits.
__global__ __launch_bounds__(256) void track_score_kernel(ScoreArgs a) {
    __shared__ int s_tally[14];                                          // [2][6], then the two change counts
    const int r = blockIdx.x, W = a.windows;
    if (threadIdx.x < 14) s_tally[threadIdx.x] = 0;
    __syncthreads();
    const int n = clamped_count(a.counts, r, W);
    int ns = a.seg_count[r];
    ns = ns < 0 ? 0 : ns > a.max_segments ? a.max_segments : ns;
    const long long* const start = a.seg_start + static_cast<size_t>(r) * a.max_segments;
    const int* const key = a.seg_key + static_cast<size_t>(r) * a.max_segments;
    const int* const pred = a.pred + static_cast<size_t>(r) * W;
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        int truth = -1, cat = -1;
        if (w < n && ns > 0) {
            bool pure;
            truth = window_truth(a, start, key, ns, w, &pure);
            const int p = pred[w];
            if (truth >= 0) {
                cat = key_relation(p, truth);
                atomicAdd(&s_tally[cat], 1);
                if (pure) atomicAdd(&s_tally[6 + cat], 1);
            }
            if (w > 0) {
                bool unused;
                if (p != pred[w - 1]) atomicAdd(&s_tally[12], 1);
                if (truth != window_truth(a, start, key, ns, w - 1, &unused)) atomicAdd(&s_tally[13], 1);
            }
        }
        if (a.truth) a.truth[static_cast<size_t>(r) * W + w] = truth;
        if (a.category) a.category[static_cast<size_t>(r) * W + w] = cat;
    }
    __syncthreads();
    if (threadIdx.x < 12) a.tally[r * 12 + threadIdx.x] = s_tally[threadIdx.x];
    else if (threadIdx.x < 14) a.changes[r * 2 + threadIdx.x - 12] = s_tally[threadIdx.x];
}

// ---- training windows: positions drawn on the device, gathered from the cached transform, labelled from the annotations ----
// (semantics: include/ake_hip.h; host models: metrics.draw_windows / metrics.window_labels)
struct DrawArgs {
    const long long* prefix;   // [R + 1] exclusive sums of the recordings' start counts; N = prefix[R]
    int recordings;
    unsigned key0, key1, epoch;
    unsigned long long first_slot;
    int batch;
    int* recording;            // [batch]
    int* start;                // [batch]
};

// One thread per slot: one Philox block -> a 64-bit word x -> index = floor(x * N / 2^64) -> (recording, start) by binary search over
// the prefix.  Integers only.  N <= 0 (the entry's contract excludes it, and the host cannot see it): -1 in both outputs.
__global__ __launch_bounds__(256) void draw_windows_kernel(DrawArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const unsigned long long j = a.first_slot + static_cast<unsigned long long>(b);
    unsigned c[4] = {static_cast<unsigned>(j), static_cast<unsigned>(j >> 32), a.epoch, 0x57494E44u};
    ake::philox4x32_10(c, a.key0, a.key1);
    const unsigned long long x = static_cast<unsigned long long>(c[0]) | static_cast<unsigned long long>(c[1]) << 32;
    const long long N = a.prefix[a.recordings];
    if (N <= 0) { a.recording[b] = -1; a.start[b] = -1; return; }
    const long long index = static_cast<long long>(__umul64hi(x, static_cast<unsigned long long>(N)));
    int lo = 0, hi = a.recordings - 1;                                   // the last i in 0..R-1 with prefix[i] <= index (prefix[0] = 0)
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (a.prefix[mid] <= index) lo = mid; else hi = mid - 1;
    }
    a.recording[b] = lo;
    a.start[b] = static_cast<int>(index - a.prefix[lo]);
}

struct BatchArgs {
    const float* src;          // as GatherArgs
    float* dst;                // [batch][P][window_frames], nullable: labels only
    int P, recordings, total_frames, window_frames;
    long long hop;
    const int* recording;      // [batch], in device memory: read clamped to 0..recordings-1
    const int* start;          // [batch], read clamped to 0..total_frames-window_frames
    const long long* seg_start;   // as ScoreArgs; null: no labels
    const int* seg_key;
    const int* seg_count;
    int max_segments;
    float min_purity;
    int uniform;
    float* key_labels;         // [batch][12]
    float* tonic_labels;       // [batch][12]
    float* sig;                // [batch][24]
    long long* seq;            // [batch]
    float* weight;             // [batch]
};

// grid (P tiles, frame tiles, batch) with a gather, (1, 1, batch) without: every block copies its tile of window blockIdx.z, and block
// (0, 0, z) also writes that window's 50 label words.  Its first 64 threads each walk the recording's segments (the same handful of
// broadcast loads; integers until the one division) and then write one word each.
template <bool FM>
__global__ __launch_bounds__(256) void window_batch_kernel(BatchArgs a) {
    __shared__ float tile[kTile][kTile + 1];
    const int b = blockIdx.z;
    int rec = a.recording[b], t0 = a.start[b];
    rec = rec < 0 ? 0 : rec >= a.recordings ? a.recordings - 1 : rec;
    t0 = t0 < 0 ? 0 : t0 > a.total_frames - a.window_frames ? a.total_frames - a.window_frames : t0;     // (>= 0: host-checked)
    if (a.dst)
        gather_tile<FM>(a.src + static_cast<long long>(rec) * a.P * a.total_frames, a.dst + static_cast<long long>(b) * a.P * a.window_frames, a.P,
                        a.total_frames, a.window_frames, t0, tile);
    const int t = threadIdx.x;
    if (!a.seg_start || blockIdx.x != 0 || blockIdx.y != 0 || t >= 50) return;
    int ns = a.seg_count[rec];
    ns = ns < 0 ? 0 : ns > a.max_segments ? a.max_segments : ns;
    const long long* const start = a.seg_start + static_cast<size_t>(rec) * a.max_segments;
    const int* const key = a.seg_key + static_cast<size_t>(rec) * a.max_segments;
    const long long lo = t0 * a.hop, hi = (static_cast<long long>(t0) + a.window_frames - 1) * a.hop;
    const long long centre = (2ll * t0 + a.window_frames - 1) * a.hop / 2;
    int truth = -1;
    for (int s = 0; s < ns; ++s) truth = start[s] <= centre ? key[s] : truth;
    long long c = 0;                                                     // samples of lo..hi inside segments that carry truth
    for (int s = 0; s < ns; ++s) {
        const long long s0 = start[s] > lo ? start[s] : lo;
        const long long last = s + 1 < ns ? start[s + 1] - 1 : LLONG_MAX;
        const long long s1 = last < hi ? last : hi;
        if (key[s] == truth && s1 >= s0) c += s1 - s0 + 1;
    }
    const float purity = static_cast<float>(static_cast<double>(c) / static_cast<double>(hi - lo + 1));
    const bool keep = truth >= 0 && !(purity < a.min_purity);
    if (t < 12) {
        const int major = truth >= 12 ? truth - 12 : (truth + 3) % 12;
        a.key_labels[b * 12 + t] = truth >= 0 && ((kMajorScale >> ((t - major + 12) % 12)) & 1) ? 1.f : 0.f;
    } else if (t < 24) {
        a.tonic_labels[b * 12 + t - 12] = truth >= 0 && t - 12 == truth % 12 ? 1.f : 0.f;
    } else if (t < 48) {
        a.sig[b * 24 + t - 24] = t - 24 == truth ? 1.f : 0.f;
    } else if (t == 48) {
        a.seq[b] = a.window_frames;
    } else {
        a.weight[b] = keep ? (a.uniform ? 1.f : purity) : 0.f;
    }
}

struct WinCarve {
    float* mel;                // [chunk][P][window_frames]
    long long* seq;            // [chunk]
    void* net_ws;
    size_t net_bytes;
    size_t total;
    int chunk;
    long long windows;         // per recording
};

int carve_windows(const ake_pcnet* net, int recordings, int total_frames, int window_frames, int stride_frames, void* ws, WinCarve* wc) {
    AKE_REQUIRE(net, AKE_ERR_INVALID, "forward_windows: null net");
    AKE_REQUIRE(ake::pcnet_local_window(net) == 0, AKE_ERR_UNSUPPORTED,
                "forward_windows: a --local net is not tracked (it has its own per-frame forward, ake_pcnet_forward_local_f32, and its rows are not time frames)");
    AKE_REQUIRE(recordings > 0 && window_frames > 0 && stride_frames > 0 && total_frames >= window_frames, AKE_ERR_INVALID,
                "forward_windows: bad shape (%d recordings, %d frames, window %d, stride %d)", recordings, total_frames, window_frames, stride_frames);
    wc->windows = (total_frames - window_frames) / stride_frames + 1;
    const long long total = wc->windows * recordings;
    AKE_REQUIRE(total <= (1ll << 30), AKE_ERR_INVALID, "forward_windows: %lld windows", total);
    wc->chunk = static_cast<int>(std::min<long long>(total, kTrackChunk));
    const int P = ake_pcnet_pitches(net);
    ake::Carver c(ws, 0);
    wc->mel = c.take<float>(static_cast<size_t>(wc->chunk) * P * window_frames);
    wc->seq = c.take<long long>(wc->chunk);
    wc->net_bytes = ake_pcnet_workspace_bytes(net, wc->chunk, window_frames);
    AKE_REQUIRE(wc->net_bytes > 0, AKE_ERR_INVALID, "forward_windows: the net has no workspace for %d x %d frames", wc->chunk, window_frames);
    wc->net_ws = c.take<char>(wc->net_bytes);
    wc->total = ake::align_up(c.off, 256);
    return AKE_OK;
}

struct TrackCarve {
    float* mel;
    void* cqt_ws;
    size_t cqt_bytes;
    void* win_ws;
    size_t win_bytes;
    size_t total;
    int T;
};

int carve_track(const ake_cqt_plan* plan, const ake_pcnet* net, int recordings, int64_t n, int window_frames, int stride_frames, void* ws,
                TrackCarve* tc) {
    AKE_REQUIRE(plan && net, AKE_ERR_INVALID, "track: null argument");
    AKE_REQUIRE(recordings > 0 && n > 0, AKE_ERR_INVALID, "track: bad recordings / n_samples");
    const int64_t T = ake_cqt_num_frames(plan, n);
    AKE_REQUIRE(T > 0 && T < (1ll << 30), AKE_ERR_INVALID, "track: bad n_samples");
    const int n_bins = ake_cqt_plan_n_bins(plan);
    AKE_REQUIRE(n_bins == ake_pcnet_pitches(net), AKE_ERR_INVALID, "track: CQT has %d bins but the net expects %d pitches", n_bins,
                ake_pcnet_pitches(net));
    tc->T = static_cast<int>(T);
    WinCarve wc;
    int rc = carve_windows(net, recordings, tc->T, window_frames, stride_frames, nullptr, &wc);
    if (rc) return rc;
    ake::Carver c(ws, 0);
    tc->mel = c.take<float>(static_cast<size_t>(recordings) * n_bins * T);
    tc->cqt_bytes = ake_cqt_workspace_bytes(plan, recordings, n);
    tc->cqt_ws = c.take<char>(tc->cqt_bytes);
    tc->win_bytes = wc.total;
    tc->win_ws = c.take<char>(tc->win_bytes);
    tc->total = ake::align_up(c.off, 256);
    return AKE_OK;
}

int track_impl(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int recordings, int64_t n_samples,
               int64_t audio_stride, const int64_t* n_clip_dev, int window_frames, int stride_frames, float* key_out, float* tonic_out,
               float* genre_out, int32_t* key_id, int32_t* sig, int32_t* tonic_id, float* confidence, int32_t* counts, void* ws,
               size_t ws_bytes, ake_stream_t stream, const int16_t* pcm16_dev = nullptr) {
    // pcm16_dev != null: the audio is 16-bit PCM (ake_cqt_logmag_pcm16_f32) and audio_dev is ignored
    AKE_REQUIRE((audio_dev || pcm16_dev) && key_out && tonic_out && key_id && sig && tonic_id && confidence && counts, AKE_ERR_INVALID, "track: null argument");
    TrackCarve tc;
    int rc = carve_track(plan, net, recordings, n_samples, window_frames, stride_frames, ws, &tc);
    if (rc) return rc;
    AKE_REQUIRE(ws && ws_bytes >= tc.total, AKE_ERR_WORKSPACE, "track: workspace %zu < %zu bytes", ws_bytes, tc.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // equal-length recordings: the CQT stays in the filter bank's own [recording][frame][bin] order (no transpose pass; the gather
    // transposes the windows it copies anyway).  Ragged recordings: [recording][bin][frame], frames behind a recording's end are zeros.
    const bool fm = !n_clip_dev && ake_cqt_frames_major_supported(plan);
    rc = pcm16_dev  ? ake_cqt_logmag_pcm16_f32(plan, pcm16_dev, recordings, n_samples, audio_stride, n_clip_dev, nullptr, tc.mel, tc.T, fm ? 1 : 0, tc.cqt_ws, tc.cqt_bytes, stream)
         : n_clip_dev ? ake_cqt_logmag_ragged_f32(plan, audio_dev, recordings, n_samples, audio_stride, n_clip_dev, tc.mel, tc.T, tc.cqt_ws, tc.cqt_bytes, stream)
         : fm       ? ake_cqt_logmag_frames_major_f32(plan, audio_dev, recordings, n_samples, audio_stride, tc.mel, tc.cqt_ws, tc.cqt_bytes, stream)
                    : ake_cqt_logmag_f32(plan, audio_dev, recordings, n_samples, audio_stride, tc.mel, tc.T, tc.cqt_ws, tc.cqt_bytes, stream);
    if (rc) return rc;
    rc = ake_pcnet_forward_windows_f32(net, tc.mel, fm ? 1 : 0, recordings, tc.T, window_frames, stride_frames, key_out, tonic_out, genre_out,
                                       tc.win_ws, tc.win_bytes, stream);
    if (rc) return rc;
    rc = ake::launch_untimed("track_counts_kernel", track_counts_kernel, dim3((recordings + 255) / 256), dim3(256), 0, s, counts,
                             reinterpret_cast<const long long*>(n_clip_dev), ake_cqt_plan_hop(plan), tc.T, window_frames, stride_frames, recordings);
    if (rc) return rc;
    const int windows = (tc.T - window_frames) / stride_frames + 1;
    return ake_decode_keys_f32(key_out, tonic_out, recordings * windows, n_clip_dev ? counts : nullptr, windows, key_id, sig, tonic_id, confidence,
                               stream);
}

}  // namespace

extern "C" {

size_t ake_pcnet_forward_windows_workspace_bytes(const ake_pcnet* net, int recordings, int total_frames, int window_frames, int stride_frames) {
    WinCarve wc;
    if (carve_windows(net, recordings, total_frames, window_frames, stride_frames, nullptr, &wc) != AKE_OK) return 0;
    return wc.total;
}

int ake_pcnet_forward_windows_f32(const ake_pcnet* net, const float* mel_dev, int frames_major, int recordings, int total_frames,
                                  int window_frames, int stride_frames, float* key_out_dev, float* tonic_out_dev, float* genre_out_dev,
                                  void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(mel_dev && key_out_dev && tonic_out_dev, AKE_ERR_INVALID, "forward_windows: null argument");
    WinCarve wc;
    int rc = carve_windows(net, recordings, total_frames, window_frames, stride_frames, workspace, &wc);
    if (rc) return rc;
    AKE_REQUIRE(workspace && workspace_bytes >= wc.total, AKE_ERR_WORKSPACE, "forward_windows: workspace %zu < %zu bytes", workspace_bytes, wc.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = ake_pcnet_pitches(net);
    const long long total = wc.windows * recordings;
    rc = ake::launch_untimed("fill_i64_kernel", fill_i64_kernel, dim3((wc.chunk + 255) / 256), dim3(256), 0, s, wc.seq, window_frames, wc.chunk);
    if (rc) return rc;
    for (long long c0 = 0; c0 < total; c0 += wc.chunk) {
        const int B = static_cast<int>(std::min<long long>(wc.chunk, total - c0));
        GatherArgs ga{mel_dev, wc.mel, P, total_frames, window_frames, stride_frames, static_cast<int>(wc.windows), static_cast<int>(c0)};
        const dim3 grid((P + kTile - 1) / kTile, (window_frames + kTile - 1) / kTile, B);
        rc = frames_major ? ake::launch("window_gather_kernel", window_gather_kernel<true>, grid, dim3(256), 0, s, ga)
                          : ake::launch("window_gather_kernel", window_gather_kernel<false>, grid, dim3(256), 0, s, ga);
        if (rc) return rc;
        rc = ake_pcnet_forward_f32(net, wc.mel, B, window_frames, reinterpret_cast<const int64_t*>(wc.seq), key_out_dev + c0 * 12, tonic_out_dev + c0 * 12,
                                   genre_out_dev ? genre_out_dev + c0 * 11 : nullptr, wc.net_ws, wc.net_bytes, stream);
        if (rc) return rc;
    }
    return AKE_OK;
}

int ake_decode_keys_f32(const float* key_dev, const float* tonic_dev, int rows, const int32_t* counts_dev, int windows_per_recording,
                        int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev, float* confidence_dev, ake_stream_t stream) {
    AKE_REQUIRE(key_dev && tonic_dev && key_id_dev && sig_dev && tonic_id_dev && confidence_dev, AKE_ERR_INVALID, "decode_keys: null argument");
    AKE_REQUIRE(rows >= 0 && (!counts_dev || (windows_per_recording > 0 && rows % windows_per_recording == 0)), AKE_ERR_INVALID,
                "decode_keys: %d rows do not divide into recordings of %d windows", rows, windows_per_recording);
    if (rows == 0) return AKE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DecodeArgs a{key_dev, tonic_dev, counts_dev, rows, counts_dev ? windows_per_recording : 1, key_id_dev, sig_dev, tonic_id_dev, confidence_dev};
    return ake::launch_flat("decode_keys_kernel", decode_keys_kernel, s, rows, a);
}

size_t ake_pipeline_track_workspace_bytes(const ake_cqt_plan* plan, const ake_pcnet* net, int recordings, int64_t n_samples, int window_frames,
                                          int stride_frames) {
    TrackCarve tc;
    if (carve_track(plan, net, recordings, n_samples, window_frames, stride_frames, nullptr, &tc) != AKE_OK) return 0;
    return tc.total;
}

int ake_pipeline_track_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int recordings, int64_t n_samples,
                           int64_t audio_stride, int window_frames, int stride_frames, float* key_out_dev, float* tonic_out_dev,
                           float* genre_out_dev, int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev, float* confidence_dev,
                           int32_t* counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    return track_impl(plan, net, audio_dev, recordings, n_samples, audio_stride, nullptr, window_frames, stride_frames, key_out_dev, tonic_out_dev,
                      genre_out_dev, key_id_dev, sig_dev, tonic_id_dev, confidence_dev, counts_dev, workspace, workspace_bytes, stream);
}

int ake_pipeline_track_ragged_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const float* audio_dev, int recordings, int64_t n_max,
                                  int64_t audio_stride, const int64_t* n_samples_dev, int window_frames, int stride_frames, float* key_out_dev,
                                  float* tonic_out_dev, float* genre_out_dev, int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev,
                                  float* confidence_dev, int32_t* counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    AKE_REQUIRE(n_samples_dev, AKE_ERR_INVALID, "ake_pipeline_track_ragged_f32: null n_samples_dev");
    return track_impl(plan, net, audio_dev, recordings, n_max, audio_stride, n_samples_dev, window_frames, stride_frames, key_out_dev, tonic_out_dev,
                      genre_out_dev, key_id_dev, sig_dev, tonic_id_dev, confidence_dev, counts_dev, workspace, workspace_bytes, stream);
}

int ake_pipeline_track_pcm16_f32(const ake_cqt_plan* plan, const ake_pcnet* net, const int16_t* audio_dev, int recordings, int64_t n_max,
                                 int64_t audio_stride, const int64_t* lengths_dev, int window_frames, int stride_frames, float* key_out_dev,
                                 float* tonic_out_dev, float* genre_out_dev, int32_t* key_id_dev, int32_t* sig_dev, int32_t* tonic_id_dev,
                                 float* confidence_dev, int32_t* counts_dev, void* workspace, size_t workspace_bytes, ake_stream_t stream) {
    return track_impl(plan, net, nullptr, recordings, n_max, audio_stride, lengths_dev, window_frames, stride_frames, key_out_dev, tonic_out_dev,
                      genre_out_dev, key_id_dev, sig_dev, tonic_id_dev, confidence_dev, counts_dev, workspace, workspace_bytes, stream, audio_dev);
}

int ake_track_score_i32(const int32_t* pred_dev, const int32_t* counts_dev, const int64_t* seg_start_dev, const int32_t* seg_key_dev,
                        const int32_t* seg_count_dev, int recordings, int windows, int max_segments, int hop, int window_frames,
                        int stride_frames, int32_t* truth_dev, int32_t* category_dev, int32_t* tally_dev, int32_t* changes_dev,
                        ake_stream_t stream) {
    AKE_REQUIRE(pred_dev && seg_start_dev && seg_key_dev && seg_count_dev && tally_dev && changes_dev, AKE_ERR_INVALID, "track_score: null argument");
    AKE_REQUIRE(recordings > 0 && windows > 0 && max_segments > 0 && static_cast<long long>(recordings) * windows <= (1ll << 30), AKE_ERR_INVALID,
                "track_score: bad shape (%d recordings, %d windows, %d segments)", recordings, windows, max_segments);
    AKE_REQUIRE(hop > 0 && window_frames > 0 && stride_frames > 0, AKE_ERR_INVALID, "track_score: bad geometry (hop %d, window %d, stride %d)", hop,
                window_frames, stride_frames);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ScoreArgs a{pred_dev, counts_dev, reinterpret_cast<const long long*>(seg_start_dev), seg_key_dev, seg_count_dev, truth_dev, category_dev,
                tally_dev, changes_dev, windows, max_segments, hop, window_frames, stride_frames};
    return ake::launch("track_score_kernel", track_score_kernel, dim3(recordings), dim3(256), 0, s, a);
}

int ake_draw_windows_i32(const int64_t* prefix_dev, int recordings, uint64_t seed, uint32_t epoch, int64_t first_slot, int batch,
                         int32_t* recording_out_dev, int32_t* start_out_dev, ake_stream_t stream) {
    AKE_REQUIRE(prefix_dev && recording_out_dev && start_out_dev, AKE_ERR_INVALID, "draw_windows: null argument");
    AKE_REQUIRE(recordings > 0 && batch >= 0 && first_slot >= 0, AKE_ERR_INVALID, "draw_windows: bad shape (%d recordings, batch %d, first slot %lld)",
                recordings, batch, static_cast<long long>(first_slot));
    if (batch == 0) return AKE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DrawArgs a{reinterpret_cast<const long long*>(prefix_dev), recordings, static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32), epoch,
               static_cast<unsigned long long>(first_slot), batch, recording_out_dev, start_out_dev};
    return ake::launch_flat("draw_windows_kernel", draw_windows_kernel, s, batch, a);
}

int ake_window_batch_f32(const float* mel_dev, int frames_major, int recordings, int total_frames, int pitches, int window_frames, int hop,
                         const int32_t* recording_dev, const int32_t* start_dev, int batch, const int64_t* seg_start_dev,
                         const int32_t* seg_key_dev, const int32_t* seg_count_dev, int max_segments, float min_purity, int uniform,
                         float* mel_out_dev, float* key_labels_dev, float* tonic_labels_dev, float* key_signature_id_dev,
                         int64_t* seq_length_dev, float* weight_dev, ake_stream_t stream) {
    AKE_REQUIRE(recording_dev && start_dev, AKE_ERR_INVALID, "window_batch: null window list");
    const int given = !!seg_start_dev + !!seg_key_dev + !!seg_count_dev + !!key_labels_dev + !!tonic_labels_dev + !!key_signature_id_dev +
                      !!seq_length_dev + !!weight_dev;
    AKE_REQUIRE(given == 0 || given == 8, AKE_ERR_INVALID, "window_batch: pass the annotations and every label output, or none of them");
    AKE_REQUIRE(!mel_out_dev || mel_dev, AKE_ERR_INVALID, "window_batch: mel_out_dev without mel_dev");
    AKE_REQUIRE(mel_out_dev || given, AKE_ERR_INVALID, "window_batch: nothing to write");
    AKE_REQUIRE(recordings > 0 && pitches > 0 && window_frames > 0 && total_frames >= window_frames && total_frames < (1 << 30) && hop > 0, AKE_ERR_INVALID,
                "window_batch: bad shape (%d recordings, %d frames, %d pitches, window %d, hop %d)", recordings, total_frames, pitches, window_frames, hop);
    AKE_REQUIRE(batch >= 0 && batch <= 65535, AKE_ERR_INVALID, "window_batch: batch %d (at most 65535)", batch);                  // (grid z)
    AKE_REQUIRE(!given || max_segments > 0, AKE_ERR_INVALID, "window_batch: max_segments %d", max_segments);
    AKE_REQUIRE(!(min_purity != min_purity), AKE_ERR_INVALID, "window_batch: min_purity is NaN");
    if (batch == 0) return AKE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    BatchArgs a{mel_dev, mel_out_dev, pitches, recordings, total_frames, window_frames, hop, recording_dev, start_dev,
                reinterpret_cast<const long long*>(seg_start_dev), seg_key_dev, seg_count_dev, max_segments, min_purity, uniform,
                key_labels_dev, tonic_labels_dev, key_signature_id_dev, reinterpret_cast<long long*>(seq_length_dev), weight_dev};
    const dim3 grid(mel_out_dev ? (pitches + kTile - 1) / kTile : 1, mel_out_dev ? (window_frames + kTile - 1) / kTile : 1, batch);
    return frames_major ? ake::launch("window_batch_kernel", window_batch_kernel<true>, grid, dim3(256), 0, s, a)
                        : ake::launch("window_batch_kernel", window_batch_kernel<false>, grid, dim3(256), 0, s, a);
}

}  // extern "C"
