// PitchClassNet on gfx950, host side: BatchNorm folding, packing, the per-kernel launchers and the C entries.  One translation unit; the
// handle (pcnet_net.h), workspace carve and route (pcnet_plan.h), forward (pcnet_forward.h) and backward pass (pcnet_backward.h) are
// included where they stood.
//
// Replaces PitchClassNet.forward (models.py:747-817) for the default architecture family
// (models.py:190-197, 227-234, 311-350).  Channel algebra follows models.py:279-308 / 693-710.
//
// HBM layout (all fp32, NCHW; the pitch stream runs in chunks of <= chunk_clips = 256 clips: measured on MI355X a larger
// launch beats Infinity-Cache residency of the 700 KB/clip activations):
//   mel      [B][1][P][T]                    caller's
//   fold0    [c][1][12][T]                   semitone conv + octave fold of layer 0
//   cat_i    [c][prev_pc + out_p][12][T_i]   concat buffer of layer i: producers write their channel slice
//   psix     [c][prev_pc][36][T_i]           up_sixth output; the x(P/36) row repeat is never materialised
//   pa / pb  [c][out_p][P][T_i]              pitch-conv ping-pong
//   pc a/b   [c][out_pc][12][T_i]            pitch-class conv ping-pong
//   pcf      [c][final][12][T_f]             time-pooled features feeding the heads
//   hid      [c][2*final][12][.]             head hidden maps;  maps [c][rows][T_m]
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "pcnet_kernels.h"
#include "pcnet_bwd_kernels.h"

using namespace ake_k;

#include "pcnet_net.h"

namespace {

// the host copy of specs[spec] (build_packs resolves every name before it packs: the pack helpers below only see valid indices)
const std::vector<float>& T(const ake_pcnet* n, int spec) { return n->host[spec].data; }

// conv weight [cout][cin][kh][kw] + bias, optionally followed by the BatchNorm `bn` (null: none) in eval mode:
//   y = (conv(x) - mean) * gamma / sqrt(var + eps) + beta  ==  conv'(x) with w' = w*s, b' = (b - mean)*s + beta
void fold(const ake_pcnet* n, int wspec, int bspec, const BnSpecs* bn, int cout, size_t per_out, bool transposed_cin_first, int cin,
          std::vector<double>& w, std::vector<double>& b) {
    const auto& w32 = T(n, wspec);
    const auto& b32 = T(n, bspec);
    w.assign(w32.begin(), w32.end());
    b.assign(b32.begin(), b32.end());
    if (!bn) return;
    if (n->tracing) const_cast<ake_pcnet*>(n)->fold_records.push_back({wspec, bspec, *bn, cout, per_out, transposed_cin_first, cin});
    const auto& g = T(n, bn->weight);
    const auto& be = T(n, bn->bias);
    const auto& mu = T(n, bn->mean);
    const auto& var = T(n, bn->var);
    for (int co = 0; co < cout; ++co) {
        const double s = static_cast<double>(g[co]) / std::sqrt(static_cast<double>(var[co]) + kBnEps);
        if (!transposed_cin_first) {
            for (size_t i = 0; i < per_out; ++i) w[co * per_out + i] *= s;
        } else {   // ConvTranspose2d weight is [cin][cout][kh][kw]
            const size_t k = per_out / cin;   // kh*kw
            for (int ci = 0; ci < cin; ++ci)
                for (size_t i = 0; i < k; ++i) w[(static_cast<size_t>(ci) * cout + co) * k + i] *= s;
        }
        b[co] = (b[co] - mu[co]) * s + be[co];
    }
}

// [cout][cin][kh][kw] -> [group][cin][kh][kw][CO] (zero padded), bias padded to groups*CO
PackedConv pack_conv(ake_pcnet* n, const std::vector<double>& w, const std::vector<double>& b, int cout, int cin, int kh, int kw) {
    PackedConv p;
    p.cin = cin; p.cout = cout; p.kh = kh; p.kw = kw;
    p.co = pick_co(cout);
    p.groups = (cout + p.co - 1) / p.co;
    auto& blob = n->blob;
    blob.resize(ake::align_up(blob.size(), 64));
    p.w_off = blob.size();
    blob.resize(blob.size() + static_cast<size_t>(p.groups) * cin * kh * kw * p.co, 0.f);
    for (int g = 0; g < p.groups; ++g)
        for (int ci = 0; ci < cin; ++ci)
            for (int dy = 0; dy < kh; ++dy)
                for (int dx = 0; dx < kw; ++dx)
                    for (int c = 0; c < p.co; ++c) {
                        const int co = g * p.co + c;
                        const double v = co < cout ? w[((static_cast<size_t>(co) * cin + ci) * kh + dy) * kw + dx] : 0.0;
                        blob[p.w_off + ((((static_cast<size_t>(g) * cin + ci) * kh + dy) * kw + dx) * p.co) + c] = static_cast<float>(v);
                    }
    blob.resize(ake::align_up(blob.size(), 64));
    p.b_off = blob.size();
    blob.resize(blob.size() + static_cast<size_t>(p.groups) * p.co, 0.f);
    for (int co = 0; co < cout; ++co) blob[p.b_off + co] = static_cast<float>(b[co]);
    if (kw == 7 || kw == 5 || kw == 3) {   // MFMA fragments (Toeplitz in time over kw taps)
        p.tb = cout >= 9 ? 1 : (cout >= 5 ? 2 : (cout >= 2 ? 4 : 16));
        p.ku = (p.tb + kw - 1 + 3) / 4 * 4;
        p.ntiles = (cout * p.tb + 15) / 16;
        p.nt = (p.tb == 1 && p.ntiles % 2 == 0 && kh <= 2) ? 2 : 1;   // tall kernels: B fragments dominate LDS, keep one N-tile
        const int ks = p.ku / 4;
        blob.resize(ake::align_up(blob.size(), 64));
        p.f_off = blob.size();
        const size_t frag = static_cast<size_t>(cin) * kh * ks * p.ntiles * 64;
        blob.resize(blob.size() + frag + static_cast<size_t>(ks) * p.ntiles * 64, 0.f);   // + one (ci,dy) of zero padding (prefetch)
        for (int ci = 0; ci < cin; ++ci)
            for (int dy = 0; dy < kh; ++dy)
                for (int s = 0; s < ks; ++s)
                    for (int nt = 0; nt < p.ntiles; ++nt)
                        for (int l = 0; l < 64; ++l) {
                            const int u = 4 * s + (l >> 4);
                            const int nn = nt * 16 + (l & 15);
                            const int co = nn / p.tb, tau = nn % p.tb;
                            const int dx = u - tau;
                            double v = 0.0;
                            if (co < cout && dx >= 0 && dx < kw) v = w[((static_cast<size_t>(co) * cin + ci) * kh + dy) * kw + dx];
                            blob[p.f_off + ((((static_cast<size_t>(ci) * kh + dy) * ks + s) * p.ntiles + nt) * 64) + l] = static_cast<float>(v);
                        }
    }
    return p;
}

// Data-gradient pack of a convolution: the transposed + flipped raw weights as a forward-type conv (cin' = cout, cout' = cin)
PackedConv dgrad_pack(ake_pcnet* n, int wspec, int cout, int cin, int kh, int kw) {
    const auto& w32 = T(n, wspec);
    std::vector<double> w(static_cast<size_t>(cin) * cout * kh * kw), b(cin, 0.0);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int dy = 0; dy < kh; ++dy)
                for (int dx = 0; dx < kw; ++dx)
                    w[((static_cast<size_t>(ci) * cout + co) * kh + (kh - 1 - dy)) * kw + (kw - 1 - dx)] =
                        w32[((static_cast<size_t>(co) * cin + ci) * kh + dy) * kw + dx];
    return pack_conv(n, w, b, cin, cout, kh, kw);
}

// --denseblock: a convolution with its raw weights (no BatchNorm behind it); a 1-wide kernel is stored as 7 taps with only the centre
// one non-zero, so that the 7-tap Toeplitz kernels run it (bspec < 0: bias=False)
PackedConv dense_conv_pack_w(ake_pcnet* n, const std::vector<float>& w32, const std::vector<float>* b32p, int cout, int cin, int kh, int kw_src);
PackedConv dense_conv_pack(ake_pcnet* n, int wspec, int bspec, int cout, int cin, int kh, int kw_src) {
    return dense_conv_pack_w(n, T(n, wspec), bspec < 0 ? nullptr : &T(n, bspec), cout, cin, kh, kw_src);
}
// the data-gradient pack of such a convolution: the weights transposed (cin <-> cout) and flipped on both axes, stored the same way
PackedConv dense_dgrad_pack(ake_pcnet* n, int wspec, int cout, int cin, int kh, int kw_src) {
    const auto& w32 = T(n, wspec);
    std::vector<float> w(static_cast<size_t>(cin) * cout * kh * kw_src);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int dy = 0; dy < kh; ++dy)
                for (int dx = 0; dx < kw_src; ++dx)
                    w[((static_cast<size_t>(ci) * cout + co) * kh + (kh - 1 - dy)) * kw_src + (kw_src - 1 - dx)] =
                        w32[((static_cast<size_t>(co) * cin + ci) * kh + dy) * kw_src + dx];
    return dense_conv_pack_w(n, w, nullptr, cin, cout, kh, kw_src);
}
PackedConv dense_conv_pack_w(ake_pcnet* n, const std::vector<float>& w32, const std::vector<float>* b32p, int cout, int cin, int kh, int kw_src) {
    std::vector<double> w(static_cast<size_t>(cout) * cin * kh * 7, 0.0), b(cout, 0.0);
    for (size_t r = 0; r < static_cast<size_t>(cout) * cin * kh; ++r) {
        if (kw_src == 7) for (int dx = 0; dx < 7; ++dx) w[r * 7 + dx] = w32[r * 7 + dx];
        else w[r * 7 + 3] = w32[r];
    }
    if (b32p) { const auto& b32 = *b32p; for (int co = 0; co < cout; ++co) b[co] = b32[co]; }
    if (kw_src == 1 && kh % 4 == 0) {   // 12 x 1: fragments [ci][row group g < kh / 4][ntile][64 lanes], lane = (k = row 4g + (l >> 4), n = co)
        PackedConv p;
        p.cin = cin; p.cout = cout; p.kh = kh; p.kw = 1; p.co = pick_co(cout); p.groups = (cout + p.co - 1) / p.co;
        p.tb = 1; p.ku = 4; p.ntiles = (cout + 15) / 16; p.nt = 1; p.row_k = 1;
        auto& blob = n->blob;
        blob.resize(ake::align_up(blob.size(), 64));
        p.w_off = blob.size();                                   // (no VALU-layout copy: only the MFMA kernel runs this form)
        p.b_off = blob.size();
        blob.resize(blob.size() + static_cast<size_t>(p.groups) * p.co, 0.f);
        for (int co = 0; co < cout; ++co) blob[p.b_off + co] = static_cast<float>(b[co]);
        blob.resize(ake::align_up(blob.size(), 64));
        p.f_off = blob.size();
        const int steps = kh / 4;
        blob.resize(blob.size() + static_cast<size_t>(cin + 1) * steps * p.ntiles * 64, 0.f);   // + one channel of zero padding (prefetch)
        for (int ci = 0; ci < cin; ++ci)
            for (int g = 0; g < steps; ++g)
                for (int nt = 0; nt < p.ntiles; ++nt)
                    for (int l = 0; l < 64; ++l) {
                        const int dy = 4 * g + (l >> 4), co = nt * 16 + (l & 15);
                        if (co < cout) blob[p.f_off + ((static_cast<size_t>(ci) * steps + g) * p.ntiles + nt) * 64 + l] = static_cast<float>(w32[(static_cast<size_t>(co) * cin + ci) * kh + dy]);
                    }
        return p;
    }
    return pack_conv(n, w, b, cout, cin, kh, 7);
}

// ---- launch helpers ---------------------------------------------------------------------

struct Tile {
    int R, TT, Tp, n_row_tiles, n_time_tiles, threads;
    size_t lds;
};

// Workgroup shape of the MFMA conv: every wave owns MT M-tiles (16 positions each), so a workgroup of W <= 8
// waves covers up to W*MT*16 positions = R rows x J frame groups; input channels are staged in chunks that fit
// the LDS budget.  Score = useful tile slots / issued, times the row-tile fill.
struct MTile { int W, cin_chunk; };
int device_cus();

// want_tiles > 1 (small batches): tilings with fewer (row, time) tiles than that lose score, so that the launch fills the chip.
bool choose_tile(bool fullrows, int cin, int H, int KH, int T_out, int TB, int KU, int NT, int MT, Tile* t, MTile* mt_out, int want_tiles = 1) {
    const int cap = 8 * MT * 16;
    const int T4 = (T_out + TW - 1) / TW * TW;
    double best = -1;
    Tile bt{};
    MTile bm{};
    for (int n_tt = 1; n_tt <= T4 / TW; ++n_tt) {
        const int TT = ((T4 / TW + n_tt - 1) / n_tt) * TW;
        const int n_tt_eff = (T_out + TT - 1) / TT;
        const int J = (TT + TB - 1) / TB;
        const int Tp = (TB * J - TB + KU + 3) / 4 * 4;
        if (Tp > 192) continue;                                          // the kernel's loader walks a patch row in at most 3 x 64 frames
        for (int R = fullrows ? H : 1; R <= (fullrows ? H : std::min(H, 64)); ++R) {
            if (R * J > cap) break;
            const int R_in = R + KH - 1;                                 // the row halo is always materialised
            const size_t per_ch = (static_cast<size_t>(R_in) * Tp + static_cast<size_t>(KH) * (KU / 4) * NT * 64) * sizeof(float);   // A rows + B fragments
            if (per_ch > kLdsBudget) break;
            const int max_chunk = static_cast<int>(std::min<size_t>(cin, std::min<size_t>(kLdsBudget, 48 * 1024) / per_ch));
            if (max_chunk < 1) continue;
            const int n_chunks = (cin + max_chunk - 1) / max_chunk;
            const int chunk = (cin + n_chunks - 1) / n_chunks;           // even split, no 7+1
            const int tiles = (R * J + 15) / 16;
            const int W = (tiles + MT - 1) / MT;
            const int row_tiles = (H + R - 1) / R;
            // useful positions / issued slots; mild preferences: fewer staged halo bytes, fuller workgroups
            const double useful = static_cast<double>(H) * T_out / TB;
            const double issued = static_cast<double>(row_tiles) * n_tt_eff * W * MT * 16;
            const double halo = static_cast<double>(R) / R_in * TT / (TT + KU);
            double eff = useful / issued * (0.85 + 0.15 * halo) * (0.9 + 0.1 * W / 8.0);
            if (want_tiles > 1) eff *= 0.3 + 0.7 * std::min(1.0, static_cast<double>((fullrows ? 1 : row_tiles) * n_tt_eff) / want_tiles);
            if (eff > best + 1e-9) {
                best = eff;
                bt = Tile{R, TT, Tp, fullrows ? 1 : row_tiles, n_tt_eff, W * 64, per_ch * chunk};
                bm = MTile{W, chunk};
            }
        }
    }
    if (best < 0) return false;
    *t = bt; *mt_out = bm;
    return true;
}

template <bool TRAIN>
int launch_mfma_t(const char* name, const PackedConv& pc, const MfmaArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
#define AKE_MFMA(KU_, NT_, MT_) return ake::launch(name, conv_mfma_kernel<KU_, NT_, MT_, TRAIN>, grid, block, lds, s, a)
    if (pc.ku == 8 && pc.nt == 1) AKE_MFMA(8, 1, 3);
    if (pc.ku == 8 && pc.nt == 2) AKE_MFMA(8, 2, 3);
    if (pc.ku == 12 && pc.nt == 1) AKE_MFMA(12, 1, 3);
    if (pc.ku == 24 && pc.nt == 1) AKE_MFMA(24, 1, 3);
    if (pc.ku == 4 && pc.nt == 1) AKE_MFMA(4, 1, 3);
    if (pc.ku == 4 && pc.nt == 2) AKE_MFMA(4, 2, 3);              // kernel_size 3: the genre head's (1, 3) conv
    if (pc.ku == 20 && pc.nt == 1) AKE_MFMA(20, 1, 3);            // kernel_size 3 / 5: the heads' one-channel last convs (16 frames per column group)
#undef AKE_MFMA
    ake::set_error("conv: no MFMA kernel for KU=%d NT=%d", pc.ku, pc.nt);
    return AKE_ERR_UNSUPPORTED;
}

// inference launches carry none of the training-mode code (pending BatchNorm on load, statistics, accumulation)
int launch_mfma(const char* name, const PackedConv& pc, const MfmaArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    const bool train = a.c.in_affine || a.c.stats || a.c.accumulate || a.c.rows_zero;      // (rows_zero: only the TRAIN form's loader zero-pads the rows)
    return train ? launch_mfma_t<true>(name, pc, a, grid, block, lds, s) : launch_mfma_t<false>(name, pc, a, grid, block, lds, s);
}

struct Src {
    const float* p0; int c0; const float* p1; int c1; int h1;
    int ctot0 = 0;           // channels of the buffer p0 points into when only its first c0 are read (0: c0)
};

struct ConvGeom {            // explicit geometry for the data-gradient convolutions
    int py, pad_l, T_out, H_out, time_circ;
};

using ake::launch_flat;

// What only some callers of run_conv set (the defaults are the inference forward's)
struct ConvOpts {
    const float* in_affine = nullptr;   // training: the input's pending [cin][3] table, applied on load
    double* stats = nullptr;            // training: the raw output's per-channel statistics land here
    const ConvGeom* geom = nullptr;     // padding and output size given outright instead of derived from `kind`
    bool accumulate = false;            // dst += instead of dst =
    const float* residual = nullptr;    // dense [B][cout][H_out][T_out], added before the LeakyReLU
    bool rows_zero = false;             // rows beyond the map are zeros, not wrapped
};

// One convolution of the net.  `kind`: 0 pitch conv (7x7 circular both axes), 1 equivariant pitch-class
// conv (12 x k, rows circular), 2 genre conv (kh in {1,2}, rows valid).
int run_conv(const ake_pcnet* n, const PackedConv& pc, int kind, Src src, int batch, int H, int T_in, bool same_time,
             bool lrelu, float* dst, int dst_ctot, int dst_coff, hipStream_t s, const char* name, const ConvOpts& o = {}) {
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    AKE_REQUIRE(pc.kw == 7 || pc.kw == 5 || pc.kw == 3 || pc.row_k, AKE_ERR_UNSUPPORTED, "conv: kernel width %d not built (3, 5, 7)", pc.kw);
    AKE_REQUIRE(src.c0 + src.c1 == pc.cin, AKE_ERR_STATE, "conv %s: cin mismatch", name);
    a.src0 = src.p0; a.c0 = src.c0; a.src1 = src.p1; a.c1 = src.c1; a.h1 = src.h1 > 0 ? src.h1 : 1;
    a.H = H; a.T_in = T_in;
    a.src0_clip_stride = static_cast<long long>(src.ctot0 > 0 ? src.ctot0 : src.c0) * H * T_in;
    a.rows_zero = o.rows_zero ? 1 : 0;
    a.src1_clip_stride = static_cast<long long>(src.c1) * a.h1 * T_in;
    const bool fullrows = kind != 0;
    if (kind == 0) { a.py = pc.kh / 2; a.pad_l = pc.kw / 2; a.time_circ = 1; a.T_out = T_in; a.H_out = H; }
    else {
        a.py = 0; a.time_circ = 0;
        a.pad_l = same_time ? pc.kw / 2 : 0;
        a.T_out = same_time ? T_in : T_in - pc.kw + 1;
        a.H_out = kind == 1 ? H : H - pc.kh + 1;
    }
    if (o.geom) { a.py = o.geom->py; a.pad_l = o.geom->pad_l; a.T_out = o.geom->T_out; a.H_out = o.geom->H_out; a.time_circ = o.geom->time_circ; }
    AKE_REQUIRE(a.T_out > 0, AKE_ERR_INVALID, "conv %s: %d frames is too short for the valid head convolutions", name, T_in);
    a.w = n->blob_dev + pc.w_off; a.bias = n->blob_dev + pc.b_off; a.cout = pc.cout;
    a.dst = dst; a.dst_coff = dst_coff; a.dst_clip_stride = static_cast<long long>(dst_ctot) * a.H_out * a.T_out;
    a.lrelu = lrelu ? 1 : 0;
    a.in_affine = o.in_affine; a.stats = o.stats; a.stats_stride = 2 * n->bn_channels; a.accumulate = o.accumulate ? 1 : 0;
    a.residual = o.residual; a.residual_clip_stride = static_cast<long long>(pc.cout) * a.H_out * a.T_out;      // dense [B][cout][H][T]
    Tile t;
    MTile mtile;
    constexpr int MT = 3;
    const int cout_tiles = std::max(1, pc.ntiles / pc.nt);
    const int want_tiles = (std::max(device_cus(), 1) + batch * cout_tiles - 1) / (batch * cout_tiles);      // 1 at the bench / training batch sizes
    AKE_REQUIRE(choose_tile(fullrows, pc.cin, H, pc.kh, a.T_out, pc.tb, pc.ku, pc.nt, MT, &t, &mtile, want_tiles), AKE_ERR_UNSUPPORTED,
                "conv %s: no tile fits LDS (cin=%d H=%d)", name, pc.cin, H);
    a.R = t.R; a.TT = t.TT; a.Tp = t.Tp; a.n_row_tiles = t.n_row_tiles; a.n_time_tiles = t.n_time_tiles;
    a.w = n->blob_dev + pc.f_off;
    MfmaArgs ma;
    ma.c = a; ma.TB = pc.tb; ma.KH = pc.row_k ? pc.kh / 4 : pc.kh; ma.ntiles_total = pc.ntiles; ma.cin_chunk = mtile.cin_chunk;
    ma.row_k = pc.row_k;
    ma.ksplit = 0;
    ma.h1_magic = (65536 + a.h1 - 1) / a.h1;
    if (mtile.W == 1 && pc.cin * pc.kh >= 16) {   // tiny M (1-channel head convs): split the (channel, dy) steps over 8 waves instead
        ma.ksplit = 1;
        mtile.W = 8;
        t.threads = 8 * 64;
        t.lds = std::max<size_t>(t.lds, static_cast<size_t>(8) * MT * pc.nt * 64 * sizeof(float) * 4);
    }
    dim3 grid(t.n_row_tiles * t.n_time_tiles, pc.ntiles / pc.nt, batch), block(t.threads);
    return launch_mfma(name, pc, ma, grid, block, t.lds, s);
}

// does inference run layer i's Pitch2Pitch stack on the bf16 kernel (everything but its first conv)?
// (the bf16 kernels keep all frames of their row tile in one LDS patch: long clips fall back to the time-tiled f32 kernel)
bool p2p_uses_f16(const ake_pcnet* n, int i, int T) {
    const auto& c = n->cfg;
    if (c.precision == AKE_PRECISION_F32X3 || c.resblock || i < 1 || c.conv_layers < 2 || n->dims[i].out_p != 8 || T > 146) return false;
    for (int j = 0; j < c.conv_layers; ++j)
        if (n->p2p[i][j].eval.bf_off < 0) return false;
    return true;
}

// does inference run layer i's PitchClass2PitchClass stack on conv_pc_bf16_kernel?
constexpr int kPcBf16MaxFrames = 120;
bool pc2pc_uses_bf16(const ake_pcnet* n, int i, int T) {
    if (n->cfg.resblock || n->pc2pc[i].empty() || T > kPcBf16MaxFrames) return false;
    for (const ConvSite& cs : n->pc2pc[i])
        if (cs.eval.bf_off < 0 || cs.eval.cout != 16) return false;
    return true;
}

// Row pitch of the pitch convs' LDS patch, in positions (16 B each): >= 2J + 6 (three halo frames either side), and 2J + 16 so that
// an M-tile that runs over a row end (m = r * J + j: its lanes then sit in two patch rows) still reads 16 distinct 16-byte slots per
// ds_read_b128 lane group -- the A-fragment address is r * Tp + 2j + q, a row change adds Tp - 2J, and the LDS has 16 slots per clock.
// With 2J + 6 the straddling tiles (40 % of them at J = 38) paid two-way conflicts: SQ_LDS_BANK_CONFLICT was 26-28 % of the LDS cycles
// of the three launches (profiles/r02_c_pmc_lds.md) in a multiply loop that is bound by exactly those reads.
inline int p2p_pitch(int J) { return 2 * J + 16; }

// 8 -> 8 channel 7x7 pitch convolution on bf16 MFMA (conv_p2p_f16_kernel): channels-last split planes in, planes or NCHW f32 out
int run_p2p_f16(const ake_pcnet* n, const PackedConv& pc, const unsigned short* xh, const Src* nchw, int batch, int H, int T,
                 float* dst_nchw, int dst_ctot, unsigned short* oh, hipStream_t s, const char* name) {
    P2pBfArgs a;
    std::memset(&a, 0, sizeof(a));
    a.xh = xh;
    if (nchw) { a.p = nchw->p0; a.c0 = nchw->c0; a.u = nchw->p1; a.c1 = nchw->c1; a.h1 = nchw->h1 > 0 ? nchw->h1 : 1; } a.bfrag = n->bf_frags_dev + pc.bf_off; a.bias = n->blob_dev + pc.b_off;
    a.dst = dst_nchw; a.dst_clip_stride = static_cast<long long>(dst_ctot) * H * T; a.dst_coff = 0;
    a.oh = oh;
    a.H = H; a.T = T;
    a.J = (T + 1) / 2;
    a.Tp = p2p_pitch(a.J);
    a.R = std::max(1, std::min(H, 8 * kP2pMT * 16 / a.J));
    auto lds_of = [&](int R) { return (static_cast<size_t>(R + 6) * a.Tp + (kP2pStreamB ? 0 : kBfFragsPerConv)) * sizeof(uint4); };
    while (a.R > 1 && lds_of(a.R) > 76 * 1024) --a.R;
    AKE_REQUIRE(lds_of(a.R) <= 150 * 1024, AKE_ERR_UNSUPPORTED, "conv %s: %d frames do not fit the bf16 kernel's LDS patch", name, T);
    a.n_row_tiles = (H + a.R - 1) / a.R;
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 150 * 1024, conv_p2p_f16_kernel<true, false>, conv_p2p_f16_kernel<false, false>, conv_p2p_f16_kernel<true, true>);
    if (rc) return rc;
    dim3 grid(a.n_row_tiles, 1, batch), block(512);
    AKE_REQUIRE(!nchw || oh, AKE_ERR_STATE, "conv %s: the assembling variant writes channels-last planes", name);
    if (nchw) return ake::launch(name, conv_p2p_f16_kernel<true, true>, grid, block, lds_of(a.R), s, a);
    if (oh) return ake::launch(name, conv_p2p_f16_kernel<true, false>, grid, block, lds_of(a.R), s, a);
    return ake::launch(name, conv_p2p_f16_kernel<false, false>, grid, block, lds_of(a.R), s, a);
}

// debug switch (ake_debug_keep_taps): keep every activation that ake_pcnet_tap_* can name in memory, i.e. no fusion across them
int g_keep_taps = 0;

int device_cus() {
    static int n_cus = 0;
    if (!n_cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n_cus = -1;
    }
    return n_cus;
}

// row-tile height of the persistent pitch-conv kernel for H x T maps (0: the shape does not qualify); `semi`: the form fused with the
// semitone conv (tiles of 3k rows, no staging slabs but a double-buffered output patch and that conv's B fragments).  nw: waves of the workgroup (8; 16: a phase of
// p2p_stack_kernel, whose semitone form always folds: its tile height also divides the octave's 36 rows)
int p2p_ps_rows(int H, int T, bool semi, int* plane_pos, size_t* lds, int nw = 8) {
    if (T < 2 || (T & 1) || device_cus() < 8) return 0;
    const int J = T / 2, Tp = p2p_pitch(J);
    auto plane_of = [&](int R) { return ((R + 6) * Tp + 63) / 64 * 64; };
    auto lds_of = [&](int R) { return (static_cast<size_t>(2) * plane_of(R) + (semi ? 2 * nw * kP2pMT * 16 * 2 + kP2pSemiFrags : nw * kP2pMT * kP2pPsStage)) * sizeof(uint4); };
    int R = std::max(1, std::min(H, nw * kP2pMT * 16 / J));
    if (semi) R = R / 3 * 3;
    while (R >= (semi ? 3 : 1) && (lds_of(R) > 156 * 1024 || plane_of(R) / 64 > nw * kP2pPieces || (semi && nw == 16 && 36 % R))) R -= semi ? 3 : 1;     // the loader: nw waves x kP2pPieces pieces
    if (R < (semi ? 3 : 1) || H < R + 6) return 0;
    if (semi && (H % 3 || (H / 3) % 12)) return 0;
    if (plane_pos) *plane_pos = plane_of(R);
    if (lds) *lds = lds_of(R);
    return R;
}

// does inference fuse the semitone conv of layer i into the last pitch conv of its stack (the pitch tensor is then never written)?
// Only in the net's last layer: an inner layer's pitch tensor is also the next layer's pitch stream (time_pool_p, models.py:395).
bool p2p_fuses_semi(const ake_pcnet* n, int i, int P, int T) {
    return !g_keep_taps && !n->cfg.p2pc_conv && !n->cfg.stay_sixth && i == n->cfg.num_layers - 1 && p2p_uses_f16(n, i, T) && static_cast<size_t>(i) < n->semi.size() && n->semi[i].eval.bf_off >= 0 &&
           p2p_ps_rows(P, T, true, nullptr, nullptr) > 0;
}

// ---- the persistent pitch conv (conv_p2p_f16_ps_kernel): one workgroup per CU walks the row tiles ----
// What one launch reads and writes.  The forms decide the kernel instance and whether a shape qualifies (p2p_ps_plan); the pointers
// only matter to the launch.
enum class P2pIn : unsigned char {
    Planes,           // the channels-last f16 plane the conv before it wrote
    Src,              // NCHW f32: the pitch stream (c0 channels) | the up_sixth map (c1 channels of h1 rows), assembled by the kernel's loader
    SrcFramesMajor,   // ... with the one pitch-stream channel stored [clip][T][H] (ake_pcnet_forward_frames_major_f32)
    SrcF16x4,         // ... both as layer 0 left them: the CQT as f16 hi | lo words (Buffers::melh), the map as f16 x 4 words (Layer0Args::psix_h)
};
enum class P2pOut : unsigned char {
    Plane,            // a channels-last f16 plane for the next conv
    Nchw,             // the pitch tensor [clip][8][H][T] f32
    Semi,             // fused with the semitone conv: the semitone maps [clip][8][H / 3][T] (the pitch tensor is never written)
    SemiFold,         // ... and with the maximum over the octaves: channels [fold_coff, fold_coff + 8) of the concat buffer [clip][dst_ctot][12][T]
};
struct P2pPsIo {
    P2pIn in = P2pIn::Planes;
    const unsigned short* planes = nullptr;       // in == Planes
    Src src{};                                    // every other input form
    P2pOut out = P2pOut::Plane;
    unsigned short* plane = nullptr;              // out == Plane
    float* dst = nullptr;                         // every other output form
    int dst_ctot = 0;                             // channels of the tensor `dst` points into
    int fold_coff = 0;                            // out == SemiFold
    const PackedConv* semi = nullptr;             // out == Semi / SemiFold: the semitone conv
};

// Launch geometry of one such conv for `batch` clips of H x T maps; ok == false: the shape does not qualify and the tiled
// conv_p2p_f16_kernel runs instead.  Taken for even frame counts and enough tiles to give every CU at least two (always for the forms
// fused with the semitone conv; the folding form wants four units per CU: a unit is n_oct tiles in a row, small batches keep the
// tile-parallel form).  ws16: the workspace (hence every buffer carved from it) is 16-byte aligned.  Launches nothing.
struct P2pPsPlan {
    bool ok = false;
    P2pIn in = P2pIn::Planes;
    P2pOut out = P2pOut::Plane;
    int R = 0, plane_pos = 0, n_row_tiles = 0, n_tiles = 0, n_oct = 0, n_units = 0, grid = 0;
    size_t lds = 0;
};
P2pPsPlan p2p_ps_plan(P2pIn in, int c0, int c1, P2pOut out, int dst_ctot, bool semi_frags, int batch, int H, int T, bool ws16) {
    P2pPsPlan g;
    g.in = in; g.out = out;
    const bool semi = out == P2pOut::Semi || out == P2pOut::SemiFold;
    g.R = p2p_ps_rows(H, T, semi, &g.plane_pos, &g.lds);
    if (g.R <= 0 || batch < 1) return g;
    const int n_cus = device_cus();
    if (in != P2pIn::Planes) {
        if (out != P2pOut::Plane || c0 < 1 || c0 + c1 > 8) return g;
        if (in != P2pIn::Src && c0 != 1) return g;
        if (in == P2pIn::SrcF16x4 && (c1 < 1 || c1 > 4)) return g;
    }
    if (semi && !semi_frags) return g;
    g.n_row_tiles = (H + g.R - 1) / g.R;
    g.n_tiles = g.n_row_tiles * batch;
    if (out == P2pOut::SemiFold) {
        if (H % 36 || 36 % g.R) return g;
        g.n_oct = H / 36; g.n_units = batch * (36 / g.R);
        if (g.n_units < 4 * n_cus) return g;
    }
    if (!semi && g.n_tiles < 2 * n_cus) return g;
    if (out == P2pOut::Nchw &&      // 16-byte stores of 4 consecutive frames
        ((g.R * T) % 4 || (static_cast<long long>(H) * T) % 4 || (static_cast<long long>(dst_ctot) * H * T) % 4 || !ws16))
        return g;
    // two workgroups per CU when the LDS allows it (the kernel is built for 4 waves per SIMD): one's epilogue (vector work) and
    // barrier waits run under the other's multiply loop (bound by its LDS reads)
    const int wg_per_cu = ((in == P2pIn::Planes || in == P2pIn::SrcF16x4) && g.lds <= 80 * 1024 && g.n_tiles >= 4 * n_cus) ? 2 : 1;
    g.grid = std::min(wg_per_cu * (n_cus / 8 * 8), (g.n_tiles + 7) / 8 * 8);
    g.ok = true;
    return g;
}

// the launch of a planned conv; a plan that does not cover the call is a broken promise of the route, not a fall-back
int run_p2p_f16_ps(const ake_pcnet* n, const PackedConv& pc, const P2pPsPlan& g, const P2pPsIo& io, int batch, int H, int T, hipStream_t s, const char* name) {
    AKE_REQUIRE(g.ok, AKE_ERR_STATE, "conv %s: the route sent a shape to the persistent kernel that does not qualify for it", name);
    AKE_REQUIRE(g.in == io.in && g.out == io.out, AKE_ERR_STATE, "conv %s: the route planned the persistent kernel for another input / output form", name);
    AKE_REQUIRE(g.n_tiles == g.n_row_tiles * batch, AKE_ERR_STATE, "conv %s: the route planned the persistent kernel for another chunk than these %d clips", name, batch);
    const bool semi = io.out == P2pOut::Semi || io.out == P2pOut::SemiFold;
    AKE_REQUIRE((io.in == P2pIn::Planes ? io.planes != nullptr : io.src.p0 != nullptr) && (io.out == P2pOut::Plane ? io.plane != nullptr : io.dst != nullptr) &&
                    (!semi || (io.semi && io.semi->bf_off >= 0)) && (io.in != P2pIn::SrcF16x4 || io.src.p1),
                AKE_ERR_STATE, "conv %s: the persistent kernel's planned form lacks a buffer", name);
    AKE_REQUIRE(io.out != P2pOut::Nchw || !(reinterpret_cast<uintptr_t>(io.dst) & 15), AKE_ERR_STATE, "conv %s: the route planned 16-byte stores to an unaligned tensor", name);
    P2pPsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = g.R; a.plane_pos = g.plane_pos;
    a.bfrag = n->bf_frags_dev + pc.bf_off; a.bias = n->blob_dev + pc.b_off;
    if (io.in == P2pIn::Planes) a.xh = io.planes;
    else {
        const Src& x = io.src;
        a.p = x.p0; a.c0 = x.c0; a.u = x.p1 ? x.p1 : x.p0; a.c1 = x.p1 ? x.c1 : 0; a.h1 = x.h1 > 0 ? x.h1 : 1;
        a.p_fm = io.in == P2pIn::SrcFramesMajor ? 1 : 0;
        if (io.in == P2pIn::SrcF16x4) {
            a.uh = reinterpret_cast<const uint2*>(x.p1);
            a.ph = reinterpret_cast<const unsigned int*>(x.p0);
        }
    }
    a.dst = io.dst; a.dst_clip_stride = static_cast<long long>(io.dst_ctot) * (semi ? H / 3 : H) * T; a.oh = io.plane;
    if (semi) { a.sfrag = n->bf_frags_dev + io.semi->bf_off; a.sbias = n->blob_dev + io.semi->b_off; }
    a.H = H; a.T = T; a.J = T / 2; a.Tp = p2p_pitch(a.J);
    a.n_row_tiles = g.n_row_tiles; a.n_tiles = g.n_tiles;
    if (io.out == P2pOut::SemiFold) {
        a.n_oct = g.n_oct; a.n_units = g.n_units;
        a.dst = io.dst + static_cast<long long>(io.fold_coff) * 12 * T;
        a.dst_clip_stride = static_cast<long long>(io.dst_ctot) * 12 * T;
    }
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 160 * 1024, conv_p2p_f16_ps_kernel<3, 0>, conv_p2p_f16_ps_kernel<1, 0>, conv_p2p_f16_ps_kernel<1, 5>,
                                        conv_p2p_f16_ps_kernel<1, 8>, conv_p2p_f16_ps_kernel<0, 0>, conv_p2p_f16_ps_kernel<2, 0>, conv_p2p_f16_ps_kernel<1, 3>);
    if (rc) return rc;
    dim3 grid(g.grid), block(512);
    switch (io.out) {
        case P2pOut::SemiFold: return ake::launch(name, conv_p2p_f16_ps_kernel<3, 0>, grid, block, g.lds, s, a);
        case P2pOut::Semi: return ake::launch(name, conv_p2p_f16_ps_kernel<2, 0>, grid, block, g.lds, s, a);
        case P2pOut::Nchw: return ake::launch(name, conv_p2p_f16_ps_kernel<0, 0>, grid, block, g.lds, s, a);
        case P2pOut::Plane:
            if (io.in == P2pIn::Planes) return ake::launch(name, conv_p2p_f16_ps_kernel<1, 0>, grid, block, g.lds, s, a);
            if (io.in == P2pIn::SrcF16x4) return ake::launch(name, conv_p2p_f16_ps_kernel<1, 3>, grid, block, g.lds, s, a);
            if (a.c0 + a.c1 <= 5) return ake::launch(name, conv_p2p_f16_ps_kernel<1, 5>, grid, block, g.lds, s, a);
            return ake::launch(name, conv_p2p_f16_ps_kernel<1, 8>, grid, block, g.lds, s, a);
    }
    return AKE_OK;
}

// ---- a layer's whole pitch stack as one launch (p2p_stack_kernel): one workgroup of 16 waves per clip walks conv after conv ----
// Geometry of the phases (first conv fed by layer 0's f16 words | inner convs | last conv + semitone conv + octave fold); ok == false:
// the stack runs as one launch per conv.  Taken when the chunk fills the machine with one clip per workgroup -- no more clips than
// CUs, and at most one CU in sixteen left idle.  Launches nothing.
struct P2pStackPlan {
    bool ok = false;
    int n = 0;                              // phases = convs of the stack
    int R[2] = {0, 0}, plane_pos[2] = {0, 0}, n_row_tiles[2] = {0, 0};     // [0]: the plane-writing phases, [1]: the folding phase
    int n_oct = 0;
    size_t lds = 0;
};
P2pStackPlan p2p_stack_plan(int convs, int c0, int c1, bool semi_frags, int batch, int H, int T) {
    P2pStackPlan g;
    const int n_cus = device_cus();
    if (convs < 2 || convs > kP2pStackMax || c0 != 1 || c1 < 1 || c1 > 4 || !semi_frags || batch < 1 || batch > n_cus || 16 * (n_cus - batch) > n_cus) return g;
    size_t lds[2] = {0, 0};
    for (int f = 0; f < 2; ++f) {
        g.R[f] = p2p_ps_rows(H, T, f == 1, &g.plane_pos[f], &lds[f], 16);
        if (g.R[f] <= 0) return g;
        g.n_row_tiles[f] = (H + g.R[f] - 1) / g.R[f];
    }
    if (H % 36 || 36 % g.R[1]) return g;
    g.n_oct = H / 36;
    g.lds = std::max(lds[0], lds[1]);
    g.n = convs;
    g.ok = true;
    return g;
}

// the launch of a planned stack (the same contract as run_p2p_f16_ps: it cannot decline).  planes[j]: where conv j < n - 1 leaves its plane
int run_p2p_stack(const ake_pcnet* n, const std::vector<ConvSite>& convs, const PackedConv& semi, const P2pStackPlan& g, const unsigned int* melh, const uint2* psix_h,
                  int c1, unsigned short* const planes[], float* cat, int cat_ctot, int fold_coff, int batch, int H, int T, hipStream_t s, const char* name) {
    AKE_REQUIRE(g.ok && g.n == static_cast<int>(convs.size()) && batch <= device_cus(), AKE_ERR_STATE,
                "conv %s: the route sent a stack to the one-launch kernel that does not qualify for it", name);
    AKE_REQUIRE(melh && psix_h && cat && semi.bf_off >= 0, AKE_ERR_STATE, "conv %s: the one-launch stack lacks a buffer", name);
    P2pStackArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.n = g.n;
    for (int j = 0; j < g.n; ++j) {
        const bool fold = j == g.n - 1;
        P2pPsArgs& a = sa.ph[j];
        AKE_REQUIRE(fold || planes[j], AKE_ERR_STATE, "conv %s: the one-launch stack lacks a plane", name);
        a.R = g.R[fold]; a.plane_pos = g.plane_pos[fold]; a.n_row_tiles = g.n_row_tiles[fold]; a.n_tiles = a.n_row_tiles * batch;
        a.bfrag = n->bf_frags_dev + convs[j].eval.bf_off; a.bias = n->blob_dev + convs[j].eval.b_off;
        a.H = H; a.T = T; a.J = T / 2; a.Tp = p2p_pitch(a.J);
        if (j == 0) { a.ph = melh; a.uh = psix_h; a.c0 = 1; a.c1 = c1; a.h1 = 36; }
        else a.xh = planes[j - 1];
        if (!fold) a.oh = planes[j];
        else {
            a.sfrag = n->bf_frags_dev + semi.bf_off; a.sbias = n->blob_dev + semi.b_off;
            a.n_oct = g.n_oct; a.n_units = batch * (36 / a.R);
            a.dst = cat + static_cast<long long>(fold_coff) * 12 * T;
            a.dst_clip_stride = static_cast<long long>(cat_ctot) * 12 * T;
        }
    }
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 160 * 1024, p2p_stack_kernel);
    if (rc) return rc;
    return ake::launch(name, p2p_stack_kernel, dim3(batch), dim3(1024), g.lds, s, sa);
}

// ---- 7 x 7 circular pitch convolution with f32-equivalent products (conv_p2p_f16x3_kernel, persistent): train-mode forward (in_aff,
// bias, statistics), f32x3 inference (bias, LeakyReLU) and data gradient (none of them) ----
// Launch geometry for c0 + c1 input and cout output channels; ok == false: the shape does not qualify (conv_mfma_kernel runs it).
// dst16: the output tensor is 16-byte aligned.  Launches nothing; a convolution also needs its f16 x 3 fragments (PackedConv::bf_off).
struct P2pX3Plan {
    bool ok = false;
    int R = 0, plane_pos = 0, n_row_tiles = 0, n_tiles = 0, grid = 0;
    size_t lds = 0;
};
P2pX3Plan p2p_f16x3_plan(int c0, int c1, int cout, int batch, int H, int T, bool dst16) {
    P2pX3Plan g;
    if (T < 2 || (T & 1) || c0 < 1 || c0 + c1 > 8 || cout > 8 || batch < 1) return g;
    const int n_cus = device_cus();
    if (n_cus < 8) return g;
    const int Tp = p2p_pitch(T / 2);
    auto plane_of = [&](int R) { return ((R + 6) * Tp + 63) / 64 * 64; };
    auto lds_of = [&](int R) { return (static_cast<size_t>(4) * plane_of(R) + 8 * kP2pMT * kP2pPsStage) * sizeof(uint4); };
    int R = std::max(1, std::min(H, 8 * kP2pMT * 16 / (T / 2)));
    while (R >= 1 && (lds_of(R) > 156 * 1024 || plane_of(R) > 3 * 512)) --R;         // (the loader: three positions per thread)
    if (R < 1 || H < R + 6) return g;
    if ((R * T) % 4 || (static_cast<long long>(H) * T) % 4 || (static_cast<long long>(cout) * H * T) % 4 || !dst16) return g;
    g.R = R; g.plane_pos = plane_of(R); g.lds = lds_of(R);
    g.n_row_tiles = (H + R - 1) / R;
    g.n_tiles = g.n_row_tiles * batch;
    g.grid = std::min(n_cus / 8 * 8, (g.n_tiles + 7) / 8 * 8);
    g.ok = true;
    return g;
}

struct P2pX3Opts {
    const unsigned int* in_amax = nullptr;   // data gradients: the bits of the input's largest |value| (see run_nchw_to_cl16_f16x2)
    bool lrelu = false;                      // f32x3 inference: LeakyReLU on the output
};

int run_p2p_f16x3(const ake_pcnet* n, const P2pX3Plan& g, long long frag_off, const Src& src, const float* in_aff, const float* bias, int batch, int H, int T,
                  float* dst, int cout, double* stats, int stats_stride, hipStream_t s, const char* name, const P2pX3Opts& o = {}) {
    AKE_REQUIRE(g.ok && frag_off >= 0 && src.ctot0 == 0, AKE_ERR_STATE, "conv %s: a convolution that does not qualify was sent to the f16 x 3 persistent kernel", name);
    AKE_REQUIRE(g.n_tiles == g.n_row_tiles * batch, AKE_ERR_STATE, "conv %s: the f16 x 3 persistent kernel was planned for another batch than these %d clips", name, batch);
    AKE_REQUIRE(!(reinterpret_cast<uintptr_t>(dst) & 15), AKE_ERR_STATE, "conv %s: the f16 x 3 persistent kernel was planned for 16-byte stores to an unaligned tensor", name);
    P2pTrArgs a;
    std::memset(&a, 0, sizeof(a));
    a.J = T / 2; a.Tp = p2p_pitch(a.J);
    a.R = g.R; a.plane_pos = g.plane_pos;
    a.H = H; a.T = T;
    a.n_row_tiles = g.n_row_tiles; a.n_tiles = g.n_tiles;
    a.p = src.p0; a.c0 = src.c0; a.u = src.p1 ? src.p1 : src.p0; a.c1 = src.p1 ? src.c1 : 0; a.h1 = src.h1 > 0 ? src.h1 : 1;
    a.in_aff = in_aff; a.bfrag = n->bf_frags_dev + frag_off; a.bias = bias;
    a.dst = dst; a.dst_clip_stride = static_cast<long long>(cout) * H * T; a.cout = cout;
    a.stats = stats; a.stats_stride = stats_stride; a.in_amax = o.in_amax; a.lrelu = o.lrelu ? 1 : 0;
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 160 * 1024, conv_p2p_f16x3_kernel);
    if (rc) return rc;
    return ake::launch(name, conv_p2p_f16x3_kernel, dim3(g.grid), dim3(512), g.lds, s, a);
}

// semitone maps [clip][C][S][T] (aff: raw, with their pending table) -> channels [coff, coff + C) of the concat buffer
// [clip][ctot][12][T]: max over the octaves
int run_fold_max(const char* label, const float* smap, const float* aff, int C, int S, int batch, int T, float* dst, int dst_ctot, int dst_coff, hipStream_t s) {
    const long long total = static_cast<long long>(batch) * C * 12 * T;
    return launch_flat(label, fold_max_kernel, s, total, smap, aff, C, S, T, dst, static_cast<long long>(dst_ctot) * 12 * T, dst_coff, total);
}

// NCHW f32 [clip][C][12][T] -> channels-last split planes [clip][12][T][16] (hi plane, then lo plane, at `planes`)
int run_nchw_to_cl16(const float* src, int C, int batch, int T, unsigned short* planes, hipStream_t s) {
    const long long npos = static_cast<long long>(batch) * 12 * T;
    return launch_flat("nchw_to_cl16_kernel", nchw_to_cl16_kernel, s, npos, src, static_cast<long long>(C) * 12 * T, C, T, planes, planes + npos * 16, npos);
}

// does inference run the last layer's pitch-class stack + its time pooling as ONE launch (pc2pc_fused_kernel)?  The stack's
// intermediate activations then never leave LDS (ake_debug_keep_taps(1) keeps the per-conv launches for bisecting).
bool pc2pc_fuses(const ake_pcnet* n, int i, int T) {
    const auto& c = n->cfg;
    if (g_keep_taps || i < 1 || i != c.num_layers - 1 || c.time_pool_size != 2 || c.conv_layers < 1 || c.conv_layers > 4) return false;
    if (!pc2pc_uses_bf16(n, i, T) || T % 4 || 12 * T > 1024 || 3 * ((T + 15) / 16) > 16) return false;   // (16 waves: 3 row groups x 16-frame tiles)
    for (const ConvSite& cs : n->pc2pc[i])
        if (cs.eval.cout != 16 || cs.eval.cin > 16 || cs.eval.kh != 12) return false;
    return pc2pc_fused_lds_bytes(T) <= 160 * 1024;                                                  // two maps + the weight ring
}

int run_pc2pc_fused(const ake_pcnet* n, int i, const float* src, int cin, int batch, int T, float* pooled, unsigned short* feat_cl, hipStream_t s) {
    Pc2pcFusedArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src = src; a.src_clip_stride = static_cast<long long>(cin) * 12 * T; a.cin = cin;
    a.n_conv = static_cast<int>(n->pc2pc[i].size());
    for (int j = 0; j < a.n_conv; ++j) { a.bfrag[j] = n->bf_frags_dev + n->pc2pc[i][j].eval.bf_off; a.bias[j] = n->blob_dev + n->pc2pc[i][j].eval.b_off; }
    a.pooled = pooled;
    if (feat_cl) { a.fh = feat_cl; a.fl = feat_cl + static_cast<long long>(batch) * 12 * (T / 2) * 16; }
    a.T = T; a.Tp = T + 8;
    const size_t lds = pc2pc_fused_lds_bytes(T);
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 160 * 1024, pc2pc_fused_kernel);
    if (rc) return rc;
    return ake::launch("pc2pc_fused_kernel", pc2pc_fused_kernel, dim3(batch), dim3(1024), lds, s, a);
}

// does the f16 x 3 training form of conv_pc_bf16_kernel take this convolution (fragments built, patch fits the LDS)?
bool pc_f16x3_ok(const PackedConv& pt, int T_in, bool same_time) {
    if (pt.bf_off < 0 || pt.cin > 16) return false;
    const int T_out = same_time ? T_in : T_in - pt.kw + 1;
    if (T_out < 1) return false;
    const size_t lds = (static_cast<size_t>(2) * 12 * (T_out + 8) * 2 + 2 * 4 * ((pt.cout + 15) / 16) * 2 * 64) * sizeof(uint4);
    return lds <= 150 * 1024;
}

// training: NCHW f32 (+ the producer's pending BatchNorm + LeakyReLU) -> f16 hi / lo * 2^11 planes [hi: batch * 12 * T * 16][lo: ...]
// (src_ctot > 0: src points at the first of C channels inside a tensor of src_ctot channels)
// amax (data gradients): the bits of the tensor's largest |value|; the planes then hold value * f16_weight_scale(max) and the convolution
// that reads them (PcBfArgs::in_amax) divides it out again
int run_nchw_to_cl16_f16x2(const float* src, int C, int batch, int T, const float* aff, unsigned short* planes, hipStream_t s, int src_ctot = 0,
                           const unsigned int* amax = nullptr) {
    const long long npos = static_cast<long long>(batch) * 12 * T;
    return launch_flat("nchw_to_cl16_f16x2_kernel", nchw_to_cl16_f16x2_kernel, s, npos, src, static_cast<long long>(src_ctot > 0 ? src_ctot : C) * 12 * T, C, T, aff, planes,
                planes + npos * 16, npos, amax);
}

struct PcBf16Opts {
    const PackedConv* pc2 = nullptr;         // a second convolution of the same geometry over the same input, written to planes_out2
    unsigned short* planes_out2 = nullptr;
    bool f16x3 = false;                      // training / data gradients: f16 hi / lo planes in, f32-equivalent products, NCHW f32 out
    double* stats = nullptr;                 // f16x3: the raw output's per-channel statistics
    int stats_stride = 0;
    const unsigned int* in_amax = nullptr;   // f16x3 data gradients: the bits of the input's largest |value| (see run_nchw_to_cl16_f16x2)
};

// pitch-class convolution on bf16 MFMA (conv_pc_bf16_kernel): channels-last planes in; planes (cout == 16) or NCHW f32 out
int run_pc_bf16(const ake_pcnet* n, const PackedConv& pc, const unsigned short* planes_in, int batch, int T_in, bool same_time, bool lrelu,
                float* dst_nchw, unsigned short* planes_out, hipStream_t s, const char* name, const PcBf16Opts& o = {}) {
    PcBfArgs a;
    std::memset(&a, 0, sizeof(a));
    const long long npos_in = static_cast<long long>(batch) * 12 * T_in;
    a.xh = planes_in; a.xl = planes_in + npos_in * 16;
    a.bfrag = n->bf_frags_dev + pc.bf_off; a.bias = n->blob_dev + pc.b_off;
    a.T_in = T_in; a.T_out = same_time ? T_in : T_in - pc.kw + 1; a.pad_l = same_time ? pc.kw / 2 : 0;
    AKE_REQUIRE(a.T_out > 0, AKE_ERR_INVALID, "conv %s: %d frames is too short for the valid head convolutions", name, T_in);
    a.Tp = a.T_out + 8;
    a.cout = pc.cout; a.lrelu = lrelu ? 1 : 0;
    a.KH = pc.kh; a.circular = pc.kh == 12 ? 1 : 0;
    const int H_out = a.circular ? 12 : 12 - pc.kh + 1;
    a.dst = dst_nchw; a.dst_clip_stride = static_cast<long long>(pc.cout) * H_out * a.T_out;
    a.cl_stride = pc.cout;
    if (planes_out) { a.oh = planes_out; a.ol = planes_out + static_cast<long long>(batch) * H_out * a.T_out * pc.cout; }
    if (o.pc2) {   // a second convolution of the same geometry over the same input, as blockIdx.y == 1 (planes out only)
        AKE_REQUIRE(planes_out && o.planes_out2 && o.pc2->cout == pc.cout && o.pc2->kh == pc.kh && o.pc2->kw == pc.kw && o.pc2->cin == pc.cin && o.pc2->bf_off >= 0,
                    AKE_ERR_STATE, "conv %s: the paired convolution differs in shape", name);
        a.bfrag2 = n->bf_frags_dev + o.pc2->bf_off; a.bias2 = n->blob_dev + o.pc2->b_off;
        a.oh2 = o.planes_out2; a.ol2 = o.planes_out2 + static_cast<long long>(batch) * H_out * a.T_out * pc.cout;
    }
    a.stats = o.stats; a.stats_stride = o.stats_stride; a.in_amax = o.in_amax;
    AKE_REQUIRE(!o.f16x3 || (dst_nchw && !planes_out && !o.pc2), AKE_ERR_STATE, "conv %s: the f16 x 3 form writes NCHW f32", name);
    const size_t lds = (static_cast<size_t>(2) * 12 * a.Tp * 2 + 2 * 4 * ((pc.cout + 15) / 16) * 2 * 64) * sizeof(uint4);   // patch + weight ring
    AKE_REQUIRE(lds <= 150 * 1024, AKE_ERR_UNSUPPORTED, "conv %s: %d frames do not fit the bf16 kernel's LDS patch", name, T_in);
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 150 * 1024, conv_pc_bf16_kernel<1, true>, conv_pc_bf16_kernel<1, false>, conv_pc_bf16_kernel<2, false>,
                                        conv_pc_bf16_kernel<2, true>, conv_pc_bf16_kernel<1, false, true>, conv_pc_bf16_kernel<2, false, true>);
    if (rc) return rc;
    const int tiles = (H_out * a.T_out + 15) / 16;
    const int waves = std::min(8, (tiles + 3) / 4);
    dim3 grid((tiles + waves * 4 - 1) / (waves * 4), o.pc2 ? 2 : 1, batch), block(waves * 64);
    if (o.f16x3 && pc.cout <= 16) return ake::launch(name, conv_pc_bf16_kernel<1, false, true>, grid, block, lds, s, a);
    if (o.f16x3) return ake::launch(name, conv_pc_bf16_kernel<2, false, true>, grid, block, lds, s, a);
    if (pc.cout == 16 && planes_out) return ake::launch(name, conv_pc_bf16_kernel<1, true>, grid, block, lds, s, a);
    if (pc.cout == 16) return ake::launch(name, conv_pc_bf16_kernel<1, false>, grid, block, lds, s, a);
    if (planes_out) return ake::launch(name, conv_pc_bf16_kernel<2, true>, grid, block, lds, s, a);
    return ake::launch(name, conv_pc_bf16_kernel<2, false>, grid, block, lds, s, a);
}

// LDS of run_pc_f16x3_full's patch + weight ring for T_dz gradient frames (T_out = T_dz + 6, Tp = T_out + 8)
size_t pc_f16x3_full_lds(int T_dz) { return (static_cast<size_t>(2) * 12 * (T_dz + 14) * 2 + 2 * 4 * 2 * 64) * sizeof(uint4); }
bool pc_f16x3_full_ok(int T_dz) { return pc_f16x3_full_lds(T_dz) <= 150 * 1024; }

// f16 x 3 data gradient of a "valid" head convolution (32 -> 16 channels seen from the gradient): full correlation (pad 6 on both sides,
// T_out = T_dz + 6) of 16 gradient channels (planes) with one half of the transposed + flipped weights; dst [clip][16][12][T_out] (+)=.
int run_pc_f16x3_full(const ake_pcnet* n, long long frag_off, int kh, const unsigned short* planes, int batch, int T_dz, float* dst, bool accumulate,
                      hipStream_t s, const char* name, const unsigned int* in_amax = nullptr) {
    PcBfArgs a;
    std::memset(&a, 0, sizeof(a));
    const long long npos_in = static_cast<long long>(batch) * 12 * T_dz;
    a.xh = planes; a.xl = planes + npos_in * 16;
    a.bfrag = n->bf_frags_dev + frag_off; a.bias = nullptr;
    a.T_in = T_dz; a.T_out = T_dz + 6; a.pad_l = 6; a.Tp = a.T_out + 8;
    a.cout = 16; a.lrelu = 0; a.KH = kh; a.circular = kh == 12 ? 1 : 0;
    AKE_REQUIRE(kh == 12 || kh == 1, AKE_ERR_STATE, "conv %s: kernel rows %d", name, kh);
    a.dst = dst; a.dst_clip_stride = static_cast<long long>(16) * 12 * a.T_out; a.cl_stride = 16;
    a.accumulate = accumulate ? 1 : 0; a.in_amax = in_amax;
    const size_t lds = pc_f16x3_full_lds(T_dz);
    AKE_REQUIRE(pc_f16x3_full_ok(T_dz), AKE_ERR_UNSUPPORTED, "conv %s: %d frames do not fit the kernel's LDS patch", name, T_dz);
    static ake::DeviceOnce attr_set;
    const int rc = ake::raise_lds_limit(attr_set, 150 * 1024, conv_pc_bf16_kernel<1, false, true>);
    if (rc) return rc;
    const int tiles = (12 * a.T_out + 15) / 16;
    const int waves = std::min(8, (tiles + 3) / 4);
    dim3 grid((tiles + waves * 4 - 1) / (waves * 4), 1, batch), block(waves * 64);
    return ake::launch(name, conv_pc_bf16_kernel<1, false, true>, grid, block, lds, s, a);
}

// the semitone kernels' arguments: src [B][pc.cin][P][T]; dst: channels [coff, ..) of [B][ctot][12][T] (semi_fold_kernel) or the dense
// semitone maps (semi_conv_stats_kernel, which reads neither ctot nor coff)
SemiArgs semi_args(const ake_pcnet* n, const PackedConv& pc, const float* src, int P, int T, float* dst, int dst_ctot = 0, int dst_coff = 0) {
    SemiArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src = src; a.C = pc.cin; a.H = P; a.T = T;
    a.src_clip_stride = static_cast<long long>(pc.cin) * P * T;
    a.w = n->blob_dev + pc.w_off; a.bias = n->blob_dev + pc.b_off;
    a.dst = dst; a.dst_coff = dst_coff; a.dst_clip_stride = static_cast<long long>(dst_ctot) * 12 * T;
    a.n_strips = (T + TW - 1) / TW;
    return a;
}

int run_semi(const ake_pcnet* n, const PackedConv& pc, const float* src, int batch, int H, int Tn, float* dst,
             int dst_ctot, int dst_coff, hipStream_t s, const char* name) {
    const SemiArgs a = semi_args(n, pc, src, H, Tn, dst, dst_ctot, dst_coff);
    const int per_clip = 12 * a.n_strips;
    const int threads = per_clip >= 256 ? 256 : (per_clip + 63) / 64 * 64;
    dim3 grid((per_clip + threads - 1) / threads, pc.groups, batch), block(threads);
    switch (pc.co) {
        case 8: return ake::launch(name, semi_fold_kernel<8>, grid, block, 0, s, a);
        case 4: return ake::launch(name, semi_fold_kernel<4>, grid, block, 0, s, a);
        case 1: return ake::launch(name, semi_fold_kernel<1>, grid, block, 0, s, a);
        default: ake::set_error("semi: bad CO"); return AKE_ERR_UNSUPPORTED;
    }
}

}  // namespace

#include "pcnet_plan.h"

// (for the other translation units of the library: the handle's layout is private to this one)
int ake::pcnet_local_window(const ake_pcnet* n) { return n ? n->cfg.local : 0; }

extern "C" {

int ake_pcnet_precision(const ake_pcnet* n) { return n ? n->cfg.precision : AKE_ERR_INVALID; }

int ake_pcnet_default_config(ake_pcnet_config* cfg, int octaves, int genre) {
    AKE_REQUIRE(cfg && octaves > 0, AKE_ERR_INVALID, "ake_pcnet_default_config: bad argument");
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->pitches = 36 * octaves;      // train_model.py:92-95
    cfg->pitch_classes = 12;
    cfg->num_layers = 2; cfg->kernel_size = 7; cfg->conv_layers = 3; cfg->n_filters = 4;   // train_model.py:190-197
    cfg->head_layers = 2; cfg->time_pool_size = 2;                                          // train_model.py:212-217
    cfg->genre = genre ? 1 : 0;
    return AKE_OK;
}

int ake_pcnet_create(const ake_pcnet_config* cfg, ake_pcnet** out) {
    AKE_REQUIRE(cfg && out, AKE_ERR_INVALID, "ake_pcnet_create: null argument");
    const ake_pcnet_config& c = *cfg;
    AKE_REQUIRE(!c.only_semitones, AKE_ERR_UNSUPPORTED, "pcnet: the only_semitones variant is not built");
    AKE_REQUIRE(!(c.denseblock && (c.resblock || c.pc2p_mem || c.p2pc_conv || c.stay_sixth || c.local || c.kernel_size != 7)), AKE_ERR_UNSUPPORTED,
                "pcnet: denseblock together with resblock / pc2p_mem / p2pc_conv / stay_sixth / local / kernel_size != 7 is not built");
    AKE_REQUIRE(!(c.stay_sixth && c.pc2p_mem), AKE_ERR_UNSUPPORTED, "pcnet: stay_sixth together with pc2p_mem is not built");
    AKE_REQUIRE(c.local >= 0, AKE_ERR_INVALID, "pcnet: local = pooling window of the --local heads (0: off)");
    AKE_REQUIRE(c.pitch_classes == 12, AKE_ERR_UNSUPPORTED, "pcnet: pitch_classes must be 12");
    AKE_REQUIRE(c.pitches > 0 && c.pitches % 36 == 0, AKE_ERR_INVALID, "pcnet: pitches must be a multiple of 36");
    // --kernel_size (train_model.py:194): 7 runs the kernels built for it; 3 and 5 run every convolution on the generic kernels (conv_mfma_kernel,
    // conv_wgrad_kernel: kernel width is a parameter of theirs), inference and training
    AKE_REQUIRE(c.kernel_size == 7 || c.kernel_size == 5 || c.kernel_size == 3, AKE_ERR_UNSUPPORTED, "pcnet: kernel_size %d is not built (3, 5, 7)", c.kernel_size);
    AKE_REQUIRE(c.num_layers >= 1 && c.num_layers <= 4 && c.conv_layers >= 1 && c.n_filters >= 1 && c.head_layers >= 1,
                AKE_ERR_INVALID, "pcnet: bad layer counts");
    AKE_REQUIRE(c.time_pool_size >= 1, AKE_ERR_INVALID, "pcnet: bad time_pool_size");
    AKE_REQUIRE(c.precision == AKE_PRECISION_MIXED || c.precision == AKE_PRECISION_F32X3, AKE_ERR_INVALID,
                "pcnet: precision must be AKE_PRECISION_MIXED (0) or AKE_PRECISION_F32X3 (1), got %d", c.precision);
    auto* n = new ake_pcnet();
    n->cfg = c;
    if (c.local > 0) n->cfg.time_pool_size = 1;           // --local: the layers do not pool over time (models.py:348, 394)
    const int nf = c.n_filters, L = c.num_layers, k = c.kernel_size;
    n->dims.resize(L);
    for (int i = 1; i < L; ++i) {           // models.py:281-308
        LayerDims d;
        if (i == 1) { d.prev_p = 1; d.prev_pc = nf; d.out_p = 2 * nf; d.out_pc = 2 * d.out_p; }
        else {
            d.prev_p = i == 2 ? 2 * nf : 2 * nf * static_cast<int>(std::pow(4, i - 2));
            d.prev_pc = 2 * d.prev_p; d.out_p = 4 * d.prev_p; d.out_pc = 4 * d.prev_pc;
        }
        n->dims[i] = d;
    }
    n->final_ch = L == 1 ? nf : n->dims[L - 1].out_pc;   // models.py:694-710
    const int growth_all = nf * c.conv_layers;           // channels one dense block appends
    if (c.denseblock) {                                  // models.py:267-278 (layers), :678-689 (heads)
        int pp = 1, ppc = 1 + growth_all;
        for (int i = 1; i < L; ++i) {
            LayerDims d;
            d.prev_p = pp; d.prev_pc = ppc;
            d.out_p = pp + growth_all + ppc;             // block input (pitch stream | repeated up_sixth map) + its growth
            d.out_pc = ppc + d.out_p + growth_all;       // block input (pitch classes | folded semitone maps) + its growth
            n->dims[i] = d;
            pp = d.out_p; ppc = d.out_pc;
        }
        n->final_ch = L == 1 ? 1 + growth_all : n->dims[L - 1].out_pc;
    }
    // one dense block: layer j reads cin + j * nf channels; bn_size = cin / 2 (1 for a single input channel), models.py:189, 226
    auto add_dense_specs = [&](const std::string& base, int cin, bool equiv) {
        const int bott = (cin > 1 ? cin / 2 : 1) * nf;
        for (int j = 0; j < c.conv_layers; ++j) {
            const std::string lp = base + "denselayer" + std::to_string(j + 1) + ".";
            const int cj = cin + j * nf;
            add_bn_specs(n, lp + "norm1", cj);
            if (equiv) add_conv_specs(n, lp + "conv1.conv2d", bott, cj, 12, 1);
            else add_spec(n, lp + "conv1.weight", {bott, cj, 1, 1});                  // bias=False, models.py:464
            add_bn_specs(n, lp + "norm2", bott);
            if (equiv) add_conv_specs(n, lp + "conv2.conv2d", nf, bott, 12, k);
            else add_spec(n, lp + "conv2.weight", {nf, bott, k, k});
        }
    };
    // ---- expected state_dict entries ----
    for (int i = 0; i < L; ++i) {
        const std::string m = "model." + std::to_string(i) + ".";
        const LayerDims& d = n->dims[i];
        const int cs = i == 0 ? 1 : d.out_p;
        if (i == 0 || !c.stay_sixth) {                                        // --stay_sixth: no semitone conv after layer 0 (models.py:336)
            add_conv_specs(n, m + "pool_semi", cs, cs, 3, 3);                 // models.py:313 / :337
            add_bn_specs(n, m + "pool_semi_b", cs);
        }
        if (c.p2pc_conv) {                                                    // models.py:118-119: Pitch2PitchClassConv
            add_conv_specs(n, m + "pool.conv", cs, cs, c.pitches / 36, 1);
            add_bn_specs(n, m + "pool.bn", cs);
        }
        const int pc_in = i == 0 ? 1 : d.out_p + d.prev_pc, pc_out = i == 0 ? nf : d.out_pc;
        if (c.denseblock) {                                                   // models.py:188-189, 225-226
            add_dense_specs(m + "pc2pc.layer.0.", pc_in, true);
            if (i >= 1) {
                add_spec(n, m + "up_sixth.weight", {d.prev_pc, d.prev_pc, 3, 1});
                add_spec(n, m + "up_sixth.bias", {d.prev_pc});
                add_bn_specs(n, m + "up_sixth_b", d.prev_pc);
                add_dense_specs(m + "p2p.layer.0.", d.prev_pc + d.prev_p, false);
            }
            continue;
        }
        if (c.resblock) {                                                     // models.py:181-187: conv + BN, then conv_layers ResBlockEquivariant
            add_conv_specs(n, m + "pc2pc.layer.0.conv2d", pc_out, pc_in, 12, k);
            add_bn_specs(n, m + "pc2pc.layer.1", pc_out);
            for (int r = 0; r < c.conv_layers; ++r) {                         // models.py:429-441
                const std::string bp = m + "pc2pc.layer." + std::to_string(3 + r) + ".";
                add_conv_specs(n, bp + "conv1.conv2d", 2 * pc_out, pc_out, 12, k);
                add_bn_specs(n, bp + "b1", 2 * pc_out);
                add_conv_specs(n, bp + "conv2.conv2d", pc_out, 2 * pc_out, 12, k);
                add_bn_specs(n, bp + "b2", pc_out);
            }
        }
        for (int j = 0; j < c.conv_layers && !c.resblock; ++j) {              // models.py:191-197
            add_conv_specs(n, m + "pc2pc.layer." + std::to_string(3 * j) + ".conv2d", pc_out, j == 0 ? pc_in : pc_out, 12, k);
            add_bn_specs(n, m + "pc2pc.layer." + std::to_string(3 * j + 1), pc_out);
        }
        if (i >= 1) {
            if (!c.stay_sixth) {                                              // --stay_sixth: plain repeat of the pitch classes (models.py:322-323)
                add_spec(n, m + "up_sixth.weight", {d.prev_pc, d.prev_pc, 3, 1}); // models.py:325
                add_spec(n, m + "up_sixth.bias", {d.prev_pc});
                add_bn_specs(n, m + "up_sixth_b", d.prev_pc);
            }
            if (c.resblock) {                                                 // models.py:218-224, 402-414
                add_conv_specs(n, m + "p2p.layer.0", d.out_p, c.pc2p_mem ? d.prev_p : d.prev_pc + d.prev_p, k, k);
                add_bn_specs(n, m + "p2p.layer.1", d.out_p);
                for (int r = 0; r < c.conv_layers; ++r) {
                    const std::string bp = m + "p2p.layer." + std::to_string(3 + r) + ".";
                    add_conv_specs(n, bp + "conv1", 2 * d.out_p, d.out_p, k, k);
                    add_bn_specs(n, bp + "b1", 2 * d.out_p);
                    add_conv_specs(n, bp + "conv2", d.out_p, 2 * d.out_p, k, k);
                    add_bn_specs(n, bp + "b2", d.out_p);
                }
            }
            for (int j = 0; j < c.conv_layers && !c.resblock; ++j) {          // models.py:228-234
                add_conv_specs(n, m + "p2p.layer." + std::to_string(3 * j), d.out_p, j == 0 ? (c.pc2p_mem ? d.prev_p : d.prev_pc + d.prev_p) : d.out_p, k, k);
                add_bn_specs(n, m + "p2p.layer." + std::to_string(3 * j + 1), d.out_p);
            }
        }
    }
    for (const char* head : {"tonic_classifier", "key_classifier", "genre_classifier"}) {   // models.py:716-737
        const bool g = std::strcmp(head, "genre_classifier") == 0;
        if (g && !c.genre) continue;
        int ch = n->final_ch;
        for (int i = 0; i < c.head_layers; ++i) {
            const std::string base = std::string(head) + "." + std::to_string(3 * i) + (g ? "" : ".conv2d");
            if (i == c.head_layers - 1) {
                add_conv_specs(n, base, 1, ch, g ? 2 : 12, k);
            } else {
                const int co = i == 0 ? 2 * ch : ch;
                add_conv_specs(n, base, co, ch, g ? 1 : 12, k);
                add_bn_specs(n, std::string(head) + "." + std::to_string(3 * i + 1), co);
                ch = co;
            }
        }
    }
    n->host.resize(n->specs.size());
    n->grad_off.assign(n->specs.size(), 0);
    size_t goff = 0;
    for (size_t i = 0; i < n->specs.size(); ++i) {
        n->grad_off[i] = goff;
        size_t cnt = 1;
        for (int d = 0; d < n->specs[i].ndim; ++d) cnt *= static_cast<size_t>(n->specs[i].shape[d]);
        goff += cnt;
    }
    n->grad_floats = goff;
    *out = n;
    return AKE_OK;
}

void ake_pcnet_destroy(ake_pcnet* n) {
    if (!n) return;
    if (n->blob_dev) (void)hipFree(n->blob_dev);
    for (void* p : {static_cast<void*>(n->map_dev), static_cast<void*>(n->fold_ch_dev), static_cast<void*>(n->fold_bn_dev),
                    static_cast<void*>(n->run_off_dev), static_cast<void*>(n->run_off2_dev), static_cast<void*>(n->folded_dev), static_cast<void*>(n->bf_frags_dev),
                    static_cast<void*>(n->dense_aff_dev), static_cast<void*>(n->dense_aff_idx_dev)})
        if (p) (void)hipFree(p);
    delete n;
}

int ake_pcnet_pitches(const ake_pcnet* n) { return n ? n->cfg.pitches : 0; }

int ake_pcnet_num_tensors(const ake_pcnet* n) { return n ? static_cast<int>(n->specs.size()) : 0; }

int ake_pcnet_tensor_info(const ake_pcnet* n, int index, const char** name, int64_t shape[4], int* ndim) {
    AKE_REQUIRE(n && index >= 0 && index < static_cast<int>(n->specs.size()), AKE_ERR_INVALID, "tensor_info: index out of range");
    const TensorSpec& s = n->specs[index];
    if (name) *name = s.name.c_str();
    if (shape) std::memcpy(shape, s.shape, sizeof(s.shape));
    if (ndim) *ndim = s.ndim;
    return AKE_OK;
}

int ake_pcnet_set_tensor(ake_pcnet* n, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    AKE_REQUIRE(n && name && host_data && shape, AKE_ERR_INVALID, "set_tensor: null argument");
    auto it = n->spec_index.find(name);
    AKE_REQUIRE(it != n->spec_index.end(), AKE_ERR_INVALID, "set_tensor: unexpected key '%s' for this configuration", name);
    const TensorSpec& s = n->specs[it->second];
    AKE_REQUIRE(ndim == s.ndim, AKE_ERR_INVALID, "set_tensor: '%s' has %d dims, expected %d", name, ndim, s.ndim);
    size_t count = 1;
    for (int i = 0; i < ndim; ++i) {
        AKE_REQUIRE(shape[i] == s.shape[i], AKE_ERR_INVALID, "set_tensor: '%s' dim %d is %lld, expected %lld", name, i,
                    static_cast<long long>(shape[i]), static_cast<long long>(s.shape[i]));
        count *= static_cast<size_t>(shape[i]);
    }
    HostTensor& h = n->host[it->second];
    h.data.assign(host_data, host_data + count);
    h.set = true;
    n->finalized = false;
    return AKE_OK;
}

// Every BatchNorm layer is referenced by exactly one site, and every parameter that is not a running statistic by exactly one site or
// BatchNorm layer: a convolution or a BatchNorm that the walk over the sites forgets would train with a gradient of exact zeros.
static int check_sites(const ake_pcnet* n) {
    std::vector<int> bn_refs(n->bns.size(), 0), spec_refs(n->specs.size(), 0);
    auto ref_bn = [&](int bn) { if (bn >= 0) ++bn_refs[bn]; };
    auto ref_spec = [&](int spec) { if (spec >= 0) ++spec_refs[spec]; };
    auto see = [&](const ConvSite& cs) { ref_bn(cs.bn); ref_spec(cs.w); ref_spec(cs.b); };
    for (const auto* v : {&n->semi, &n->up, &n->foldc})
        for (const ConvSite& cs : *v) see(cs);
    for (const auto* vv : {&n->pc2pc, &n->p2p})
        for (const auto& v : *vv)
            for (const ConvSite& cs : v) see(cs);
    for (const Head& h : n->heads)
        for (const ConvSite& cs : h.convs) see(cs);
    for (const auto* vv : {&n->dense_pc, &n->dense_p})
        for (const auto& v : *vv)
            for (const DensePack& dp : v) { ref_bn(dp.bn1); ref_bn(dp.bn2); ref_spec(dp.w1); ref_spec(dp.b1); ref_spec(dp.w2); ref_spec(dp.b2); }
    for (size_t i = 0; i < n->bns.size(); ++i) {
        AKE_REQUIRE(bn_refs[i] == 1, AKE_ERR_STATE, "finalize: BatchNorm '%s' belongs to %d sites, not one", n->bns[i].name.c_str(), bn_refs[i]);
        ref_spec(n->bns[i].p.weight); ref_spec(n->bns[i].p.bias);
        spec_refs[n->bns[i].p.mean] = spec_refs[n->bns[i].p.var] = 1;      // running statistics: no gradient, their BatchNorm owns them
    }
    for (size_t i = 0; i < n->specs.size(); ++i)
        AKE_REQUIRE(spec_refs[i] == 1, AKE_ERR_STATE, "finalize: parameter '%s' belongs to %d sites, not one", n->specs[i].name.c_str(), spec_refs[i]);
    return AKE_OK;
}

// Packs every convolution of the net into the blob and resolves its site.  train == false (the first pass; it starts the sites afresh):
// eval-mode BatchNorm folded into w/b.  train == true: raw weights, the data-gradient packs, and each BatchNorm registered as a layer of
// its own (gamma/beta in the blob); the sites get their BatchNorm and parameter indices here.  This is the one place that spells the
// reference's state_dict names: a name that does not resolve, or a parameter left without a site, is AKE_ERR_STATE.
static int build_packs(ake_pcnet* n, bool train) {
    const auto& c = n->cfg;
    const int L = c.num_layers, k = c.kernel_size;
    if (!train) {
        n->semi.assign(L, {}); n->up.assign(L, {}); n->foldc.assign(L, {});
        n->pc2pc.assign(L, {}); n->p2p.assign(L, {});
        n->dense_pc.assign(L, {}); n->dense_p.assign(L, {});
        for (Head& h : n->heads) h.convs.clear();
    }
    std::string missing;             // the first name that did not resolve
    auto spec = [&](const std::string& name) {
        const auto it = n->spec_index.find(name);
        if (it != n->spec_index.end()) return it->second;
        if (missing.empty()) missing = name;
        return -1;
    };
    auto bn_specs = [&](const std::string& prefix) {
        return BnSpecs{spec(prefix + ".weight"), spec(prefix + ".bias"), spec(prefix + ".running_mean"), spec(prefix + ".running_var")};
    };
    auto add_bn = [&](const std::string& prefix, const BnSpecs& p, int C) {      // training pass: registers the layer, returns its index
        ake_pcnet::BnLayer l;
        l.name = prefix; l.C = C; l.ch_off = n->bn_channels; l.p = p;
        n->blob.resize(ake::align_up(n->blob.size(), 64));
        l.gamma_off = n->blob.size();
        for (float v : T(n, p.weight)) n->blob.push_back(v);
        l.beta_off = n->blob.size();
        for (float v : T(n, p.bias)) n->blob.push_back(v);
        n->bns.push_back(l);
        n->bn_channels += C;
        return static_cast<int>(n->bns.size()) - 1;
    };
    // One site: convolution `conv` (+ BatchNorm `bnp`, empty: none).  The eval pass folds and packs it, the training pass registers the
    // BatchNorm, packs the raw values and records the indices; pack(w, b) lays the values out in the blob.
    auto site = [&](ConvSite& cs, const std::string& conv, const std::string& bnp, int cout, size_t per_out, bool transposed, int cin, auto&& pack) {
        const int w = spec(conv + ".weight"), b = spec(conv + ".bias");
        const BnSpecs p = bnp.empty() ? BnSpecs{} : bn_specs(bnp);
        if (!missing.empty()) return;
        if (train) { cs.w = w; cs.b = b; cs.bn = bnp.empty() ? -1 : add_bn(bnp, p, cout); }
        std::vector<double> wv, bv;
        fold(n, w, b, train || bnp.empty() ? nullptr : &p, cout, per_out, transposed, cin, wv, bv);
        (train ? cs.train : cs.eval) = pack(wv, bv);
    };
    auto conv_site = [&](ConvSite& cs, const std::string& conv, const std::string& bnp, int cout, int cin, int kh, int kw) {
        site(cs, conv, bnp, cout, static_cast<size_t>(cin) * kh * kw, false, cin,
             [&](const std::vector<double>& w, const std::vector<double>& b) { return pack_conv(n, w, b, cout, cin, kh, kw); });
    };
    auto dgrad_site = [&](ConvSite& cs) {      // training pass: the data-gradient pack of a site conv_site has packed
        if (train && cs.w >= 0) cs.dgrad = dgrad_pack(n, cs.w, cs.train.cout, cs.train.cin, cs.train.kh, cs.train.kw);
    };
    // ch -> ch channels over kh taps, the values as they are stored ([ci][co][3] for up_sixth, [co][ci][n_oct] for the octave fold)
    auto plain = [&](int ch, int kh) {
        return [n, ch, kh](const std::vector<double>& w, const std::vector<double>& b) {
            PackedConv u;
            u.cin = u.cout = ch; u.kh = kh; u.kw = 1;
            n->blob.resize(ake::align_up(n->blob.size(), 64));
            u.w_off = n->blob.size();
            for (double v : w) n->blob.push_back(static_cast<float>(v));
            n->blob.resize(ake::align_up(n->blob.size(), 64));
            u.b_off = n->blob.size();
            for (double v : b) n->blob.push_back(static_cast<float>(v));
            return u;
        };
    };
    // a stack: conv_layers x (conv + BatchNorm), or --resblock's [conv0, (conv1, conv2) per block] with the data-gradient packs behind each block's two
    auto stack = [&](std::vector<ConvSite>& st, const std::string& prefix, const char* cv, int cin0, int cout, int kh) {
        st.resize(c.resblock ? 1 + 2 * c.conv_layers : c.conv_layers);
        if (c.resblock) {
            conv_site(st[0], prefix + "0" + cv, prefix + "1", cout, cin0, kh, k);
            dgrad_site(st[0]);
            for (int r = 0; r < c.conv_layers; ++r) {
                const std::string bp = prefix + std::to_string(3 + r) + ".";
                conv_site(st[1 + 2 * r], bp + "conv1" + cv, bp + "b1", 2 * cout, cout, kh, k);
                conv_site(st[2 + 2 * r], bp + "conv2" + cv, bp + "b2", cout, 2 * cout, kh, k);
                dgrad_site(st[1 + 2 * r]);
                dgrad_site(st[2 + 2 * r]);
            }
            return;
        }
        for (int j = 0; j < c.conv_layers; ++j) {
            conv_site(st[j], prefix + std::to_string(3 * j) + cv, prefix + std::to_string(3 * j + 1), cout, j == 0 ? cin0 : cout, kh, k);
            dgrad_site(st[j]);
        }
    };
    // --denseblock: layer j of a block reads cin + j * nf channels.  The convolutions keep their raw weights in both modes (the eval packs
    // serve the training forward); the training pass adds the blocks' BatchNorm layers in forward order and the data-gradient packs
    auto dense_block = [&](const std::string& base, int cin, bool equiv, std::vector<DensePack>& packs) {
        const int nf = c.n_filters, bott = (cin > 1 ? cin / 2 : 1) * nf;
        auto table = [&](const BnSpecs& bnp, int C, float slope) {
            const size_t off = n->dense_aff_floats;
            n->aff_recs.push_back({bnp, C, slope, off});
            n->dense_aff_floats += static_cast<size_t>(3) * C;
            return off;
        };
        packs.resize(c.conv_layers);
        for (int j = 0; j < c.conv_layers; ++j) {
            const std::string lp = base + "denselayer" + std::to_string(j + 1) + ".", cv = equiv ? ".conv2d" : "";
            const int cj = cin + j * nf;
            DensePack& dp = packs[j];
            const BnSpecs n1 = bn_specs(lp + "norm1"), n2 = bn_specs(lp + "norm2");
            const int w1 = spec(lp + "conv1" + cv + ".weight"), w2 = spec(lp + "conv2" + cv + ".weight");
            const int b1 = equiv ? spec(lp + "conv1" + cv + ".bias") : -1, b2 = equiv ? spec(lp + "conv2" + cv + ".bias") : -1;      // plain Conv2d: bias=False, models.py:464
            if (!missing.empty()) return;
            if (!train) {
                dp.aff1 = table(n1, cj, 0.01f);                                        // relu1 = nn.LeakyReLU, models.py:463 / :526
                dp.c1 = dense_conv_pack(n, w1, b1, bott, cj, equiv ? 12 : 1, 1);
                dp.aff2 = table(n2, bott, 0.f);                                        // relu2 = nn.ReLU, models.py:467 / :530
                dp.c2 = dense_conv_pack(n, w2, b2, nf, bott, equiv ? 12 : k, k);
            } else {
                dp.w1 = w1; dp.b1 = b1; dp.w2 = w2; dp.b2 = b2;
                dp.bn1 = add_bn(lp + "norm1", n1, cj);
                dp.bn2 = add_bn(lp + "norm2", n2, bott);
                dp.d1 = dense_dgrad_pack(n, w1, bott, cj, equiv ? 12 : 1, 1);
                dp.d2 = dense_dgrad_pack(n, w2, nf, bott, equiv ? 12 : k, k);
            }
        }
    };
    for (int i = 0; i < L; ++i) {
        const std::string m = "model." + std::to_string(i) + ".";
        const LayerDims& d = n->dims[i];
        const int cs = i == 0 ? 1 : d.out_p;
        if (i >= 1) {   // creation order mirrors the forward order: up_sixth, p2p, pool_semi, pc2pc
            if (!c.stay_sixth)      // ConvTranspose2d: the weight is [cin][cout][3]
                site(n->up[i], m + "up_sixth", m + "up_sixth_b", d.prev_pc, static_cast<size_t>(d.prev_pc) * 3, true, d.prev_pc, plain(d.prev_pc, 3));
            if (c.denseblock) dense_block(m + "p2p.layer.0.", d.prev_pc + d.prev_p, false, n->dense_p[i]);
            else stack(n->p2p[i], m + "p2p.layer.", "", c.pc2p_mem ? d.prev_p : d.prev_pc + d.prev_p, d.out_p, k);
        }
        if (i == 0 || !c.stay_sixth) conv_site(n->semi[i], m + "pool_semi", m + "pool_semi_b", cs, cs, 3, 3);
        if (c.p2pc_conv)
            site(n->foldc[i], m + "pool.conv", m + "pool.bn", cs, static_cast<size_t>(cs) * (c.pitches / 36), false, cs, plain(cs, c.pitches / 36));
        const int pc_in = i == 0 ? 1 : d.out_p + d.prev_pc, pc_out = i == 0 ? c.n_filters : d.out_pc;
        if (c.denseblock) dense_block(m + "pc2pc.layer.0.", pc_in, true, n->dense_pc[i]);
        else stack(n->pc2pc[i], m + "pc2pc.layer.", ".conv2d", pc_in, pc_out, 12);
    }
    for (int h : {1, 0, 2}) {       // tonic, key, genre: the order the reference creates them in (models.py:716-737)
        Head& hd = n->heads[h];
        const bool g = hd.kind == 2;
        if (g && !c.genre) continue;
        hd.convs.resize(c.head_layers);
        int ch = n->final_ch;
        for (int i = 0; i < c.head_layers; ++i) {
            const std::string base = std::string(hd.nm) + "." + std::to_string(3 * i) + (hd.conv2d ? ".conv2d" : "");
            if (i == c.head_layers - 1) conv_site(hd.convs[i], base, "", 1, ch, g ? 2 : 12, k);
            else {
                const int co = i == 0 ? 2 * ch : ch;
                conv_site(hd.convs[i], base, std::string(hd.nm) + "." + std::to_string(3 * i + 1), co, ch, g ? 1 : 12, k);
                ch = co;
            }
            dgrad_site(hd.convs[i]);
        }
    }
    if (!missing.empty()) {
        ake::set_error("finalize: the net reads tensor '%s', which this configuration's state_dict does not have", missing.c_str());
        return AKE_ERR_STATE;
    }
    if (!train) return AKE_OK;
    // raw copies of every tensor (small backward kernels read the reference layout)
    n->raw_w_off.assign(n->specs.size(), 0);
    for (size_t i = 0; i < n->specs.size(); ++i) {
        n->blob.resize(ake::align_up(n->blob.size(), 64));
        n->raw_w_off[i] = n->blob.size();
        for (float v : n->host[i].data) n->blob.push_back(v);
    }
    return check_sites(n);
}

constexpr int32_t kMapFolded = 1 << 30, kMapIndex = kMapFolded - 1;

namespace {

__global__ void fold_params_kernel(const float* __restrict__ params, const int32_t* __restrict__ fold_ch, const int32_t* __restrict__ fold_bn,
                                   float* __restrict__ folded, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = params[i];
    const int32_t f = fold_ch[i];
    if (f >= 0) {
        const int32_t* o = fold_bn + 4 * (f >> 1);
        const double s = static_cast<double>(params[o[0]]) / sqrt(static_cast<double>(params[o[3]]) + 1e-5);
        v = (f & 1) ? static_cast<float>((static_cast<double>(v) - static_cast<double>(params[o[2]])) * s + static_cast<double>(params[o[1]]))
                    : static_cast<float>(static_cast<double>(v) * s);
    }
    folded[i] = v;
}

__global__ void gather_blob_kernel(const float* __restrict__ params, const float* __restrict__ folded, const int32_t* __restrict__ map,
                                   float* __restrict__ blob, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t m = map[j];
    blob[j] = m < 0 ? 0.f : ((m & kMapFolded) ? folded : params)[m & kMapIndex];
}

// nn.BatchNorm2d's train-mode side effect on the flat parameter buffer: running <- (1-m)*running + m*(mean, unbiased var)
__global__ void running_stats_kernel(const float* __restrict__ bstats, const int32_t* __restrict__ run_off, float* __restrict__ params,
                                     float momentum, int n_ch) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_ch || run_off[2 * c] < 0) return;
    const float mean = bstats[3 * c], var = bstats[3 * c + 1], cnt = bstats[3 * c + 2];
    const float unbiased = var * cnt / fmaxf(cnt - 1.f, 1.f);
    float* rm = params + run_off[2 * c];
    float* rv = params + run_off[2 * c + 1];
    *rm = (1.f - momentum) * *rm + momentum * mean;
    *rv = (1.f - momentum) * *rv + momentum * unbiased;
}

void reset_packs(ake_pcnet* n) {
    n->blob.clear();
    n->bns.clear(); n->bn_channels = 0;
    n->aff_recs.clear(); n->dense_aff_floats = 0;
}


// The blob layout is a pure function of the configuration: build it once with index-coded values to learn, for every
// blob float, which flat parameter it comes from.  (Indices + 1 < 2^24 are exact in f32; the eval fold is neutralised by
// gamma = 1, beta = mean = 0, var = 1 - eps so that folded values still round to the index.)
int trace_maps(ake_pcnet* n) {
    std::vector<std::vector<float>> saved(n->specs.size());
    for (size_t i = 0; i < n->specs.size(); ++i) saved[i] = n->host[i].data;
    AKE_REQUIRE(n->grad_floats + 1 < (1u << 24), AKE_ERR_UNSUPPORTED, "finalize: %zu parameters exceed the index-trace range", n->grad_floats);
    auto ends_with = [](const std::string& a, const char* suf) { const size_t l = std::strlen(suf); return a.size() >= l && a.compare(a.size() - l, l, suf) == 0; };
    auto is_bn = [&](size_t i) {     // BatchNorm tensors are the ones that come with running statistics
        const std::string& nm = n->specs[i].name;
        const std::string prefix = nm.substr(0, nm.rfind('.'));
        return n->spec_index.count(prefix + ".running_mean") > 0;
    };
    auto fill_index = [&](size_t i) { for (size_t j = 0; j < n->host[i].data.size(); ++j) n->host[i].data[j] = static_cast<float>(n->grad_off[i] + j + 1); };
    // pass A: eval packs
    for (size_t i = 0; i < n->specs.size(); ++i) {
        const std::string& nm = n->specs[i].name;
        if (!is_bn(i)) { fill_index(i); continue; }
        const float v = ends_with(nm, ".weight") ? 1.f : (ends_with(nm, ".running_var") ? 1.f - 1e-5f : 0.f);
        std::fill(n->host[i].data.begin(), n->host[i].data.end(), v);
    }
    reset_packs(n);
    n->fold_records.clear();
    n->tracing = true;
    int rc = build_packs(n, false);
    n->tracing = false;
    const size_t eval_end = n->blob.size();
    // pass B: training packs (raw values everywhere)
    for (size_t i = 0; i < n->specs.size(); ++i) fill_index(i);
    if (!rc) rc = build_packs(n, true);
    for (size_t i = 0; i < n->specs.size(); ++i) n->host[i].data = saved[i];
    if (rc) return rc;
    n->blob.resize(ake::align_up(n->blob.size() + 64, 64), 0.f);
    n->map_host.assign(n->blob.size(), -1);
    for (size_t j = 0; j < n->blob.size(); ++j) {
        const long v = std::lround(static_cast<double>(n->blob[j]));
        if (v <= 0) continue;
        AKE_REQUIRE(static_cast<size_t>(v) <= n->grad_floats, AKE_ERR_STATE, "finalize: index trace out of range at blob[%zu]", j);
        n->map_host[j] = static_cast<int32_t>(v - 1) | (j < eval_end ? kMapFolded : 0);
    }
    return AKE_OK;
}

int upload_i32(const std::vector<int32_t>& v, int32_t** dev) {
    if (*dev) { (void)hipFree(*dev); *dev = nullptr; }
    AKE_HIP_CHECK(hipMalloc(dev, std::max<size_t>(v.size(), 1) * sizeof(int32_t)));
    AKE_HIP_CHECK(hipMemcpy(*dev, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return AKE_OK;
}

// --denseblock: (re)compute the BatchNorm-on-load tables from the flat parameter buffer on the device
int rebuild_dense_affine(ake_pcnet* n, const float* params_dev, hipStream_t s) {
    if (n->aff_recs.empty()) return AKE_OK;
    const int rows = static_cast<int>(n->dense_aff_floats / 3);
    if (!n->dense_aff_dev) {
        std::vector<int32_t> idx;
        idx.reserve(static_cast<size_t>(rows) * 5);
        for (const auto& r : n->aff_recs)
            for (int ch = 0; ch < r.C; ++ch) {
                int32_t bits;
                std::memcpy(&bits, &r.slope, sizeof(bits));
                for (int spec : {r.bn.weight, r.bn.bias, r.bn.mean, r.bn.var}) idx.push_back(static_cast<int32_t>(n->grad_off[spec]) + ch);
                idx.push_back(bits);
            }
        int rc = upload_i32(idx, &n->dense_aff_idx_dev);
        if (rc) return rc;
        AKE_HIP_CHECK(hipMalloc(&n->dense_aff_dev, n->dense_aff_floats * sizeof(float)));
    }
    return launch_flat("dense_affine_kernel", dense_affine_kernel, s, rows, params_dev, n->dense_aff_idx_dev, n->dense_aff_dev, rows);
}

int build_fold_tables(ake_pcnet* n) {
    std::vector<int32_t> fold_ch(n->grad_floats, -1), fold_bn, run_off(static_cast<size_t>(n->bn_channels) * 2, 0), run_off2(static_cast<size_t>(n->bn_channels) * 2, -1);
    n->recomputed_bn_channels = 0;
    auto off = [&](int spec) { return static_cast<int32_t>(n->grad_off[spec]); };
    int base = 0;
    for (const auto& r : n->fold_records) {
        const int32_t w0 = off(r.w), b0 = off(r.b);
        const size_t total = r.per_out * r.cout, k = r.transposed ? r.per_out / r.cin : 0;
        for (size_t i = 0; i < total; ++i) {
            const int co = r.transposed ? static_cast<int>((i / k) % r.cout) : static_cast<int>(i / r.per_out);
            fold_ch[w0 + i] = (base + co) << 1;
        }
        for (int co = 0; co < r.cout; ++co) {
            fold_ch[b0 + co] = ((base + co) << 1) | 1;
            for (int spec : {r.bn.weight, r.bn.bias, r.bn.mean, r.bn.var}) fold_bn.push_back(off(spec) + co);
        }
        base += r.cout;
    }
    for (const auto& l : n->bns)
        for (int c = 0; c < l.C; ++c) {
            run_off[2 * (l.ch_off + c)] = off(l.p.mean) + c;
            run_off[2 * (l.ch_off + c) + 1] = off(l.p.var) + c;
            // --denseblock: the reference checkpoints norm1 + conv1 of every dense layer (models.py:484-489, 553): autograd's backward runs that
            // half again, in train mode -- its BatchNorm blends the batch statistics into the running ones a second time
            const bool again = n->cfg.denseblock && l.name.size() > 6 && l.name.compare(l.name.size() - 6, 6, ".norm1") == 0;
            if (again) {
                run_off2[2 * (l.ch_off + c)] = run_off[2 * (l.ch_off + c)];
                run_off2[2 * (l.ch_off + c) + 1] = run_off[2 * (l.ch_off + c) + 1];
                ++n->recomputed_bn_channels;
            }
        }
    int rc;
    if ((rc = upload_i32(fold_ch, &n->fold_ch_dev)) || (rc = upload_i32(fold_bn, &n->fold_bn_dev)) || (rc = upload_i32(run_off, &n->run_off_dev)) || (rc = upload_i32(run_off2, &n->run_off2_dev)) ||
        (rc = upload_i32(n->map_host, &n->map_dev)))
        return rc;
    if (n->folded_dev) { (void)hipFree(n->folded_dev); n->folded_dev = nullptr; }
    AKE_HIP_CHECK(hipMalloc(&n->folded_dev, n->grad_floats * sizeof(float)));
    return AKE_OK;
}

// Inference runs the 8 -> 8 channel 7x7 pitch convolutions (every conv of a Pitch2Pitch stack but the first) on bf16 MFMA
// with split operands; their weight fragments are derived on the device from the eval packs, after every (re)pack.
bool pc_bf16_eligible(const PackedConv& pc) { return (pc.kh == 12 || pc.kh == 1) && pc.kw == 7 && pc.cin <= 16 && (pc.cout == 16 || pc.cout == 32); }

int rebuild_bf16_frags(ake_pcnet* n, hipStream_t s, bool train_only = false) {
    size_t count = 0;
    for (auto& layer : n->p2p)
        for (ConvSite& cs : layer) {
            PackedConv& pc = cs.eval;
            pc.bf_off = -1;
            if (pc.cin <= 8 && pc.cout == 8 && pc.kh == 7 && pc.kw == 7 && pc.co == 8) { pc.bf_off = static_cast<long long>(count); count += kBfFragsPerConv; }
        }
    // train-mode forward and data gradient of the pitch convs (conv_p2p_f16x3_kernel): f16 hi + lo fragments from the raw weights
    struct TrainFrag { PackedConv* pc; size_t raw; int cin, cout, flip; };
    std::vector<TrainFrag> tfr;
    if (!n->raw_w_off.empty())
        for (size_t i = 1; i < n->p2p.size(); ++i)
            for (ConvSite& cs : n->p2p[i]) {
                PackedConv& pt = cs.train;
                PackedConv& pd = cs.dgrad;
                pt.bf_off = pd.bf_off = -1;
                if (pt.kh != 7 || pt.kw != 7 || pt.cin > 8 || pt.cout > 8 || n->cfg.resblock || n->cfg.denseblock) continue;
                const size_t raw = n->raw_w_off[cs.w];
                pt.bf_off = static_cast<long long>(count); count += kBfFragsPerConv;
                tfr.push_back({&pt, raw, pt.cin, pt.cout, 0});
                pd.bf_off = static_cast<long long>(count); count += kBfFragsPerConv;
                tfr.push_back({&pd, raw, pt.cin, pt.cout, 1});
            }
    // training-mode forward of the pitch-class convs with 16 / 32 output channels (conv_pc_bf16_kernel<.., F16X3>): f16 hi + lo fragments
    // from the training packs (raw weights in the VALU layout)
    std::vector<PackedConv*> tpc;
    if (!n->raw_w_off.empty() && !n->cfg.resblock && !n->cfg.denseblock) {
        for (size_t i = 1; i < n->pc2pc.size(); ++i)
            for (ConvSite& cs : n->pc2pc[i]) tpc.push_back(&cs.train);
        for (Head& h : n->heads)
            if (h.kind == 2 ? h.convs.size() == 2 : !h.convs.empty()) tpc.push_back(&h.convs[0].train);
    }
    for (PackedConv* pc : tpc) {
        pc->bf_off = -1;
        if (pc_bf16_eligible(*pc)) { pc->bf_off = static_cast<long long>(count); count += static_cast<size_t>(pc->kh) * 4 * (pc->cout / 16) * 2 * 64 + 64; }
    }
    // data gradients of the pitch-class stacks of layers >= 1 (16 gradient channels in, <= 32 out: the first conv's is 24 wide) on the same
    // f16 x 3 kernel; the transposed + flipped weights are the data-gradient packs
    std::vector<PackedConv*> tpd;
    if (!n->raw_w_off.empty() && !n->cfg.resblock && !n->cfg.denseblock)
        for (size_t i = 1; i < n->pc2pc.size(); ++i)
            for (ConvSite& cs : n->pc2pc[i]) tpd.push_back(&cs.dgrad);
    for (PackedConv* pc : tpd) {
        pc->bf_off = -1;
        if (pc->kh == 12 && pc->kw == 7 && pc->cin == 16 && pc->cout <= 32) {
            pc->bf_off = static_cast<long long>(count);
            count += static_cast<size_t>(pc->kh) * 4 * ((pc->cout + 15) / 16) * 2 * 64 + 64;
        }
    }
    // ... and of the heads' first convolutions (32 gradient channels -> 16 features: two 16-channel halves, bf_off / bf_off2)
    std::vector<PackedConv*> thd;
    if (!n->raw_w_off.empty() && !n->cfg.resblock && !n->cfg.denseblock && n->cfg.head_layers == 2)
        for (Head& h : n->heads)
            if (!h.convs.empty()) thd.push_back(&h.convs[0].dgrad);
    for (PackedConv* pc : thd) {
        pc->bf_off = pc->bf_off2 = -1;
        if ((pc->kh == 12 || pc->kh == 1) && pc->kw == 7 && pc->cin == 32 && pc->cout == 16) {
            const size_t one = static_cast<size_t>(pc->kh) * 4 * 2 * 64 + 64;
            pc->bf_off = static_cast<long long>(count); pc->bf_off2 = static_cast<long long>(count + one);
            count += 2 * one;
        }
    }
    std::vector<PackedConv*> pcs;                             // pitch-class convolutions: the PitchClass2PitchClass stacks and the heads' first conv
    for (auto& layer : n->pc2pc)
        for (ConvSite& cs : layer) pcs.push_back(&cs.eval);
    for (Head& h : n->heads)                                  // (the genre head's is 1 x 7: rows independent)
        if (h.kind == 2 ? h.convs.size() == 2 : !h.convs.empty()) pcs.push_back(&h.convs[0].eval);
    for (PackedConv* pc : pcs) {
        pc->bf_off = -1;
        if (pc_bf16_eligible(*pc)) { pc->bf_off = static_cast<long long>(count); count += static_cast<size_t>(pc->kh) * 4 * (pc->cout / 16) * 2 * 64; }
    }
    std::vector<PackedConv*> h1;                              // 32 -> 1 last convolutions of the key / tonic heads (2-conv heads only)
    for (Head& h : n->heads)                                  // (the genre head's is 2 x 7 over valid rows)
        if (h.convs.size() == 2) h1.push_back(&h.convs[1].eval);
    for (PackedConv* pc : h1) {
        pc->bf_off = -1;
        if ((pc->kh == 12 || pc->kh == 2) && pc->kw == 7 && pc->cout == 1 && pc->co == 1 && pc->cin == 32) { pc->bf_off = static_cast<long long>(count); count += static_cast<size_t>(head1_ksteps(pc->kh)) * 2 * 64; }
    }
    if (!n->pc2pc.empty())                                   // layer 0's pitch-class stack (<= 4 channels): layer0_mfma_kernel
        for (ConvSite& cs : n->pc2pc[0]) {
            PackedConv& pc = cs.eval;
            pc.l0_off = -1;
            if (n->cfg.num_layers > 1 && pc.kh == 12 && pc.kw == 7 && pc.co == 4 && pc.groups == 1 && pc.cout <= 4 && pc.cin <= 4) {
                pc.l0_off = static_cast<long long>(count); count += 24 * 64 + 64;     // ... and the 4 inverse channel scales
            }
        }
    for (size_t i = 1; i < n->semi.size(); ++i) {            // semitone convs that follow an 8-channel pitch stack: fused into its last conv
        PackedConv& pc = n->semi[i].eval;
        pc.bf_off = -1;
        if (pc.cin == 8 && pc.co == 8 && pc.groups == 1 && i < n->p2p.size() && !n->p2p[i].empty() && n->p2p[i].back().eval.bf_off >= 0) {
            pc.bf_off = static_cast<long long>(count); count += 6 * 64 + 64;      // ... and the 8 inverse channel scales
        }
    }
    if (count == 0) return AKE_OK;
    if (n->bf_frags_count != count) {
        if (n->bf_frags_dev) { (void)hipFree(n->bf_frags_dev); n->bf_frags_dev = nullptr; }
        AKE_HIP_CHECK(hipMalloc(&n->bf_frags_dev, count * sizeof(uint4)));
        n->bf_frags_count = count;
    }
    ake::ProfScope ps("pack_bf16_kernels", s);               // one timer entry for all the packing launches of a load
    int rc;
    // train_only (ake_pcnet_load_for_training_f32, after every optimizer step): only the fragments the training-mode forward and the backward
    // read -- the inference kernels' (20 of the 40 launches; 0.2 ms of a 7 ms step) are rebuilt by the next full load
    n->eval_frags_stale = train_only;
    if (!train_only)
    for (const auto& layer : n->p2p)
        for (const ConvSite& cs : layer)
            if (cs.eval.bf_off >= 0 && (rc = ake::launch_untimed("pack_p2p_f16_kernel", pack_p2p_f16_kernel, dim3((14 * 64 + 255) / 256), dim3(256), 0, s,
                                                                 n->blob_dev + cs.eval.w_off, n->bf_frags_dev + cs.eval.bf_off, cs.eval.cin)))
                return rc;
    if (!train_only)
    for (const PackedConv* pc : pcs)
        if (pc->bf_off >= 0) {
            const int NT = pc->cout / 16;
            if ((rc = ake::launch_untimed("pack_pc_bf16_kernel", pack_pc_bf16_kernel, dim3((pc->kh * 4 * NT * 64 + 255) / 256), dim3(256), 0, s,
                                          n->blob_dev + pc->w_off, n->bf_frags_dev + pc->bf_off, pc->cin, pc->cout, pc->co, NT, pc->kh)))
                return rc;
        }
    if (!train_only && !n->pc2pc.empty())
        for (const ConvSite& cs : n->pc2pc[0])
            if (cs.eval.l0_off >= 0 && (rc = ake::launch_untimed("pack_l0_f16_kernel", pack_l0_f16_kernel, dim3(3), dim3(256), 0, s, n->blob_dev + cs.eval.w_off,
                                                                 n->bf_frags_dev + cs.eval.l0_off, cs.eval.cin, cs.eval.cout)))
                return rc;
    {   // the training-mode packs (pitch-class stacks, their data gradients, the heads' data gradients; the pitch convs' raw forms): ONE launch per
        // kernel for all of them, the jobs in the kernel argument (28 dependent launches of a few microseconds of work each were 0.39 ms per step)
        std::vector<PcPackJob> jobs;
        auto add = [&](const PackedConv* pc, long long off, int NT, int dy_rot, int ci_off) {
            jobs.push_back(PcPackJob{n->blob_dev + pc->w_off, n->bf_frags_dev + off, pc->cin, pc->cout, pc->co, NT, pc->kh, dy_rot, ci_off});
        };
        for (const PackedConv* pc : tpc)
            if (pc->bf_off >= 0) add(pc, pc->bf_off, pc->cout / 16, 0, 0);
        for (const PackedConv* pc : tpd)
            if (pc->bf_off >= 0) add(pc, pc->bf_off, (pc->cout + 15) / 16, pc->kh - 1, 0);
        for (const PackedConv* pc : thd)
            if (pc->bf_off >= 0)
                for (int half = 0; half < 2; ++half) add(pc, half ? pc->bf_off2 : pc->bf_off, 1, pc->kh - 1, 16 * half);
        for (size_t j0 = 0; j0 < jobs.size(); j0 += kMaxPackJobs) {
            PcPackJobs js;
            js.n = static_cast<int>(std::min<size_t>(kMaxPackJobs, jobs.size() - j0));
            int max_cout = 1, max_blocks = 1;
            for (int k = 0; k < js.n; ++k) {
                js.j[k] = jobs[j0 + k];
                max_cout = std::max(max_cout, js.j[k].cout);
                max_blocks = std::max(max_blocks, (js.j[k].KH * 4 * js.j[k].NT * 64 + 255) / 256);
            }
            if ((rc = ake::launch_untimed("pc_weight_scale_jobs_kernel", pc_weight_scale_jobs_kernel, dim3(max_cout, js.n), dim3(256), 0, s, js))) return rc;
            if ((rc = ake::launch_untimed("pack_pc_f16x3_jobs_kernel", pack_pc_f16x3_jobs_kernel, dim3(max_blocks, js.n), dim3(256), 0, s, js))) return rc;
        }
        for (size_t j0 = 0; j0 < tfr.size(); j0 += kMaxPackJobs) {
            P2pRawJobs js;
            js.n = static_cast<int>(std::min<size_t>(kMaxPackJobs, tfr.size() - j0));
            for (int k = 0; k < js.n; ++k) {
                const TrainFrag& t = tfr[j0 + k];
                js.j[k] = P2pRawJob{n->blob_dev + t.raw, n->bf_frags_dev + t.pc->bf_off, t.cin, t.cout, t.flip};
            }
            if ((rc = ake::launch_untimed("pack_p2p_f16_raw_jobs_kernel", pack_p2p_f16_raw_jobs_kernel, dim3((14 * 64 + 255) / 256, js.n), dim3(256), 0, s, js)))
                return rc;
        }
    }
    for (size_t i = 1; !train_only && i < n->semi.size(); ++i)
        if (n->semi[i].eval.bf_off >= 0 && (rc = ake::launch_untimed("pack_semi_f16_kernel", pack_semi_f16_kernel, dim3(1), dim3(192), 0, s,
                                                                     n->blob_dev + n->semi[i].eval.w_off, n->bf_frags_dev + n->semi[i].eval.bf_off)))
            return rc;
    if (!train_only)
    for (const PackedConv* pc : h1)
        if (pc->bf_off >= 0 && (rc = ake::launch_untimed("pack_head1_bf16_kernel", pack_head1_bf16_kernel, dim3((head1_ksteps(pc->kh) * 64 + 255) / 256),
                                                         dim3(256), 0, s, n->blob_dev + pc->w_off, n->bf_frags_dev + pc->bf_off, pc->cin, pc->kh)))
            return rc;
    return AKE_OK;
}

}  // namespace

int ake_pcnet_finalize(ake_pcnet* n) {
    AKE_REQUIRE(n, AKE_ERR_INVALID, "finalize: null handle");
    for (size_t i = 0; i < n->specs.size(); ++i)
        AKE_REQUIRE(n->host[i].set, AKE_ERR_STATE, "finalize: missing key '%s' (load_state_dict strict=True)", n->specs[i].name.c_str());
    int rc;
    if (n->map_host.empty()) {
        if ((rc = trace_maps(n))) return rc;
        if ((rc = build_fold_tables(n))) return rc;
    }
    reset_packs(n);
    if ((rc = build_packs(n, false)) || (rc = build_packs(n, true))) return rc;
    n->blob.resize(ake::align_up(n->blob.size() + 64, 64), 0.f);
    AKE_REQUIRE(n->blob.size() == n->map_host.size(), AKE_ERR_STATE, "finalize: blob layout changed between builds");
    if (!n->blob_dev) AKE_HIP_CHECK(hipMalloc(&n->blob_dev, n->blob.size() * sizeof(float)));
    AKE_HIP_CHECK(hipMemcpy(n->blob_dev, n->blob.data(), n->blob.size() * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = rebuild_bf16_frags(n, nullptr))) return rc;
    if (!n->aff_recs.empty()) {   // --denseblock: the tables come from the same kernel as in ake_pcnet_load_from_device_f32, fed a staged copy
        std::vector<float> flat(n->grad_floats);
        for (size_t i = 0; i < n->specs.size(); ++i) std::copy(n->host[i].data.begin(), n->host[i].data.end(), flat.begin() + n->grad_off[i]);
        float* tmp = nullptr;
        AKE_HIP_CHECK(hipMalloc(&tmp, flat.size() * sizeof(float)));
        AKE_HIP_CHECK(hipMemcpy(tmp, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
        rc = rebuild_dense_affine(n, tmp, nullptr);
        AKE_HIP_CHECK(hipStreamSynchronize(nullptr));
        (void)hipFree(tmp);
        if (rc) return rc;
    }
    AKE_HIP_CHECK(hipStreamSynchronize(nullptr));
    n->finalized = true;
    return AKE_OK;
}

// Device-resident parameters: (re)build every packed weight from a flat f32 parameter buffer on the device (layout =
// ake_pcnet_grad_offset).  No host round trip after the first call; asynchronous on `stream`.
namespace {
int load_from_device_impl(ake_pcnet* n, const float* params_dev, ake_stream_t stream, bool train_only) {
    AKE_REQUIRE(n && params_dev, AKE_ERR_INVALID, "load_from_device: null argument");
    if (n->map_host.empty()) {          // first use: learn the layout (values are irrelevant; host tensors only need their sizes)
        for (size_t i = 0; i < n->specs.size(); ++i) {
            size_t cnt = 1;
            for (int d = 0; d < n->specs[i].ndim; ++d) cnt *= static_cast<size_t>(n->specs[i].shape[d]);
            if (n->host[i].data.size() != cnt) n->host[i].data.assign(cnt, 0.f);
        }
        int rc;
        if ((rc = trace_maps(n))) return rc;
        if ((rc = build_fold_tables(n))) return rc;
        if (!n->blob_dev) AKE_HIP_CHECK(hipMalloc(&n->blob_dev, n->blob.size() * sizeof(float)));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = static_cast<int>(n->grad_floats), NB = static_cast<int>(n->map_host.size());
    int rc;
    if ((rc = launch_flat("fold_params_kernel", fold_params_kernel, s, P, params_dev, n->fold_ch_dev, n->fold_bn_dev, n->folded_dev, P))) return rc;
    if ((rc = launch_flat("gather_blob_kernel", gather_blob_kernel, s, NB, params_dev, n->folded_dev, n->map_dev, n->blob_dev, NB))) return rc;
    if ((rc = rebuild_bf16_frags(n, s, train_only))) return rc;
    if ((rc = rebuild_dense_affine(n, params_dev, s))) return rc;
    n->finalized = true;
    return AKE_OK;
}
}  // namespace
int ake_pcnet_load_from_device_f32(ake_pcnet* n, const float* params_dev, ake_stream_t stream) { return load_from_device_impl(n, params_dev, stream, false); }
int ake_pcnet_load_for_training_f32(ake_pcnet* n, const float* params_dev, ake_stream_t stream) { return load_from_device_impl(n, params_dev, stream, true); }

// running_mean / running_var inside the flat parameter buffer <- momentum blend with the batch statistics that
// ake_pcnet_forward_train_f32 returned in bn_stats (torch semantics: unbiased variance; models use momentum 0.1).
int ake_pcnet_update_running_stats_f32(const ake_pcnet* n, const float* bn_stats_dev, float* params_dev, float momentum, ake_stream_t stream) {
    AKE_REQUIRE(n && bn_stats_dev && params_dev, AKE_ERR_INVALID, "update_running_stats: null argument");
    AKE_REQUIRE(n->finalized && n->run_off_dev, AKE_ERR_STATE, "update_running_stats: the handle has no parameters yet");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return ake::launch("running_stats_kernel", running_stats_kernel, dim3((n->bn_channels + 63) / 64), dim3(64), 0, s, bn_stats_dev, n->run_off_dev,
                       params_dev, momentum, n->bn_channels);
}

// The BatchNorm layers whose forward the reference's BACKWARD pass runs a second time (checkpointed halves: every dense layer's norm1,
// models.py:484-489, 553): the same blend once more, with the batch statistics of the forward this backward belongs to.  Returns the number
// of channels it touches through *channels (nullable); a no-op for nets without such layers.
int ake_pcnet_update_recomputed_running_stats_f32(const ake_pcnet* n, const float* bn_stats_dev, float* params_dev, float momentum, int* channels,
                                                  ake_stream_t stream) {
    AKE_REQUIRE(n, AKE_ERR_INVALID, "update_recomputed_running_stats: null handle");
    if (channels) *channels = n->recomputed_bn_channels;
    if (n->recomputed_bn_channels == 0) return AKE_OK;
    AKE_REQUIRE(bn_stats_dev && params_dev, AKE_ERR_INVALID, "update_recomputed_running_stats: null argument");
    AKE_REQUIRE(n->finalized && n->run_off2_dev, AKE_ERR_STATE, "update_recomputed_running_stats: the handle has no parameters yet");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return ake::launch("running_stats_kernel", running_stats_kernel, dim3((n->bn_channels + 63) / 64), dim3(64), 0, s, bn_stats_dev, n->run_off2_dev,
                       params_dev, momentum, n->bn_channels);
}

// BatchNorm layers of the training-mode forward, in forward order (valid after ake_pcnet_create; channel counts only
// need the configuration, names are the reference module paths, e.g. "model.1.p2p.layer.1").
int ake_pcnet_num_bn(const ake_pcnet* n) { return n ? static_cast<int>(n->bns.size()) : 0; }

int ake_pcnet_bn_info(const ake_pcnet* n, int index, const char** name, int* channels, int* channel_offset) {
    AKE_REQUIRE(n && index >= 0 && index < static_cast<int>(n->bns.size()), AKE_ERR_INVALID, "bn_info: index out of range (finalize first)");
    if (name) *name = n->bns[index].name.c_str();
    if (channels) *channels = n->bns[index].C;
    if (channel_offset) *channel_offset = n->bns[index].ch_off;
    return AKE_OK;
}

size_t ake_pcnet_workspace_bytes(const ake_pcnet* n, int batch, int frames) {
    if (!n || batch <= 0 || frames <= 0) return 0;
    Buffers b;
    if (plan_buffers(n, batch, std::min(batch, n->chunk_clips), frames, nullptr, &b) != AKE_OK) return 0;
    return b.bytes;
}

size_t ake_pcnet_train_workspace_bytes(const ake_pcnet* n, int batch, int frames) {
    if (!n || batch <= 0 || frames <= 0) return 0;
    Buffers b;
    if (plan_buffers(n, batch, batch, frames, nullptr, &b, true) != AKE_OK) return 0;   // batch statistics: no chunking
    return b.bytes;
}

#include "pcnet_forward.h"

#include "pcnet_backward.h"

// Flat gradient buffer: float entries of the state_dict in ake_pcnet_tensor_info order (running statistics get zeros).
size_t ake_pcnet_grad_floats(const ake_pcnet* n) { return n ? n->grad_floats : 0; }

int64_t ake_pcnet_grad_offset(const ake_pcnet* n, const char* name) {
    if (!n || !name) return -1;
    auto it = n->spec_index.find(name);
    if (it == n->spec_index.end()) return -1;
    return static_cast<int64_t>(n->grad_off[it->second]);
}

int ake_pcnet_backward_f32(const ake_pcnet* n, const float* mel, int batch, int frames, const int64_t* seq_length, const float* key_out,
                           const float* d_key, const float* d_tonic, const float* d_genre, float* grads_out, int accumulate,
                           void* workspace, size_t ws_bytes, ake_stream_t stream) {
    AKE_REQUIRE(n && mel && key_out && d_key && d_tonic && grads_out, AKE_ERR_INVALID, "pcnet backward: null argument");
    AKE_REQUIRE(n->finalized, AKE_ERR_STATE, "pcnet: ake_pcnet_finalize has not been called");
    AKE_REQUIRE(!n->cfg.genre || d_genre, AKE_ERR_INVALID, "pcnet backward: genre head enabled but d_genre is null");
    AKE_REQUIRE(!(n->cfg.p2pc_conv && n->cfg.stay_sixth), AKE_ERR_UNSUPPORTED, "pcnet: training a --p2pc_conv --stay_sixth net is not built");
    Buffers b;
    int rc = plan_buffers(n, batch, batch, frames, workspace, &b, true);
    if (rc) return rc;
    AKE_REQUIRE(workspace && ws_bytes >= b.bytes, AKE_ERR_WORKSPACE, "pcnet backward: workspace %zu < %zu bytes", ws_bytes, b.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    AKE_HIP_CHECK(hipMemsetAsync(b.gslots, 0, sizeof(gfx_t) * n->grad_floats * kGradSlots, s));
    AKE_HIP_CHECK(hipMemsetAsync(b.stats2, 0, sizeof(double) * (static_cast<size_t>(3) * n->bn_channels * kBwdStatSlots + n->bns.size() * (kAmaxSlots / 2)), s));
    Bwd bw{n, b, s, b.gslots, batch};
    rc = bw.run(mel, seq_length, d_key, d_tonic, d_genre, key_out);
    if (rc) return rc;
    return launch_flat("grad_reduce_kernel", grad_reduce_kernel, s, n->grad_floats, b.gslots, grads_out, static_cast<long long>(n->grad_floats), accumulate ? 1 : 0);
}

int ake_pcnet_local_frames(const ake_pcnet* n, int frames, int* pooled_frames, int* map_frames) {
    AKE_REQUIRE(n && n->cfg.local > 0, AKE_ERR_STATE, "pcnet: the net was not created with local > 0");
    int t = frames;
    for (int i = 1; i < n->cfg.num_layers; ++i) t /= n->cfg.time_pool_size;
    t -= (n->cfg.kernel_size - 1) * n->cfg.head_layers;
    if (map_frames) *map_frames = t;
    if (pooled_frames) *pooled_frames = t - n->cfg.local + 1;
    return AKE_OK;
}

int ake_pcnet_forward_local_f32(const ake_pcnet* n, const float* mel, int batch, int frames, float* key_out, float* tonic_out, float* genre_out,
                                void* workspace, size_t ws_bytes, ake_stream_t stream) {
    AKE_REQUIRE(n && n->cfg.local > 0, AKE_ERR_STATE, "pcnet: the net was not created with local > 0");
    return forward_impl(n, false, mel, batch, frames, nullptr, key_out, tonic_out, genre_out, nullptr, workspace, ws_bytes, stream);
}

int ake_pcnet_forward_f32(const ake_pcnet* n, const float* mel, int batch, int frames, const int64_t* seq_length,
                          float* key_out, float* tonic_out, float* genre_out, void* workspace, size_t ws_bytes,
                          ake_stream_t stream) {
    AKE_REQUIRE(!n || n->cfg.local == 0, AKE_ERR_STATE, "pcnet: a --local net returns per-frame outputs: call ake_pcnet_forward_local_f32");
    return forward_impl(n, false, mel, batch, frames, seq_length, key_out, tonic_out, genre_out, nullptr, workspace, ws_bytes, stream);
}

// mel as the CQT filter bank writes it, [batch][frames][pitches] (ake_cqt_logmag_frames_major_f32): the two kernels that read the CQT
// (layer 0 and the first pitch convolution) transpose while they stage it, so the [batch][pitches][frames] tensor of the
// reference's interface -- a 48 MB round trip per 256 clips -- is never written.  Taken by the default architecture on the fused
// inference path only: ask ake_pcnet_accepts_frames_major first (other configurations return AKE_ERR_UNSUPPORTED).
int ake_pcnet_accepts_frames_major(const ake_pcnet* n, int batch, int frames) {
    if (!n || !n->finalized || batch <= 0 || frames <= 0) return 0;
    return build_route(n, false, batch, std::min(batch, n->chunk_clips), frames, nullptr, nullptr, true).frames_major ? 1 : 0;
}

int ake_pcnet_forward_frames_major_f32(const ake_pcnet* n, const float* mel_fm, int batch, int frames, const int64_t* seq_length,
                                       float* key_out, float* tonic_out, float* genre_out, void* workspace, size_t ws_bytes,
                                       ake_stream_t stream) {
    AKE_REQUIRE(!n || n->cfg.local == 0, AKE_ERR_UNSUPPORTED, "pcnet: a --local net does not take the frames-major input");
    return forward_impl(n, false, mel_fm, batch, frames, seq_length, key_out, tonic_out, genre_out, nullptr, workspace, ws_bytes, stream, true);
}

int ake_pcnet_forward_train_f32(const ake_pcnet* n, const float* mel, int batch, int frames, const int64_t* seq_length,
                                float* key_out, float* tonic_out, float* genre_out, float* bn_stats_out, void* workspace,
                                size_t ws_bytes, ake_stream_t stream) {
    AKE_REQUIRE(!n || !(n->cfg.p2pc_conv && n->cfg.stay_sixth), AKE_ERR_UNSUPPORTED, "pcnet: training a --p2pc_conv --stay_sixth net is not built (inference only)");
    return forward_impl(n, true, mel, batch, frames, seq_length, key_out, tonic_out, genre_out, bn_stats_out, workspace, ws_bytes, stream);
}

// ---- debug taps ---------------------------------------------------------------------------
// train:raw/<bn prefix> and train:aff/<bn prefix> (default architecture family): the raw convolution output z that the BatchNorm
// normalises, [B][C][H][T], and its [C][3] = (scale, shift, negative slope) table as the forward left it -- exactly the (z, aff) pair that
// Bwd::run hands to affine_act for that site, so a caller can restate every LeakyReLU sign / max-pool winner the backward pass re-derives.
// *clip_stride (floats) differs from C * H * T where the tensor is a channel slice of a wider buffer.
static int train_site_lookup(const ake_pcnet* n, const Buffers& b, const std::string& t, int batch, float** p, int64_t shape[4], long long* clip_stride) {
    const auto& c = n->cfg;
    const bool want_aff = t.compare(0, 4, "aff/") == 0;
    std::string site = t.substr(4);
    if (!site.empty() && site.back() == '.') site.pop_back();
    AKE_REQUIRE(!c.resblock && !c.denseblock && !c.p2pc_conv && !c.stay_sixth && !c.pc2p_mem && c.local == 0, AKE_ERR_INVALID,
                "tap: 'train:%s': the raw / table taps cover the default architecture family only", t.c_str());
    AKE_REQUIRE(n->finalized, AKE_ERR_STATE, "tap: 'train:%s': ake_pcnet_finalize has not been called", t.c_str());
    const int L = c.num_layers, P = c.pitches;
    float *z = nullptr, *aff = nullptr;
    int64_t C = 0, H = 0, Tn = 0;
    long long stride = 0;
    bool hit = false;            // (the pointers are null in the dry run of ake_pcnet_tap_info)
    auto found = [&](Slot t_, int64_t C_, int64_t H_, int64_t T_, long long stride_ = 0) { z = t_.p; aff = t_.aff; C = C_; H = H_; Tn = T_; stride = stride_; hit = true; };
    auto is = [&](const ConvSite& cs) { return !hit && cs.bn >= 0 && site == n->bns[cs.bn].name; };      // the sites know their BatchNorm's name
    for (int i = 0; i < L; ++i) {
        const LayerDims& d = n->dims[i];
        const int Ti = b.Tl[i];
        if (is(n->semi[i])) found(Slot{b.semi_raw[i], b.aff_semi[i]}, i == 0 ? 1 : d.out_p, P / 3, Ti);
        if (is(n->up[i])) found(Slot{b.psix[i], b.aff_p2pin[i] ? b.aff_p2pin[i] + 3 * d.prev_p : nullptr}, d.prev_pc, 36, Ti);
        for (int j = 0; j < static_cast<int>(n->p2p[i].size()); ++j)
            if (is(n->p2p[i][j])) found(b.p_out(true, i, j), d.out_p, P, Ti);
        for (int j = 0; j < static_cast<int>(n->pc2pc[i].size()); ++j)
            if (is(n->pc2pc[i][j])) {
                // layer 0's last convolution of a deeper net writes channels [0, n_filters) of layer 1's concat buffer (table: aff_cat[1])
                if (i == 0 && L > 1 && j == c.conv_layers - 1) {
                    found(b.cat_slot(true, 1), c.n_filters, 12, Ti, static_cast<long long>(b.cat_ch(1)) * 12 * Ti);
                } else found(b.pc_out(true, i, j), i == 0 ? c.n_filters : d.out_pc, 12, Ti);
            }
    }
    for (int h = 0; h < 3; ++h)
        for (int j = 0; j < static_cast<int>(n->heads[h].convs.size()); ++j)
            if (is(n->heads[h].convs[j])) found(b.head_out(true, h, j, false), n->heads[h].convs[j].train.cout, 12, b.Tf - (j + 1) * (c.kernel_size - 1));
    AKE_REQUIRE(hit && Tn >= 1, AKE_ERR_INVALID, "tap: 'train:%s' names no BatchNorm of this net", t.c_str());
    if (want_aff) { *p = aff; shape[0] = C; shape[1] = 3; shape[2] = 1; shape[3] = 1; }
    else { *p = z; shape[0] = batch; shape[1] = C; shape[2] = H; shape[3] = Tn; if (clip_stride) *clip_stride = stride; }
    return AKE_OK;
}

static int tap_lookup(const ake_pcnet* n, const char* name, int batch, int frames, const void* ws, float** p, int64_t shape[4],
                      int* channels_last = nullptr, long long* clip_stride = nullptr) {
    if (channels_last) *channels_last = 0;
    if (clip_stride) *clip_stride = 0;
    AKE_REQUIRE(n && name, AKE_ERR_INVALID, "tap: null argument");
    AKE_REQUIRE(batch <= n->chunk_clips, AKE_ERR_INVALID, "tap: batch %d exceeds the chunk size %d", batch, n->chunk_clips);
    Buffers b;
    const bool tr = std::strncmp(name, "train:", 6) == 0;      // buffers of the training-mode workspace (debugging the backward pass)
    int rc = plan_buffers(n, batch, batch, frames, const_cast<void*>(ws), &b, tr);
    if (rc) return rc;
    const auto& c = n->cfg;
    if (tr) {
        const std::string t = name + 6;
        if (t.compare(0, 4, "raw/") == 0 || t.compare(0, 4, "aff/") == 0) return train_site_lookup(n, b, t, batch, p, shape, clip_stride);
        const int L1 = c.num_layers - 1;
        const LayerDims& dd = n->dims[L1];
        *p = nullptr;
        shape[0] = batch; shape[1] = 0;
        if (t == "g_p") { *p = b.g_p[L1]; shape[1] = dd.out_p; shape[2] = c.pitches; shape[3] = b.Tl[L1]; }
        if (t == "g_semi") { *p = b.g_semi[L1]; shape[1] = dd.out_p; shape[2] = c.pitches / 3; shape[3] = b.Tl[L1]; }
        if (t == "g_cat") { *p = b.g_cat[L1]; shape[1] = dd.prev_pc + dd.out_p; shape[2] = 12; shape[3] = b.Tl[L1]; }
        if (t == "g_pin") { *p = b.g_pin[L1]; shape[1] = dd.prev_pc + dd.prev_p; shape[2] = c.pitches; shape[3] = b.Tl[L1]; }
        if (t == "z_p_last") { *p = b.pst[L1].back(); shape[1] = dd.out_p; shape[2] = c.pitches; shape[3] = b.Tl[L1]; }
        AKE_REQUIRE(shape[1] > 0, AKE_ERR_INVALID, "tap: unknown training buffer '%s'", name);
        return AKE_OK;
    }
    const int L = c.num_layers, P = c.pitches;
    const std::string nm = name;
    // what a forward of this shape launches under the current ake_debug_keep_taps setting: which activations exist, and in which layout
    const Route r = build_route(n, false, batch, batch, frames, nullptr, ws, false);
    auto set = [&](float* ptr, int64_t C, int64_t H, int64_t Tn) { *p = ptr; shape[0] = batch; shape[1] = C; shape[2] = H; shape[3] = Tn; return AKE_OK; };
    if (nm == "model.0.pool") return set(b.fold0, 1, 12, frames);
    if (c.resblock && (std::strstr(name, "pc2pc.layer.") || std::strstr(name, "p2p.layer."))) {
        ake::set_error("tap: '%s': the stacks of a --resblock net are not tapped", name);
        return AKE_ERR_INVALID;
    }
    for (int i = 0; i < L; ++i) {
        const std::string m = "model." + std::to_string(i) + ".";
        const LayerDims& d = n->dims[i];
        const int Ti = b.Tl[i];
        const int last_j = c.conv_layers - 1;
        for (int j = 0; j < c.conv_layers; ++j) {
            // ping-pong buffers: only the last two outputs of a stack are still in memory after the forward
            if (nm == m + "pc2pc.layer." + std::to_string(3 * j + 2)) {
                const bool to_cat = i == 0 && L > 1;             // layer 0's last conv writes into cat[1]
                if (to_cat && j == last_j) break;                // strided inside the concat buffer: use "model.1.cat"
                if (j < last_j - (to_cat ? 2 : 1)) break;
                if (i == L - 1 && r.pc == PcStack::Fused) {
                    ake::set_error("tap: '%s' stays in LDS (the stack runs as one launch); ake_debug_keep_taps(1) before the forward keeps it", name);
                    return AKE_ERR_INVALID;
                }
                if (j < last_j && i == L - 1 && r.pc == PcStack::Bf16 && channels_last) *channels_last = 1;
                if (i == 0 && r.l0.form == L0Form::FusedMfma && !g_keep_taps) {      // (the VALU form writes every conv's output)
                    ake::set_error("tap: '%s' stays in LDS (layer 0 runs as one launch); ake_debug_keep_taps(1) before the forward writes it", name);
                    return AKE_ERR_INVALID;
                }
                return set(b.pc_out(false, i, j).p, i == 0 ? c.n_filters : d.out_pc, 12, Ti);
            }
            if (i >= 1 && nm == m + "p2p.layer." + std::to_string(3 * j + 2)) {
                if (j < last_j - 1) break;
                if (j == last_j && r.p[i].stack == PStack::F16 && r.p[i].k[0].last.out != P2pOut::Nchw) {
                    ake::set_error("tap: '%s' is fused with the semitone conv that follows it (never written); ake_debug_keep_taps(1) before the forward keeps it", name);
                    return AKE_ERR_INVALID;
                }
                // inference keeps the stack's intermediate activations as channels-last split-bf16 planes (conv_p2p_f16_kernel)
                if (j < last_j && r.p[i].stack == PStack::F16 && channels_last) *channels_last = 2;      // one f16 plane
                return set(b.p_out(false, i, j).p, d.out_p, P, Ti);
            }
        }
        if (i >= 1 && nm == m + "up_sixth_a") {
            if (i == 1 && r.psix_f16) {
                ake::set_error("tap: '%s' is held as f16 words for the pitch conv that reads it; ake_debug_keep_taps(1) before the forward writes it as f32", name);
                return AKE_ERR_INVALID;
            }
            return set(b.psix[i], d.prev_pc, 36, Ti);
        }
        if (i >= 1 && nm == m + "cat") return set(b.cat[i], d.prev_pc + d.out_p, 12, Ti);
        if (i == L - 1 && i >= 1 && nm == m + "time_pool_pc") return set(b.pcf, d.out_pc, 12, b.Tf);
    }
    const int Tm = b.Tf - (c.kernel_size - 1) * c.head_layers;
    if (nm == "key_map") return set(b.map_k, 1, 12, Tm);
    if (nm == "tonic_map") return set(b.map_t, 1, 12, Tm);
    if (nm == "genre_map" && c.genre) return set(b.map_g, 1, 11, Tm);
    ake::set_error("tap: '%s' is not a materialised activation", name);
    return AKE_ERR_INVALID;
}

int ake_debug_keep_taps(int on) {
    const int old = g_keep_taps;
    g_keep_taps = on != 0;
    return old;
}

int ake_pcnet_tap_info(const ake_pcnet* n, const char* name, int batch, int frames, int64_t shape[4]) {
    float* p = nullptr;
    return tap_lookup(n, name, batch, frames, nullptr, &p, shape);
}

int ake_pcnet_tap_copy(const ake_pcnet* n, const char* name, int batch, int frames, const void* workspace, float* out_dev,
                       ake_stream_t stream) {
    AKE_REQUIRE(workspace && out_dev, AKE_ERR_INVALID, "tap_copy: null argument");
    float* p = nullptr;
    int64_t shape[4];
    int cl = 0;
    long long clip_stride = 0;
    int rc = tap_lookup(n, name, batch, frames, workspace, &p, shape, &cl, &clip_stride);
    if (rc) return rc;
    if (clip_stride) {   // a channel slice of a wider buffer: one row per clip
        const size_t row = sizeof(float) * shape[1] * shape[2] * shape[3];
        AKE_HIP_CHECK(hipMemcpy2DAsync(out_dev, row, p, sizeof(float) * clip_stride, row, shape[0], hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
        return AKE_OK;
    }
    if (cl) {
        const long long total = shape[0] * shape[1] * shape[2] * shape[3];
        const unsigned short* h = reinterpret_cast<const unsigned short*>(p);
        return ake::launch_untimed("cl_to_nchw_kernel", cl_to_nchw_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0,
                                   static_cast<hipStream_t>(stream), h, cl == 2 ? nullptr : h + total, out_dev, shape[1], shape[2], shape[3], total);
    }
    AKE_HIP_CHECK(hipMemcpyAsync(out_dev, p, sizeof(float) * shape[0] * shape[1] * shape[2] * shape[3], hipMemcpyDeviceToDevice,
                                 static_cast<hipStream_t>(stream)));
    return AKE_OK;
}

}  // extern "C"
