// The workspace carve (Buffers, plan_buffers) and the route of one forward call (Route, build_route) (implementation include of pcnet.hip; lives in its translation unit).
#pragma once

namespace {

// A tensor and the pending BatchNorm + LeakyReLU table its readers apply while loading (null: the tensor is final), see Fwd
struct Slot {
    float* p = nullptr;
    float* aff = nullptr;
};

struct Buffers {           // workspace carve
    // per chunk (pitch stream): everything up to the last layer's semitone fold
    float* fold0 = nullptr;
    unsigned int* melh = nullptr;   // inference: the log-CQT as f16 hi | lo words, [batch][P][T] (layer0_mfma_kernel -> conv_p2p_f16_ps_kernel<1, 3>)
    float* smap = nullptr;     // --p2pc_conv only
    float* p0 = nullptr;       // --stay_sixth only
    std::vector<float*> pcd;   // --stay_sixth only
    std::vector<float*> cat, psix, pa, pb, pca, pcb, ppool, pin;
    // whole batch (pitch-class tail): last layer's concat buffer, its pc stack, pooled features, heads
    float *pcf = nullptr, *hid_k = nullptr, *hid_t = nullptr, *hid_g = nullptr;
    float *map_k = nullptr, *map_t = nullptr, *map_g = nullptr;
    size_t hid_half = 0;    // floats of one of the two maps a head's hid_* buffer holds
    std::vector<int> Tl;    // frames at layer i
    int Tf = 0;             // frames after the last layer
    size_t bytes = 0;
    // training-mode forward only: BatchNorm statistics, raw semitone-conv outputs and the pending-affine table
    // ([C][3] = scale, shift, negative slope) of every buffer that can hold a raw (pre-BatchNorm) tensor
    double* stats = nullptr;           // [kStatSlots][bn_channels][2]
    float* bstats = nullptr;           // [bn_channels][3] batch mean, biased variance, element count
    std::vector<float*> semi_raw, aff_semi, aff_cat, aff_p2pin;
    std::vector<float*> foldc_raw, aff_foldc, g_foldc;                // --p2pc_conv training: raw fold-conv output [B][C][12][T], pool.bn's table, its gradient
    // every convolution keeps its own raw output in training mode (the backward pass needs all of them)
    std::vector<std::vector<float*>> pst, aff_pst, pcst, aff_pcst;   // [layer][conv]
    std::vector<float*> hst[3], aff_hst[3];                            // [head][hidden conv]
    // backward
    double* stats2 = nullptr;          // [bn_channels][3]  (sum g1, sum g1*zhat, sum (z - mean)); then one 8-byte cell per BatchNorm layer: the bits of max |dz| (dz_amax)
    gfx_t* gslots = nullptr;           // [kGradSlots][grad_floats] partial weight gradients (backward), 64-bit fixed point
    float* wg_partial = nullptr;       // per-workgroup partial weight gradients of one convolution (conv_wgrad_kernel), reduced in order
    size_t wg_partial_floats = 0;
    unsigned short* feat_cl = nullptr; // [2 planes][B][12][Tf][16]
    float* coef = nullptr;             // [bn_channels][4]  (c0, c1, c2, mean)
    float* g_map[3] = {nullptr, nullptr, nullptr};
    float *g_hid = nullptr, *g_pcf = nullptr, *g_fold0 = nullptr;
    std::vector<float*> g_pc, g_cat, g_semi, g_p, g_pin, g_psix;      // per layer (g_pc / g_p: ping-pong pair packed as 2x)
    // --denseblock training, per block kind (0: the layers' pitch blocks, 1: their pitch-class blocks) and [layer][dense layer]: the bottleneck
    // map (kept for the backward pass) and the two on-load tables (norm1 over the block's features so far, norm2 over the bottleneck map);
    // one gradient buffer of the kind's widest bottleneck
    struct DenseBufs { std::vector<std::vector<float*>> bott, aff1, aff2; float* gbott = nullptr; } dn[2];
    const ake_pcnet* n = nullptr;      // the net this carve is for

    // Layer i's concat buffer [clip][cat_ch][12][Tl[i]] (pitch classes of the layer below | folded semitone maps | --denseblock: the block's
    // growth) and up_sixth map: the part of a chunk that starts at clip c0 -- those of layer 1 and the concat buffer of the last layer hold the
    // whole batch, the others one chunk
    int cat_ch(int i) const { return n->dims[i].prev_pc + n->dims[i].out_p + (n->cfg.denseblock ? n->cfg.n_filters * n->cfg.conv_layers : 0); }
    float* cat_at(int i, int c0) const { return cat[i] + (i == 1 || i == n->cfg.num_layers - 1 ? static_cast<size_t>(c0) * cat_ch(i) * 12 * Tl[i] : 0); }
    float* psix_at(int i, int c0) const { return psix[i] + (i == 1 ? static_cast<size_t>(c0) * n->dims[i].prev_pc * 36 * Tl[i] : 0); }

    // Where conv j of a stack writes: training keeps every raw output next to its table (the backward pass reads all of them), inference
    // ping-pongs between two buffers of final activations.  p_out: layer i's pitch stack, pc_out: its pitch-class stack, head_out: head
    // h (key, tonic, genre), whose last conv writes the head's map (no BatchNorm); cat_slot: layer i's concat buffer.
    Slot p_out(bool train, int i, int j) const { return train ? Slot{pst[i][j], aff_pst[i][j]} : Slot{(j & 1) ? pb[i] : pa[i], nullptr}; }
    Slot pc_out(bool train, int i, int j) const { return train ? Slot{pcst[i][j], aff_pcst[i][j]} : Slot{(j & 1) ? pcb[i] : pca[i], nullptr}; }
    Slot head_out(bool train, int h, int j, bool last) const {
        float* const hid[3] = {hid_k, hid_t, hid_g};
        float* const map[3] = {map_k, map_t, map_g};
        if (last) return Slot{map[h], nullptr};
        return train ? Slot{hst[h][j], aff_hst[h][j]} : Slot{hid[h] + (j & 1) * hid_half, nullptr};
    }
    Slot cat_slot(bool train, int i) const { return Slot{cat[i], train ? aff_cat[i] : nullptr}; }
    // training: what layer i's pitch / pitch-class stack leaves (the last conv's raw output, or a --resblock stack's last block output)
    Slot p_last(int i) const { return Slot{pst[i].back(), aff_pst[i].back()}; }
    Slot pc_last(int i) const { return Slot{pcst[i].back(), aff_pcst[i].back()}; }
};

// frames at every layer (layers 0 and 1 see the clip as it is, each later one the pooled frames of the layer below) and behind the last one
void layer_frames(const ake_pcnet_config& c, int frames, int* Tl, int* Tf) {
    for (int i = 0; i < c.num_layers; ++i) Tl[i] = i < 2 ? frames : Tl[i - 1] / c.time_pool_size;
    *Tf = c.num_layers > 1 ? Tl[c.num_layers - 1] / c.time_pool_size : frames;
}

// chunk = clips per pitch-stream pass, batch = clips of the call (tail buffers)
int plan_buffers(const ake_pcnet* n, int batch, int chunk, int frames, void* ws, Buffers* b, bool train = false) {
    const auto& c = n->cfg;
    const int L = c.num_layers, P = c.pitches;
    ake::Carver cv(ws, 0);
    b->n = n;
    b->Tl.resize(L);
    layer_frames(c, frames, b->Tl.data(), &b->Tf);
    AKE_REQUIRE(b->Tf >= 1, AKE_ERR_INVALID, "pcnet: %d frames vanish under the time pooling", frames);
    b->cat.assign(L + 1, nullptr); b->psix.assign(L, nullptr); b->pa.assign(L, nullptr); b->pb.assign(L, nullptr);
    b->pca.assign(L, nullptr); b->pcb.assign(L, nullptr); b->ppool.assign(L, nullptr); b->pin.assign(L, nullptr);
    const size_t C = chunk, B = batch;
    const size_t dg = c.denseblock ? static_cast<size_t>(c.n_filters) * c.conv_layers : 0;   // channels a dense block appends in place
    b->fold0 = cv.take<float>(B * (L == 1 ? 1 + dg : 1) * 12 * frames);
    if (!train && L > 1) b->melh = cv.take<unsigned int>(B * P * frames);
    if (c.stay_sixth) {  // --stay_sixth: layer 0's activated semitone map is the pitch stream; dense copies of the pitch-class stream for the repeat
        b->p0 = cv.take<float>(B * (P / 3) * frames);
        b->pcd.assign(L, nullptr);
        for (int i = 1; i < L; ++i) b->pcd[i] = cv.take<float>(C * n->dims[i].prev_pc * 12 * b->Tl[i]);
    }
    if (c.p2pc_conv) {   // --p2pc_conv: raw semitone maps between the semitone conv and the octave-fold conv (largest layer)
        size_t m = B * (P / 3) * frames;
        for (int i = 1; i < L; ++i) m = std::max(m, C * n->dims[i].out_p * (P / 3) * b->Tl[i]);
        b->smap = cv.take<float>(m);
    }
    for (int i = 0; i < L; ++i) {
        const int Ti = b->Tl[i];
        const auto& d = n->dims[i];
        const bool last = i == L - 1;
        const int pc_out = i == 0 ? c.n_filters : d.out_pc;
        if (i >= 1) {
            b->cat[i] = cv.take<float>((last || i == 1 ? B : C) * b->cat_ch(i) * 12 * Ti);
            b->psix[i] = cv.take<float>((i == 1 ? B : C) * d.prev_pc * 36 * Ti);
            if (c.pc2p_mem) b->pin[i] = cv.take<float>(C * d.prev_p * P * Ti);             // --pc2p_mem: pitch stream + summed up_sixth map
            b->pa[i] = cv.take<float>(C * d.out_p * P * Ti);
            b->pb[i] = cv.take<float>((c.resblock ? 2 : 1) * C * (c.denseblock ? static_cast<size_t>((d.prev_pc + d.prev_p) / 2) * c.n_filters : d.out_p) * P * Ti);   // --resblock: the blocks' 2C-channel hidden map; --denseblock: the bottleneck map
            if (!last) b->ppool[i] = cv.take<float>(C * d.out_p * P * (Ti / c.time_pool_size));
        }
        const size_t pca_ch = (c.denseblock && i >= 1) ? static_cast<size_t>((d.out_p + d.prev_pc) / 2) * c.n_filters : pc_out;   // --denseblock: bottleneck
        b->pca[i] = cv.take<float>((last || i == 0 ? B : C) * pca_ch * 12 * Ti);
        b->pcb[i] = cv.take<float>((c.resblock ? 2 : 1) * (last || i == 0 ? B : C) * pc_out * 12 * Ti);
    }
    b->pcf = cv.take<float>(B * n->final_ch * 12 * b->Tf);
    const size_t hid = B * 2 * n->final_ch * 12 * b->Tf;
    b->hid_half = hid;
    b->hid_k = cv.take<float>(2 * hid); b->hid_t = cv.take<float>(2 * hid);
    b->feat_cl = cv.take<unsigned short>(B * 12 * b->Tf * 16 * 2);     // channels-last split copy of the head input (bf16 head convs)
    b->map_k = cv.take<float>(B * 12 * b->Tf); b->map_t = cv.take<float>(B * 12 * b->Tf);
    if (c.genre) { b->hid_g = cv.take<float>(2 * hid); b->map_g = cv.take<float>(B * 12 * b->Tf); }
    if (train) {
        b->stats = cv.take<double>(static_cast<size_t>(n->bn_channels) * 2 * kStatSlots);
        b->stats2 = cv.take<double>(static_cast<size_t>(n->bn_channels) * 3 * kBwdStatSlots + n->bns.size() * (kAmaxSlots / 2));       // [slot][bn_channels][3], then [bn layer][kAmaxSlots] unsigned: partial maxima of |dz| (float bits)
        b->gslots = cv.take<gfx_t>(static_cast<size_t>(kGradSlots) * n->grad_floats);
        b->wg_partial_floats = static_cast<size_t>(B) * 98304;                         // 384 KB per clip: e.g. two workgroups per clip x the 43 K weights of a head conv
        b->wg_partial = cv.take<float>(b->wg_partial_floats);
        b->bstats = cv.take<float>(static_cast<size_t>(n->bn_channels) * 3);
        b->coef = cv.take<float>(static_cast<size_t>(n->bn_channels) * 4);
        for (auto* v : {&b->semi_raw, &b->aff_semi, &b->aff_cat, &b->aff_p2pin, &b->g_pc, &b->g_cat, &b->g_semi, &b->g_p, &b->g_pin, &b->g_psix,
                        &b->foldc_raw, &b->aff_foldc, &b->g_foldc})
            v->assign(L + 1, nullptr);
        b->pst.assign(L, {}); b->aff_pst.assign(L, {}); b->pcst.assign(L, {}); b->aff_pcst.assign(L, {});
        for (int i = 0; i < L; ++i) {
            const auto& d = n->dims[i];
            const int Ti = b->Tl[i];
            const int cs = i == 0 ? 1 : d.out_p, pc_out = i == 0 ? c.n_filters : d.out_pc;
            b->semi_raw[i] = cv.take<float>(B * cs * (P / 3) * Ti);
            b->g_semi[i] = cv.take<float>(B * cs * (P / 3) * Ti);
            if (c.p2pc_conv) {
                b->foldc_raw[i] = cv.take<float>(B * cs * 12 * Ti);
                b->g_foldc[i] = cv.take<float>(B * cs * 12 * Ti);
                b->aff_foldc[i] = cv.take<float>(3 * cs);
            }
            b->aff_semi[i] = cv.take<float>(3 * cs);
            // --resblock: [conv0, (conv1 (2C), conv2, block output) per block] (res_stack_train); gradients: g, skip copy, 2C hidden map
            const int n_st = c.denseblock ? 0 : (c.resblock ? 1 + 3 * c.conv_layers : c.conv_layers);
            auto width = [&](int j) { return c.resblock && j % 3 == 1 ? 2 : 1; };
            for (int j = 0; j < n_st; ++j) {
                b->pcst[i].push_back(cv.take<float>(width(j) * B * pc_out * 12 * Ti));
                b->aff_pcst[i].push_back(cv.take<float>(3 * width(j) * pc_out));
            }
            b->g_pc[i] = cv.take<float>((c.resblock ? 4 : 2) * B * (c.denseblock && i == 0 ? 1 + dg : pc_out) * 12 * Ti);   // (--denseblock, one layer: dL/d(fold | growth))
            if (i >= 1) {
                b->aff_cat[i] = cv.take<float>(3 * (d.prev_pc + d.out_p));
                b->aff_p2pin[i] = cv.take<float>(3 * (d.prev_pc + d.prev_p));
                b->g_cat[i] = cv.take<float>(B * b->cat_ch(i) * 12 * Ti);
                for (int j = 0; j < n_st; ++j) {
                    b->pst[i].push_back(cv.take<float>(width(j) * B * d.out_p * P * Ti));
                    b->aff_pst[i].push_back(cv.take<float>(3 * width(j) * d.out_p));
                }
                b->g_p[i] = cv.take<float>((c.resblock ? 4 : 2) * B * d.out_p * P * Ti);
                b->g_pin[i] = cv.take<float>(B * (d.prev_p + d.prev_pc) * P * Ti);
                b->g_psix[i] = cv.take<float>(B * d.prev_pc * 36 * Ti);
            }
        }
        if (c.denseblock) {
            size_t widest[2] = {0, 0};
            for (Buffers::DenseBufs& dn : b->dn) { dn.bott.assign(L, {}); dn.aff1.assign(L, {}); dn.aff2.assign(L, {}); }
            for (int i = 0; i < L; ++i)
                for (int kind : {1, 0})      // a layer's pitch-class block first: the order of the carve is the workspace layout
                    for (const DensePack& dp : kind ? n->dense_pc[i] : n->dense_p[i]) {
                        if (kind == 0 && i < 1) break;      // layer 0 has no pitch block
                        Buffers::DenseBufs& dn = b->dn[kind];
                        const size_t map = B * dp.c1.cout * (kind ? 12 : P) * b->Tl[i];
                        dn.bott[i].push_back(cv.take<float>(map));
                        dn.aff1[i].push_back(cv.take<float>(3 * static_cast<size_t>(dp.c1.cin)));
                        dn.aff2[i].push_back(cv.take<float>(3 * static_cast<size_t>(dp.c1.cout)));
                        widest[kind] = std::max(widest[kind], map);
                    }
            for (int kind : {1, 0}) b->dn[kind].gbott = cv.take<float>(widest[kind]);
        }
        b->g_fold0 = cv.take<float>(B * 12 * frames);
        b->g_pcf = cv.take<float>(B * n->final_ch * 12 * b->Tf);
        b->g_hid = cv.take<float>(hid);
        for (int h = 0; h < 3; ++h) {
            if (h == 2 && !c.genre) break;
            for (int j = 0; j + 1 < c.head_layers; ++j) {
                b->hst[h].push_back(cv.take<float>(hid));
                b->aff_hst[h].push_back(cv.take<float>(3 * 2 * n->final_ch));
            }
            b->g_map[h] = cv.take<float>(B * 12 * b->Tf);
        }
    }
    b->bytes = ake::align_up(cv.off, 256);
    return AKE_OK;
}

// ---- the route: which kernel form every stage of one forward call launches -------------------------------------------------------
// Decided once per call by build_route() from the handle, the mode, the shape, the two alignments that are conditions and
// ake_debug_keep_taps; plain data, no allocation.  Fwd launches what it says, ake_pcnet_accepts_frames_major returns its flag and the
// debug taps answer from it, so none of them can disagree about what was written where.  It does not touch the workspace layout
// (plan_buffers knows nothing of it).
enum class L0Form : unsigned char { Generic, FusedValu, FusedMfma };       // layer 0 + layer 1's up_sixth: per-stage kernels | layer0_fused_kernel | layer0_mfma_kernel
enum class PStack : unsigned char { Generic, F16x3, F16 };                 // a layer's pitch convs: conv_mfma_kernel | conv_p2p_f16x3_kernel where `x3_convs` says | the f16 kernels
enum class PcStack : unsigned char { Generic, F16x3, Bf16, Fused };        // the last pitch-class stack: conv_mfma_kernel | conv_pc_f16x3 where `pc_x3_convs` says | conv_pc_bf16_kernel | pc2pc_fused_kernel
enum class HeadForm : unsigned char { Generic, Bf16First, Head1, Fused };  // key / tonic heads: conv_mfma_kernel | bf16 first conv | + conv_head1_bf16_kernel | heads_fused_kernel

struct Layer0Plan {
    L0Form form = L0Form::Generic;
    int RP = 0, RPp = 0;
    size_t lds = 0;
    // FusedMfma: where float (bin r, frame t) of the clip's CQT sits in the LDS image (Layer0Args::img_*).  A frames-major clip is stored
    // tiled, [frame quad][bin & 3][bin >> 2][frame & 3]: its loader's 16-byte stores (a thread's 4 frames of one bin, adjacent lanes 4 bins
    // apart) then lie side by side, and a frame quad's pitch of 4 (mod 32) floats keeps the semitone phase's frame-wise reads on 32 banks
    bool tiled = false;
    int img_sq = 0, img_sb = 0, img_sr = 0;
    // FusedMfma: the convs >= 1 find their weight fragments in two LDS regions laid over the dead image (else, where the maps leave no room
    // for them -- few bins, many frames -- every conv fetches its own from global memory at its start)
    bool frag_lds = false;
};

struct Route {
    bool frames_major = false;       // the call was asked to read mel frames-major and every reader of mel takes it
    Layer0Plan l0;
    bool psix_f16 = false;           // layer 0 leaves layer 1's up_sixth map as f16 x 4 words in psix[1] (and the CQT in melh) for conv_p2p_f16_ps_kernel<1, 3>
    int chunk_clips[2] = {0, 0};     // clips of a full pitch_chunk call and of the remainder call (0: none); `k` below indexes them
    struct Pitch {                   // layers >= 1
        PStack stack = PStack::Generic;
        unsigned x3_convs = 0;       // F16x3: bit j = conv j runs on conv_p2p_f16x3_kernel
        struct PerChunk {
            P2pPsPlan first, mid, last;   // F16: the persistent form of the first / an inner / the last conv (!ok: the tiled conv_p2p_f16_kernel);
                                          // last.out: plain (Nchw), semitone conv fused (Semi), semitone conv and fold fused (SemiFold)
            P2pStackPlan stack;           // F16, ok: the whole stack is ONE launch of p2p_stack_kernel, and first / mid / last launch nothing
            P2pX3Plan x3[2];              // F16x3: geometry of conv 0 and of the later convs
        } k[2];
    } p[4];
    PcStack pc = PcStack::Generic;
    unsigned pc_x3_convs = 0;
    HeadForm heads = HeadForm::Generic;
    bool genre_bf = false;           // Head1 / Fused: the genre head rides in the same launches
    bool heads_pool = false;         // Head1 / Fused: the masked mean + sigmoid ride in the launch
    int heads_mt = 0;                // Fused: M-tiles per wave of phase A (heads_fused_kernel<MT>)
    int T1 = 0, T2 = 0, TpB = 0;     // Head1 / Fused: frames after each head conv, phase B's patch pitch
    size_t hf_lds = 0;               // Fused

    int chunk_kind(int B) const { return B == chunk_clips[0] ? 0 : 1; }
};

// layer 0 as one launch per clip (default family, inference): which form fits, and its LDS geometry
constexpr size_t kL0MaxLds = 160 * 1024;      // layer0_mfma_kernel's dynamic LDS limit (at the rule's edge, T = 86 frames-major, it takes 152.6 KiB)
Layer0Plan layer0_plan(const ake_pcnet* n, int T0, bool mel16, bool mel_fm) {
    const auto& c = n->cfg;
    const int P = c.pitches, NF = c.n_filters;
    Layer0Plan g;
    if (c.num_layers < 2 || c.resblock || c.denseblock || c.p2pc_conv || c.stay_sixth || NF < 2 || NF > 4 || c.conv_layers < 1 || c.conv_layers > 4 || c.kernel_size != 7 || P % 36 || T0 < 1) return g;
    const PackedConv& sp = n->semi[0].eval;
    if (sp.cin != 1 || sp.co != 1) return g;
    bool mfma = c.precision == AKE_PRECISION_MIXED;      // (the MFMA form multiplies f16 x f16; f32x3: the exact-f32 VALU form)
    for (int j = 0; j < c.conv_layers; ++j) {
        const PackedConv& pc = n->pc2pc[0][j].eval;
        if (pc.co != 4 || pc.groups != 1 || pc.kh != 12 || pc.kw != 7 || pc.cout != NF || pc.cin != (j == 0 ? 1 : NF)) return g;
        mfma = mfma && pc.l0_off >= 0;
    }
    if (n->dims[1].prev_pc != NF) return g;
    g.RP = 4 * ((T0 + 3) / 4) + 8;
    g.RPp = (T0 + 8 + 1) / 2 * 2;
    const size_t lds_v = (static_cast<size_t>(9) * 12 * g.RP + static_cast<size_t>(P) * T0) * sizeof(float);   // maps + the clip's CQT
    if (lds_v > 150 * 1024 || (static_cast<long long>(P) * T0) % 4 || !mel16) return g;
    const size_t lds_m = (static_cast<size_t>(4) * 12 * g.RP + static_cast<size_t>(2) * 12 * g.RPp * 4 + static_cast<size_t>(P) * T0) * sizeof(float);
    const bool take_mfma = mfma && lds_m <= 150 * 1024;
    if (mel_fm && (!take_mfma || P % 4)) return g;        // only the MFMA form's loader transposes
    g.form = take_mfma ? L0Form::FusedMfma : L0Form::FusedValu;
    g.lds = take_mfma ? lds_m : lds_v;
    if (take_mfma) {      // what the kernel really takes (lds_m stays the rule): the maps, then the image or the fragment regions laid over it
        const size_t maps = lds_m - static_cast<size_t>(P) * T0 * sizeof(float);
        const size_t frag_bytes = c.conv_layers > 1 ? static_cast<size_t>(2) * 24 * 64 * sizeof(uint4) : 0;
        const int sq = 4 * P + ((36 - (4 * P & 31)) & 31);
        const size_t tiled_bytes = static_cast<size_t>((T0 + 3) / 4) * sq * sizeof(float);
        // The untiled frames-major image (every frame through the scalar stores that otherwise take the frames past the last quad) is for
        // pitch counts far above any net that is tested as a whole clip: at 288 and 360 bins the tiled image fits at every eligible frame count.
        g.tiled = mel_fm && maps + tiled_bytes <= kL0MaxLds;
        g.img_sq = g.tiled ? sq : 4;
        g.img_sb = g.tiled ? P : T0;
        g.img_sr = g.tiled ? 4 : 4 * T0;
        const size_t img_bytes = g.tiled ? tiled_bytes : static_cast<size_t>(P) * T0 * sizeof(float);
        g.frag_lds = frag_bytes && maps + std::max(img_bytes, frag_bytes) <= kL0MaxLds;
        g.lds = maps + (g.frag_lds ? std::max(img_bytes, frag_bytes) : img_bytes);       // <= kL0MaxLds either way: lds_m <= 150 KiB
    }
    return g;
}

// mel, ws: only their 16-byte alignment is read (null counts as aligned).  chunk: clips per pitch_chunk call.
Route build_route(const ake_pcnet* n, bool train, int batch, int chunk, int frames, const float* mel, const void* ws, bool mel_fm) {
    Route r;
    const auto& c = n->cfg;
    const int L = c.num_layers;
    const bool ws16 = !(reinterpret_cast<uintptr_t>(ws) & 15);
    int Tl[4], Tf;
    layer_frames(c, frames, Tl, &Tf);
    if (batch < 1 || chunk < 1 || Tf < 1) return r;
    r.chunk_clips[0] = std::min(batch, chunk);
    r.chunk_clips[1] = batch > chunk ? batch % chunk : 0;

    // ---- layer 0 ----
    if (!train && L > 1) r.l0 = layer0_plan(n, Tl[0], !(reinterpret_cast<uintptr_t>(mel) & 15), mel_fm);
    // the up_sixth map as f16 x 4 when the conv that reads it is the persistent f16 kernel for every chunk of this batch (it rounds to f16
    // itself otherwise: same values); psix[1]'s buffer holds either form
    if (r.l0.form == L0Form::FusedMfma && !g_keep_taps && !c.pc2p_mem && n->dims[1].prev_p == 1 && p2p_uses_f16(n, 1, Tl[1])) {
        r.psix_f16 = true;
        for (int k = 0; k < 2 && r.psix_f16; ++k)
            if (r.chunk_clips[k])
                r.psix_f16 = p2p_ps_plan(P2pIn::SrcF16x4, 1, n->dims[1].prev_pc, P2pOut::Plane, n->dims[1].out_p, false, r.chunk_clips[k], c.pitches, Tl[1], ws16).ok;
    }

    // ---- pitch stacks of the layers >= 1 (--denseblock runs its own blocks, --resblock the f32 MFMA kernel) ----
    const int P = c.stay_sixth ? c.pitches / 3 : c.pitches;
    int cp = 1;
    for (int i = 1; i < L && !c.denseblock && !c.resblock; ++i) {
        const LayerDims& d = n->dims[i];
        Route::Pitch& rp = r.p[i];
        const int Ti = Tl[i], c0 = cp, c1 = c.pc2p_mem ? 0 : d.prev_pc;     // (--pc2p_mem: the summed map was added to the pitch stream)
        if (!train && p2p_uses_f16(n, i, Ti)) {
            rp.stack = PStack::F16;
            const bool semi = p2p_fuses_semi(n, i, P, Ti);
            for (int k = 0; k < 2; ++k) {
                const int B = r.chunk_clips[k];
                if (!B) continue;
                const P2pIn in0 = (i == 1 && r.psix_f16) ? P2pIn::SrcF16x4 : ((mel_fm && i == 1) ? P2pIn::SrcFramesMajor : P2pIn::Src);
                rp.k[k].first = p2p_ps_plan(in0, c0, c1, P2pOut::Plane, d.out_p, false, B, P, Ti, ws16);
                rp.k[k].mid = p2p_ps_plan(P2pIn::Planes, 0, 0, P2pOut::Plane, d.out_p, false, B, P, Ti, ws16);
                P2pPsPlan& last = rp.k[k].last;
                if (semi) last = p2p_ps_plan(P2pIn::Planes, 0, 0, P2pOut::SemiFold, d.prev_pc + d.out_p, true, B, P, Ti, ws16);
                if (semi && !last.ok) last = p2p_ps_plan(P2pIn::Planes, 0, 0, P2pOut::Semi, d.out_p, true, B, P, Ti, ws16);
                if (!last.ok) last = p2p_ps_plan(P2pIn::Planes, 0, 0, P2pOut::Nchw, d.out_p, false, B, P, Ti, ws16);
                // one launch for the stack: fed by layer 0's f16 words, its last conv fused with the semitone conv (what was written where
                // stays as the taps know it: planes in the ping-pong buffers, the folded maps in `cat`)
                if (in0 == P2pIn::SrcF16x4 && semi) rp.k[k].stack = p2p_stack_plan(c.conv_layers, c0, c1, true, B, P, Ti);
            }
        } else if (!c.pc2p_mem && !c.stay_sixth && (train || (c.precision == AKE_PRECISION_F32X3 && !g_keep_taps))) {
            // training: f16 x 3 on the persistent form (f32-equivalent products).  Inference in the f32x3 precision mode: the same kernel with
            // the EVAL fragments (BatchNorm folded; three products: f32-equivalent to 2^-22) and LeakyReLU in its epilogue
            for (int k = 0; k < 2; ++k) {
                const int B = r.chunk_clips[k];
                if (!B) continue;
                rp.k[k].x3[0] = p2p_f16x3_plan(c0, c1, d.out_p, B, P, Ti, ws16);
                rp.k[k].x3[1] = p2p_f16x3_plan(d.out_p, 0, d.out_p, B, P, Ti, ws16);
            }
            for (int j = 0; j < c.conv_layers && j < 32; ++j)          // (eligibility does not depend on the clip count)
                if ((train ? n->p2p[i][j].train : n->p2p[i][j].eval).bf_off >= 0 && rp.k[0].x3[j > 0].ok) rp.x3_convs |= 1u << j;
            if (rp.x3_convs) rp.stack = PStack::F16x3;
        }
        cp = d.out_p;
    }
    r.frames_major = mel_fm && !train && L == 2 && !c.resblock && !c.denseblock && !c.pc2p_mem && !c.p2pc_conv && !c.stay_sixth && !c.local &&
                     batch <= chunk && r.l0.form == L0Form::FusedMfma && r.p[1].stack == PStack::F16 && r.p[1].k[0].first.ok;

    // ---- the last layer's pitch-class stack ----
    const int i = L - 1, Ti = Tl[i];
    if (!train && L > 1 && !c.denseblock && pc2pc_fuses(n, i, Ti)) r.pc = PcStack::Fused;
    else if (!train && pc2pc_uses_bf16(n, i, Ti)) r.pc = PcStack::Bf16;
    else if (train && L > 1 && !c.resblock && !c.denseblock) {
        for (int j = 0; j < c.conv_layers && j < 32; ++j)
            if (pc_f16x3_ok(n->pc2pc[i][j].train, Ti, true)) r.pc_x3_convs |= 1u << j;
        if (r.pc_x3_convs) r.pc = PcStack::F16x3;
    }

    // ---- heads (training keeps its own per-conv choices in Fwd::heads_generic) ----
    // key / tonic heads: the first convolution (16 -> 32 channels, most of a head's work) on the bf16 kernel
    const std::vector<ConvSite>&hk = n->heads[0].convs, &ht = n->heads[1].convs, &hg = n->heads[2].convs;      // key, tonic, genre
    const bool head_bf = !train && L > 1 && n->final_ch == 16 && c.head_layers >= 2 && hk[0].eval.bf_off >= 0 && ht[0].eval.bf_off >= 0 &&
                         Tf <= kPcBf16MaxFrames;
    if (!head_bf) return r;
    r.heads = HeadForm::Bf16First;
    // two-conv heads: conv0 leaves its 32 channels as channels-last planes and ONE launch of conv_head1_bf16_kernel finishes both maps
    r.T1 = Tf - (c.kernel_size - 1); r.T2 = r.T1 - (c.kernel_size - 1);
    const int T1 = r.T1, T2 = r.T2;
    if (!(c.head_layers == 2 && hk[1].eval.bf_off >= 0 && ht[1].eval.bf_off >= 0 && T2 > 0 && (12 * ((T2 + 15) / 16) + 15) / 16 <= kHead1MT)) return r;
    r.heads = HeadForm::Head1;
    r.genre_bf = c.genre && hg.size() == 2 && hg[0].eval.bf_off >= 0 && hg[1].eval.bf_off >= 0 && hg[0].eval.kh == 1 && hg[1].eval.kh == 2;
    r.heads_pool = c.local == 0;
    // ... and when the stack above ran as one launch both convolutions of a head run as ONE launch too (heads_fused_kernel): the 32 hidden
    // channels stay in LDS.  ake_debug_keep_taps(1), other head depths and shapes whose patches do not fit keep the two launches.
    r.TpB = 16 * ((T2 + 15) / 16 - 1) + 22;
    r.hf_lds = std::max({(static_cast<size_t>(2) * 12 * (T1 + 8) * 2 + 2 * 4 * 2 * 2 * 64) * sizeof(uint4),      // phase A: patch + weight ring
                         static_cast<size_t>(2) * 12 * r.TpB * 4 * sizeof(uint4),                                // phase B: patch,
                         static_cast<size_t>(8) * kHead1MT * 4 * 64 * sizeof(float)}) +                          // then the partial tiles
               static_cast<size_t>(12) * T2 * sizeof(float);                                                     // the finished map
    if (r.pc == PcStack::Fused && !g_keep_taps && c.local == 0 && hk[0].eval.cout == 32 && ht[0].eval.cout == 32 && hk[0].eval.kh == 12 &&
        ht[0].eval.kh == 12 && hk[1].eval.kh == 12 && ht[1].eval.kh == 12 && (!r.genre_bf || hg[0].eval.cout == 32) &&
        (12 * T1 + 15) / 16 <= 32 && r.hf_lds <= 150 * 1024) {
        r.heads = HeadForm::Fused;
        // phase A's M-tiles over the 8 waves: three each where 24 cover the hidden map (12 x 32 positions and fewer), else four
        r.heads_mt = (12 * T1 + 15) / 16 <= 24 ? 3 : 4;
    }
    return r;
}

}  // namespace
