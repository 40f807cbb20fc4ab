// Forward pass orchestration (implementation include of pcnet.hip; lives in its translation unit).
#pragma once

namespace {

// One forward pass.  In eval mode BatchNorm is folded into the convolutions and every tensor is final.  In training
// mode a convolution followed by BatchNorm leaves its RAW output plus a pending (scale, shift, slope) table that the
// next reader applies while loading: the two travel together as a Slot (aff null = nothing pending), handed out by Buffers.
struct Fwd {
    const ake_pcnet* n;
    Buffers& b;
    hipStream_t s;
    bool train;
    const Route& r;                  // what this call launches (build_route)

    // training: the rows of layer i's pitch-stack input table that belong to the up_sixth map (they follow the pitch stream's prev_p rows)
    float* p2pin_up(int i) const { return train ? b.aff_p2pin[i] + 3 * n->dims[i].prev_p : nullptr; }
    // training: where the statistics of BatchNorm layer `bn` (an index into ake_pcnet::bns) are summed, and the stride between the slots
    double* stats_of(int bn) const { return b.stats + 2 * n->bns[bn].ch_off; }
    int stats_stride() const { return 2 * n->bn_channels; }

    // launch BatchNorm finalisation of layer `bn` (count values per channel) into the affine table `aff_out`
    int finalize_bn(int bn, double count, float* aff_out, float slope = kSlope) {
        const auto& l = n->bns[bn];
        // the element count rides along for the unbiased running variance (written by the host-visible copy below)
        return ake::launch("bn_finalize_kernel", bn_finalize_kernel, dim3((l.C + 63) / 64), dim3(64), 0, s, stats_of(bn), stats_stride(),
                           count, n->blob_dev + l.gamma_off, n->blob_dev + l.beta_off, aff_out, b.bstats + 3 * l.ch_off, l.C, slope);
    }
    int identity(float* aff, int C) {
        return ake::launch_untimed("affine_identity_kernel", affine_identity_kernel, dim3((C + 63) / 64), dim3(64), 0, s, aff, C);
    }

    // the convolution of site `cs` (+ its BatchNorm + LeakyReLU where it has one).  Inference: the folded pack, dst is final.  Training: the
    // raw pack, dst is raw and the BatchNorm's table lands in aff_dst with the negative slope of the activation behind it.
    // residual (inference): added before the LeakyReLU.
    int conv(const ConvSite& cs, int kind, Src src, const float* in_aff, int B, int H, int T_in, bool same, float* dst, int ctot, int coff,
             float* aff_dst, const char* name, const float* residual = nullptr, float slope = kSlope) {
        ConvOpts o;
        const bool has_bn = cs.bn >= 0;
        if (!train) {
            o.residual = residual;
            return run_conv(n, cs.eval, kind, src, B, H, T_in, same, has_bn, dst, ctot, coff, s, name, o);
        }
        const PackedConv& pt = cs.train;
        o.in_affine = in_aff;
        if (has_bn) o.stats = stats_of(cs.bn);
        const int rc = run_conv(n, pt, kind, src, B, H, T_in, same, false, dst, ctot, coff, s, name, o);
        if (rc || !has_bn) return rc;
        const int T_out = same ? T_in : T_in - pt.kw + 1, H_out = kind == 2 ? H - pt.kh + 1 : H;
        return finalize_bn(cs.bn, static_cast<double>(B) * H_out * T_out, aff_dst, slope);
    }

    // --denseblock (models.py:584-648): layer i's pitch block (kind 0) or pitch-class block (kind 1) IN PLACE on feat [B][ctot][H][T] whose
    // channels [0, cin) are filled; dense layer j reads channels [0, cin + j*nf) through its norm1 table, writes the bottleneck map, and its
    // k-wide convolution (input through the norm2 table, ReLU) appends nf channels at cin + j*nf.  kind 0: plain Conv2d -- 1 x 1, then
    // k x k ZERO-padded on both axes; kind 1: equivariant 12 x 1 and 12 x k (rows circular, frames zero-padded).
    // Inference: the tables are the folded ones of n->dense_aff_dev and every layer's bottleneck map goes to `bott`.
    // Training (batch statistics): BatchNorm sits in FRONT of both convolutions here, so every norm1 needs the statistics of features other
    // kernels produced: the block input's are taken by channel_stats_kernel, a layer's new features leave theirs in the NEXT layer's norm1
    // cells (conv2's statistics epilogue) and every later norm1 copies the prefix it shares (stats_copy_kernel).  The bottleneck maps and
    // both tables of every layer stay in the workspace (Buffers::dn) for the backward pass.
    int dense_stack(int i, int kind, float* feat, int ctot, int cin, int B, int H, int T, float* bott, const char* label) {
        const std::vector<DensePack>& packs = kind == 0 ? n->dense_p[i] : n->dense_pc[i];
        const Buffers::DenseBufs& dn = b.dn[kind];
        const int nf = n->cfg.n_filters, k = n->cfg.kernel_size;
        const double count = static_cast<double>(B) * H * T;
        int rc;
        if (train && (rc = ake::launch("channel_stats_kernel", channel_stats_kernel, dim3(cin, 1, B), dim3(256), 0, s, feat, static_cast<long long>(ctot) * H * T,
                                       static_cast<long long>(H) * T, stats_of(packs[0].bn1), stats_stride())))
            return rc;
        for (size_t j = 0; j < packs.size(); ++j) {
            const DensePack& dp = packs[j];
            const int cj = cin + static_cast<int>(j) * nf;
            AKE_REQUIRE(dp.c1.cin == cj && cj + nf <= ctot && (!train || (dp.bn1 >= 0 && dp.bn2 >= 0)), AKE_ERR_STATE, "dense %s: channel bookkeeping", label);
            if (train && j > 0) {   // the statistics of channels [0, cj - nf): the previous norm1 has them (its own copy or the block input's)
                const int C = cj - nf;
                if ((rc = launch_flat("stats_copy_kernel", stats_copy_kernel, s, kStatSlots * 2 * C, b.stats, stats_stride(), n->bns[packs[j - 1].bn1].ch_off,
                                      n->bns[dp.bn1].ch_off, C)))
                    return rc;
            }
            if (train && (rc = finalize_bn(dp.bn1, count, dn.aff1[i][j], kSlope))) return rc;   // relu1 = nn.LeakyReLU
            float* const bott_j = train ? dn.bott[i][j] : bott;
            const ConvGeom g1{0, 3, T, H, 0};                  // the single tap sits at offset 3 of the 7 stored
            ConvOpts o1;
            o1.in_affine = train ? dn.aff1[i][j] : n->dense_aff_dev + dp.aff1;
            if (train) o1.stats = stats_of(dp.bn2);
            if (kind == 0) o1.geom = &g1;
            if ((rc = run_conv(n, dp.c1, kind, Src{feat, cj, nullptr, 0, 0, ctot}, B, H, T, true, false, bott_j, dp.c1.cout, 0, s, label, o1))) return rc;
            if (train && (rc = finalize_bn(dp.bn2, count, dn.aff2[i][j], 0.f))) return rc;      // relu2 = nn.ReLU
            const ConvGeom g2{k / 2, k / 2, T, H, 0};
            ConvOpts o2;
            o2.in_affine = train ? dn.aff2[i][j] : n->dense_aff_dev + dp.aff2;
            if (train && j + 1 < packs.size()) o2.stats = stats_of(packs[j + 1].bn1) + 2 * cj;
            if (kind == 0) { o2.geom = &g2; o2.rows_zero = true; }
            if ((rc = run_conv(n, dp.c2, kind, Src{bott_j, dp.c1.cout, nullptr, 0, 0}, B, H, T, true, false, feat, ctot, cj, s, label, o2))) return rc;
        }
        return AKE_OK;
    }

    // --resblock stack (models.py:181-187 / 218-224, 402-454), inference: st = [conv0, (conv1, conv2) per block].  x lives in X
    // (C channels, dense), a block's hidden map (2C channels) in Hb; conv2 adds x before its LeakyReLU, in place -- the last block
    // may write channels [0, C) of a wider buffer instead (final_dst with final_ctot channels).
    int res_stack(const std::vector<ConvSite>& st, int kind, Src first, int B, int H, int T, float* X, float* Hb, float* final_dst,
                  int final_ctot, const char* label) {
        const int C = st[0].eval.cout;
        int rc = conv(st[0], kind, first, nullptr, B, H, T, true, X, C, 0, nullptr, label);
        if (rc) return rc;
        const int nb = (static_cast<int>(st.size()) - 1) / 2;
        for (int r = 0; r < nb; ++r) {
            if ((rc = conv(st[1 + 2 * r], kind, Src{X, C, nullptr, 0, 0}, nullptr, B, H, T, true, Hb, 2 * C, 0, nullptr, label))) return rc;
            const bool to_final = r == nb - 1 && final_dst;
            if ((rc = conv(st[2 + 2 * r], kind, Src{Hb, 2 * C, nullptr, 0, 0}, nullptr, B, H, T, true, to_final ? final_dst : X,
                           to_final ? final_ctot : C, 0, nullptr, label, X)))
                return rc;
        }
        return AKE_OK;
    }

    // --resblock stack, training (batch statistics): st = the sites [conv0, (conv1, conv2) per block].  Every tensor the backward needs stays: z = [conv0 raw, (conv1 raw (2C), conv2 raw,
    // block output) per block] with the pending tables in aff (b2's carries slope 1: no activation of its own; a block output's is
    // the identity).  The last block writes channels [0, C) of final_dst (final_ctot channels) instead of z.back() when given.
    int res_stack_train(const std::vector<ConvSite>& st, int kind, Src first, const float* first_aff, int B, int H, int T,
                        const std::vector<float*>& z, const std::vector<float*>& aff, float* final_dst, int final_ctot, const char* label) {
        const int C = st[0].train.cout;
        const int nb = (static_cast<int>(st.size()) - 1) / 2;
        AKE_REQUIRE(static_cast<int>(z.size()) == 1 + 3 * nb && z.size() == aff.size(), AKE_ERR_STATE, "resblock %s: buffer bookkeeping", label);
        int rc = conv(st[0], kind, first, first_aff, B, H, T, true, z[0], C, 0, aff[0], label);
        if (rc) return rc;
        const float* x = z[0];
        const float* x_aff = aff[0];
        for (int r = 0; r < nb; ++r) {
            float* z1 = z[1 + 3 * r];
            float* z2 = z[2 + 3 * r];
            if ((rc = conv(st[1 + 2 * r], kind, Src{x, C, nullptr, 0, 0}, x_aff, B, H, T, true, z1, 2 * C, 0, aff[1 + 3 * r], label)))
                return rc;
            if ((rc = conv(st[2 + 2 * r], kind, Src{z1, 2 * C, nullptr, 0, 0}, aff[1 + 3 * r], B, H, T, true, z2, C, 0, aff[2 + 3 * r], label, nullptr, 1.f)))
                return rc;
            const bool to_final = r == nb - 1 && final_dst;
            float* xo = to_final ? final_dst : z[3 + 3 * r];
            const long long total = static_cast<long long>(B) * C * H * T;
            if ((rc = launch_flat("res_add_act_kernel", res_add_act_kernel, s, total, z2, aff[2 + 3 * r], x, x_aff, xo, C, H * T, to_final ? final_ctot : C, total)))
                return rc;
            if ((rc = identity(aff[3 + 3 * r], C))) return rc;
            x = xo; x_aff = aff[3 + 3 * r];
        }
        return AKE_OK;
    }

    // semi_conv_stats_kernel's arguments for the plain conv (no table on load, no statistics, no LeakyReLU): the callers set what they add
    SemiTrainArgs semi_train_args(const PackedConv& pc, const float* src, int P, int Tn, float* dst) const {
        SemiTrainArgs ta;
        std::memset(&ta, 0, sizeof(ta));
        ta.s = semi_args(n, pc, src, P, Tn, dst);
        return ta;
    }

    // one launch of semi_conv_stats_kernel over [B][pc.cin][P][ta.s.T]: thread = (semitone row, strip of frames), CO channels per thread
    int launch_semi_conv(const PackedConv& pc, const SemiTrainArgs& ta, int P, int B) {
        const int per_clip = (P / 3) * ta.s.n_strips;
        const int threads = per_clip >= 256 ? 256 : (per_clip + 63) / 64 * 64;
        dim3 grid((per_clip + threads - 1) / threads, pc.groups, B), block(threads);
        switch (pc.co) {
            case 8: return ake::launch("semi_conv_stats_kernel", semi_conv_stats_kernel<8>, grid, block, 0, s, ta);
            case 4: return ake::launch("semi_conv_stats_kernel", semi_conv_stats_kernel<4>, grid, block, 0, s, ta);
            case 1: return ake::launch("semi_conv_stats_kernel", semi_conv_stats_kernel<1>, grid, block, 0, s, ta);
            default: ake::set_error("semi: bad CO"); return AKE_ERR_UNSUPPORTED;
        }
    }

    // pool_semi (+BN+LReLU) + octave fold of `src` [B][C][P][T] into channels [coff, coff+C) of dst [B][ctot][12][T]
    int semi(int layer, const float* src, const float* in_aff, int B, int P, int Tn, float* dst, int ctot, int coff, float* aff_cat_rows) {
        const char* nm = layer == 0 ? "semi_fold_kernel/L0" : "semi_fold_kernel/L1+";
        int rc;
        if (!train && n->cfg.p2pc_conv)     // semitone conv (raw, BatchNorm folded) -> octave-fold convolution (LeakyReLU applied on load)
            return (rc = semi_map(layer, src, B, P, Tn, b.smap, true)) ? rc : fold_maps(layer, b.smap, n->semi[layer].eval.cin, P / 3, B, Tn, dst, ctot, coff, true);
        if (!train) return run_semi(n, n->semi[layer].eval, src, B, P, Tn, dst, ctot, coff, s, nm);
        const PackedConv& pc = n->semi[layer].train;
        const int bn = n->semi[layer].bn;
        SemiTrainArgs ta = semi_train_args(pc, src, P, Tn, b.semi_raw[layer]);
        ta.in_affine = in_aff; ta.stats = stats_of(bn); ta.stats_stride = stats_stride();
        if ((rc = launch_semi_conv(pc, ta, P, B))) return rc;
        if ((rc = finalize_bn(bn, static_cast<double>(B) * (P / 3) * Tn, b.aff_semi[layer]))) return rc;
        const long long total = static_cast<long long>(B) * pc.cin * 12 * Tn;
        if (n->cfg.p2pc_conv) {   // models.py:108-133: the fold is a learned convolution over the octaves + BatchNorm (batch statistics) + LeakyReLU
            const PackedConv& fc = n->foldc[layer].train;
            const int bnf = n->foldc[layer].bn;
            AKE_REQUIRE(pc.cin <= 64, AKE_ERR_UNSUPPORTED, "p2pc_conv training: %d channels", pc.cin);
            if ((rc = launch_flat("fold_conv_kernel", fold_conv_train_kernel, s, total, b.semi_raw[layer], b.aff_semi[layer], n->blob_dev + fc.w_off,
                                  n->blob_dev + fc.b_off, b.foldc_raw[layer], stats_of(bnf), stats_stride(), pc.cin, P / 36, Tn, total)))
                return rc;
            if ((rc = finalize_bn(bnf, static_cast<double>(B) * 12 * Tn, b.aff_foldc[layer]))) return rc;
            // the folded channels are materialised as final activations: every reader of the concat buffer takes them as they are
            if ((rc = launch_flat("apply_affine_kernel", apply_affine_kernel, s, total, b.foldc_raw[layer], b.aff_foldc[layer], dst, pc.cin,
                                  static_cast<long long>(12) * Tn, ctot, coff, total)))
                return rc;
        } else if ((rc = run_fold_max("fold_affine_kernel", b.semi_raw[layer], b.aff_semi[layer], pc.cin, P / 3, B, Tn, dst, ctot, coff, s))) return rc;
        return aff_cat_rows ? identity(aff_cat_rows, pc.cin) : AKE_OK;     // the folded channels are final activations
    }

    int up_sixth(int layer, const float* src, long long src_clip_stride, const float* in_aff, int B, int C, int Tn, float* dst, float* aff_dst) {
        const long long total = static_cast<long long>(B) * C * 36 * Tn;
        if (!train)
            return launch_flat("up_sixth_kernel", up_sixth_kernel<false>, s, total, src, src_clip_stride, nullptr, n->blob_dev + n->up[layer].eval.w_off,
                               n->blob_dev + n->up[layer].eval.b_off, dst, nullptr, 0, C, Tn, total);
        const int bn = n->up[layer].bn;
        AKE_REQUIRE(C <= kBlockStatCh, AKE_ERR_UNSUPPORTED, "up_sixth training: %d channels", C);
        const int rc = launch_flat("up_sixth_train_kernel", up_sixth_kernel<true>, s, total, src, src_clip_stride, in_aff, n->blob_dev + n->up[layer].train.w_off,
                                   n->blob_dev + n->up[layer].train.b_off, dst, stats_of(bn), stats_stride(), C, Tn, total);
        return rc ? rc : finalize_bn(bn, static_cast<double>(B) * 36 * Tn, aff_dst);
    }

    int time_pool(const float* src, const float* in_aff, int B, int C, int H, int Tn, float* dst, int ctot, int coff) {
        const int tp = n->cfg.time_pool_size;
        const long long total = static_cast<long long>(B) * C * H * (Tn / tp);
        return launch_flat("time_pool_kernel", time_pool_kernel, s, total, src, in_aff, dst, C, H, Tn, tp, ctot, coff, total);
    }

    // inference: semitone conv + BN + LeakyReLU of `src` [B][C][P][T] as a map of its own [B][C][P / 3][T] (raw = before the LeakyReLU)
    int semi_map(int layer, const float* src, int B, int P, int Tn, float* dst, bool raw) {
        const PackedConv& pc = n->semi[layer].eval;
        SemiTrainArgs ta = semi_train_args(pc, src, P, Tn, dst);
        ta.out_lrelu = raw ? 0 : 1;
        return launch_semi_conv(pc, ta, P, B);
    }

    // the octave fold of ready maps [B][C][S][T] into channels [coff, coff + C) of dst: max (models.py:95-106) or --p2pc_conv's convolution
    // (raw: the maps come before their LeakyReLU, which the convolution applies on load)
    int fold_maps(int layer, const float* maps, int C, int S, int B, int Tn, float* dst, int ctot, int coff, bool raw = false) {
        if (!n->cfg.p2pc_conv) return run_fold_max("fold_max_kernel", maps, nullptr, C, S, B, Tn, dst, ctot, coff, s);
        const PackedConv& fc = n->foldc[layer].eval;
        const long long total = static_cast<long long>(B) * C * 12 * Tn;
        return launch_flat("fold_conv_kernel", fold_conv_kernel, s, total, maps, n->blob_dev + fc.w_off, n->blob_dev + fc.b_off, dst, C, S / 12, Tn, raw ? 1 : 0,
                           static_cast<long long>(ctot) * 12 * Tn, coff, total);
    }

    // inference, default family: the whole of phase A as one launch, one workgroup per clip (the form and geometry are the route's)
    int layer0_fused(const float* mel, int B) {
        const auto& c = n->cfg;
        const int P = c.pitches, T0 = b.Tl[0], NF = c.n_filters;
        const bool take_mfma = r.l0.form == L0Form::FusedMfma;
        AKE_REQUIRE(r.l0.form != L0Form::Generic && r.l0.lds > 0 && !(reinterpret_cast<uintptr_t>(mel) & 15), AKE_ERR_STATE,
                    "pcnet: the route sent layer 0 to its one-launch form, which this call does not qualify for");
        AKE_REQUIRE(!r.frames_major || take_mfma, AKE_ERR_STATE, "pcnet: the route promised the frames-major input to a layer-0 form that cannot read it");
        AKE_REQUIRE(!r.psix_f16 || (take_mfma && b.melh), AKE_ERR_STATE, "pcnet: the route promised the f16 up_sixth map to a layer-0 form that does not write it");
        const PackedConv& sp = n->semi[0].eval;
        Layer0Args a;
        std::memset(&a, 0, sizeof(a));
        a.RP = r.l0.RP; a.RPp = r.l0.RPp;
        a.mel = mel; a.sw = n->blob_dev + sp.w_off; a.sb = n->blob_dev + sp.b_off;
        const int ctot1 = b.cat_ch(1);
        for (int j = 0; j < c.conv_layers; ++j) {
            const PackedConv& pc = n->pc2pc[0][j].eval;
            const bool lastj = j == c.conv_layers - 1;
            a.w[j] = n->blob_dev + pc.w_off; a.b[j] = n->blob_dev + pc.b_off;
            if (take_mfma) a.frag[j] = n->bf_frags_dev + pc.l0_off;
            a.dst[j] = lastj ? b.cat[1] : b.pc_out(false, 0, j).p;
            a.dst_clip_stride[j] = static_cast<long long>(lastj ? ctot1 : NF) * 12 * T0;
        }
        a.uw = n->blob_dev + n->up[1].eval.w_off; a.ub = n->blob_dev + n->up[1].eval.b_off;
        a.fold0 = b.fold0; a.psix = b.psix[1];
        a.H = P; a.T = T0; a.NF = NF; a.n_conv = c.conv_layers;
        static ake::DeviceOnce fused_attr, mfma_attr;
        int rc;
        if ((rc = ake::raise_lds_limit(fused_attr, 150 * 1024, layer0_fused_kernel))) return rc;
        if ((rc = ake::raise_lds_limit(mfma_attr, static_cast<int>(kL0MaxLds), layer0_mfma_kernel))) return rc;
        a.mel_fm = r.frames_major ? 1 : 0;
        a.frag_lds = r.l0.frag_lds ? 1 : 0;
        a.img_tiled = r.l0.tiled ? 1 : 0; a.img_sq = r.l0.img_sq; a.img_sb = r.l0.img_sb; a.img_sr = r.l0.img_sr;
        AKE_REQUIRE(!r.l0.tiled || r.frames_major, AKE_ERR_STATE, "pcnet: layer 0's image was planned for a frames-major input that the route refused");
        AKE_REQUIRE(r.l0.lds <= kL0MaxLds, AKE_ERR_STATE, "pcnet: layer 0's one-launch form does not fit the LDS at this shape");
        a.taps = g_keep_taps ? 1 : 0;
        if (r.psix_f16) { a.psix_h = reinterpret_cast<uint2*>(b.psix[1]); a.psix = nullptr; a.melh = b.melh; }
        if (take_mfma) return ake::launch("layer0_fused_kernel", layer0_mfma_kernel, dim3(B), dim3(512), r.l0.lds, s, a);
        return ake::launch("layer0_fused_kernel", layer0_fused_kernel, dim3(B), dim3(512), r.l0.lds, s, a);
    }

    // A convolution on its f16 x 3 kernel (f32-equivalent products), BatchNorm finalised behind it in training.  Pitch conv
    // (conv_p2p_f16x3_kernel): training, or f32x3 inference with the folded pack and LeakyReLU in the epilogue
    int p2p_x3(const ConvSite& cs, const P2pX3Plan& g, const Src& src, const float* in_aff, int B, int P, int T, Slot dst) {
        const PackedConv& px = train ? cs.train : cs.eval;
        P2pX3Opts ox;
        ox.lrelu = !train;
        const int rc = run_p2p_f16x3(n, g, px.bf_off, src, in_aff, n->blob_dev + px.b_off, B, P, T, dst.p, px.cout, train ? stats_of(cs.bn) : nullptr,
                                     train ? stats_stride() : 0, s, "conv_p2p_f16x3_kernel/p2p", ox);
        return rc || !train ? rc : finalize_bn(cs.bn, static_cast<double>(B) * P * T, dst.aff);
    }
    // ... pitch-class conv (conv_pc_bf16_kernel's f16 x 3 form), training only: `planes` holds the input (run_nchw_to_cl16_f16x2), the
    // output has H_out rows
    int pc_x3_train(const ConvSite& cs, const unsigned short* planes, int B, int T_in, bool same, int H_out, Slot dst, const char* name) {
        PcBf16Opts o;
        o.f16x3 = true; o.stats = stats_of(cs.bn); o.stats_stride = stats_stride();
        const int rc = run_pc_bf16(n, cs.train, planes, B, T_in, same, false, dst.p, nullptr, s, name, o);
        return rc ? rc : finalize_bn(cs.bn, static_cast<double>(B) * H_out * (same ? T_in : T_in - cs.train.kw + 1), dst.aff);
    }

    // Layer i's pitch stack (kind 0) or pitch-class stack (kind 1) on the generic kernels: --resblock's blocks, or conv after conv, each
    // writing where Buffers says (p_out / pc_out).  `final` set: the stack's last output goes to channels [0, cout) of that buffer of
    // final_ctot channels instead.  x3: bit j = conv j runs on the f16 x 3 kernel of its kind (x3_plans: the pitch form's geometry for conv 0
    // and for the later ones).  *left: the stack's output.
    int stack(int kind, int i, Src src, const float* src_aff, int B, int H, int T, const char* label, Slot* left, unsigned x3 = 0,
              const P2pX3Plan* x3_plans = nullptr, Slot final = {}, int final_ctot = 0) {
        const std::vector<ConvSite>& st = kind == 0 ? n->p2p[i] : n->pc2pc[i];
        const int cout = st[0].eval.cout;
        auto out = [&](bool tr, int j) { return kind == 0 ? b.p_out(tr, i, j) : b.pc_out(tr, i, j); };
        int rc;
        if (n->cfg.resblock && train) {   // a last block's output in `final` is a final activation (identity table)
            if ((rc = res_stack_train(st, kind, src, src_aff, B, H, T, kind == 0 ? b.pst[i] : b.pcst[i], kind == 0 ? b.aff_pst[i] : b.aff_pcst[i], final.p,
                                      final_ctot, label)))
                return rc;
            *left = final.p ? final : (kind == 0 ? b.p_last(i) : b.pc_last(i));
            return final.p ? identity(final.aff, cout) : AKE_OK;
        }
        if (n->cfg.resblock) {
            *left = final.p ? final : out(false, 0);
            return res_stack(st, kind, src, B, H, T, out(false, 0).p, out(false, 1).p, final.p, final_ctot, label);
        }
        for (int j = 0; j < n->cfg.conv_layers; ++j) {
            const bool to_final = final.p && j == n->cfg.conv_layers - 1;
            const Slot dst = to_final ? final : out(train, j);
            if (!(x3 >> j & 1)) rc = conv(st[j], kind, src, src_aff, B, H, T, true, dst.p, to_final ? final_ctot : cout, 0, dst.aff, label);
            else if (kind == 0) rc = p2p_x3(st[j], x3_plans[j > 0], src, src_aff, B, H, T, dst);
            else {   // the input's f16 planes go to the inference ping-pong buffer (idle in training)
                unsigned short* planes = reinterpret_cast<unsigned short*>(b.pcb[i]);
                if ((rc = run_nchw_to_cl16_f16x2(src.p0, src.c0, B, T, src_aff, planes, s))) return rc;
                rc = pc_x3_train(st[j], planes, B, T, true, 12, dst, "conv_pc_f16x3_kernel/pc2pc");
            }
            if (rc) return rc;
            src = Src{dst.p, cout, nullptr, 0, 0}; src_aff = dst.aff; *left = dst;
        }
        return AKE_OK;
    }

    // Phase A, whole batch: layer 0 (models.py:361-369) and layer 1's up_sixth (models.py:372-374).
    int entry(const float* mel, int B) {
        const auto& c = n->cfg;
        const int L = c.num_layers, P = c.pitches, T0 = b.Tl[0];
        int rc;
        if (r.l0.form != L0Form::Generic) return layer0_fused(mel, B);
        if (c.stay_sixth && L > 1 && !train) {   // models.py:366-367: the activated semitone map is the pitch stream from here on; its fold feeds pc2pc
            if ((rc = semi_map(0, mel, B, P, T0, b.p0, false))) return rc;
            if ((rc = fold_maps(0, b.p0, 1, P / 3, B, T0, b.fold0, 1, 0))) return rc;
        } else if (c.denseblock) {   // the fold is channel 0 of the block's feature buffer (L == 1: fold0 itself, else layer 1's concat buffer)
            const int ctot1 = L == 1 ? n->final_ch : b.cat_ch(1);
            float* feat = L == 1 ? b.fold0 : b.cat[1];
            if ((rc = semi(0, mel, nullptr, B, P, T0, feat, ctot1, 0, nullptr))) return rc;
            if (L == 1) return AKE_OK;                           // its block runs in the tail
            if ((rc = dense_stack(0, 1, feat, ctot1, 1, B, 12, T0, b.pca[0], "conv_mfma_kernel/pc2pc0"))) return rc;
            // training: the raw up_sixth map + its table (rows [prev_p, ..) of the pitch block's input table, as in the default net)
            return up_sixth(1, feat, static_cast<long long>(ctot1) * 12 * T0, nullptr, B, n->dims[1].prev_pc, T0, b.psix[1], p2pin_up(1));
        } else if ((rc = semi(0, mel, nullptr, B, P, T0, b.fold0, 1, 0, nullptr))) return rc;      // (--stay_sixth training: semi_raw[0] + its table are the pitch stream)
        if (L == 1) return AKE_OK;                               // its pc2pc runs in the tail
        const LayerDims& d1 = n->dims[1];
        const int ctot1 = b.cat_ch(1);
        Slot pc0;                                                // the stack's output = channels [0, nf) of layer 1's concat buffer
        if ((rc = stack(1, 0, Src{b.fold0, 1, nullptr, 0, 0}, nullptr, B, 12, T0, "conv_mfma_kernel/pc2pc0", &pc0, 0, nullptr, b.cat_slot(train, 1), ctot1)))
            return rc;
        if (c.stay_sixth) return AKE_OK;                         // no up_sixth: the pitch classes are repeated as they are
        // psix's BatchNorm lands in rows [prev_p, ..) of the pitch-conv input table (row 0.. = the pitch stream itself)
        if (train && (rc = identity(b.aff_p2pin[1], d1.prev_p))) return rc;
        return up_sixth(1, b.cat[1], static_cast<long long>(ctot1) * 12 * T0, b.cat_slot(train, 1).aff, B, d1.prev_pc, T0, b.psix[1], p2pin_up(1));
    }

    // Phase B, per chunk of clips [c0, c0+B): pitch convs -> semitone fold for every layer >= 1 (plus pc2pc / pooling /
    // the next up_sixth for the inner layers of deeper nets).
    int pitch_chunk(const float* mel, int c0, int B) {
        const auto& c = n->cfg;
        const int L = c.num_layers;
        const int P = c.stay_sixth ? c.pitches / 3 : c.pitches;  // rows of the pitch stream (--stay_sixth: semitones)
        int rc;
        // pitch stream [B][cp][P][T]: a final activation, except --stay_sixth in training (layer 0's raw semitone map + aff_semi[0])
        const float* p_cur = c.stay_sixth ? (train ? b.semi_raw[0] : b.p0 + static_cast<size_t>(c0) * P * b.Tl[0]) : mel;
        int cp = 1;
        const float* pc_cur = nullptr;
        for (int i = 1; i < L; ++i) {
            const int Ti = b.Tl[i];
            const LayerDims& d = n->dims[i];
            const bool last = i == L - 1;
            const int ctot = b.cat_ch(i);         // this chunk's concat buffer (--denseblock: ctot = d.out_pc, the block's growth included) and up_sixth map
            float* cat = b.cat_at(i, c0);
            float* psix = b.psix_at(i, c0);
            if (c.denseblock) {   // models.py:370-396 with dense stacks: both blocks grow their concat buffers in place
                if (i > 1 && (rc = up_sixth(i, pc_cur, static_cast<long long>(ctot) * 12 * Ti, nullptr, B, d.prev_pc, Ti, psix, p2pin_up(i)))) return rc;
                float* fp = b.pa[i];                                                  // [B][out_p][P][Ti]
                const long long total = static_cast<long long>(B) * (cp + d.prev_pc) * P * Ti;
                if ((rc = launch_flat("concat_repeat_kernel", concat_repeat_kernel, s, total, p_cur, cp, psix, d.prev_pc, 36, fp, d.out_p, P, Ti, total, p2pin_up(i))))
                    return rc;
                if ((rc = dense_stack(i, 0, fp, d.out_p, cp + d.prev_pc, B, P, Ti, b.pb[i], "conv_mfma_kernel/p2p"))) return rc;
                if ((rc = semi(i, fp, nullptr, B, P, Ti, cat, ctot, d.prev_pc, nullptr))) return rc;
                if (last) return AKE_OK;                                              // its pitch-class block + pooling + heads run batch-wide
                if ((rc = dense_stack(i, 1, cat, ctot, d.prev_pc + d.out_p, B, 12, Ti, b.pca[i], "conv_mfma_kernel/pc2pc"))) return rc;
                float* catn = b.cat_at(i + 1, c0);
                if ((rc = time_pool(cat, nullptr, B, ctot, 12, Ti, catn, b.cat_ch(i + 1), 0))) return rc;
                if ((rc = time_pool(fp, nullptr, B, d.out_p, P, Ti, b.ppool[i], d.out_p, 0))) return rc;
                pc_cur = catn; p_cur = b.ppool[i]; cp = d.out_p;
                continue;
            }
            if (i > 1 && !c.stay_sixth) {   // layer 1's up_sixth ran batch-wide in entry(); pc_cur = pooled (final) features here
                if (train && (rc = identity(b.aff_p2pin[i], d.prev_p))) return rc;
                if ((rc = up_sixth(i, pc_cur, static_cast<long long>(ctot) * 12 * Ti, nullptr, B, d.prev_pc, Ti, psix, p2pin_up(i)))) return rc;
            }
            // models.py:378-384  repeat + concat (never materialised) + pitch convs
            Src sdesc{p_cur, cp, psix, d.prev_pc, 36};
            if (c.stay_sixth) {   // models.py:322-323, 379-383: the pitch classes themselves, repeated over the octaves (a dense copy: they live
                                  // in channels [0, prev_pc) of a concat buffer)
                const float* pcs = i == 1 ? cat : pc_cur;
                const long long per_clip = static_cast<long long>(d.prev_pc) * 12 * Ti, total = per_clip * B;
                if ((rc = launch_flat("slice_channels_kernel", slice_channels_kernel, s, total, pcs, static_cast<long long>(ctot) * 12 * Ti, b.pcd[i], per_clip, total)))
                    return rc;
                sdesc = Src{p_cur, cp, b.pcd[i], d.prev_pc, 12};
                if (train) {   // the stack's input table: the pitch stream's rows, then the pitch classes' (they were copied raw)
                    if (i == 1) AKE_HIP_CHECK(hipMemcpyAsync(b.aff_p2pin[i], b.aff_semi[0], sizeof(float) * 3 * cp, hipMemcpyDeviceToDevice, s));
                    else if ((rc = identity(b.aff_p2pin[i], cp))) return rc;
                    AKE_HIP_CHECK(hipMemcpyAsync(b.aff_p2pin[i] + 3 * cp, b.aff_cat[i], sizeof(float) * 3 * d.prev_pc, hipMemcpyDeviceToDevice, s));
                }
            }
            if (c.pc2p_mem) {   // models.py:376-377: no concat, the summed up_sixth map is added to the pitch stream
                const long long total = static_cast<long long>(B) * cp * P * Ti;
                // (training: psix is raw, its up_sixth_b table sits behind the pitch stream's identity rows; the sum itself is final)
                if ((rc = launch_flat("pc2p_mem_kernel", pc2p_mem_kernel, s, total, p_cur, psix, b.pin[i], cp, d.prev_pc / cp, P, Ti, total, p2pin_up(i)))) return rc;
                sdesc = Src{b.pin[i], cp, nullptr, 0, 0};
            }
            const float* in_aff = train ? b.aff_p2pin[i] : nullptr;
            Slot out;                             // the stack's last output
            // inference: the stack runs on f16 MFMA (f16 activations x hi + lo f16 weights, see conv_p2p_f16_kernel); the activations
            // between its convs are ONE channels-last f16 plane (16 B per position) in the same ping-pong buffers
            const Route::Pitch& rp = r.p[i];
            const Route::Pitch::PerChunk& rk = rp.k[r.chunk_kind(B)];
            P2pOut last_out = P2pOut::Nchw;       // what the stack's last launch left: the pitch tensor, the semitone maps, or the folded maps in `cat`
            if (rp.stack == PStack::F16 && rk.stack.ok) {      // the whole stack, semitone conv and fold as one launch
                unsigned short* planes[kP2pStackMax];
                for (int j = 0; j < kP2pStackMax; ++j) planes[j] = reinterpret_cast<unsigned short*>(b.p_out(false, i, j).p);
                if ((rc = run_p2p_stack(n, n->p2p[i], n->semi[i].eval, rk.stack, b.melh + static_cast<size_t>(c0) * P * Ti,
                                        reinterpret_cast<const uint2*>(b.psix[1]) + static_cast<size_t>(c0) * 36 * Ti, d.prev_pc, planes, cat, ctot, d.prev_pc, B, P, Ti, s,
                                        "conv_p2p_f16_kernel")))
                    return rc;
                out = b.p_out(false, i, c.conv_layers - 1);
                last_out = P2pOut::SemiFold;
            } else if (rp.stack == PStack::F16) {
                for (int j = 0; j < c.conv_layers; ++j) {
                    out = b.p_out(false, i, j);
                    const bool last_conv = j == c.conv_layers - 1;
                    const P2pPsPlan& g = j == 0 ? rk.first : (last_conv ? rk.last : rk.mid);
                    P2pPsIo io;
                    io.in = g.in; io.out = g.out;
                    io.dst_ctot = d.out_p;
                    if (j > 0) io.planes = reinterpret_cast<const unsigned short*>(b.p_out(false, i, j - 1).p);
                    else if (g.in == P2pIn::SrcF16x4)   // layer 0 left the CQT and the up_sixth map as f16 words (8 bytes per position of the map, clip stride 36 T words)
                        io.src = Src{reinterpret_cast<const float*>(b.melh + static_cast<size_t>(c0) * P * Ti), 1,
                                     reinterpret_cast<const float*>(reinterpret_cast<const uint2*>(b.psix[1]) + static_cast<size_t>(c0) * 36 * Ti), d.prev_pc, 36};
                    else io.src = sdesc;              // the stack's input (pitch stream | repeated up_sixth output) is assembled by the kernel's own loader
                    switch (g.out) {
                        case P2pOut::Plane: io.plane = reinterpret_cast<unsigned short*>(out.p); break;
                        case P2pOut::Nchw: io.dst = out.p; break;
                        case P2pOut::Semi: io.dst = out.p; io.semi = &n->semi[i].eval; break;       // `out` receives the semitone maps [clip][8][P / 3][T]
                        case P2pOut::SemiFold: io.dst = cat; io.dst_ctot = ctot; io.fold_coff = d.prev_pc; io.semi = &n->semi[i].eval; break;
                    }
                    if (last_conv) last_out = g.out;
                    AKE_REQUIRE(g.ok || g.in == P2pIn::Planes || g.in == P2pIn::Src, AKE_ERR_STATE,
                                "pcnet: the route promised an input form only the persistent pitch conv reads, for a chunk (%d clips) it does not take", B);
                    if (g.ok) rc = run_p2p_f16_ps(n, n->p2p[i][j].eval, g, io, B, P, Ti, s, "conv_p2p_f16_kernel");
                    else rc = run_p2p_f16(n, n->p2p[i][j].eval, io.planes, j == 0 ? &io.src : nullptr, B, P, Ti, io.dst, d.out_p, io.plane, s, "conv_p2p_f16_kernel");
                    if (rc) return rc;
                }
            } else if ((rc = stack(0, i, sdesc, in_aff, B, P, Ti, "conv_mfma_kernel/p2p", &out, rp.x3_convs, rk.x3))) return rc;      // (f16 x 3 on the persistent form where x3_convs says)
            // models.py:386-392  pool_semi -> fold, written next to pc in the concat buffer
            if (last_out == P2pOut::SemiFold) {
            } else if (last_out == P2pOut::Semi) {
                if ((rc = run_fold_max("fold_max_kernel", out.p, nullptr, d.out_p, P / 3, B, Ti, cat, ctot, d.prev_pc, s))) return rc;
            } else if (c.stay_sixth && train) {   // ... through the last conv's pending BatchNorm + LeakyReLU
                if ((rc = run_fold_max("fold_affine_kernel", out.p, out.aff, d.out_p, P, B, Ti, cat, ctot, d.prev_pc, s))) return rc;
                if ((rc = identity(b.aff_cat[i] + 3 * d.prev_pc, d.out_p))) return rc;
            } else if (c.stay_sixth) {   // models.py:391: the stack's output is folded as it is (no semitone conv)
                if ((rc = fold_maps(i, out.p, d.out_p, P, B, Ti, cat, ctot, d.prev_pc))) return rc;
            } else if ((rc = semi(i, out.p, out.aff, B, P, Ti, cat, ctot, d.prev_pc, train ? b.aff_cat[i] + 3 * d.prev_pc : nullptr))) return rc;
            if (last) return AKE_OK;                             // pc2pc + pooling + heads run batch-wide
            // inner layers of deeper nets: pc2pc, then both time pools (models.py:393-396)
            Slot pdst;
            if ((rc = stack(1, i, Src{cat, ctot, nullptr, 0, 0}, b.cat_slot(train, i).aff, B, 12, Ti, "conv_mfma_kernel/pc2pc", &pdst))) return rc;
            float* catn = b.cat_at(i + 1, c0);
            if ((rc = time_pool(pdst.p, pdst.aff, B, d.out_pc, 12, Ti, catn, b.cat_ch(i + 1), 0))) return rc;
            if (train && (rc = identity(b.aff_cat[i + 1], d.out_pc))) return rc;
            if ((rc = time_pool(out.p, out.aff, B, d.out_p, P, Ti, b.ppool[i], d.out_p, 0))) return rc;
            pc_cur = catn; p_cur = b.ppool[i]; cp = d.out_p;
        }
        return AKE_OK;
    }

    // The last layer's pitch-class stack and its time pool (models.py:396; the last layer's pitch stream feeds nothing, its pool is skipped),
    // whole batch.  *feat: the features the heads read.
    int last_pc_stack(int B, Slot* feat) {
        const auto& c = n->cfg;
        const int L = c.num_layers, i = L - 1, Ti = b.Tl[i];
        const Slot src = L == 1 ? Slot{b.fold0, nullptr} : b.cat_slot(train, i);
        const int cin = L == 1 ? 1 : n->dims[i].prev_pc + n->dims[i].out_p;      // (--denseblock: the block's input, its growth follows)
        const char* const label = L == 1 ? "conv_mfma_kernel/pc2pc0" : "conv_mfma_kernel/pc2pc";
        int rc;
        *feat = Slot{b.pcf, nullptr};
        if (r.pc == PcStack::Fused)      // stack + pool as one launch; it also writes the channels-last copy that heads on the bf16 kernels read
            return run_pc2pc_fused(n, i, src.p, cin, B, Ti, b.pcf, r.heads != HeadForm::Generic ? b.feat_cl : nullptr, s);
        Slot out;
        if (r.pc == PcStack::Bf16) {
            // inference, 16-channel stacks: bf16 MFMA with split operands; the stack's input is converted to channels-last planes once,
            // the intermediate activations stay in that format (same 64 B per position as 16 f32 channels: the ping-pong buffers are
            // reused), the last convolution writes NCHW f32 for the pooling / heads
            const unsigned short* in = reinterpret_cast<const unsigned short*>(b.pcb[i]);
            if ((rc = run_nchw_to_cl16(src.p, cin, B, Ti, reinterpret_cast<unsigned short*>(b.pcb[i]), s))) return rc;
            for (int j = 0; j < c.conv_layers; ++j) {
                const bool last_conv = j == c.conv_layers - 1;
                out = b.pc_out(false, i, j);
                if ((rc = run_pc_bf16(n, n->pc2pc[i][j].eval, in, B, Ti, true, true, last_conv ? out.p : nullptr,
                                      last_conv ? nullptr : reinterpret_cast<unsigned short*>(out.p), s, "conv_pc_bf16_kernel/pc2pc")))
                    return rc;
                in = reinterpret_cast<const unsigned short*>(out.p);
            }
        } else if (c.denseblock) {   // the last layer's pitch-class block, in place on its concat buffer: the features are the buffer itself
            if ((rc = dense_stack(i, 1, src.p, n->final_ch, cin, B, 12, Ti, b.pca[i], label))) return rc;
            out = Slot{src.p, nullptr};
        } else if ((rc = stack(1, i, Src{src.p, cin, nullptr, 0, 0}, src.aff, B, 12, Ti, label, &out, r.pc_x3_convs))) return rc;
        if (L == 1) { *feat = out; return AKE_OK; }
        return time_pool(out.p, out.aff, B, n->final_ch, 12, Ti, b.pcf, n->final_ch, 0);
    }

    // Heads on the bf16 kernels (key, tonic and, where the route says so, genre): *Tm = frames of the finished maps, *pooled = heads whose
    // outputs the launch also pooled.  Both convolutions of every head as ONE launch (heads_fused_kernel) ...
    int heads_fused(int B, const PoolArgs& pool, float* const outs[3], int* Tm, int* pooled) {
        const int nh = r.genre_bf ? 3 : 2, Tf = b.Tf;
        float* const maps[3] = {b.map_k, b.map_t, b.map_g};
        HeadsFusedArgs ha;
        std::memset(&ha, 0, sizeof(ha));
        ha.xh = b.feat_cl; ha.xl = b.feat_cl + static_cast<long long>(B) * 12 * Tf * 16;
        for (int h = 0; h < nh; ++h) {
            const PackedConv& p0 = n->heads[h].convs[0].eval;
            const PackedConv& p1 = n->heads[h].convs[1].eval;
            ha.bfragA[h] = n->bf_frags_dev + p0.bf_off; ha.biasA[h] = n->blob_dev + p0.b_off; ha.KHA[h] = p0.kh;
            ha.bfragB[h] = n->bf_frags_dev + p1.bf_off; ha.biasB[h] = n->blob_dev + p1.b_off; ha.KHB[h] = p1.kh;
            ha.dst[h] = maps[h];
            ha.pout[h] = outs[h];
        }
        // workgroups [i * B, (i + 1) * B) run head hs[i]; with a genre head its short workgroups come first: they hand their slots on early
        if (r.genre_bf) { ha.hs[0] = 2; ha.hs[1] = 0; ha.hs[2] = 1; }
        else { ha.hs[0] = 0; ha.hs[1] = 1; ha.hs[2] = 1; }
        ha.batch = B; ha.T_in = Tf; ha.T1 = r.T1; ha.T2 = r.T2; ha.TpA = r.T1 + 8; ha.TpB = r.TpB; ha.JB = (r.T2 + 15) / 16;
        ha.fin_off = static_cast<int>(r.hf_lds / sizeof(float)) - 12 * r.T2;
        ha.pool = pool;
        *Tm = r.T2; *pooled = nh;
        static ake::DeviceOnce hf_attr;
        const int rc = ake::raise_lds_limit(hf_attr, 150 * 1024, heads_fused_kernel<3>, heads_fused_kernel<4>);
        if (rc) return rc;
        return r.heads_mt == 3 ? ake::launch("heads_fused_kernel", heads_fused_kernel<3>, dim3(nh * B), dim3(512), r.hf_lds, s, ha)
                               : ake::launch("heads_fused_kernel", heads_fused_kernel<4>, dim3(nh * B), dim3(512), r.hf_lds, s, ha);
    }

    // ... or the first convolutions leave their 32 channels as channels-last planes and ONE launch of conv_head1_bf16_kernel finishes the maps
    int heads_head1(int B, const PoolArgs& pool, float* const outs[3], int* Tm, int* pooled) {
        const int nh = r.genre_bf ? 3 : 2, Tf = b.Tf, T1 = r.T1, T2 = r.T2;
        const Head* const heads = n->heads;
        float* const maps[3] = {b.map_k, b.map_t, b.map_g};
        Head1BfArgs ha;
        std::memset(&ha, 0, sizeof(ha));
        int rc;
        for (int h = 0; h < nh; ++h) {
            const PackedConv& p0 = heads[h].convs[0].eval;
            const PackedConv& p1 = heads[h].convs[1].eval;
            unsigned short* planes = reinterpret_cast<unsigned short*>(b.head_out(false, h, 0, false).p);
            if (h == 0) {   // the key and the tonic head read the same features with the same geometry: one launch, blockIdx.y picks the head
                PcBf16Opts tonic;
                tonic.pc2 = &heads[1].convs[0].eval; tonic.planes_out2 = reinterpret_cast<unsigned short*>(b.head_out(false, 1, 0, false).p);
                if ((rc = run_pc_bf16(n, p0, b.feat_cl, B, Tf, false, true, nullptr, planes, s, "conv_pc_bf16_kernel/head", tonic))) return rc;
            }
            if (h == 2 && (rc = run_pc_bf16(n, p0, b.feat_cl, B, Tf, false, true, nullptr, planes, s, "conv_pc_bf16_kernel/genre_head")))
                return rc;
            ha.xh[h] = planes; ha.xl[h] = planes + static_cast<long long>(B) * 12 * T1 * 32;
            ha.bfrag[h] = n->bf_frags_dev + p1.bf_off; ha.bias[h] = n->blob_dev + p1.b_off; ha.dst[h] = maps[h];
            ha.KH[h] = p1.kh; ha.circular[h] = p1.kh == 12 ? 1 : 0; ha.H_out[h] = ha.circular[h] ? 12 : 12 - p1.kh + 1;
        }
        ha.T_in = T1; ha.T_out = T2; ha.JB = (T2 + 15) / 16; ha.Tp = r.TpB;
        // the patch, and after the multiply loop the partial tiles of the 8 waves in the same bytes (two workgroups per CU fit)
        size_t lds = std::max(static_cast<size_t>(2) * 12 * ha.Tp * 4 * sizeof(uint4), static_cast<size_t>(8) * kHead1MT * 4 * 64 * sizeof(float));
        if (r.heads_pool) {   // the masked mean + sigmoid of each finished map in the same launch (its LDS copy sits behind the patch / partial tiles)
            ha.fin_off = static_cast<int>(lds / sizeof(float));
            lds += static_cast<size_t>(12) * T2 * sizeof(float);
            for (int h = 0; h < nh; ++h) ha.pout[h] = outs[h];
            ha.pool = pool;
        }
        *Tm = T2; *pooled = r.heads_pool ? nh : 0;
        static ake::DeviceOnce h1_attr;
        if ((rc = ake::raise_lds_limit(h1_attr, 150 * 1024, conv_head1_bf16_kernel))) return rc;
        AKE_REQUIRE(lds <= 150 * 1024, AKE_ERR_UNSUPPORTED, "heads: %d frames do not fit conv_head1_bf16_kernel", T1);
        return ake::launch("conv_head1_bf16_kernel", conv_head1_bf16_kernel, dim3(B, nh), dim3(512), lds, s, ha);
    }

    // The heads from `first` on, one launch per convolution; *Tm = frames of their maps where it runs any
    int heads_generic(int first, Slot feat, int B, int* Tm) {
        const auto& c = n->cfg;
        const Head* const heads = n->heads;     // key, tonic, genre
        const int Tf = b.Tf;
        bool head_planes_ready = false;           // training: the f16 hi / lo planes of the pooled features (b.feat_cl) exist
        int rc;
        for (int h = first; h < (c.genre ? 3 : 2); ++h) {
            for (int j = 0; j < c.head_layers; ++j) {
                const ConvSite& cs = heads[h].convs[j];
                const PackedConv& pe = cs.eval;
                const bool lastj = j == c.head_layers - 1;
                // conv j reads the features or conv j - 1's output, hc channels of Tcur frames
                const Slot src = j == 0 ? feat : b.head_out(train, h, j - 1, false);
                const int hc = j == 0 ? n->final_ch : heads[h].convs[j - 1].eval.cout, Tcur = Tf - j * (c.kernel_size - 1);
                const Slot dst = b.head_out(train, h, j, lastj);
                // key / tonic heads: the first convolution (16 -> 32 channels, most of a head's work) on the bf16 kernel; both read the same
                // channels-last copy of the features
                if (r.heads != HeadForm::Generic && h < 2 && j == 0) {
                    if ((rc = run_pc_bf16(n, pe, b.feat_cl, B, Tcur, false, true, dst.p, nullptr, s, "conv_pc_bf16_kernel/head"))) return rc;
                    continue;
                }
                if (train && j == 0 && !lastj && pc_f16x3_ok(cs.train, Tcur, false)) {   // the heads' first convs: f16 x 3 MFMA
                    if (!head_planes_ready) {               // one conversion of the pooled features serves the three heads
                        if ((rc = run_nchw_to_cl16_f16x2(src.p, hc, B, Tcur, src.aff, b.feat_cl, s))) return rc;
                        head_planes_ready = true;
                    }
                    if ((rc = pc_x3_train(cs, b.feat_cl, B, Tcur, false, heads[h].kind == 2 ? 12 - cs.train.kh + 1 : 12, dst,
                                          h == 2 ? "conv_pc_f16x3_kernel/genre_head" : "conv_pc_f16x3_kernel/head")))
                        return rc;
                    continue;
                }
                if (train && lastj && j > 0 && pe.cout == 1 && pe.kw == 7 && !n->raw_w_off.empty()) {   // cin -> 1: one workgroup per clip, f32 VALU
                    const size_t lds = (static_cast<size_t>(hc) * 12 * Tcur + static_cast<size_t>(hc) * pe.kh * 7) * sizeof(float);
                    if (lds <= 150 * 1024 && Tcur - 6 >= 1) {
                        static ake::DeviceOnce hl_attr;
                        if ((rc = ake::raise_lds_limit(hl_attr, 150 * 1024, conv_head_last_kernel))) return rc;
                        if ((rc = ake::launch(h == 2 ? "conv_head_last_kernel/genre" : "conv_head_last_kernel", conv_head_last_kernel, dim3(B), dim3(384), lds, s,
                                              src.p, src.aff, n->blob_dev + n->raw_w_off[cs.w], n->blob_dev + n->raw_w_off[cs.b], dst.p, hc, pe.kh,
                                              heads[h].kind == 2 ? 0 : 1, Tcur, Tcur - 6)))
                            return rc;
                        continue;
                    }
                }
                if ((rc = conv(cs, heads[h].kind, Src{src.p, hc, nullptr, 0, 0}, src.aff, B, 12, Tcur, false, dst.p, pe.cout, 0, dst.aff,
                               h == 2 ? "conv_mfma_kernel/genre_head" : "conv_mfma_kernel/head")))
                    return rc;
            }
            *Tm = Tf - c.head_layers * (c.kernel_size - 1);
        }
        return AKE_OK;
    }

    // The maps of Tm frames -> the outputs: --local's sliding-window max, or the masked temporal mean + sigmoid of the heads from `pooled` on
    int pool_maps(int B, int Tm, int pooled, const PoolArgs& pool, float* const outs[3]) {
        const auto& c = n->cfg;
        if (c.local > 0) {   // per-frame outputs (models.py:720-722, 805-810)
            AKE_REQUIRE(Tm >= c.local, AKE_ERR_INVALID, "pcnet --local: %d map frames are fewer than the pooling window %d", Tm, c.local);
            LocalPoolArgs la;
            std::memset(&la, 0, sizeof(la));
            la.maps[0] = b.map_k; la.maps[1] = b.map_t; la.maps[2] = c.genre ? b.map_g : nullptr;
            for (int h = 0; h < 3; ++h) la.outs[h] = outs[h];
            la.Tm = Tm; la.Tq = Tm - c.local + 1; la.W = c.local; la.batch = B;
            return ake::launch("local_pool_kernel", local_pool_kernel, dim3(static_cast<unsigned>((static_cast<long long>(B) * 12 * Tm + 255) / 256), 3), dim3(256),
                               0, s, la);
        }
        PoolHeadArgs pa;     // models.py:754-804
        std::memset(&pa, 0, sizeof(pa));
        pa.maps[0] = b.map_k; pa.maps[1] = b.map_t; pa.maps[2] = c.genre ? b.map_g : nullptr;
        for (int h = 0; h < pooled; ++h) pa.maps[h] = nullptr;
        if (!pa.maps[0] && !pa.maps[1] && !pa.maps[2]) return AKE_OK;
        for (int h = 0; h < 3; ++h) pa.outs[h] = outs[h];
        pa.rows[0] = 12; pa.rows[1] = 12; pa.rows[2] = 11;
        pa.Tm = Tm; pa.batch = B; pa.pool = pool;
        return ake::launch("head_pool_kernel", head_pool_kernel, dim3((B * 12 + 63) / 64, 3), dim3(64), 0, s, pa);
    }

    // Phase C, whole batch: last layer's pc2pc, time pool, heads (models.py:750-753), pooling.
    int tail(int B, const int64_t* seq, float* key_out, float* tonic_out, float* genre_out) {
        const auto& c = n->cfg;
        float* const outs[3] = {key_out, tonic_out, genre_out};
        PoolArgs pool;
        pool.seq = reinterpret_cast<const long long*>(seq);
        pool.n_pool_layers = c.num_layers - 1; pool.tp = c.time_pool_size; pool.shrink = (c.kernel_size - 1) * c.head_layers; pool.max_pool = c.max_pool; pool.clip0 = 0;
        Slot feat;
        int rc, Tm = b.Tf, pooled = 0;
        if ((rc = last_pc_stack(B, &feat))) return rc;
        const bool one_launch = r.heads == HeadForm::Head1 || r.heads == HeadForm::Fused;      // (key, tonic and the genre head where genre_bf says so)
        // heads on the bf16 kernels read a channels-last copy of the pooled features (the fused stack wrote it itself)
        if (r.heads != HeadForm::Generic && r.pc != PcStack::Fused && (rc = run_nchw_to_cl16(feat.p, n->final_ch, B, b.Tf, b.feat_cl, s))) return rc;
        if (one_launch && (rc = r.heads == HeadForm::Fused ? heads_fused(B, pool, outs, &Tm, &pooled) : heads_head1(B, pool, outs, &Tm, &pooled))) return rc;
        if ((rc = heads_generic(one_launch ? (r.genre_bf ? 3 : 2) : 0, feat, B, &Tm))) return rc;
        return pool_maps(B, Tm, pooled, pool, outs);
    }
};

int forward_impl(const ake_pcnet* n, bool train, const float* mel, int batch, int frames, const int64_t* seq_length, float* key_out,
                 float* tonic_out, float* genre_out, float* bn_stats_out, void* workspace, size_t ws_bytes, ake_stream_t stream,
                 bool mel_frames_major = false) {
    AKE_REQUIRE(n && mel && key_out && tonic_out, AKE_ERR_INVALID, "pcnet forward: null argument");
    AKE_REQUIRE(n->finalized, AKE_ERR_STATE, "pcnet: ake_pcnet_finalize has not been called");
    AKE_REQUIRE(train || !n->eval_frags_stale, AKE_ERR_STATE,
                "pcnet: the last weight load was ake_pcnet_load_for_training_f32 (training fragments only): call ake_pcnet_load_from_device_f32 before inference");
    AKE_REQUIRE(batch > 0 && frames > 0, AKE_ERR_INVALID, "pcnet: bad batch/frames");
    AKE_REQUIRE(!n->cfg.genre || genre_out, AKE_ERR_INVALID, "pcnet: genre head enabled but genre_out is null");
    const int chunk = train ? batch : std::min(batch, n->chunk_clips);     // batch statistics need the whole batch at once
    Buffers b;
    int rc = plan_buffers(n, batch, chunk, frames, workspace, &b, train);
    if (rc) return rc;
    AKE_REQUIRE(workspace && ws_bytes >= b.bytes, AKE_ERR_WORKSPACE, "pcnet: workspace %zu < %zu bytes", ws_bytes, b.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Route route = build_route(n, train, batch, chunk, frames, mel, workspace, mel_frames_major);
    AKE_REQUIRE(!mel_frames_major || route.frames_major, AKE_ERR_UNSUPPORTED,
                "pcnet: this configuration does not take the frames-major input (ake_pcnet_accepts_frames_major)");
    if (train) AKE_HIP_CHECK(hipMemsetAsync(b.stats, 0, sizeof(double) * 2 * n->bn_channels * kStatSlots, s));
    Fwd f{n, b, s, train, route};
    if ((rc = f.entry(mel, batch))) return rc;
    for (int c0 = 0; c0 < batch && n->cfg.num_layers > 1; c0 += chunk) {
        const int B = std::min(chunk, batch - c0);
        if ((rc = f.pitch_chunk(mel + static_cast<size_t>(c0) * n->cfg.pitches * frames, c0, B))) return rc;
    }
    if ((rc = f.tail(batch, seq_length, key_out, tonic_out, genre_out))) return rc;
    if (train && bn_stats_out)
        AKE_HIP_CHECK(hipMemcpyAsync(bn_stats_out, b.bstats, sizeof(float) * 3 * n->bn_channels, hipMemcpyDeviceToDevice, s));
    return AKE_OK;
}

}  // namespace
