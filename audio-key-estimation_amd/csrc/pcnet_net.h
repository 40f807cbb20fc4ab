// The net's handle: tensor registry, packed convolutions and their sites (implementation include of pcnet.hip; lives in its translation unit).
#pragma once

namespace {

constexpr double kBnEps = 1e-5;          // nn.BatchNorm2d default
constexpr size_t kLdsBudget = 64 * 1024; // dynamic LDS per workgroup we allow ourselves
constexpr size_t kBfFragsPerConv = 14 * 2 * 64 + 64;   // uint4 entries per 8->8 pitch convolution: f16 weight fragments [14 k-steps][hi|lo][64 lanes], then the 8 inverse channel scales

struct TensorSpec {
    std::string name;
    int64_t shape[4];
    int ndim;
};

struct HostTensor {
    std::vector<float> data;
    bool set = false;
};

struct PackedConv {          // device-resident folded + packed convolution
    int cin = 0, cout = 0, kh = 0, kw = 0, co = 1, groups = 1;
    size_t w_off = 0, b_off = 0;   // float offsets into the blob (VALU layout [group][ci][dy][dx][CO])
    // f32-MFMA fragment layout [ci][dy][s][ntile][64 lanes] (Toeplitz over TB frames), see pcnet_kernels.h
    int tb = 0, ku = 0, ntiles = 0, nt = 1;
    int row_k = 0;                 // 1: 12 x 1 kernel in the row-k fragment form (k = four consecutive rows, kh / 4 steps per channel)
    size_t f_off = 0;
    long long bf_off = -1;         // 16-byte offset of the bf16x3 fragments in ake_pcnet::bf_frags_dev (8 -> 8 channel 7x7 pitch convs), or -1
    long long l0_off = -1;         // ... of the layer-0 form (layer0_mfma_kernel: <= 4 channels, 12 x 7), or -1
    long long bf_off2 = -1;        // ... of input channels [16, 32) of a 32-channel data-gradient pack (heads' first conv, f16 x 3), or -1
};

struct LayerDims {
    int prev_p = 0, prev_pc = 0, out_p = 0, out_pc = 0;
};

// --denseblock: one _DenseLayer / _DenseLayerEquivariant (models.py:456-582).  Both convolutions keep their raw weights; the BatchNorm +
// activation in FRONT of each is a row table (scale, shift, negative slope) in ake_pcnet::dense_aff_dev that the kernel applies on load.
struct DensePack {
    PackedConv c1, c2;       // 1-wide bottleneck (stored as 7 taps, centre one non-zero), k-wide convolution
    size_t aff1 = 0, aff2 = 0;   // float offsets of the two (eval-mode) tables
    // training: the two BatchNorm layers (indices into ake_pcnet::bns), the data-gradient packs (transposed + flipped weights, stored like c1 / c2)
    // and the parameters (indices into ake_pcnet::specs)
    int bn1 = -1, bn2 = -1;
    PackedConv d1, d2;
    int w1 = -1, b1 = -1, w2 = -1, b2 = -1;     // b1 / b2 == -1: bias=False (the plain Conv2d form)
};

// One convolution of the net, resolved once by build_packs: its three packs, the BatchNorm behind it and its parameters.  Fwd, Bwd, the
// fragment packing and the train-mode taps all take their tensors from here: none of them spells a state_dict name.
struct ConvSite {
    PackedConv eval, train, dgrad;   // BatchNorm folded (inference) | raw weights (training) | transposed + flipped raw weights (data gradient)
    int bn = -1;                     // index into ake_pcnet::bns, -1: no BatchNorm behind it (a head's last conv)
    int w = -1, b = -1;              // indices into ake_pcnet::specs
};

struct BnSpecs { int weight = -1, bias = -1, mean = -1, var = -1; };   // one BatchNorm's tensors, indices into ake_pcnet::specs

struct Head {
    std::vector<ConvSite> convs;     // head_layers entries (empty: a net without the genre head)
    int kind;                        // run_conv's: 1 rows circular (12 x k), 2 rows valid (the genre head)
    const char* nm;                  // module name
    bool conv2d;                     // its convolutions are wrappers ("<nm>.<3j>.conv2d.weight")
};

int pick_co(int cout) { return cout >= 8 ? 8 : (cout >= 2 ? 4 : 1); }

}  // namespace

struct ake_pcnet {
    ake_pcnet_config cfg;
    std::vector<LayerDims> dims;
    int final_ch = 0;
    std::vector<TensorSpec> specs;
    std::map<std::string, int> spec_index;
    std::vector<HostTensor> host;
    bool finalized = false;
    bool eval_frags_stale = false;   // ake_pcnet_load_for_training_f32 skipped the MFMA fragments only the inference kernels read
    int chunk_clips = 256;

    // packed parameters
    std::vector<float> blob;
    float* blob_dev = nullptr;
    std::vector<ConvSite> foldc;                  // per layer: --p2pc_conv's octave-fold convolution [co][ci][n_oct] (no dgrad pack)
    std::vector<ConvSite> semi;                   // per layer (no dgrad pack)
    std::vector<std::vector<ConvSite>> pc2pc;     // per layer, conv_layers entries (--resblock: conv0, then conv1, conv2 per block)
    std::vector<ConvSite> up;                     // per layer (index 0 unused; no dgrad pack)
    std::vector<std::vector<ConvSite>> p2p;       // per layer (index 0 empty)
    Head heads[3] = {{{}, 1, "key_classifier", true}, {{}, 1, "tonic_classifier", true}, {{}, 2, "genre_classifier", false}};

    // the BatchNorm layers of the training-mode forward, in forward order (gamma / beta in the blob)
    struct BnLayer { std::string name; int C; size_t gamma_off, beta_off; int ch_off; BnSpecs p; };
    std::vector<BnLayer> bns;
    int bn_channels = 0;
    std::vector<size_t> grad_off;      // float offset of specs[i] in the flat gradient buffer
    size_t grad_floats = 0;
    std::vector<size_t> raw_w_off;     // float offset in the blob of specs[i]'s raw values (convolution weights used by small kernels)

    // device-side rebuild of the blob from a flat parameter buffer (same layout as the gradient buffer):
    //   folded[i] = eval-mode BatchNorm folded into params[i] (conv weights / biases in front of a BatchNorm), else params[i]
    //   blob[j]   = map[j] < 0 ? 0 : (map[j] & kMapFolded ? folded : params)[map[j] & kMapIndex]
    struct FoldRecord { int w, b; BnSpecs bn; int cout; size_t per_out; bool transposed; int cin; };
    std::vector<FoldRecord> fold_records;
    std::vector<int32_t> map_host;     // one entry per blob float
    int32_t* map_dev = nullptr;
    int32_t* fold_ch_dev = nullptr;    // per flat float: -1, or (eval BatchNorm channel << 1) | is_bias
    int32_t* fold_bn_dev = nullptr;    // per eval BatchNorm channel: flat offsets of gamma, beta, running_mean, running_var
    int32_t* run_off_dev = nullptr;    // per training BatchNorm channel (BnLayer::ch_off order): flat offsets of running_mean, running_var
    int32_t* run_off2_dev = nullptr;   // the same for the layers the reference's BACKWARD runs a second time (checkpointed halves: --denseblock's norm1), -1 elsewhere
    int recomputed_bn_channels = 0;
    float* folded_dev = nullptr;
    bool tracing = false;
    std::vector<std::vector<DensePack>> dense_pc, dense_p;   // --denseblock: per layer, conv_layers entries
    struct AffRec { BnSpecs bn; int C; float slope; size_t off; };
    std::vector<AffRec> aff_recs;      // BatchNorm layers behind dense_aff_dev, in table order
    size_t dense_aff_floats = 0;
    float* dense_aff_dev = nullptr;
    int32_t* dense_aff_idx_dev = nullptr;
    uint4* bf_frags_dev = nullptr;     // split-bf16 weight fragments of conv_p2p_f16_kernel, rebuilt from the eval packs on the device
    size_t bf_frags_count = 0;         // uint4 entries
};

namespace {

void add_spec(ake_pcnet* n, const std::string& name, std::initializer_list<int64_t> shape) {
    TensorSpec s;
    s.name = name;
    s.ndim = static_cast<int>(shape.size());
    int i = 0;
    for (auto v : shape) s.shape[i++] = v;
    for (; i < 4; ++i) s.shape[i] = 1;
    n->spec_index[name] = static_cast<int>(n->specs.size());
    n->specs.push_back(s);
}

void add_conv_specs(ake_pcnet* n, const std::string& prefix, int cout, int cin, int kh, int kw) {
    add_spec(n, prefix + ".weight", {cout, cin, kh, kw});
    add_spec(n, prefix + ".bias", {cout});
}

void add_bn_specs(ake_pcnet* n, const std::string& prefix, int c) {
    for (const char* f : {".weight", ".bias", ".running_mean", ".running_var"}) add_spec(n, prefix + f, {c});
}

}  // namespace
