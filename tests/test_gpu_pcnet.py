"""PARITY (GPU): the HIP PitchClassNet forward, called through the C ABI, against the reference fixtures and the oracle.

Tolerance: BASELINE.json states 1e-3 relative (fp32 path vs the reference's fp64 outputs); measured as
max|a-b| / max|b| per tensor.  The kernels land around 1e-6, so we assert 1e-4 to catch
regressions long before the stated budget.

What these assertions cannot see: the weights here are seeded-random, their outputs almost constant (the default fixture's key output
moves by 1e-4 of its maximum between its input and silence), so output parity at TOL does not resolve the input-dependent part -- a
front-end or plumbing fault passes.  tests/test_gpu_sensitive.py holds the same routes on calibrated and trained weights
(tests/sensitive.py, tests/test_sensitive_host.py).
"""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from conftest import golden_state_dict, rel_err
from oracle import mirex_oracle, pcnet_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-4          # asserted;  north_star budget is 1e-3
DEV = "cuda:0"


def make_net(gold, **opt_kw):
    opt = Namespace(**json.loads(str(gold["opt"])))
    for k, v in opt_kw.items():
        setattr(opt, k, v)
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return net.to(DEV).eval(), opt


def test_native_library_is_the_compute_path():
    assert torch.cuda.is_available()
    import ctypes
    assert isinstance(ake_amd._lib.lib(), ctypes.CDLL)


def test_default_config_against_reference_fixture(gold_default):
    net, _ = make_net(gold_default)
    x = torch.from_numpy(gold_default["x"]).to(DEV)
    seq = torch.from_numpy(gold_default["seq_length"]).to(DEV)
    key, tonic, genre = net(x, seq)
    assert key.shape == (4, 12) and tonic.shape == (4, 12) and genre.shape == (4, 11) and key.dtype == torch.float32
    assert rel_err(key.cpu(), gold_default["key"]) < TOL
    assert rel_err(tonic.cpu(), gold_default["tonic"]) < TOL
    assert rel_err(genre.cpu(), gold_default["genre"]) < TOL
    key, tonic, genre = net(x, None)                              # models.py:786-797 branch
    assert rel_err(key.cpu(), gold_default["key_noseq"]) < TOL
    assert rel_err(tonic.cpu(), gold_default["tonic_noseq"]) < TOL
    assert rel_err(genre.cpu(), gold_default["genre_noseq"]) < TOL
    # float64 in -> float64 out, as reference scripts expect (train_model.py:105 .double())
    k64 = net(x.double(), seq)[0]
    assert k64.dtype == torch.float64 and rel_err(k64.cpu(), gold_default["key"]) < TOL


def test_every_layer_against_reference_taps(gold_default, gold_taps):
    net, _ = make_net(gold_default)
    x = torch.from_numpy(gold_taps["x"]).to(DEV)
    outs = net(x, torch.from_numpy(gold_taps["seq_length"]).to(DEV))
    for got, n in zip(outs, ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_taps[n]) < TOL
    # inference fuses the semitone conv into the stack's last pitch conv: that conv's output is never written ...
    with pytest.raises(ake_amd._lib.AkeError, match="fused with the semitone conv"):
        net.tap("model.1.p2p.layer.8")
    with pytest.raises(ake_amd._lib.AkeError, match="stays in LDS"):                       # ... nor the inside of the fused pitch-class stack
        net.tap("model.1.pc2pc.layer.5")
    assert rel_err(net.tap("model.1.time_pool_pc").cpu().numpy(), gold_taps["tap/model.1.time_pool_pc"]) < TOL
    fused_cat = net.tap("model.1.cat").clone()
    # ... unless the debug switch keeps every nameable activation in memory (the unfused kernels: f32 semitone conv)
    was = net.keep_taps(True)
    try:
        outs = net(x, torch.from_numpy(gold_taps["seq_length"]).to(DEV))
        _check_taps(net, outs, gold_taps)
        # (the fused launch hands the semitone conv the last pitch conv's output as f16, the unfused one as f32: one more rounding unit)
        assert rel_err(fused_cat.cpu(), net.tap("model.1.cat").cpu()) < 1e-3
    finally:
        net.keep_taps(was)


def _check_taps(net, outs, gold_taps):
    for got, n in zip(outs, ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_taps[n]) < TOL
    # (the first conv of a 3-conv stack is overwritten by the third: ping-pong buffers; its effect is covered by the next tap)
    direct = ["model.0.pool", "model.0.pc2pc.layer.2", "model.0.pc2pc.layer.5", "model.1.up_sixth_a",
              "model.1.p2p.layer.5", "model.1.p2p.layer.8", "model.1.pc2pc.layer.5", "model.1.pc2pc.layer.8",
              "model.1.time_pool_pc", "key_map", "tonic_map", "genre_map"]
    for name in direct:
        got = net.tap(name).cpu().numpy()
        ref = gold_taps["tap/" + name]
        assert got.shape == ref.shape, name
        # the pitch convs multiply ONE f16 value per activation (2^-11 = 4.9e-4 relative rounding at the worst element, unbiased; see
        # conv_p2p_f16_kernel): inside the pitch stack single elements are off by that much; after the octave max and the
        # pitch-class stack the taps are back under TOL, and the outputs are held to TOL like everything else
        # (layer 0's stack too, and what is computed straight from its last conv's output)
        f16_inside = name.startswith("model.1.p2p.layer.") or name in ("model.0.pc2pc.layer.2", "model.0.pc2pc.layer.5", "model.1.up_sixth_a")
        assert rel_err(got, ref) < (1e-3 if f16_inside else TOL), name
    with pytest.raises(ake_amd._lib.AkeError, match="not a materialised"):
        net.tap("model.1.p2p.layer.2")
    cat = net.tap("model.1.cat").cpu().numpy()                    # [pc | pc2] concat, models.py:392
    assert rel_err(cat[:, :4], gold_taps["tap/model.0.pc2pc.layer.8"]) < 1e-3          # f16 operands inside layer 0's stack, see above
    pool_ref = gold_taps["tap/model.1.pool"]                      # semitone conv + octave max of the f16 pitch stack: see above
    assert rel_err(cat[:, 4:], pool_ref) < 1e-3
    # (rms error / rms value = 2.5e-4 .. 4e-4 here: f16 rounding units, 2^-12 -- these sums cancel, they do not average; the averaging that
    # brings the outputs to 1e-5 happens in the 1344-term pitch-class convolutions and the temporal mean behind this tap)
    assert float(np.sqrt(np.mean((cat[:, 4:] - pool_ref) ** 2)) / np.sqrt(np.mean(pool_ref ** 2))) < 6e-4


def test_guard_octave_equivariance_all_12_shifts(gold_guard):
    """equivariance_test.py as an assertion: 360-bin net, +-1..12 semitone zero-fill shifts roll key and tonic."""
    net, opt = make_net(gold_guard)
    assert opt.octaves == 10 and not net.genre
    mel = gold_guard["mel"].astype(np.float64)
    mel_g = np.concatenate([np.zeros((36, 40)), mel, np.zeros((36, 40))])
    seq = torch.tensor(40).reshape(1, 1)                          # equivariance_test.py:188
    rows_k, rows_t = [], []
    for i in range(0, 13):
        k, t = net(torch.from_numpy(mirex_oracle.mel_shifting_up(mel_g, i)).reshape(1, 1, 360, 40).to(DEV), seq)
        rows_k.insert(0, k[0].cpu().numpy()); rows_t.insert(0, t[0].cpu().numpy())
    for i in range(1, 13):
        k, t = net(torch.from_numpy(mirex_oracle.mel_shifting_down(mel_g, i)).reshape(1, 1, 360, 40).to(DEV), seq)
        rows_k.append(k[0].cpu().numpy()); rows_t.append(t[0].cpu().numpy())
    K, T = np.stack(rows_k), np.stack(rows_t)
    assert K.shape == (25, 12)
    assert rel_err(K, gold_guard["key_eval"]) < TOL and rel_err(T, gold_guard["tonic_eval"]) < TOL
    for s in range(1, 13):                                        # <= 1e-5 abs on the fp32 path
        assert np.abs(K[12 - s] - np.roll(K[12], s)).max() <= 1e-5
        assert np.abs(K[12 + s] - np.roll(K[12], -s)).max() <= 1e-5
        assert np.abs(T[12 - s] - np.roll(T[12], s)).max() <= 1e-5
        assert np.abs(T[12 + s] - np.roll(T[12], -s)).max() <= 1e-5


def test_circular_roll_on_training_geometry(gold_default):
    net, _ = make_net(gold_default)
    x = torch.from_numpy(gold_default["x"]).to(DEV)
    k0, t0, g0 = net(x, None)
    for s in (1, 5, 11):
        k1, t1, _ = net(torch.roll(x, 3 * s, dims=2), None)
        assert (k1 - torch.roll(k0, s, dims=1)).abs().max() <= 1e-5
        assert (t1 - torch.roll(t0, s, dims=1)).abs().max() <= 1e-5


@pytest.mark.parametrize("cfg", [dict(num_layers=1), dict(num_layers=3), dict(head_layers=1), dict(head_layers=3),
                                 dict(conv_layers=2, n_filters=2), dict(n_filters=3), dict(max_pool=True), dict(time_pool_size=4)])
def test_other_configurations_against_oracle(cfg):
    """Non-default sizes of the default family: random weights, oracle as the checker."""
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5)
    num_layers = cfg.pop("num_layers", 2)
    for k, v in cfg.items():
        setattr(opt, k, v)
    torch.manual_seed(11)
    net = ake_amd.PitchClassNet(288, 12, num_layers, 7, opt)
    g = torch.Generator().manual_seed(3)
    for name, mod in net.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
            mod.weight.data.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    sd64 = pcnet_oracle.to_dtype(net.state_dict(), torch.float64)
    T = 120 if (num_layers == 3 or opt.time_pool_size == 4 or opt.head_layers == 3) else 52
    x = torch.rand((3, 1, 288, T), generator=g) * 2.5
    seq = torch.tensor([T, T - 9, T - 20])
    ref = pcnet_oracle.pcnet_forward(sd64, x.double(), seq, head_layers=opt.head_layers, time_pool_size=opt.time_pool_size,
                                     max_pool=opt.max_pool)
    got = net.to(DEV).eval()(x.to(DEV), seq.to(DEV))
    for a, b in zip(got, ref):
        assert rel_err(a.cpu(), b) < TOL


def test_weights_follow_parameter_updates(gold_default):
    """The device copy is refreshed when parameters change in place (optimizer step / load_state_dict)."""
    net, _ = make_net(gold_default)
    x = torch.from_numpy(gold_default["x"]).to(DEV)
    k0 = net(x, None)[0].clone()
    with torch.no_grad():
        net.key_classifier[3].conv2d.bias.add_(0.5)
    k1 = net(x, None)[0]
    sd = pcnet_oracle.to_dtype({k: v.cpu() for k, v in net.state_dict().items()}, torch.float64)
    ref = pcnet_oracle.pcnet_forward(sd, x.cpu().double(), None)[0]
    assert (k1 - k0).abs().max() > 1e-3 and rel_err(k1.cpu(), ref) < TOL


def test_full_size_batch_properties(gold_default):
    """BASELINE config-2 size (B=256, T=76): clips are independent (chunking at 64 must not leak), the batch
    is a permutation-equivariant map, and 8 of the clips are checked against the oracle."""
    net, _ = make_net(gold_default)
    g = torch.Generator().manual_seed(9)
    x = (torch.rand((256, 1, 288, 76), generator=g) * 2.5).to(DEV)
    seq = torch.randint(30, 77, (256,), generator=g).to(DEV)
    key, tonic, genre = net(x, seq)
    assert torch.isfinite(key).all() and torch.isfinite(tonic).all() and torch.isfinite(genre).all()
    perm = torch.randperm(256, generator=g).to(DEV)
    kp, tp, gp = net(x[perm], seq[perm])
    assert torch.equal(kp, key[perm]) and torch.equal(tp, tonic[perm]) and torch.equal(gp, genre[perm])
    idx = [0, 1, 63, 64, 65, 127, 128, 255]
    ks, ts, gs = net(x[idx], seq[idx])
    assert torch.equal(ks, key[idx]) and torch.equal(ts, tonic[idx])
    sd = golden_state_dict(gold_default, torch.float64)
    ref = pcnet_oracle.pcnet_forward(sd, x[idx].cpu().double(), seq[idx].cpu())
    for a, b in zip((ks, ts, gs), ref):
        assert rel_err(a.cpu(), b) < TOL


def test_batch_larger_than_the_pitch_stream_chunk(gold_default):
    """B = 300 > the 256-clip chunk of the pitch stream: the second chunk (44 clips) reuses the ping-pong buffers of the first;
    the pitch-class stack and the heads run batch-wide.  Every clip must equal its result in a batch of its own."""
    net, _ = make_net(gold_default)
    g = torch.Generator().manual_seed(21)
    x = (torch.rand((300, 1, 288, 40), generator=g) * 2.5).to(DEV)
    seq = torch.randint(30, 41, (300,), generator=g).to(DEV)
    key, tonic, genre = net(x, seq)
    idx = [0, 255, 256, 257, 299]
    ks, ts, gs = net(x[idx], seq[idx])
    assert torch.equal(ks, key[idx]) and torch.equal(ts, tonic[idx]) and torch.equal(gs, genre[idx])


@pytest.mark.parametrize("B,T", [(24, 76), (40, 52), (64, 30), (20, 120)])
def test_persistent_pitch_conv_equals_per_tile_kernel_and_oracle(gold_default, B, T):
    """Batches with >= 2 row tiles per CU run the 8 -> 8 pitch convolutions as ONE persistent launch (conv_p2p_f16_ps_kernel: LDS-DMA
    double buffer, weights in registers, staged 16-byte stores); smaller batches take conv_p2p_f16_kernel (one workgroup per tile).
    Same arithmetic in the same order => bit-identical outputs; partial last row tiles (288 = 20 x 14 + 8 at T = 52) and tile
    counts that do not divide by the grid are covered by the shapes.  Three clips are also held against the oracle."""
    net, _ = make_net(gold_default)
    g = torch.Generator().manual_seed(100 + T)
    x = (torch.rand((B, 1, 288, T), generator=g) * 2.5).to(DEV)
    seq = torch.randint(26, T + 1, (B,), generator=g).to(DEV)
    key, tonic, genre = net(x, seq)
    last = net.tap("model.1.cat").clone()                          # [pitch-class stream | folded semitone maps of the pitch stack]
    for lo in range(0, B, 4):                                      # 4 clips: far below two tiles per CU -> per-tile kernel
        ks, ts, gs = net(x[lo:lo + 4], seq[lo:lo + 4])
        assert torch.equal(net.tap("model.1.cat"), last[lo:lo + 4]), lo
        assert torch.equal(ks, key[lo:lo + 4]) and torch.equal(ts, tonic[lo:lo + 4]) and torch.equal(gs, genre[lo:lo + 4]), lo
    idx = [0, B // 2, B - 1]
    sd = golden_state_dict(gold_default, torch.float64)
    ref = pcnet_oracle.pcnet_forward(sd, x[idx].cpu().double(), seq[idx].cpu())
    for a, b in zip((key[idx], tonic[idx], genre[idx]), ref):
        assert rel_err(a.cpu(), b) < TOL


def test_f16_pitch_convs_with_wide_batchnorm_scales(gold_default):
    """The pitch convolutions multiply f16 activations and f16 weights (conv_p2p_f16_kernel).  LeakyReLU is positively homogeneous, so
    scaling a BatchNorm's (gamma, beta) per channel and dividing the next convolution's weights of that input channel leaves the
    network's function unchanged -- while activations and folded weights now span 1e-3 .. 1e3 across channels.  Every output
    channel's weights are scaled into f16's normal range by their own power of two before rounding (the epilogue undoes it), so the
    outputs must still agree with the oracle; without that scaling the small weights would be f16 subnormals."""
    sd32 = golden_state_dict(gold_default)
    scale = torch.tensor([300.0, 1 / 300.0, 1.0, 30.0, 1 / 30.0, 1000.0, 1e-3, 1.0])
    for bn, nxt in (("model.1.p2p.layer.1", "model.1.p2p.layer.3.weight"), ("model.1.p2p.layer.4", "model.1.p2p.layer.6.weight"),
                    ("model.1.p2p.layer.7", "model.1.pool_semi.weight")):
        sd32[bn + ".weight"] = sd32[bn + ".weight"] * scale
        sd32[bn + ".bias"] = sd32[bn + ".bias"] * scale
        sd32[nxt] = sd32[nxt] / scale.reshape(1, 8, 1, 1)
        scale = scale.flip(0)
    opt = Namespace(**json.loads(str(gold_default["opt"])))
    net = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
    net.load_state_dict(sd32, strict=True)
    net = net.to(DEV).eval()
    x = torch.from_numpy(gold_default["x"])
    seq = torch.from_numpy(gold_default["seq_length"])
    ref = pcnet_oracle.pcnet_forward({k: v.double() if v.is_floating_point() else v for k, v in sd32.items()}, x.double(), seq)
    for n, r in zip(("key", "tonic", "genre"), ref):                     # the function did not change
        assert rel_err(r, gold_default[n]) < 1e-6
    got = net(x.to(DEV), seq.to(DEV))
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and rel_err(a.cpu(), b) < TOL, rel_err(a.cpu(), b)


def test_local_heads_against_reference_fixture(gold_default, gold_local):
    """--local (models.py:720-722, 805-810): same state_dict, per-frame key / tonic / genre; the fixture is the
    reference's own output with opt.local.  A long song (T = 1500, time-tiled kernels) is checked against the oracle."""
    net, opt = make_net(gold_default, local=True)
    assert net.local_window == int(gold_local["window"]) == 38
    x = torch.from_numpy(gold_local["x"]).to(DEV)
    key, tonic, genre = net(x, torch.tensor([120, 120]))
    assert key.shape == (2, 71, 12) and tonic.shape == (2, 71, 12) and genre.shape == (2, 108, 11)
    assert rel_err(key.cpu(), gold_local["key"]) < TOL
    assert rel_err(tonic.cpu(), gold_local["tonic"]) < TOL
    assert rel_err(genre.cpu(), gold_local["genre"]) < TOL
    g = torch.Generator().manual_seed(77)
    xl = torch.rand((1, 1, 288, 1500), generator=g) * 2.5
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), xl.double(), None, local_window=38)
    got = net(xl.to(DEV), None)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and rel_err(a.cpu(), b) < TOL
    with pytest.raises(ake_amd._lib.AkeError, match="pooling window"):
        net(torch.zeros(1, 1, 288, 40, device=DEV), None)
    # training mode: the same per-frame shapes, BatchNorm on the batch statistics (gradients: test_gpu_backward.test_local_net_gradients)
    tr = net.train()(x, None)
    ref_tr = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), x.cpu().double(), None, training=True, local_window=38)
    for a, b in zip(tr, ref_tr):
        assert a.shape == b.shape and rel_err(a.detach().cpu(), b) < TOL


def test_resblock_against_reference_fixture(gold_resblock):
    """--resblock (the first architecture variant; models.py:181-187, 218-224, 402-454), inference: the reference's
    own outputs for its own seeded weights; a second shape (three layers deep would change the family: two layers, B = 3, T = 52) against
    the oracle."""
    net, opt = make_net(gold_resblock)
    assert net.resblock
    x = torch.from_numpy(gold_resblock["x"]).to(DEV)
    seq = torch.from_numpy(gold_resblock["seq_length"]).to(DEV)
    key, tonic, genre = net(x, seq)
    assert rel_err(key.cpu(), gold_resblock["key"]) < TOL
    assert rel_err(tonic.cpu(), gold_resblock["tonic"]) < TOL
    assert rel_err(genre.cpu(), gold_resblock["genre"]) < TOL
    g = torch.Generator().manual_seed(8)
    x2 = torch.rand((3, 1, 288, 52), generator=g) * 2.5
    seq2 = torch.tensor([52, 40, 31])
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_resblock, torch.float64), x2.double(), seq2)
    for a, b in zip(net(x2.to(DEV), seq2.to(DEV)), ref):
        assert rel_err(a.cpu(), b) < TOL
    # train mode (batch statistics; gradients: tests/test_gpu_backward.py::test_resblock_net_gradients)
    ref_t = pcnet_oracle.pcnet_forward(golden_state_dict(gold_resblock, torch.float64), x2.double(), seq2, training=True)
    with torch.no_grad():
        for a, b in zip(net.train()(x2.to(DEV), seq2.to(DEV)), ref_t):
            assert rel_err(a.cpu(), b) < TOL
    with pytest.raises(ake_amd._lib.AkeError, match="not tapped"):
        net.eval()(x, seq); net.tap("model.1.p2p.layer.5")


def test_pc2p_mem_against_reference_fixture(gold_pc2pmem):
    """--pc2p_mem (models.py:145-166), inference: the reference's own outputs for its own seeded weights (small batch: per-tile kernels),
    then the BASELINE shape with a batch large enough for the persistent kernels (B = 20, T = 76) against the oracle."""
    net, opt = make_net(gold_pc2pmem)
    assert net.pc2p_mem
    x = torch.from_numpy(gold_pc2pmem["x"]).to(DEV)
    seq = torch.from_numpy(gold_pc2pmem["seq_length"]).to(DEV)
    for got, name in zip(net(x, seq), ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_pc2pmem[name]) < TOL, name
    g = torch.Generator().manual_seed(18)
    x2 = torch.rand((20, 1, 288, 76), generator=g) * 2.5
    seq2 = torch.randint(30, 77, (20,), generator=g)
    got = net(x2.to(DEV), seq2.to(DEV))
    idx = [0, 7, 19]
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_pc2pmem, torch.float64), x2[idx].double(), seq2[idx])
    for a, b in zip(got, ref):
        assert rel_err(a[idx].cpu(), b) < TOL
    # train mode (batch statistics; gradients: tests/test_gpu_backward.py::test_pc2p_mem_net_gradients)
    ref_t = pcnet_oracle.pcnet_forward(golden_state_dict(gold_pc2pmem, torch.float64), x2[:6].double(), seq2[:6], training=True)
    with torch.no_grad():
        for a, b in zip(net.train()(x2[:6].to(DEV), seq2[:6].to(DEV)), ref_t):
            assert rel_err(a.cpu(), b) < TOL


def test_p2pc_conv_against_reference_fixture(gold_p2pcconv):
    """--p2pc_conv (models.py:108-133), inference: the reference's own outputs for its own seeded weights, and a second shape
    (B = 5, T = 76) against the oracle."""
    net, opt = make_net(gold_p2pcconv)
    assert net.p2pc_conv
    x = torch.from_numpy(gold_p2pcconv["x"]).to(DEV)
    seq = torch.from_numpy(gold_p2pcconv["seq_length"]).to(DEV)
    for got, name in zip(net(x, seq), ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_p2pcconv[name]) < TOL, name
    g = torch.Generator().manual_seed(28)
    x2 = torch.rand((5, 1, 288, 76), generator=g) * 2.5
    seq2 = torch.randint(30, 77, (5,), generator=g)
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_p2pcconv, torch.float64), x2.double(), seq2)
    for a, b in zip(net(x2.to(DEV), seq2.to(DEV)), ref):
        assert rel_err(a.cpu(), b) < TOL
    # train mode (batch statistics; gradients: tests/test_gpu_backward.py::test_variant_net_gradients)
    ref_t = pcnet_oracle.pcnet_forward(golden_state_dict(gold_p2pcconv, torch.float64), x2.double(), seq2, training=True)
    with torch.no_grad():
        for a, b in zip(net.train()(x2.to(DEV), seq2.to(DEV)), ref_t):
            assert rel_err(a.cpu(), b) < TOL


def test_stay_sixth_against_reference_fixture(gold_staysixth):
    """--stay_sixth (models.py:322-323, 336, 366-367), inference: the reference's own outputs for its own seeded weights (per-tile
    kernels on the 96-row pitch stream), then B = 24, T = 76 (persistent kernels) against the oracle."""
    net, opt = make_net(gold_staysixth)
    assert net.stay_sixth
    x = torch.from_numpy(gold_staysixth["x"]).to(DEV)
    seq = torch.from_numpy(gold_staysixth["seq_length"]).to(DEV)
    for got, name in zip(net(x, seq), ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_staysixth[name]) < TOL, name
    g = torch.Generator().manual_seed(38)
    x2 = torch.rand((64, 1, 288, 76), generator=g) * 2.5
    seq2 = torch.randint(30, 77, (64,), generator=g)
    got = net(x2.to(DEV), seq2.to(DEV))
    idx = [0, 31, 63]
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_staysixth, torch.float64), x2[idx].double(), seq2[idx])
    for a, b in zip(got, ref):
        assert rel_err(a[idx].cpu(), b) < TOL
    # train mode (batch statistics; gradients: tests/test_gpu_backward.py::test_variant_net_gradients)
    ref_t = pcnet_oracle.pcnet_forward(golden_state_dict(gold_staysixth, torch.float64), x2[:6].double(), seq2[:6], training=True)
    with torch.no_grad():
        for a, b in zip(net.train()(x2[:6].to(DEV), seq2[:6].to(DEV)), ref_t):
            assert rel_err(a.cpu(), b) < TOL


@pytest.mark.parametrize("ksz", [3, 5])
def test_kernel_size_3_and_5_against_reference_fixture(ksz):
    """--kernel_size 3 / 5 (train_model.py:194): the reference's own outputs for its own seeded weights (every convolution on the generic
    kernels: the kernel width is a parameter of theirs), with and without seq_length; then B = 24, T = 76 and the train-mode forward
    against the oracle.  Gradients: tests/test_gpu_backward.py::test_kernel_size_gradients."""
    from conftest import load_golden
    gold = load_golden(f"pcnet_k{ksz}_T40.npz")
    net, opt = make_net(gold)
    assert opt.kernel_size == ksz and net.kernel_size == ksz
    x = torch.from_numpy(gold["x"]).to(DEV)
    seq = torch.from_numpy(gold["seq_length"]).to(DEV)
    for got, name in zip(net(x, seq), ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold[name]) < TOL, name
    for got, name in zip(net(x, None), ("key_noseq", "tonic_noseq", "genre_noseq")):
        assert rel_err(got.cpu(), gold[name]) < TOL, name
    g = torch.Generator().manual_seed(40 + ksz)
    x2 = torch.rand((24, 1, 288, 76), generator=g) * 2.5
    seq2 = torch.randint(30, 77, (24,), generator=g)
    got = net(x2.to(DEV), seq2.to(DEV))
    idx = [0, 11, 23]
    sd64 = golden_state_dict(gold, torch.float64)
    ref = pcnet_oracle.pcnet_forward(sd64, x2[idx].double(), seq2[idx], kernel_size=ksz)
    for a, b in zip(got, ref):
        assert rel_err(a[idx].cpu(), b) < TOL
    ref_t = pcnet_oracle.pcnet_forward(sd64, x2[:6].double(), seq2[:6], kernel_size=ksz, training=True)
    with torch.no_grad():
        for a, b in zip(net.train()(x2[:6].to(DEV), seq2[:6].to(DEV)), ref_t):
            assert rel_err(a.cpu(), b) < TOL


def test_denseblock_against_reference_fixture(gold_denseblock):
    """--denseblock (models.py:188-189, 225-226, 456-648), inference: the reference's own outputs for its own seeded weights (n_filters = 2,
    conv_layers = 2), then other shapes against the oracle, then the DEFAULT widths (n_filters = 4, conv_layers = 3: 28- and 76-channel
    bottlenecks, 51 -> 102 channel heads) with seeded weights against the oracle (which make_golden.py pinned on the reference at those
    widths too)."""
    net, opt = make_net(gold_denseblock)
    assert net.denseblock
    x = torch.from_numpy(gold_denseblock["x"]).to(DEV)
    seq = torch.from_numpy(gold_denseblock["seq_length"]).to(DEV)
    for got, name in zip(net(x, seq), ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_denseblock[name]) < TOL, name
    g = torch.Generator().manual_seed(48)
    sd = golden_state_dict(gold_denseblock, torch.float64)
    for B, T in ((5, 76), (1, 33), (2, 151)):
        x2 = torch.rand((B, 1, 288, T), generator=g) * 2.5
        seq2 = torch.randint(T - 6, T + 1, (B,), generator=g)
        ref = pcnet_oracle.pcnet_forward(sd, x2.double(), seq2)
        for a, b in zip(net(x2.to(DEV), seq2.to(DEV)), ref):
            assert rel_err(a.cpu(), b) < TOL, (B, T)
    # train mode (batch statistics; gradients and running statistics: tests/test_gpu_backward.py::test_denseblock_*)
    ref_t = pcnet_oracle.pcnet_forward(sd, x.double().cpu(), seq.cpu(), training=True)
    with torch.no_grad():
        for a, b in zip(net.train()(x, seq), ref_t):
            assert rel_err(a.cpu(), b) < TOL
    net.eval()
    # default widths
    torch.manual_seed(7)
    big = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True, denseblock=True))
    gb = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for name, buf in big.named_buffers():                       # non-trivial running statistics, as make_golden.py does
            if name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=gb) * 0.2)
            elif name.endswith("running_var"):
                buf.copy_(torch.rand(buf.shape, generator=gb) * 1.5 + 0.5)
        for name, p in big.named_parameters():
            if p.dim() == 1 and ("norm" in name or "_b." in name or name.split(".")[-2].isdigit()):
                p.copy_(torch.rand(p.shape, generator=gb) + 0.5 if name.endswith("weight") else torch.randn(p.shape, generator=gb) * 0.1)
    sd_big = {k: (v.detach().double().clone() if v.is_floating_point() else v.clone()) for k, v in big.state_dict().items()}
    big = big.to(DEV).eval()
    x3 = torch.rand((3, 1, 288, 60), generator=g) * 2.5
    seq3 = torch.tensor([60, 51, 44])
    ref = pcnet_oracle.pcnet_forward(sd_big, x3.double(), seq3)
    for a, b in zip(big(x3.to(DEV), seq3.to(DEV)), ref):
        assert rel_err(a.cpu(), b) < TOL


@pytest.mark.parametrize("variant", ["resblock", "pc2p_mem", "p2pc_conv", "stay_sixth", "local"])
def test_variants_keep_the_circular_shift_equivariance(variant, gold_default, gold_resblock, gold_pc2pmem, gold_p2pcconv, gold_staysixth):
    """The invariant of equivariance_test.py on every built variant: rolling the CQT by 3 s bins (one semitone = 3 bins) rolls the key and
    tonic outputs by s pitch classes.  (--pc2p_mem: its reshape ties eight CONSECUTIVE rows to one third-semitone index,
    models.py:158-162, so the semitone roll is not guaranteed by construction -- with these weights it still holds to 1e-6 -- and only
    the octave roll is asserted.)"""
    gold = {"resblock": gold_resblock, "pc2p_mem": gold_pc2pmem, "p2pc_conv": gold_p2pcconv, "stay_sixth": gold_staysixth, "local": gold_default}[variant]
    net, _ = make_net(gold, **({"local": True} if variant == "local" else {}))
    g = torch.Generator().manual_seed(5)
    T = 120 if variant == "local" else 40
    x = (torch.rand((2, 1, 288, T), generator=g) * 2.5).to(DEV)
    k0, t0 = net(x, None)[:2]
    pc_axis = 2 if variant == "local" else 1
    for s_ in ((12,) if variant == "pc2p_mem" else (1, 5, 11)):
        k1, t1 = net(torch.roll(x, 3 * s_, dims=2), None)[:2]
        if variant == "local":                                     # per-frame outputs in the reference's reshape order: undo it first
            unr = lambda a: a.reshape(a.shape[0], 12, -1)
            assert (unr(k1) - torch.roll(unr(k0), s_, dims=1)).abs().max() <= 1e-5
            assert (unr(t1) - torch.roll(unr(t0), s_, dims=1)).abs().max() <= 2e-5 * float(t0.abs().max())
        else:
            assert (k1 - torch.roll(k0, s_, dims=pc_axis)).abs().max() <= 1e-5, s_
            assert (t1 - torch.roll(t0, s_, dims=pc_axis)).abs().max() <= 2e-5 * max(1.0, float(t0.abs().max())), s_


def test_edge_shapes(gold_default):
    net, _ = make_net(gold_default)
    sd = golden_state_dict(gold_default, torch.float64)
    g = torch.Generator().manual_seed(1)
    # minimum length, odd lengths, long clips (time tiling; from 500 frames on the heads' 32 -> 1 conv needs more than one time tile:
    # its patch rows were once wider than the loader's 192 frames, and the last frames of the maps came out wrong)
    for B, T in ((1, 26), (1, 27), (2, 33), (1, 151), (1, 300), (1, 500), (2, 1000), (1, 1501)):
        x = torch.rand((B, 1, 288, T), generator=g) * 2.5
        ref = pcnet_oracle.pcnet_forward(sd, x.double(), None)
        got = net(x.to(DEV), None)
        for a, b in zip(got, ref):
            assert rel_err(a.cpu(), b) < TOL, (B, T)
    with pytest.raises(ake_amd._lib.AkeError, match="too short"):
        net(torch.zeros(1, 1, 288, 24, device=DEV), None)                 # T/2 - 12 <= 0 frames left for the heads
    # seq_length shorter than the heads' receptive field -> mean over an empty slice = NaN, as torch.mean does
    out = net(torch.rand(1, 1, 288, 76, device=DEV), torch.tensor([24], device=DEV))
    assert torch.isnan(out[1]).all()


def test_f32x3_precision_against_the_reference_fixtures(gold_default, gold_taps):
    """opt.precision = "f32x3" (ake_pcnet_config::precision = AKE_PRECISION_F32X3): no operand rounded below 2^-17 --
    the outputs AND every tap inside the pitch stack (1e-3 in the default "mixed" mode, one f16 rounding unit) are held to 1e-4 of the
    reference fixture; the handle reports the mode it runs."""
    net, _ = make_net(gold_default, precision="f32x3")
    assert net.precision == 1 and "exact f32" in net.precision_dtype()
    x = torch.from_numpy(gold_default["x"]).to(DEV)
    seq = torch.from_numpy(gold_default["seq_length"]).to(DEV)
    for got, name in zip(net(x, seq), ("key", "tonic", "genre")):
        assert rel_err(got.cpu(), gold_default[name]) < 2e-5, name
    for got, name in zip(net(x, None), ("key_noseq", "tonic_noseq", "genre_noseq")):
        assert rel_err(got.cpu(), gold_default[name]) < 2e-5, name
    was = net.keep_taps(True)
    try:
        xt = torch.from_numpy(gold_taps["x"]).to(DEV)
        outs = net(xt, torch.from_numpy(gold_taps["seq_length"]).to(DEV))
        for got, n in zip(outs, ("key", "tonic", "genre")):
            assert rel_err(got.cpu(), gold_taps[n]) < 2e-5
        for name in ("model.0.pool", "model.0.pc2pc.layer.2", "model.0.pc2pc.layer.5", "model.1.up_sixth_a", "model.1.p2p.layer.5",
                     "model.1.p2p.layer.8", "model.1.pc2pc.layer.5", "model.1.pc2pc.layer.8", "model.1.time_pool_pc", "key_map", "tonic_map",
                     "genre_map"):
            assert rel_err(net.tap(name).cpu().numpy(), gold_taps["tap/" + name]) < TOL, name
    finally:
        net.keep_taps(was)
    mixed, _ = make_net(gold_default)
    assert mixed.precision == 0 and "f16 activations x f16 weights" in mixed.precision_dtype()


def test_f32x3_precision_at_the_bench_shape():
    """256-clip batches of 76 frames (the persistent / fused kernels' shapes) in both precisions against the float64 oracle on 8 of the clips."""
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5, octaves=8, num_layers=2, kernel_size=7)
    torch.manual_seed(21)
    base = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 1.5)
    sd = {k: v.clone() for k, v in base.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    x = torch.rand((256, 1, 288, 76), generator=g) * 2.5
    seq = torch.randint(60, 77, (256,), generator=g)
    pick = [0, 15, 16, 100, 127, 128, 254, 255]
    ref = pcnet_oracle.pcnet_forward(pcnet_oracle.to_dtype(sd, torch.float64), x[pick].double(), seq[pick])
    errs = {}
    for prec in ("mixed", "f32x3"):
        o = Namespace(**vars(opt), precision=prec)
        net = ake_amd.PitchClassNet(288, 12, 2, 7, o)
        net.load_state_dict(sd, strict=True)
        out = net.to(DEV).eval()(x.to(DEV), seq.to(DEV))
        errs[prec] = max(rel_err(a[pick].cpu(), b) for a, b in zip(out, ref))
    print("\nmax rel err vs float64 at 256 x 76:", errs)
    assert errs["mixed"] < TOL and errs["f32x3"] < 2e-5, errs
