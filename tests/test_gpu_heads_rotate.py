"""PARITY (GPU): the last convolution of the circular heads with the 12 output pitch classes as the MFMA's N dimension
(head1_multiply_store: 84 dense k-steps (input row r, tap dx) and B[ci][y] = w[ci][(r - y) mod 12][dx], instead of 264 Toeplitz-in-time
k-steps of which 15 in 22 were zeros), in the fused launch (heads_fused_kernel) and in the two launches (conv_head1_bf16_kernel).

Both paths against the float64 oracle at the bounds test_gpu_heads_fused.py holds them to (TOL; an f32x3 net: outputs at that mode's
2e-5, maps at TOL as that mode's own tests hold them), the path read from the kernel timer.  Frame counts: 44 (hidden map 16 frames,
finished map 10: one frame block), 76 (32 -> 26: two frame blocks), 48 and 80 (hidden maps of 18 and 34 frames: M-tiles of the first
conv that straddle rows), 28 (finished map of 2 frames).

The two paths share one body and agree bit for bit wherever they read the same features: test_the_two_paths_agree_bit_for_bit.

The fixture's head weights barely respond to the input, so a wrong (r - y) mod 12 could hide below TOL of the map's maximum: two cases
redraw the head convolutions from a seeded normal and scale the last one so that every map has unit spread over its positions.
"""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
import sensitive
from conftest import golden_state_dict
from oracle import pcnet_oracle
from test_gpu_heads_fused import DEV, MAPS, TOL_F32X3, both_paths, forward_timed, assert_path, make_net

pytestmark = pytest.mark.gpu
FEATURES = "model.1.time_pool_pc"      # the pooled features both heads' paths read

HEAD_CONVS = {"key_map": ("key_classifier.0.conv2d.weight", "key_classifier.3.conv2d.weight", "key_classifier.3.conv2d.bias"),
              "tonic_map": ("tonic_classifier.0.conv2d.weight", "tonic_classifier.3.conv2d.weight", "tonic_classifier.3.conv2d.bias"),
              "genre_map": ("genre_classifier.0.weight", "genre_classifier.3.weight", "genre_classifier.3.bias")}


def batch(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 1, 288, T), generator=g) * 2.5
    seq = torch.randint(26, T + 1, (B,), generator=g)
    return x, seq


@pytest.mark.parametrize("T", [44, 76, 48, 80, 28])
@pytest.mark.parametrize("B", [1, 3])
def test_both_paths_against_the_oracle(gold_default, B, T):
    net, sd64 = make_net(gold_default)
    x, seq = batch(B, T, 7000 + 10 * T + B)
    both_paths(net, sd64, x, seq, list(range(B)))
    both_paths(net, sd64, x, None, list(range(B)))


STACK_CONVS = tuple(f"model.1.pc2pc.layer.{j}.conv2d.weight" for j in (0, 3, 6))
SEMI_CONV = "model.1.pool_semi.weight"


def order_free_stack_net(gold, seed):
    """A net whose layers in front of the heads give the same bits on both routes, so that the heads' two paths can be compared bit
    for bit.  keep_taps(True) is the only switch to the heads' two launches, and it unfuses what stands in front of them as well:
    the last pitch conv no longer runs the semitone conv on its own tiles (the stack's input `model.1.cat` then differs by 1.4e-4
    between the routes), and the last pitch-class stack leaves its one launch, which walks the k-steps in another order than
    conv_pc_bf16_kernel.  On the fixture's dense weights the heads of the two paths therefore never read the same features: measured
    at 44 / 76 / 80 frames the pooled features differ by 7.8e-6 / 9.8e-6 / 9.7e-6, the maps by 1.1e-6 .. 2.1e-6 (the genre map,
    whose code has one form, included) and the outputs by 1.2e-7 .. 9.9e-7, with the same figures on the code before the dense last
    convolution.  Here (a) the semitone conv's weights are zero, so its eight channels are BatchNorm(bias) on either route, and (b)
    every output channel of the three convolutions of the stack has ONE tap (one input channel, one kernel row, one column; a seeded
    normal value): an output is the sum of one weight's three split products and zeros, the same float32 number in whatever order
    a kernel walks its k-steps.  Everything else in front of the heads is pointwise or a maximum.  The features still follow the input
    through the four channels that come from layer 0."""
    opt = Namespace(**json.loads(str(gold["opt"])))
    sd = golden_state_dict(gold)
    g = torch.Generator().manual_seed(seed)
    for k in STACK_CONVS:
        w = torch.zeros_like(sd[k])
        co, ci, kh, kw = w.shape
        for o in range(co):
            pick = [int(torch.randint(0, n, (1,), generator=g)) for n in (ci, kh, kw)]
            w[o, pick[0], pick[1], pick[2]] = float(torch.randn((), generator=g))
        sd[k] = w
    sd[SEMI_CONV] = torch.zeros_like(sd[SEMI_CONV])
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


@pytest.mark.parametrize("T", [44, 76, 80])
def test_the_two_paths_agree_bit_for_bit(gold_default, T):
    """Fused == two launches, torch.equal on outputs and maps, on features that are themselves equal bit for bit (asserted first, and
    that they vary over the frames): see order_free_stack_net."""
    net = order_free_stack_net(gold_default, 7150 + T)
    x, seq = batch(3, T, 7100 + T)
    outs, res = forward_timed(net, x.to(DEV), seq.to(DEV))
    assert_path(res, True)
    maps = {name: net.tap(name).clone() for name in MAPS + (FEATURES,)}
    feat = maps[FEATURES]
    assert float(feat.std(dim=3).max()) > 1e-3 * float(feat.abs().max()) > 0     # (the features are no constants)
    was = net.keep_taps(True)
    try:
        outs_k, res = forward_timed(net, x.to(DEV), seq.to(DEV))
        assert_path(res, False)
        assert torch.equal(net.tap(FEATURES), feat), float((net.tap(FEATURES) - feat).abs().max())
        differ = [name for name in MAPS if not torch.equal(net.tap(name), maps[name])]
        differ += [name for name, a, b in zip(("key", "tonic", "genre"), outs, outs_k) if not torch.equal(a, b)]
        for name in differ:
            a, b = (net.tap(name), maps[name]) if name in maps else (outs_k[("key", "tonic", "genre").index(name)], outs[("key", "tonic", "genre").index(name)])
            print(f"  {name}: max |two launches - fused| {float((a - b).abs().max()):.2e}", end="")
        assert not differ, differ
    finally:
        net.keep_taps(was)


def responding_net(gold, x, seed):
    """An f32x3 net on the fixture with BatchNorm statistics calibrated on `x` (tests/sensitive.py: the features the heads read then vary
    as much as they are large) and the heads' convolutions redrawn from a seeded normal.  The first convolution of a head is scaled per
    channel, and its bias set, so that its output has the mean and variance its BatchNorm holds; the last one so that the map has unit
    spread over its positions (float64 oracle, on `x`)."""
    opt = Namespace(**json.loads(str(gold["opt"])))
    opt.precision = "f32x3"
    sd = sensitive.calibrate(pcnet_oracle.to_dtype(golden_state_dict(gold), torch.float64), x.double(), None)
    g = torch.Generator().manual_seed(seed)
    feat = pcnet_oracle.forward_features(sd, x.double(), opt.time_pool_size, False, None)[1]
    for name, (first, last, last_bias) in HEAD_CONVS.items():
        for k in (first, last):
            sd[k] = torch.randn(sd[k].shape, generator=g).double()
        if name == "genre_map":
            z = torch.nn.functional.conv2d(feat, sd[first])
        else:
            z = pcnet_oracle.equiv_pc_conv(feat, sd[first], None, same=False)
        bn = first.split(".")[0] + ".1."
        scale = (sd[bn + "running_var"] + 1e-5).sqrt() / z.std(dim=(0, 2, 3))
        sd[first] = sd[first] * scale[:, None, None, None]
        sd[first.replace("weight", "bias")] = sd[bn + "running_mean"] - scale * z.mean(dim=(0, 2, 3))
    taps = {}
    pcnet_oracle.pcnet_forward(sd, x.double(), None, taps=taps)
    for name, (_, last, last_bias) in HEAD_CONVS.items():
        spread = float((taps[name] - sd[last_bias].item()).std())
        assert spread > 0, name
        sd[last] = sd[last] / spread
    sd32 = pcnet_oracle.to_dtype(sd, torch.float32)              # what the device holds; the reference is float64 on the same values
    sd64 = pcnet_oracle.to_dtype(sd32, torch.float64)
    taps = {}
    ref = pcnet_oracle.pcnet_forward(sd64, x.double(), None, taps=taps)
    sensitive.assert_responds(sd64, x.double(), None, ref, what="redrawn heads")
    for name in MAPS:                                              # O(1) maps whose spread over the positions is a good part of their maximum
        m = taps[name].numpy()
        print(f"  {name}: std {m.std():.2f} max {np.abs(m).max():.2f}", end="")
        assert 0.9 < m.std() < 1.1 and np.abs(m).max() < 8, name
    print()
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(sd32, strict=True)
    net = net.to(DEV).eval()
    assert net.precision == 1
    return net, sd64


@pytest.mark.parametrize("T", [76, 44])
def test_responding_maps_on_both_paths(gold_default, T):
    """Outputs and maps at TOL.  The net is an f32x3 one (the heads' kernels are the same in both modes) because `mixed` cannot be held to
    TOL on weights that respond: the float64 oracle under the rounding model of the `mixed` route (pcnet_oracle.rounding_model: the f16
    operands of the layers in front of the heads) is 5e-4 .. 4e-3 away from the plain float64 oracle on these weights, and a `mixed` device
    forward measured 8.5e-4 (76 frames) and 4.6e-4 (44) on the key output.  Under the f32x3 route the model is 9e-6 .. 3.4e-5 away."""
    x, seq = batch(3, T, 7200 + T)
    net, sd64 = responding_net(gold_default, x, 7300 + T)
    both_paths(net, sd64, x, seq, [0, 1, 2])


def test_f32x3_net(gold_default):
    net, sd64 = make_net(gold_default, precision="f32x3")
    assert net.precision == 1
    x, seq = batch(3, 76, 7400)
    both_paths(net, sd64, x, seq, [0, 1, 2], tol=TOL_F32X3)


def test_without_the_genre_head(gold_default):
    net, sd64 = make_net(gold_default, genre=False)
    x, seq = batch(3, 44, 7500)
    ((outs, _), _) = both_paths(net, sd64, x, seq, [0, 1, 2])
    assert len(outs) == 2
