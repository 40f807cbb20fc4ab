"""PARITY (GPU): the last pitch-class stack + its time pooling as one launch (pc2pc_fused_kernel: weight chunks through a ring of three
LDS slots by LDS-DMA two chunks ahead, a kernel row's fragment registers refilled as the row retires, only the halo frames zeroed,
packed bf16 splits in the epilogues), against the float64 oracle on `model.1.time_pool_pc` and the three outputs.

Frame counts: 4 (one frame tile, three active waves; the heads refuse so short a clip AFTER the stack has run, so only the tap is
read), 16, 20 (a ragged second tile), 76, 80 (five full tiles, the largest LDS need), 84 (six tiles: the per-conv launches).
`conv_layers` 1, 2 and 4: odd and even ping-pong, the ring handed from conv to conv zero, one and three times.  The stack's input has
12 channels in every net that fuses (n_filters = 4: 4 from layer 0 + 8 from the semitone conv; other widths do not give the 16 output
channels the launch needs), so channels 12 .. 15 of the first map are the zeros the conversion writes in every case here.

Bounds: 1e-4 of the tensor's maximum (tests/test_gpu_heads_rotate.py) on an `f32x3` net with seeded weights and BatchNorm statistics
calibrated on the input, so that the pooled features vary over the frames as much as they are large; the fixture net in `mixed` at TOL
of tests/test_gpu_pcnet.py.  Every case reads from the kernel timer which route ran.  A misplaced DMA wait or ring slot shows as wrong
values here, not as a hang: the launch has no wait between workgroups.
"""
import json
from argparse import Namespace

import pytest
import torch

import ake_amd
import sensitive
from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4                  # test_gpu_pcnet.TOL, test_gpu_heads_fused.TOL
TOL_PAIR = 1e-3             # test_gpu_pcnet.test_every_layer_against_reference_taps: the fused route against ake_debug_keep_taps(1)
FEATURES = "model.1.time_pool_pc"
FUSED, PER_CONV = "pc2pc_fused_kernel", "conv_pc_bf16_kernel/pc2pc"
OUTPUTS = ("key", "tonic", "genre")


def batch(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, 1, 288, T), generator=g) * 2.5


def forward_timed(net, x, expect_too_short=False):
    """One forward under the kernel timer -> (outputs or None, {kernel name: (ms, launches)})."""
    ake_amd._lib.prof_results()                                    # (reset)
    ake_amd._lib.prof_enable("", True)
    try:
        if expect_too_short:
            with pytest.raises(ake_amd._lib.AkeError, match="too short"):
                net(x, None)
            outs = None
        else:
            outs = net(x, None)
        res = ake_amd._lib.prof_results()
    finally:
        ake_amd._lib.prof_enable("", False)
    return outs, res


def assert_route(res, fused):
    names = set(res)
    if fused:
        assert FUSED in names and PER_CONV not in names, sorted(names)
        assert res[FUSED][1] == 1, res[FUSED]
    else:
        assert PER_CONV in names and FUSED not in names, sorted(names)


_CACHE = {}


def seeded_net(conv_layers, head_layers, T, B):
    """An `f32x3` net of seeded weights whose BatchNorm running statistics are those of the case's own input (clips of at least 28 frames
    for the calibration: the oracle's heads need them) -> (net on the device, float64 state_dict, input)."""
    key = (conv_layers, head_layers, T, B)
    if key not in _CACHE:
        opt = Namespace(conv_layers=conv_layers, n_filters=4, head_layers=head_layers, time_pool_size=2, genre=True, max_pool=False, frames=5,
                        precision="f32x3")
        torch.manual_seed(8100 + 10 * conv_layers + head_layers)
        net = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
        x = batch(B, T, 8200 + 10 * T + B)
        sd = pcnet_oracle.to_dtype({k: v.detach().clone() for k, v in net.state_dict().items()}, torch.float64)
        sd = sensitive.calibrate(sd, (x if T >= 28 else batch(3, 28, 8300 + T)).double(), None, head_layers=head_layers)
        sd32 = pcnet_oracle.to_dtype(sd, torch.float32)            # what the device holds; the reference is float64 on the same values
        net.load_state_dict(sd32, strict=True)
        net = net.to(DEV).eval()
        assert net.precision == 1
        _CACHE.clear()                                             # (one net at a time stays alive)
        _CACHE[key] = (net, pcnet_oracle.to_dtype(sd32, torch.float64), x)
    return _CACHE[key]


def check_features(net, sd64, x, tol):
    taps = {}
    pcnet_oracle.forward_features(sd64, x.double(), 2, False, taps)
    ref = taps[FEATURES]
    got = net.tap(FEATURES).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = rel_err(got, ref)
    print(f"  {FEATURES}: {e:.2e} (max {float(ref.abs().max()):.2f})", end="")
    assert e < tol, e
    return ref


def check_outputs(outs, sd64, x, tol, **oracle_kw):
    ref = pcnet_oracle.pcnet_forward(sd64, x.double(), None, **oracle_kw)
    assert len(outs) == len(ref)
    for name, a, b in zip(OUTPUTS, outs, ref):
        e = rel_err(a.cpu(), b)
        print(f"  {name}: {e:.2e}", end="")
        assert e < tol, (name, e)
    print()


def run_seeded(conv_layers, T, B):
    head_layers = 2 if T >= 28 else 1                             # (a head conv takes 6 of the T / 2 pooled frames)
    net, sd64, x = seeded_net(conv_layers, head_layers, T, B)
    outs, res = forward_timed(net, x.to(DEV))
    assert_route(res, T <= 80)
    ref = check_features(net, sd64, x, TOL)
    assert float(ref.std(dim=3).max()) > 100 * TOL * float(ref.abs().max()) > 0     # the features follow the input over the frames
    check_outputs(outs, sd64, x, TOL, head_layers=head_layers)


@pytest.mark.parametrize("T", [16, 20, 76, 80, 84])
@pytest.mark.parametrize("B", [1, 3])
def test_seeded_f32x3_net_against_the_oracle(B, T):
    run_seeded(3, T, B)


@pytest.mark.parametrize("conv_layers", [1, 2, 4])
@pytest.mark.parametrize("B,T", [(3, 20), (1, 76)])
def test_other_stack_depths(conv_layers, B, T):
    run_seeded(conv_layers, T, B)


@pytest.mark.parametrize("B", [1, 3])
def test_four_frames(B):
    """One frame tile of which 4 frames are stored, 3 of 16 waves active.  2 pooled frames are too few for the heads, which refuse the
    clip when their first conv is reached: the stack has run by then (the kernel timer says so) and its tap is there to read."""
    net, sd64, x = seeded_net(3, 2, 4, B)
    _, res = forward_timed(net, x.to(DEV), expect_too_short=True)
    assert_route(res, True)
    net._last_shape = (B, 4)                                       # (what a forward that returns leaves behind for `tap`)
    ref = check_features(net, sd64, x, TOL)
    assert float(ref.std(dim=3).max()) > 100 * TOL * float(ref.abs().max()) > 0
    print()


def fixture_net(gold):
    opt = Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return net.to(DEV).eval(), golden_state_dict(gold, torch.float64)


@pytest.mark.parametrize("T", [76, 80, 84])
@pytest.mark.parametrize("B", [1, 3])
def test_fixture_net_in_mixed_precision(gold_default, B, T):
    net, sd64 = fixture_net(gold_default)
    assert net.precision == 0
    x = batch(B, T, 8400 + 10 * T + B)
    outs, res = forward_timed(net, x.to(DEV))
    assert_route(res, T <= 80)
    check_features(net, sd64, x, TOL)
    check_outputs(outs, sd64, x, TOL)


def test_fused_against_the_per_conv_launches(gold_default):
    """The one launch against ake_debug_keep_taps(1).  The two routes add in different orders (and keep_taps unfuses the layers in front
    as well), so they were never bit-equal: the tolerance is the one test_gpu_pcnet holds this pair to."""
    net, _ = fixture_net(gold_default)
    x = batch(3, 76, 8500).to(DEV)
    outs, res = forward_timed(net, x)
    assert_route(res, True)
    feat = net.tap(FEATURES).clone()
    was = net.keep_taps(True)
    try:
        outs_k, res = forward_timed(net, x)
        assert_route(res, False)
        e = rel_err(feat.cpu(), net.tap(FEATURES).cpu())
        print(f"  {FEATURES}: fused against per-conv {e:.2e}", end="")
        assert e < TOL_PAIR, e
        for name, a, b in zip(OUTPUTS, outs, outs_k):
            e = rel_err(a.cpu(), b.cpu())
            print(f"  {name}: {e:.2e}", end="")
            assert e < TOL_PAIR, (name, e)
        print()
    finally:
        net.keep_taps(was)
