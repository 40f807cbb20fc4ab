"""PARITY (GPU): the classifier heads as one launch (heads_fused_kernel: both convolutions of a head + the masked pooling, the 32 hidden
channels never leave the LDS) and as the two launches that remain for every other shape, ake_debug_keep_taps(1) and training
(conv_pc_bf16_kernel/head + conv_head1_bf16_kernel).

Both paths are held to the float64 oracle at the bound the other tests hold the same quantities to in "mixed" mode (TOL of
test_gpu_pcnet.py: outputs and the key / tonic / genre maps alike), and every case reads from the kernel timer which path ran, so a gate
that falls back cannot pass as a test of the fused launch.  The fused launch needs the last pitch-class stack to run fused as well
(frame counts that are multiples of 4 up to 80) and more than 24 frames.
"""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-4          # test_gpu_pcnet.TOL
TOL_F32X3 = 2e-5    # test_gpu_pcnet.test_f32x3_precision_against_the_reference_fixtures
DEV = "cuda:0"
FUSED = {"heads_fused_kernel"}
TWO_LAUNCH = {"conv_pc_bf16_kernel/head", "conv_head1_bf16_kernel"}
MAPS = ("key_map", "tonic_map", "genre_map")


def make_net(gold, **opt_kw):
    opt = Namespace(**json.loads(str(gold["opt"])))
    for k, v in opt_kw.items():
        setattr(opt, k, v)
    sd = golden_state_dict(gold)
    if not getattr(opt, "genre", True):
        sd = {k: v for k, v in sd.items() if not k.startswith("genre_classifier")}
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval(), {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def forward_timed(net, x, seq):
    """One forward under the kernel timer -> (outputs, {kernel name: (ms, launches)})."""
    ake_amd._lib.prof_results()                                    # (reset)
    ake_amd._lib.prof_enable("", True)
    try:
        outs = net(x, seq)
        res = ake_amd._lib.prof_results()
    finally:
        ake_amd._lib.prof_enable("", False)
    return outs, res


def assert_path(res, fused):
    names = set(res)
    if fused:
        assert FUSED <= names and not (TWO_LAUNCH & names) and "conv_pc_bf16_kernel/genre_head" not in names, sorted(names)
    else:
        assert TWO_LAUNCH <= names and not any(n.startswith("heads_fused_kernel") for n in names), sorted(names)
    assert "head_pool_kernel" not in names, sorted(names)           # the masked mean + sigmoid ride in the heads' launch on both paths


def err_with_nan(got, ref):
    """rel_err over the finite entries; the NaN entries (mean over an empty slice) must coincide."""
    got, ref = np.asarray(got.detach().cpu(), np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return rel_err(got[ok], ref[ok]) if ok.any() else 0.0


def check_against_oracle(net, sd64, x, seq, rows, fused, tol=TOL, tol_maps=TOL):
    """Forward on the whole batch; outputs and maps of `rows` against the float64 oracle; returns (outputs, maps) for further checks."""
    outs, res = forward_timed(net, x.to(DEV), None if seq is None else seq.to(DEV))
    assert_path(res, fused)
    taps = {}
    ref = pcnet_oracle.pcnet_forward(sd64, x[rows].double(), None if seq is None else seq[rows], taps=taps)
    assert len(outs) == len(ref)
    for name, a, b in zip(("key", "tonic", "genre"), outs, ref):
        e = err_with_nan(a[rows], b)
        print(f"  {name}: {e:.2e}", end="")
        assert e < tol, (name, e)
    maps = {}
    for name in MAPS[:len(ref)]:
        maps[name] = net.tap(name)
        b = taps[name].numpy()
        e = rel_err(maps[name][rows].cpu().numpy().reshape(b.shape), b)
        print(f"  {name}: {e:.2e}", end="")
        assert e < tol_maps, (name, e)
    print()
    return outs, maps


def both_paths(net, sd64, x, seq, rows, **kw):
    """The fused launch, then the same batch under keep_taps(True): the two launches, the same bound."""
    fused = check_against_oracle(net, sd64, x, seq, rows, True, **kw)
    was = net.keep_taps(True)
    try:
        plain = check_against_oracle(net, sd64, x, seq, rows, False, **kw)
    finally:
        net.keep_taps(was)
    return fused, plain


# 76: 32 -> 26 frames, two frame blocks in the last conv; 80: 34 -> 28, M-tiles of the first conv that straddle rows; 52: 20 -> 14, one
# frame block; 28: 8 -> 2, the smallest map
@pytest.mark.parametrize("T", [76, 80, 52, 28])
@pytest.mark.parametrize("B", [1, 3])
def test_small_batches_on_both_paths(gold_default, B, T):
    net, sd64 = make_net(gold_default)
    g = torch.Generator().manual_seed(1000 * B + T)
    x = torch.rand((B, 1, 288, T), generator=g) * 2.5
    seq = torch.randint(26, T + 1, (B,), generator=g)
    both_paths(net, sd64, x, seq, list(range(B)))
    both_paths(net, sd64, x, None, list(range(B)))                  # models.py:786-797: no seq_length, plain mean


@pytest.mark.parametrize("T", [76, 80, 52, 28])
def test_bench_batch_on_both_paths(gold_default, T):
    """256 clips: the first, the last and 14 seeded inner rows against the oracle; clips are independent, so reversing the batch
    reverses the rows of the outputs and of the maps bit for bit."""
    net, sd64 = make_net(gold_default)
    g = torch.Generator().manual_seed(5000 + T)
    x = torch.rand((256, 1, 288, T), generator=g) * 2.5
    seq = torch.randint(26, T + 1, (256,), generator=g)
    rows = sorted({0, 255} | set((1 + torch.randperm(254, generator=g)[:14]).tolist()))
    assert len(rows) == 16
    (outs, maps), _ = both_paths(net, sd64, x, seq, rows)
    rev = torch.arange(255, -1, -1)
    outs_r, res = forward_timed(net, x[rev].contiguous().to(DEV), seq[rev].to(DEV))
    assert_path(res, True)
    for a, b in zip(outs_r, outs):
        assert torch.equal(a, b[rev.to(DEV)])
    for name in MAPS:
        assert torch.equal(net.tap(name), maps[name][rev.to(DEV)]), name


def test_ragged_lengths_with_an_empty_slice(gold_default):
    """seq_length 24 and 25 leave 24 // 2 - 12 = 0 map frames: the mean over an empty slice is NaN, as torch.mean; 26 leaves one frame."""
    net, sd64 = make_net(gold_default)
    g = torch.Generator().manual_seed(31)
    x = torch.rand((6, 1, 288, 76), generator=g) * 2.5
    seq = torch.tensor([76, 24, 51, 26, 25, 63])
    ((outs, _), (outs_k, _)) = both_paths(net, sd64, x, seq, list(range(6)))
    for o in (outs, outs_k):
        for a in o:
            assert torch.isnan(a[[1, 4]]).all() and torch.isfinite(a[[0, 2, 3, 5]]).all()


@pytest.mark.parametrize("T", [76, 28])
def test_without_the_genre_head(gold_default, T):
    net, sd64 = make_net(gold_default, genre=False)
    g = torch.Generator().manual_seed(47 + T)
    x = torch.rand((3, 1, 288, T), generator=g) * 2.5
    seq = torch.randint(26, T + 1, (3,), generator=g)
    ((outs, _), _) = both_paths(net, sd64, x, seq, [0, 1, 2])
    assert len(outs) == 2


def test_local_net_keeps_the_two_launches(gold_default):
    """--local nets do not pool over time, so their last pitch-class stack does not run fused and the heads keep the two launches
    (the per-frame sliding maximum is local_pool_kernel's); 76 frames -> 64 map frames, window 38."""
    net, sd64 = make_net(gold_default, local=True)
    g = torch.Generator().manual_seed(53)
    x = torch.rand((3, 1, 288, 76), generator=g) * 2.5
    outs, res = forward_timed(net, x.to(DEV), None)
    names = set(res)
    assert TWO_LAUNCH <= names and "local_pool_kernel" in names and not any(n.startswith("heads_fused_kernel") for n in names), sorted(names)
    taps = {}
    ref = pcnet_oracle.pcnet_forward(sd64, x.double(), None, taps=taps, local_window=net.local_window)
    for a, b in zip(outs, ref):
        assert a.shape == b.shape and rel_err(a.cpu(), b) < TOL
    for name in MAPS:
        b = taps[name].numpy()
        assert rel_err(net.tap(name).cpu().numpy().reshape(b.shape), b) < TOL, name


def test_f32x3_net_takes_the_fused_launch(gold_default):
    """precision = "f32x3" shares the heads' bf16 kernels (three split products: f32-equivalent) and the same gate: outputs at that
    mode's bound, the maps at TOL as its own test holds them."""
    net, sd64 = make_net(gold_default, precision="f32x3")
    assert net.precision == 1
    g = torch.Generator().manual_seed(59)
    x = torch.rand((3, 1, 288, 76), generator=g) * 2.5
    seq = torch.tensor([76, 40, 61])
    both_paths(net, sd64, x, seq, [0, 1, 2], tol=TOL_F32X3)


def test_kernel_timer_names_the_fused_launch(gold_default):
    net, _ = make_net(gold_default)
    x = torch.rand((4, 1, 288, 76), generator=torch.Generator().manual_seed(3)) * 2.5
    _, res = forward_timed(net, x.to(DEV), None)
    assert "heads_fused_kernel" in res and "conv_head1_bf16_kernel" not in res
    assert res["heads_fused_kernel"][0] > 0 and sum(n for k, (_, n) in res.items() if k.startswith("heads_fused_kernel")) in (1, 2)
    _, res = forward_timed(net, torch.rand((2, 1, 288, 31), device=DEV) * 2.5, None)          # 31 frames: the stack does not fuse
    assert_path(res, False)
