"""PARITY (GPU): a layer's three 7x7 pitch convs as ONE launch (p2p_stack_kernel: a workgroup of 16 waves owns a clip and walks conv
after conv, a workgroup barrier between them) against the routes that launch each conv on its own.

The one-launch route is taken when a chunk fills the machine with one clip per workgroup (no more clips than CUs, at most one CU in
sixteen idle); it multiplies the same numbers in the same order as conv_p2p_f16_ps_kernel (8 waves, one launch per conv) and
conv_p2p_f16_kernel (one workgroup per tile) -- only the tile height differs -- so every comparison between routes is torch.equal.
Which route a forward took is read from the kernel timer: all of them book their launches as "conv_p2p_f16_kernel", so the count is
1 for the one-launch route and 3 for the others.  Batch sizes follow the device's CU count N.

Tile geometry of the cases (288 rows): T = 76: 20-row tiles, 14 x 20 + 8 (ragged last tile of the first two convs), the folding conv
18 rows = 16 tiles; T = 52: 29-row tiles, 9 x 29 + 27, fold 18; T = 30, N - N/16 clips (grid below the CU count): 51-row tiles, fold 36.
"""
import json
from argparse import Namespace

import pytest
import torch

import ake_amd
from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-4          # test_gpu_pcnet.TOL
DEV = "cuda:0"
KEY = "conv_p2p_f16_kernel"


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def make_net(gold):
    opt = Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return net.to(DEV).eval()


def inputs(B, T):
    """As test_gpu_pcnet.test_persistent_pitch_conv_equals_per_tile_kernel_and_oracle."""
    g = torch.Generator().manual_seed(100 + T)
    x = (torch.rand((B, 1, 288, T), generator=g) * 2.5).to(DEV)
    seq = torch.randint(26, T + 1, (B,), generator=g).to(DEV)
    return x, seq


def forward_timed(net, x, seq, tap=True):
    """One forward under the kernel timer -> ((key, tonic, genre, tap model.1.cat), launches booked as conv_p2p_f16_kernel); tap=False:
    without the tap (a batch beyond the pitch stream's chunk has none)."""
    ake_amd._lib.prof_results()                                    # (reset)
    ake_amd._lib.prof_enable("", True)
    try:
        key, tonic, genre = net(x, seq)
        res = ake_amd._lib.prof_results()
    finally:
        ake_amd._lib.prof_enable("", False)
    return (key, tonic, genre) + ((net.tap("model.1.cat").clone(),) if tap else ()), res[KEY][1]


def assert_rows_equal(part, whole, rows, what):
    for name, a, b in zip(("key", "tonic", "genre", "model.1.cat"), part, whole):
        assert torch.equal(a, b[rows]), (what, name)


def check_against_separate_launches(net, x, seq, whole):
    """The same clips as two halves (conv_p2p_f16_ps_kernel, 3 launches) and the first, a middle and the last group of four
    (conv_p2p_f16_kernel, 3 launches)."""
    B = x.shape[0]
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        part, launches = forward_timed(net, x[lo:hi], seq[lo:hi])
        assert launches == 3, (lo, hi, launches)
        assert_rows_equal(part, whole, slice(lo, hi), f"half {lo}:{hi}")
    for lo in (0, (B // 2) // 4 * 4, B - 4):
        part, launches = forward_timed(net, x[lo:lo + 4], seq[lo:lo + 4])
        assert launches == 3, (lo, launches)
        assert_rows_equal(part, whole, slice(lo, lo + 4), f"clips {lo}:{lo + 4}")


@pytest.fixture(scope="module")
def bench_shape(gold_default):
    """N clips of 76 frames through the one-launch route, computed once: (net, x, seq, outputs)."""
    net = make_net(gold_default)
    x, seq = inputs(n_cus(), 76)
    whole, launches = forward_timed(net, x, seq)
    print(f"  T=76 B={n_cus()}: {launches} launch(es)")
    assert launches == 1, launches
    return net, x, seq, whole


def test_one_launch_equals_separate_launches_at_the_bench_shape(bench_shape):
    net, x, seq, whole = bench_shape
    check_against_separate_launches(net, x, seq, whole)


@pytest.mark.parametrize("T,fewer", [(52, 0), (30, 1)])
def test_other_frame_counts_and_a_grid_below_the_cu_count(gold_default, T, fewer):
    """A shape the plan declines shows 3 launches and must still pass."""
    net = make_net(gold_default)
    B = n_cus() - (n_cus() // 16 if fewer else 0)
    x, seq = inputs(B, T)
    whole, launches = forward_timed(net, x, seq)
    print(f"  T={T} B={B}: {launches} launch(es)")
    assert launches in (1, 3), launches
    check_against_separate_launches(net, x, seq, whole)


def test_another_shape_than_the_bench_shape_takes_the_one_launch_route(gold_default):
    net = make_net(gold_default)
    N = n_cus()
    taken = [forward_timed(net, *inputs(B, T))[1] == 1 for B, T in ((N, 52), (N - N // 16, 30))]
    assert any(taken), taken


def test_batches_outside_the_gate_take_the_separate_launches(bench_shape):
    """N + 1 clips (more clips than CUs; past the pitch stream's chunk they run as two chunks of 3 launches each) and N - N/8 clips
    (too many idle CUs): one launch per conv, and every clip equals its result in the one-launch batch."""
    net, x, seq, whole = bench_shape
    N = n_cus()
    x1 = (torch.rand((1, 1, 288, 76), generator=torch.Generator().manual_seed(7)) * 2.5).to(DEV)
    seq1 = torch.tensor([61], device=DEV)
    got, launches = forward_timed(net, torch.cat([x, x1]), torch.cat([seq, seq1]), tap=False)        # (outputs only)
    assert launches in (3, 6), launches
    assert_rows_equal([t[:N] for t in got], whole, slice(0, N), "N + 1")
    alone, _ = forward_timed(net, torch.cat([x[N - 3:], x1]), torch.cat([seq[N - 3:], seq1]))      # (four clips: the per-tile kernel)
    assert_rows_equal([t[3:] for t in alone], got, slice(N, N + 1), "clip N")
    B = N - N // 8
    got, launches = forward_timed(net, x[:B], seq[:B])
    assert launches == 3, launches
    assert_rows_equal(got, whole, slice(0, B), "N - N/8")


def test_keep_taps_keeps_the_separate_launches(gold_default, bench_shape):
    """ake_debug_keep_taps(1) writes every nameable activation: three launches, the semitone conv on its own f32 kernel (one rounding
    less than the fused form, so these outputs are not the fused ones bit for bit: test_gpu_pcnet holds the two taps to 1e-3).  Held
    equal to the same clips as halves under the same switch, to the fused tap at that 1e-3, in key, tonic and genre of all clips to the
    one launch's within 2 TOL, and three clips to the oracle at TOL."""
    net, x, seq, whole = bench_shape
    was = net.keep_taps(True)
    try:
        kept, launches = forward_timed(net, x, seq)
        assert launches == 3, launches
        h = x.shape[0] // 2
        for lo, hi in ((0, h), (h, x.shape[0])):
            part, _ = forward_timed(net, x[lo:hi], seq[lo:hi])
            assert_rows_equal(part, kept, slice(lo, hi), f"keep_taps half {lo}:{hi}")
    finally:
        net.keep_taps(was)
    assert rel_err(whole[3].cpu(), kept[3].cpu()) < 1e-3
    # key, tonic and genre of every clip: both routes are held to the float64 oracle at TOL, so they stand within 2 TOL of each other
    for name, a, b in zip(("key", "tonic", "genre"), whole[:3], kept[:3]):
        e = rel_err(a.cpu(), b.cpu())
        print(f"  keep_taps vs one launch, {name}: {e:.2e}", end="")
        assert e < 2 * TOL, (name, e)
    idx = [0, x.shape[0] // 2, x.shape[0] - 1]
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), x[idx].cpu().double(), seq[idx].cpu())
    for a, b in zip(kept[:3], ref):
        assert rel_err(a[idx].cpu(), b) < TOL
    again, launches = forward_timed(net, x, seq)                    # the switch is off again: one launch, the same bits as before
    assert launches == 1
    assert_rows_equal(again, whole, slice(0, x.shape[0]), "after keep_taps")


def test_three_clips_against_the_float64_oracle(gold_default, bench_shape):
    net, x, seq, whole = bench_shape
    idx = [0, x.shape[0] // 2, x.shape[0] - 1]
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), x[idx].cpu().double(), seq[idx].cpu())
    for name, a, b in zip(("key", "tonic", "genre"), whole[:3], ref):
        e = rel_err(a[idx].cpu(), b)
        print(f"  {name}: {e:.2e}", end="")
        assert e < TOL, (name, e)
