"""GPU: layer 0's one-launch MFMA form (layer0_mfma_kernel) after its loaders, its LDS image and its multiply loop were rebuilt.

The kernel's arithmetic did not change, so everything here is held to what held before: the float64 oracle at test_gpu_pcnet's TOL,
bit equality between the two input orders and between the two hand-over formats, and the debug taps at _check_taps' bounds.  The
shapes are the smallest at which each rebuilt piece can go wrong:
  76 frames  the bench shape: whole frame quads only, 29 tiles over 8 waves
  86 frames  the edge of layer0_plan's LDS rule (the tiled image of a frames-major clip is largest here), two frames past the last quad
  77 frames  odd: rows that are not 16-byte aligned, one frame past the last quad, a ragged last tile
  27 frames  fewer tiles (11) than two per wave, an image smaller than the weight-fragment regions laid over it
All on tests/golden/pcnet_default.npz, input rand * 2.5 seeded per shape.  One more net, of one octave (36 bins, seeded weights): there
the maps, not the image, fill the LDS, and past 190 frames the weight-fragment regions no longer fit beside them.
"""
import functools
from argparse import Namespace

import pytest
import torch

import ake_amd
from conftest import golden_state_dict, load_golden, rel_err
from oracle import pcnet_oracle
from test_gpu_pcnet import TOL, make_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def net(gold_default):
    return make_net(gold_default)[0]


def _mel(B, T):
    g = torch.Generator().manual_seed(7000 + 100 * B + T)
    return torch.rand((B, 1, 288, T), generator=g) * 2.5


@functools.lru_cache(maxsize=None)
def _oracle(B, T):
    """(input, outputs, activations) of the float64 oracle, computed once per shape and shared by the tests below (read only)."""
    sd64 = golden_state_dict(load_golden("pcnet_default.npz"), torch.float64)
    x = _mel(B, T)
    taps = {}
    ref = pcnet_oracle.pcnet_forward(sd64, x.double(), torch.full((B,), T), taps=taps)
    return x, ref, taps


@pytest.mark.parametrize("B,T", [(3, 76), (3, 86), (3, 77), (2, 27)])
def test_parity_against_the_oracle(net, B, T):
    x, ref, _ = _oracle(B, T)
    seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
    ake_amd._lib.prof_enable("", True)
    try:
        outs = net(x.to(DEV), seq)
        launched = ake_amd._lib.prof_results()
    finally:
        ake_amd._lib.prof_enable("", False)
    if T == 86:
        assert "layer0_fused_kernel" in launched, sorted(launched)    # the one-launch form still takes the rule's last frame count
    for name, a, b in zip(("key", "tonic", "genre"), outs, ref):
        err = rel_err(a.cpu(), b)
        print(f"{B} x {T} {name}: {err:.2e}")
        assert err < TOL, (name, B, T, err)


def test_frames_major_equals_nchw(net):
    """The tiled image and its 16-byte transposed stores (frames-major) against the straight copy (NCHW): the same bits out."""
    L = ake_amd._lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ran = 0
    for B, T in ((24, 76), (24, 86)):
        x = _mel(B, T).to(DEV)
        seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
        want = net(x, seq)                                            # (also creates the handle)
        if not L.ake_pcnet_accepts_frames_major(net.handle, B, T):
            continue
        x_fm = x[:, 0].transpose(1, 2).contiguous()                   # [clip][frame][bin]
        outs = [torch.full((B, n), -7.0, dtype=torch.float32, device=DEV) for n in (12, 12, 11)]
        ws = torch.empty(L.ake_pcnet_workspace_bytes(net.handle, B, T), dtype=torch.uint8, device=DEV)
        ake_amd._lib.check(L.ake_pcnet_forward_frames_major_f32(net.handle, x_fm.data_ptr(), B, T, seq.data_ptr(), outs[0].data_ptr(),
                                                                 outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), ws.numel(), stream),
                           "ake_pcnet_forward_frames_major_f32")
        for name, a, b in zip(("key", "tonic", "genre"), outs, want):
            assert torch.equal(a, b), (name, B, T)
        ran += 1
    assert ran >= 1


def test_hand_over_formats_agree(net):
    """24 x 76 hands the persistent first pitch conv f16 words (melh, the up_sixth map as f16 x 4); four clips at a time hand the per-tile
    kernel the f32 map.  Same values either way: the outputs and layer 1's concat buffer are equal bit for bit.  Which format a call
    used is read from the up_sixth tap: refused by name where the map is held as f16 words, served where it is f32."""
    B, T = 24, 76
    x = _mel(B, T).to(DEV)
    seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
    key, tonic, genre = net(x, seq)
    cat = net.tap("model.1.cat").clone()
    with pytest.raises(ake_amd._lib.AkeError, match="held as f16 words"):
        net.tap("model.1.up_sixth_a")
    for lo in range(0, B, 4):
        ks, ts, gs = net(x[lo:lo + 4], seq[lo:lo + 4])
        assert net.tap("model.1.up_sixth_a").shape == (4, 4, 36, T), lo          # the f32 map
        assert torch.equal(net.tap("model.1.cat"), cat[lo:lo + 4]), lo
        assert torch.equal(ks, key[lo:lo + 4]) and torch.equal(ts, tonic[lo:lo + 4]) and torch.equal(gs, genre[lo:lo + 4]), lo


@pytest.mark.parametrize("B,T", [(3, 76), (3, 77)])
def test_layer0_taps(net, B, T):
    """keep_taps: the launch also writes its intermediate conv outputs.  Every layer-0 name _check_taps lists (it lives in
    test_gpu_pcnet; test_gpu_route imports it) and the up_sixth map, at that function's bounds (TOL for the exact f32 fold, 1e-3 for
    what has f16 operands behind it)."""
    x, _, taps = _oracle(B, T)
    was = net.keep_taps(True)
    try:
        net(x.to(DEV), torch.full((B,), T, dtype=torch.int64, device=DEV))
        for name, bound in (("model.0.pool", TOL), ("model.0.pc2pc.layer.2", 1e-3), ("model.0.pc2pc.layer.5", 1e-3), ("model.1.up_sixth_a", 1e-3)):
            got = net.tap(name).cpu().numpy()
            ref = taps[name].numpy()
            assert got.shape == ref.shape, name
            err = rel_err(got, ref)
            print(f"{B} x {T} {name}: {err:.2e}")
            assert err < bound, (name, err)
        cat = net.tap("model.1.cat").cpu().numpy()
        err = rel_err(cat[:, :4], taps["model.0.pc2pc.layer.8"].numpy())
        print(f"{B} x {T} model.0.pc2pc.layer.8: {err:.2e}")
        assert err < 1e-3, err
    finally:
        net.keep_taps(was)


@pytest.mark.parametrize("T", [190, 206])
def test_one_octave_long_clip(T):
    """36 bins: layer0_plan's rule admits the one-launch form up to 206 frames, and the maps alone take 115 KiB and more of the LDS.  At 190
    frames the two weight-fragment regions still fit beside them (159.8 KiB in all); from 191 on they do not and every conv fetches its
    fragments from global memory.  Both ends against the float64 oracle, and the launch must be the one-launch form at both."""
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5)
    torch.manual_seed(13)
    n1 = ake_amd.PitchClassNet(36, 12, 2, 7, opt)
    g = torch.Generator().manual_seed(5)
    for _, mod in n1.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
            mod.weight.data.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    sd64 = pcnet_oracle.to_dtype(n1.state_dict(), torch.float64)
    x = torch.rand((2, 1, 36, T), generator=g) * 2.5
    seq = torch.tensor([T, T - 9])
    ref = pcnet_oracle.pcnet_forward(sd64, x.double(), seq)
    n1 = n1.to(DEV).eval()
    ake_amd._lib.prof_enable("", True)
    try:
        got = n1(x.to(DEV), seq.to(DEV))
        launched = ake_amd._lib.prof_results()
    finally:
        ake_amd._lib.prof_enable("", False)
    assert "layer0_fused_kernel" in launched, sorted(launched)
    for name, a, b in zip(("key", "tonic", "genre"), got, ref):
        err = rel_err(a.cpu(), b)
        print(f"36 bins x {T} {name}: {err:.2e}")
        assert err < TOL, (name, T, err)
