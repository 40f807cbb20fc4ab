"""Every configuration's convolution sites, through the C ABI: set_tensor + finalize, one training forward, one backward.

ake_pcnet_finalize resolves each convolution's packs, BatchNorm and gradient slots once (ConvSite, csrc/pcnet_net.h) and refuses a net in
which a BatchNorm or a parameter belongs to no site.  A site that the forward or the backward walk then skipped would still leave that
parameter's gradient at exact zeros, which the gradient tests only notice for the few configurations they cover.  This file runs the wider
matrix at the smallest shapes and asks only what does not need a reference: the calls return 0, every learnable tensor has a range of
its own in the flat gradient buffer, and no gradient is non-finite, and no BatchNorm weight or convolution weight gradient is all zeros.

tests/tools/sites_zero_scan.py runs the same cases through the float64 oracle's autograd on the CPU: none of those gradients is zero
there for the seeds below (a case whose oracle gradient were zero would have to take another seed).
"""
import ctypes as C
from argparse import Namespace
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

import ake_amd
from ake_amd import _lib

DEV = "cuda:0"

Case = namedtuple("Case", "variant num_layers n_filters kernel_size genre local seed")
VARIANTS = ("default", "resblock", "denseblock", "stay_sixth", "p2pc_conv", "pc2p_mem")


def _cases():
    out = []
    for v in VARIANTS:
        for L in (1, 2, 3):
            out.append(Case(v, L, 2 if L == 3 else 4, 7, True, False, 1))
        out.append(Case(v, 2, 2, 7, False, False, 2))            # the narrow net, without the genre head
        if v != "denseblock":                                    # (--denseblock is built for kernel_size 7 only)
            out.append(Case(v, 2, 4, 3, True, False, 3))
    out.append(Case("default", 2, 4, 7, True, True, 4))          # --local
    return out


CASES = _cases()


def case_id(c):
    return f"{c.variant}-L{c.num_layers}-nf{c.n_filters}-k{c.kernel_size}" + ("" if c.genre else "-nogenre") + ("-local" if c.local else "")


def frames_of(c):
    """The shapes the gradient tests use for these nets: 40 frames, 96 with three layers (two time pools), 120 for --local."""
    return 120 if c.local else (96 if c.num_layers == 3 else 40)


def make_net(c):
    """The module on the CPU with seeded weights (never moved to the device: the handle under test is a raw one)."""
    opt = Namespace(conv_layers=2, n_filters=c.n_filters, head_layers=2, time_pool_size=2, genre=c.genre, max_pool=False, frames=5, local=c.local,
                    kernel_size=c.kernel_size)
    if c.variant != "default":
        setattr(opt, c.variant, True)
    torch.manual_seed(100 + c.seed)
    net = ake_amd.PitchClassNet(288, 12, c.num_layers, c.kernel_size, opt)
    assert c.variant == "default" or getattr(net, c.variant)
    return net


def make_input(c):
    """2 clips of rand * 2.5 and the labels of `loss_of`."""
    B, T = 2, frames_of(c)
    g = torch.Generator().manual_seed(c.seed)
    x = torch.rand((B, 1, 288, T), generator=g) * 2.5
    seq = None if c.local else torch.tensor([T, T - 6])
    rnd = {"key": torch.rand((B, 4096, 12), generator=g), "tonic": torch.randint(0, 12, (B, 4096), generator=g),
           "genre": torch.randint(0, 11, (B, 4096), generator=g)}
    return x, seq, rnd


def loss_of(c, key, tonic, genre, rnd):
    """general_step's losses (models.py:861-893): BCE on the key, cross entropy on the tonic, 0.1 x cross entropy on the genre; per frame with --local."""
    dev = key.device
    if c.local:
        Tq, Tm = key.shape[1], (genre.shape[1] if genre is not None else 0)
        loss = F.binary_cross_entropy(key, (rnd["key"][:, :Tq] > 0.5).to(key.dtype).to(dev)) + F.cross_entropy(tonic.flatten(0, 1), rnd["tonic"][:, :Tq].flatten().to(dev))
        if genre is not None:
            loss = loss + 0.1 * F.cross_entropy(genre.flatten(0, 1), rnd["genre"][:, :Tm].flatten().to(dev))
        return loss
    loss = F.binary_cross_entropy(key, (rnd["key"][:, 0] > 0.5).to(key.dtype).to(dev)) + F.cross_entropy(tonic, rnd["tonic"][:, 0].to(dev))
    if genre is not None:
        loss = loss + 0.1 * F.cross_entropy(genre, rnd["genre"][:, 0].to(dev))
    return loss


def is_bn_weight(name, sd):
    return name.endswith(".weight") and name[:-len("weight")] + "running_mean" in sd


def is_conv_weight(name, sd):
    return name.endswith(".weight") and sd[name].dim() == 4


def run_case(c):
    """set_tensor + finalize + forward_train + backward on a raw handle.  Returns (return codes, {name: (offset, count)}, {name: gradient on
    the CPU}, outputs, BatchNorm statistics, the float32 state_dict)."""
    L = _lib.lib()
    net = make_net(c)
    sd = {k: v.detach().float().contiguous() for k, v in net.state_dict().items() if v.is_floating_point()}
    cfg = net._config()
    h = C.c_void_p()
    _lib.check(L.ake_pcnet_create(C.byref(cfg), C.byref(h)), "ake_pcnet_create")
    try:
        rcs = {}
        for k, v in sd.items():
            shape = (C.c_int64 * max(1, v.dim()))(*v.shape)
            _lib.check(L.ake_pcnet_set_tensor(h, k.encode(), v.data_ptr(), shape, v.dim()), k)
        rcs["finalize"] = L.ake_pcnet_finalize(h)
        assert rcs["finalize"] == 0, L.ake_last_error()
        x, seq, rnd = make_input(c)
        B, T = x.shape[0], x.shape[3]
        x = x.to(DEV)
        seq = None if seq is None else seq.to(DEV)
        if c.local:
            tq, tm = C.c_int(), C.c_int()
            _lib.check(L.ake_pcnet_local_frames(h, T, C.byref(tq), C.byref(tm)), "ake_pcnet_local_frames")
            shapes = [(B, tq.value, 12), (B, tq.value, 12), (B, tm.value, 11)]
        else:
            shapes = [(B, 12), (B, 12), (B, 11)]
        key, tonic, genre = (torch.empty(s, device=DEV) for s in shapes)
        if not c.genre:
            genre = None
        n_ch = 0
        for i in range(L.ake_pcnet_num_bn(h)):
            name, ch, off = C.c_char_p(), C.c_int(), C.c_int()
            _lib.check(L.ake_pcnet_bn_info(h, i, C.byref(name), C.byref(ch), C.byref(off)), "ake_pcnet_bn_info")
            n_ch += ch.value
        stats = torch.empty((n_ch, 3), device=DEV)
        ws = torch.empty(int(L.ake_pcnet_train_workspace_bytes(h, B, T)), dtype=torch.uint8, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        rcs["forward"] = L.ake_pcnet_forward_train_f32(h, x.data_ptr(), B, T, ptr(seq), key.data_ptr(), tonic.data_ptr(), ptr(genre), stats.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), stream)
        assert rcs["forward"] == 0, L.ake_last_error()
        outs = [None if t is None else t.detach().clone().requires_grad_(True) for t in (key, tonic, genre)]
        loss_of(c, outs[0], outs[1], outs[2], rnd).backward()
        d = [None if t is None else t.grad.contiguous() for t in outs]
        flat = torch.empty(int(L.ake_pcnet_grad_floats(h)), device=DEV)
        rcs["backward"] = L.ake_pcnet_backward_f32(h, x.data_ptr(), B, T, ptr(seq), key.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), ptr(d[2]),
                                                   flat.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream)
        assert rcs["backward"] == 0, L.ake_last_error()
        torch.cuda.synchronize()
        ranges = {name: (int(L.ake_pcnet_grad_offset(h, name.encode())), p.numel()) for name, p in net.named_parameters()}
        flat = flat.cpu()
        grads = {name: flat[off:off + cnt] for name, (off, cnt) in ranges.items() if off >= 0}
        return rcs, ranges, grads, [None if t is None else t.cpu() for t in (key, tonic, genre)], stats.cpu(), sd
    finally:
        L.ake_pcnet_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_site_trains(c):
    rcs, ranges, grads, outs, stats, sd = run_case(c)
    assert rcs == {"finalize": 0, "forward": 0, "backward": 0}
    # every learnable tensor has a slot in the flat gradient buffer, and no two share a float
    assert all(off >= 0 for off, _ in ranges.values()), [n for n, (off, _) in ranges.items() if off < 0]
    spans = sorted((off, off + cnt, name) for name, (off, cnt) in ranges.items())
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        assert end <= start, (a, b)
    assert all(torch.isfinite(t).all() for t in outs if t is not None) and torch.isfinite(stats).all()
    not_finite = [n for n, g in grads.items() if not torch.isfinite(g).all()]
    assert not not_finite, not_finite
    bn_w = [n for n in grads if is_bn_weight(n, sd)]
    conv_w = [n for n in grads if is_conv_weight(n, sd)]
    assert bn_w and conv_w and len(bn_w) + len(conv_w) < len(grads)
    zero = [n for n in bn_w + conv_w if not grads[n].any()]
    assert not zero, f"BatchNorm / convolution weights whose gradient is exactly zero: {zero}"
