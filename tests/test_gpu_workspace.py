"""GPU: every entry point that works out of a caller-provided workspace is held to the bytes it asked for and to arbitrary content in
them.  The contract (include/ake_hip.h): workspace content on entry is arbitrary; nothing outside the given bytes and the documented
outputs is written; the one exception is the backward pass, which reads what its forward left.

Every call goes straight through the C ABI, on a workspace exactly *_workspace_bytes long with a guard band on both sides
(tests/ws_guard.py), and writes into output tensors that are 16-byte-aligned slices between guards of their own, pre-filled with 0xFF
bytes.  Each case runs on four workspace contents:
    (a) 0x00   (b) 0xFF: NaN in every float format, -1 as an integer   (c) 0x77: about 5e33 as f32 / bf16, 30576 as f16 -- finite and
    large, for the fmax chains (octave fold, max pools, the --local sliding max) that swallow a NaN
    (d) real stale content: what calls of other shapes (and, where there is one, of another route) left in the same bytes
and asserts: (a) twice gives the same bits (the entry is reproducible); (b), (c) and (d) give the bits of (a); no output element keeps
its 0xFF fill; every guard is intact.  The outputs under (c) are also held to the float64 oracle at the tolerance the entry's own test
uses, so "all four agree" cannot mean "all four wrong".

Before poisoning, the carves were read for regions that carry indices, offsets or counts a kernel reads before the call writes them:
  - the net (plan_buffers, csrc/pcnet_plan.h): activations (f32, f16 / split-bf16 words), per-channel tables, fixed-point partial sums and
    statistics that are memset at the start of the call that reads them -- no index-bearing region;
  - forward_windows / pipeline / track (csrc/track.hip, csrc/pipeline.hip): the gathered or transformed mel, a seq_length table that is
    refilled before every forward, then the embedded CQT and net workspaces;
  - the CQT of the equal-hop entries (ake_cqt_workspace_bytes, csrc/cqt.hip): split-bf16 level planes and float scratch -- no indices
    (only the per-clip-hop form, which no entry here embeds, holds row indices);
  - ake_general_step_local_f32: double partial sums; ake_synth_partials_f32: one peak cell per recording, memset by the call.
So no region had to be restricted to (a) and (d).
"""
import ctypes as C
import functools
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib
from conftest import golden_state_dict, load_golden, rel_err
from oracle import pcnet_oracle
from test_gpu_p2p_stack import KEY as P2P_KEY, n_cus
from test_gpu_pcnet import TOL, make_net
from ws_guard import Guarded, GuardedTensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FIXTURES = {"default": "pcnet_default.npz", "resblock": "pcnet_resblock_T28.npz", "pc2p_mem": "pcnet_pc2pmem_T40.npz",
            "p2pc_conv": "pcnet_p2pcconv_T40.npz", "stay_sixth": "pcnet_staysixth_T40.npz", "denseblock": "pcnet_denseblock_T40.npz",
            "k3": "pcnet_k3_T40.npz"}


def stream():
    return torch.cuda.current_stream().cuda_stream


def seeded_net(num_layers):
    """The seeded weights of test_gpu_pcnet.test_other_configurations_against_oracle."""
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5)
    torch.manual_seed(11)
    net = ake_amd.PitchClassNet(288, 12, num_layers, 7, opt)
    g = torch.Generator().manual_seed(3)
    for _, mod in net.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
            mod.weight.data.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    sd64 = pcnet_oracle.to_dtype({k: v.detach().clone() for k, v in net.state_dict().items()}, torch.float64)
    return net.to(DEV).eval(), sd64


@functools.lru_cache(maxsize=None)
def get_net(name):
    """-> (module with its device handle loaded for inference and training, float64 state_dict, the oracle's keyword arguments)."""
    kw = {}
    if name in FIXTURES:
        gold = load_golden(FIXTURES[name])
        net, opt = make_net(gold)
        sd64 = golden_state_dict(gold, torch.float64)
        if name == "k3":
            kw = dict(kernel_size=3)
    elif name in ("f32x3", "local"):
        gold = load_golden(FIXTURES["default"])
        net, _ = make_net(gold, **({"precision": "f32x3"} if name == "f32x3" else {"local": True}))
        sd64 = golden_state_dict(gold, torch.float64)
        if name == "local":
            kw = dict(local_window=net.local_window)
    elif name == "nogenre":
        gold = load_golden(FIXTURES["default"])
        opt = Namespace(**json.loads(str(gold["opt"])))
        opt.genre = False
        net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
        keep = set(net.state_dict())
        net.load_state_dict({k: v for k, v in golden_state_dict(gold).items() if k in keep}, strict=True)
        net = net.to(DEV).eval()
        sd64 = {k: v for k, v in golden_state_dict(gold, torch.float64).items() if k in keep}
    else:
        net, sd64 = seeded_net({"layers1": 1, "layers3": 3}[name])
    net.prepare()
    return net, sd64, kw


def inputs(B, T, seed=0, seq="random"):
    g = torch.Generator().manual_seed(1000 + 131 * seed + 7 * B + T)
    x = (torch.rand((B, 1, 288, T), generator=g) * 2.5).to(DEV)
    if seq == "random":
        s = torch.randint(26, T + 1, (B,), generator=g).to(DEV)
    else:
        s = None
    return x, s


def out_shapes(net, B, T):
    if net.local:
        tq, tm = C.c_int(), C.c_int()
        _lib.check(_lib.lib().ake_pcnet_local_frames(net.handle, T, C.byref(tq), C.byref(tm)), "ake_pcnet_local_frames")
        shapes = [(B, 12 * tq.value), (B, 12 * tq.value), (B, 11 * tm.value)]
    else:
        shapes = [(B, 12), (B, 12), (B, 11)]
    return shapes if net.genre else shapes[:2]


def finish(outs, what):
    """Synchronise, check the guards of every output and return copies of the outputs."""
    for o in outs:
        o.check(f"{what}: output")
    return [o.t.clone() for o in outs]


def forward_call(net, x, B, T, seq, entry="ake_pcnet_forward_f32"):
    """-> (workspace bytes, call(ws, what) -> [key, tonic(, genre)]) for one inference entry of the net."""
    L, h = _lib.lib(), net.handle
    local = entry == "ake_pcnet_forward_local_f32"

    def call(ws, what):
        outs = [GuardedTensor(s) for s in out_shapes(net, B, T)]
        ptrs = [o.t.data_ptr() for o in outs] + [None] * (3 - len(outs))
        lead = (h, x.data_ptr(), B, T) + (() if local else (seq.data_ptr() if seq is not None else None,))
        _lib.check(getattr(L, entry)(*lead, *ptrs, ws.data_ptr(), ws.numel(), stream()), entry)
        return finish(outs, what)

    nbytes = int(L.ake_pcnet_workspace_bytes(h, B, T))
    assert nbytes > 0
    return nbytes, call


def same_bits(ref, got, what):
    """Bit equality of two output lists (NaN payloads included), and no float element of `got` still holds its 0xFF fill."""
    assert len(ref) == len(got)
    for i, (r, g) in enumerate(zip(ref, got)):
        rb, gb = (t.contiguous().view(torch.int32) for t in (r, g))
        if g.is_floating_point():
            unwritten = int((gb == -1).sum())
            assert unwritten == 0, f"{what}: output {i}: {unwritten} of {g.numel()} elements were never written"
        if not torch.equal(rb, gb):
            bad = torch.nonzero((rb != gb).flatten()).flatten()
            k = int(bad[0])
            raise AssertionError(f"{what}: output {i} differs in {bad.numel()} of {g.numel()} elements, first at flat index {k}: "
                                 f"{r.flatten()[k].item()!r} on the zeroed workspace, {g.flatten()[k].item()!r} here")


def hold(label, nbytes, call, stale, oracle=None):
    """The four contents for one case.  `call(ws, what)` runs the entry on the workspace view `ws` and returns its outputs; `stale` is a
    list of (bytes, call) run in order on one buffer whose leading bytes then become content (d)."""
    def run(fill, what, pre=()):
        g = Guarded(nbytes, fill)
        if pre:
            big = Guarded(max(nb for nb, _ in pre), 0x00)
            for nb, c in pre:
                c(big.view[:nb], f"{label}: stale call")
            big.check(f"{label}: stale calls")
            m = min(big.nbytes, nbytes)
            g.view[:m].copy_(big.view[:m])
            del big
        outs = call(g.view, f"{label} on {what}")
        g.check(f"{label} on {what}: workspace")
        return outs

    a = run(0x00, "0x00")
    same_bits(a, run(0x00, "0x00 again"), f"{label}: two runs on a zeroed workspace (the entry is not reproducible)")
    same_bits(a, run(0xFF, "0xFF"), f"{label}: workspace of 0xFF against zeros")
    c = run(0x77, "0x77")
    same_bits(a, c, f"{label}: workspace of 0x77 against zeros")
    if oracle is not None:
        oracle(c)
    assert stale, label
    same_bits(a, run(0x00, "stale content", pre=stale), f"{label}: stale workspace against zeros")
    print(f"  {label}: {nbytes} workspace bytes, reproducible, 0xFF / 0x77 / stale equal to zeros, guards intact")
    return a


def oracle_check(name, x, seq, idx=None, training=False, label=""):
    """Outputs against pcnet_oracle at TOL, on the clips `idx` (inference: clips are independent) or on all of them."""
    _, sd64, kw = get_net(name)

    def check(outs):
        i = list(range(x.shape[0])) if idx is None else idx
        ref = pcnet_oracle.pcnet_forward(sd64, x[i].cpu().double(), None if seq is None else seq[i].cpu(), training=training, **kw)
        for nm, a, b in zip(("key", "tonic", "genre"), outs, ref):
            e = rel_err(a[i].cpu().reshape(b.shape), b.detach())
            print(f"  {label} {nm} vs float64: {e:.2e}", end="")
            assert e < TOL, (label, nm, e)
    return check


def timed(nbytes, call):
    """One run on a zeroed workspace under the kernel timer -> {kernel name: (ms, launches)}."""
    g = Guarded(nbytes, 0x00)
    _lib.prof_results()
    _lib.prof_enable("", True)
    try:
        call(g.view, "route")
        res = _lib.prof_results()
    finally:
        _lib.prof_enable("", False)
    return res


def tap_answer(net, name, B, T):
    """(rc, message) of ake_pcnet_tap_info: whether a forward of this shape writes the activation `name`, from the call's route."""
    shape = (C.c_int64 * 4)()
    rc = _lib.lib().ake_pcnet_tap_info(net.handle, name.encode(), B, T, shape)
    return rc, (_lib.lib().ake_last_error() or b"").decode() if rc else ""


def stale_forwards(net, shapes, seed=50):
    out = []
    for k, (B, T) in enumerate(shapes):
        x, seq = inputs(B, T, seed + k, "none" if net.local else "random")
        entry = "ake_pcnet_forward_local_f32" if net.local else "ake_pcnet_forward_f32"
        out.append(forward_call(net, x, B, T, seq, entry))
    return out


def persistent_batch(net):
    """The smallest batch at 76 frames that takes the persistent pitch convs (and with them melh and the f16 form of psix[1])."""
    L = _lib.lib()
    for B in (16, 17, 18, 19, 24, 64):
        if L.ake_pcnet_accepts_frames_major(net.handle, B, 76) == 1:
            return B
    raise AssertionError("no batch in (16, 17, 18, 19, 24, 64) takes the frames-major route at 76 frames")


# ---- inference -----------------------------------------------------------------------------------------------------------------------

def picks(B):
    return None if B <= 4 else sorted({0, B // 2, B - 1})


@pytest.mark.parametrize("case", ["3x76", "2x100", "1x27", "3x77", "3x76-noseq", "persistent", "persistent-frames-major", "one-launch",
                                  "257x40", "keep-taps", "f32x3"])
def test_default_net_inference(case):
    """The default net (gold_default weights): mixed precision unless the case says otherwise, x = rand * 2.5, seq_length random in
    [26, T].  A case that names a route proves from the kernel timer and the tap answers that the route ran; the stale content comes
    from a call that dirties the whole workspace followed by one on another route (2 x 100: per-stage layer 0, up_sixth as f32; for
    2 x 100 itself the persistent batch, so the f16 form of psix[1] lies under the f32 form and the other way round)."""
    net = get_net("f32x3" if case == "f32x3" else "default")[0]
    name = "f32x3" if case == "f32x3" else "default"
    L = _lib.lib()
    Bp = persistent_batch(get_net("default")[0])
    B, T = {"3x76": (3, 76), "2x100": (2, 100), "1x27": (1, 27), "3x77": (3, 77), "3x76-noseq": (3, 76), "persistent": (Bp, 76),
            "persistent-frames-major": (Bp, 76), "one-launch": (n_cus(), 76), "257x40": (257, 40), "keep-taps": (3, 76), "f32x3": (3, 76)}[case]
    x, seq = inputs(B, T, 1, "none" if case == "3x76-noseq" else "random")
    idx = [0, 255, 256] if case == "257x40" else picks(B)
    was = L.ake_debug_keep_taps(1) if case == "keep-taps" else None
    try:
        if case == "persistent-frames-major":
            x_fm = x[:, 0].transpose(1, 2).contiguous()
            nbytes, call = forward_call(net, x_fm, B, T, seq, "ake_pcnet_forward_frames_major_f32")
        else:
            nbytes, call = forward_call(net, x, B, T, seq)
        # the route
        launches = timed(nbytes, call).get(P2P_KEY, (0.0, 0))[1]         # (f32x3 books its pitch convs under other names: 0)
        accepts = L.ake_pcnet_accepts_frames_major(net.handle, B, T)
        if B <= 256:                                                     # (the taps answer for one chunk of the pitch stream)
            (l0_rc, l0_msg), (p8_rc, p8_msg), (up_rc, up_msg) = (tap_answer(net, nm, B, T) for nm in
                                                                 ("model.0.pc2pc.layer.2", "model.1.p2p.layer.8", "model.1.up_sixth_a"))
            print(f"\n  {case}: {B} x {T}, {launches} launch(es) booked as {P2P_KEY}, frames-major {accepts}, layer 0 stack "
                  f"{'in LDS' if l0_rc else 'written'}, last pitch conv {'fused' if p8_rc else 'written'}, up_sixth {'f16 words' if up_rc else 'f32'}")
        else:
            print(f"\n  {case}: {B} x {T}, {launches} launch(es) booked as {P2P_KEY}, frames-major {accepts}")
        if case == "3x76":
            assert launches == 3 and accepts == 0, (launches, accepts)
            assert l0_rc and "stays in LDS (layer 0 runs as one launch)" in l0_msg, l0_msg
            assert p8_rc and "fused with the semitone conv" in p8_msg, p8_msg
        if case == "2x100":
            assert accepts == 0 and l0_rc == 0 and up_rc == 0, (accepts, l0_msg, up_msg)
        if case in ("1x27", "3x77"):
            assert accepts == 0, accepts
        if case.startswith("persistent"):
            assert accepts == 1 and up_rc and "held as f16 words" in up_msg, (accepts, up_msg)
        if case == "one-launch":
            assert launches == 1, launches
        if case == "257x40":
            assert launches in (4, 6), launches                          # two chunks: one or three launches, then the one-clip remainder's three
        if case == "keep-taps":
            assert launches == 3 and p8_rc == 0 and l0_rc == 0, (launches, p8_msg, l0_msg)
        other = (Bp, 76) if case == "2x100" else (2, 100)
        stale = stale_forwards(get_net("default")[0] if case == "keep-taps" else net, [(B + 1, T + 16), other])
        outs = hold(case, nbytes, call, stale, oracle_check(name, x, seq, idx, label=case))
        if case == "persistent-frames-major":                           # the same bits as the plain entry on the transposed tensor
            nb, plain = forward_call(net, x, B, T, seq)
            g = Guarded(nb, 0x77)
            same_bits(plain(g.view, case), outs, "frames-major against the plain entry")
            g.check(case)
    finally:
        if was is not None:
            L.ake_debug_keep_taps(was)


@pytest.mark.parametrize("name,B,T", [("resblock", 3, 52), ("pc2p_mem", 3, 52), ("p2pc_conv", 3, 52), ("stay_sixth", 3, 52),
                                      ("denseblock", 3, 52), ("k3", 3, 52), ("layers1", 3, 52), ("layers3", 3, 120), ("local", 2, 120)])
def test_variant_inference(name, B, T):
    """The architecture variants from their own fixtures (seeded weights for one and three layers), and the --local forward: each carves
    buffers the default net does not have (smap, p0 / pcd, pin, the doubled pb).  Stale content: two other shapes on the same net."""
    net = get_net(name)[0]
    local = name == "local"
    x, seq = inputs(B, T, 2, "none" if local else "random")
    nbytes, call = forward_call(net, x, B, T, seq, "ake_pcnet_forward_local_f32" if local else "ake_pcnet_forward_f32")
    print()
    hold(f"{name} {B} x {T}", nbytes, call, stale_forwards(net, [(B + 1, T + 16), (2, T + 40)]), oracle_check(name, x, seq, label=name))


# ---- training ------------------------------------------------------------------------------------------------------------------------

def bn_channels(net):
    return sum(c for _, c, _ in net._bn_layers())


def train_call(net, x, B, T, seq, d_outs, accumulate_onto=None):
    """Forward in train mode, then the backward pass, on one workspace -> (bytes, call -> [key, tonic(, genre), bn_stats, gradients]).
    Only the forward sees the content the workspace was given: the backward reads what the forward left, as the ABI documents."""
    L, h = _lib.lib(), net.handle
    n_grad = int(L.ake_pcnet_grad_floats(h))

    def call(ws, what):
        outs = [GuardedTensor(s) for s in out_shapes(net, B, T)]
        stats, grads = GuardedTensor((bn_channels(net), 3)), GuardedTensor((n_grad,))
        if accumulate_onto is not None:
            grads.t.copy_(accumulate_onto)
        ptrs = [o.t.data_ptr() for o in outs] + [None] * (3 - len(outs))
        sp = seq.data_ptr() if seq is not None else None
        _lib.check(L.ake_pcnet_forward_train_f32(h, x.data_ptr(), B, T, sp, *ptrs, stats.t.data_ptr(), ws.data_ptr(), ws.numel(), stream()),
                   "ake_pcnet_forward_train_f32")
        dp = [d.data_ptr() for d in d_outs] + [None] * (3 - len(d_outs))
        _lib.check(L.ake_pcnet_backward_f32(h, x.data_ptr(), B, T, sp, outs[0].t.data_ptr(), *dp, grads.t.data_ptr(),
                                            0 if accumulate_onto is None else 1, ws.data_ptr(), ws.numel(), stream()), "ake_pcnet_backward_f32")
        return finish(outs + [stats, grads], what)

    nbytes = int(L.ake_pcnet_train_workspace_bytes(h, B, T))
    assert nbytes > 0
    return nbytes, call


@pytest.mark.parametrize("name,B,T", [("default", 4, 40), ("resblock", 3, 52), ("pc2p_mem", 3, 52), ("p2pc_conv", 3, 52),
                                      ("stay_sixth", 3, 52), ("local", 2, 120), ("nogenre", 4, 40)])
def test_training_forward_and_backward(name, B, T):
    """ake_pcnet_forward_train_f32 then ake_pcnet_backward_f32 on one workspace, poisoned before the forward only.  Compared bit for bit:
    key, tonic, genre, bn_stats_out and the whole gradient buffer (ake_pcnet_grad_floats floats between guards, pre-filled with 0xFF,
    accumulate = 0).  The forward outputs under 0x77 are held to the float64 oracle's train-mode forward at TOL.
    accumulate = 1 onto a known buffer: the reduction is `out[i] = out[i] + s` with s the float the accumulate = 0 call writes, one
    IEEE float32 addition (grad_reduce_kernel), so the result equals buffer + gradients to the last bit, which is what is asserted."""
    net = get_net(name)[0]
    local = name == "local"
    x, seq = inputs(B, T, 3, "none" if local else "random")
    if not local:
        seq = seq.clamp_min(T - 12)                                   # as test_gpu_training.make_batch: a frame count the heads can pool
    g = torch.Generator().manual_seed(17)
    d_outs = [(torch.randn(s, generator=g) * 0.1).to(DEV) for s in out_shapes(net, B, T)]
    nbytes, call = train_call(net, x, B, T, seq, d_outs)
    others = []
    for k, (b2, t2) in enumerate([(B + 1, T + 16), (2, T + 40)]):
        x2, s2 = inputs(b2, t2, 60 + k, "none" if local else "random")
        d2 = [torch.zeros(s, device=DEV) for s in out_shapes(net, b2, t2)]
        others.append(train_call(net, x2, b2, t2, s2, d2))
    print()
    outs = hold(f"train {name} {B} x {T}", nbytes, call, others, oracle_check(name, x, seq, training=True, label=f"train {name}"))
    grads = outs[-1]
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    base = (torch.randn(grads.shape, generator=g) * float(grads.abs().max())).to(DEV)
    _, acc_call = train_call(net, x, B, T, seq, d_outs, accumulate_onto=base)
    ws = Guarded(nbytes, 0x77)
    acc = acc_call(ws.view, "accumulate = 1")
    ws.check("accumulate = 1: workspace")
    same_bits([base + grads], acc[-1:], f"train {name}: accumulate = 1 against buffer + gradients")
    same_bits(outs[:-1], acc[:-1], f"train {name}: outputs and statistics of the accumulating call")


# ---- composite entries and small workspaces --------------------------------------------------------------------------------------------

HOP = 4410                                                             # 22050 Hz at 5 frames per second


@functools.lru_cache(maxsize=None)
def estimator():
    return ake_amd.KeyEstimator(get_net("default")[0], 22050, 5)


def audio(B, n, seed):
    """Noise with a few sines, amplitude below 1: (B, n) float32 on the device."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    rows = []
    for _ in range(B):
        f = 110.0 * 2 ** (torch.rand(3, generator=g, dtype=torch.float64) * 4)
        rows.append((0.2 * torch.sin(2 * np.pi * f[:, None] * t[None]).sum(0) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float())
    return torch.stack(rows).to(DEV).contiguous()


def pipeline_call(kind, y, lengths):
    """ake_pipeline_forward_f32 | _ragged_f32 | _pcm16_f32 on (B, n) audio -> (bytes, call -> [key, tonic, genre])."""
    L, est = _lib.lib(), estimator()
    B, n = y.shape
    src = torch.round(y * 32767).to(torch.int16).contiguous() if kind == "pcm16" else y
    assert src.stride(0) % 2 == 0

    def call(ws, what):
        outs = [GuardedTensor((B, k)) for k in (12, 12, 11)]
        ptrs = [o.t.data_ptr() for o in outs]
        tail = (ws.data_ptr(), ws.numel(), stream())
        lp = lengths.data_ptr() if lengths is not None else None
        if kind == "equal":
            rc = L.ake_pipeline_forward_f32(est.plan.handle, est.net.handle, src.data_ptr(), B, n, src.stride(0), *ptrs, *tail)
        elif kind == "ragged":
            rc = L.ake_pipeline_forward_ragged_f32(est.plan.handle, est.net.handle, src.data_ptr(), B, n, src.stride(0), lp, *ptrs, *tail)
        else:
            rc = L.ake_pipeline_forward_pcm16_f32(est.plan.handle, est.net.handle, src.data_ptr(), B, n, src.stride(0), lp, *ptrs, *tail)
        _lib.check(rc, f"ake_pipeline_forward ({kind})")
        return finish(outs, what)

    nbytes = int(L.ake_pipeline_workspace_bytes(est.plan.handle, est.net.handle, B, n))
    assert nbytes > 0
    return nbytes, call


@pytest.mark.parametrize("kind", ["equal", "ragged", "pcm16", "pcm16-ragged"])
def test_pipeline_entries(kind):
    """3 clips of 75 hops (the shortest audio that gives 76 frames): the mel, the seq_length table, the CQT workspace and the net's in one
    carve, all poisoned.  Stale content: 4 longer clips through the ragged entry, then 2 clips of 100 frames.  Held to the float64 oracle
    on the plan's own transform (the CQT has its own tests) at TOL."""
    est = estimator()
    n = 75 * HOP
    assert est.plan.num_frames(n) == 76 and est.plan.num_frames(n - 1) == 75
    y = audio(3, n, 5)
    lengths = torch.tensor([n, n - 3 * HOP - 17, n - 11 * HOP], dtype=torch.int64, device=DEV) if "ragged" in kind else None
    nbytes, call = pipeline_call(kind.split("-")[0], y, lengths)
    y2, y3 = audio(4, n + 16 * HOP, 6), audio(2, 99 * HOP, 7)
    stale = [pipeline_call("ragged", y2, torch.tensor([y2.shape[1] - 5 * HOP * k for k in range(4)], dtype=torch.int64, device=DEV)),
             pipeline_call("equal", y3, None)]

    def oracle(outs):
        src = torch.round(y * 32767).to(torch.int16) if kind.startswith("pcm16") else y
        mel = est.plan.logmag(src, lengths=lengths)
        seq = torch.full((3,), 76, dtype=torch.int64) if lengths is None else 1 + lengths.cpu() // HOP
        ref = pcnet_oracle.pcnet_forward(get_net("default")[1], mel[:, None].cpu().double(), seq)
        for nm, a, b in zip(("key", "tonic", "genre"), outs, ref):
            e = rel_err(a.cpu(), b)
            print(f"  pipeline {kind} {nm} vs float64 on the plan's transform: {e:.2e}", end="")
            assert e < TOL, (kind, nm, e)

    print()
    hold(f"pipeline {kind}", nbytes, call, stale, oracle)


def windows_call(mel, fm, R, T, wf, sf):
    L, net = _lib.lib(), get_net("default")[0]
    W = (T - wf) // sf + 1

    def call(ws, what):
        outs = [GuardedTensor((R, W, k)) for k in (12, 12, 11)]
        _lib.check(L.ake_pcnet_forward_windows_f32(net.handle, mel.data_ptr(), int(fm), R, T, wf, sf, *[o.t.data_ptr() for o in outs],
                                                   ws.data_ptr(), ws.numel(), stream()), "ake_pcnet_forward_windows_f32")
        return finish(outs, what)

    nbytes = int(L.ake_pcnet_forward_windows_workspace_bytes(net.handle, R, T, wf, sf))
    assert nbytes > 0
    return nbytes, call


@pytest.mark.parametrize("fm", [False, True])
def test_forward_windows(fm):
    """2 recordings of 226 frames, window 76, stride 25: 14 windows.  Against the oracle on the materialised windows."""
    R, T, wf, sf = 2, 226, 76, 25
    g = torch.Generator().manual_seed(31)
    mel = torch.rand((R, 288, T), generator=g) * 2.5
    dev = (mel.transpose(1, 2) if fm else mel).contiguous().to(DEV)
    nbytes, call = windows_call(dev, fm, R, T, wf, sf)
    mel2 = (torch.rand((3, 288, 300), generator=g) * 2.5).to(DEV)
    stale = [windows_call(mel2, False, 3, 300, 92, 30), windows_call(mel2, False, 3, 300, 100, 100)]

    def oracle(outs):
        W = (T - wf) // sf + 1
        win = torch.stack([mel[r, :, w * sf:w * sf + wf] for r in range(R) for w in range(W)])[:, None]
        pick = [0, W - 1, W, R * W - 1]
        ref = pcnet_oracle.pcnet_forward(get_net("default")[1], win[pick].double(), torch.full((len(pick),), wf))
        for nm, a, b in zip(("key", "tonic", "genre"), outs, ref):
            e = rel_err(a.cpu().flatten(0, 1)[pick], b)
            print(f"  windows {nm} vs float64: {e:.2e}", end="")
            assert e < TOL, (nm, e)

    print()
    hold(f"forward_windows frames_major={int(fm)}", nbytes, call, stale, oracle)


def track_call(y, lengths, wf, sf):
    L, est = _lib.lib(), estimator()
    R, n = y.shape
    T = est.plan.num_frames(n)
    W = (T - wf) // sf + 1

    def call(ws, what):
        outs = [GuardedTensor((R, W, k)) for k in (12, 12, 11)]
        outs += [GuardedTensor((R, W), torch.int32) for _ in range(3)] + [GuardedTensor((R, W)), GuardedTensor((R,), torch.int32)]
        ptrs = [o.t.data_ptr() for o in outs]
        if lengths is None:
            rc = L.ake_pipeline_track_f32(est.plan.handle, est.net.handle, y.data_ptr(), R, n, y.stride(0), wf, sf, *ptrs, ws.data_ptr(), ws.numel(), stream())
        else:
            rc = L.ake_pipeline_track_ragged_f32(est.plan.handle, est.net.handle, y.data_ptr(), R, n, y.stride(0), lengths.data_ptr(), wf, sf, *ptrs,
                                                 ws.data_ptr(), ws.numel(), stream())
        _lib.check(rc, "ake_pipeline_track")
        return finish(outs, what)

    nbytes = int(L.ake_pipeline_track_workspace_bytes(est.plan.handle, est.net.handle, R, n, wf, sf))
    assert nbytes > 0
    return nbytes, call


@pytest.mark.parametrize("ragged", [False, True])
def test_track_entries(ragged):
    """2 recordings of 126 frames, window 76, stride 25 (3 windows each): key / tonic / genre rows, the decoded ids, the confidence and
    the counts.  The first recording's windows are held to the oracle on the plan's own transform."""
    est = estimator()
    n, wf, sf = 125 * HOP, 76, 25
    y = audio(2, n, 9)
    lengths = torch.tensor([n, n - 30 * HOP - 5], dtype=torch.int64, device=DEV) if ragged else None
    nbytes, call = track_call(y, lengths, wf, sf)
    y2 = audio(3, 140 * HOP, 10)
    stale = [track_call(y2, torch.tensor([140 * HOP, 120 * HOP, 100 * HOP], dtype=torch.int64, device=DEV), 92, 20), track_call(y2, None, 100, 40)]

    def oracle(outs):
        mel = est.plan.logmag(y, lengths=lengths)[0].cpu().double()
        win = torch.stack([mel[:, w * sf:w * sf + wf] for w in range(3)])[:, None]
        ref = pcnet_oracle.pcnet_forward(get_net("default")[1], win, torch.full((3,), wf))
        for nm, a, b in zip(("key", "tonic", "genre"), outs, ref):
            e = rel_err(a[0].cpu(), b)
            print(f"  track {nm} vs float64 on the plan's transform: {e:.2e}", end="")
            assert e < TOL, (nm, e)
        counts = outs[-1].cpu().tolist()
        assert counts == ([3, 1] if ragged else [3, 3]), counts

    print()
    hold(f"track ragged={int(ragged)}", nbytes, call, stale, oracle)


def local_step_call(B, T, R, seed, valid):
    L = _lib.lib()
    g = torch.Generator().manual_seed(seed)
    key = torch.sigmoid(torch.randn((B, T, 12), generator=g)).to(DEV)
    tonic = torch.randn((B, T, 12), generator=g).to(DEV)
    k = torch.randint(0, 24, (B, R), generator=g)
    rows = torch.from_numpy(np.asarray(ake_amd.KEY_SIGNATURE_MAP, dtype=np.float32))
    kl = rows[k % rows.shape[0]].to(DEV).contiguous()
    tl = torch.nn.functional.one_hot(k % 12, 12).float().to(DEV).contiguous()
    sl = torch.nn.functional.one_hot(k, 24).float().to(DEV).contiguous()
    n_dev = torch.tensor(valid, dtype=torch.int32, device=DEV)

    def call(ws, what):
        outs = [GuardedTensor((10,)), GuardedTensor((B, T, 12)), GuardedTensor((B, T, 12))]
        _lib.check(L.ake_general_step_local_f32(key.data_ptr(), tonic.data_ptr(), kl.data_ptr(), tl.data_ptr(), 0, sl.data_ptr(), 0, n_dev.data_ptr(),
                                                B, T, R, 1.0, 0.7, *[o.t.data_ptr() for o in outs], ws.data_ptr(), ws.numel(), stream()),
                   "ake_general_step_local_f32")
        return finish(outs, what)

    nbytes = int(L.ake_general_step_local_workspace_bytes(B, T))
    assert nbytes > 0
    return (nbytes, call), (key, tonic, kl, tl, sl)


def test_general_step_local():
    """3 clips of 300 output frames (more than one chunk of rows per clip), valid counts that end inside the first chunk, inside a later
    one and at the end: the per-chunk partial sums of the chunks behind a clip's count are read by the finishing kernel.  Held to the
    float64 per-clip loop of tests/test_gpu_local_loss.py at its tolerances."""
    from test_gpu_local_loss import loop_f64
    valid = [300, 130, 5]
    (nbytes, call), (key, tonic, kl, tl, sl) = local_step_call(3, 300, 310, 1, valid)
    stale = [local_step_call(4, 420, 420, 2, [420, 400, 3, 77])[0], local_step_call(2, 90, 90, 3, [90, 40])[0]]

    def oracle(outs):
        ref, gk, gt = loop_f64(key.cpu(), tonic.cpu(), kl.cpu(), tl.cpu(), sl.cpu(), valid, (1.0, 0.7))
        scal = outs[0].cpu().numpy()
        print(f"  general_step_local loss {scal[0]:.7f} vs float64 {float(ref[0]):.7f}", end="")
        assert abs(scal[0] - ref[0]) < 3e-7 * abs(ref[0]), (scal[0], ref[0])
        assert np.abs(scal[1:] - ref[1:]).max() < 1e-6, (scal[1:], ref[1:])
        for a, b in ((outs[1], gk), (outs[2], gt)):
            got = a.cpu().numpy()
            for i, nv in enumerate(valid):
                assert np.abs(got[i, :nv] - b[i, :nv]).max() < 1e-6 * np.abs(b[i, :nv]).max(), i
                assert (got[i, nv:] == 0).all(), i

    print()
    hold("general_step_local", nbytes, call, stale, oracle)


def synth_call(R, n_list, seed):
    L = _lib.lib()
    g = torch.Generator().manual_seed(seed)
    per = 5
    offsets = torch.arange(0, per * (R + 1), per, dtype=torch.int32).to(DEV)
    cps = (torch.rand(per * R, generator=g, dtype=torch.float64) * 0.05 + 0.005).to(DEV)
    phase = torch.rand(per * R, generator=g, dtype=torch.float64).to(DEV)
    amp = (torch.rand(per * R, generator=g) + 0.1).to(DEV)
    n_max = max(n_list)
    start = torch.randint(-200, n_max // 2, (per * R,), generator=g).to(DEV)
    end = (start + torch.randint(300, n_max, (per * R,), generator=g).to(DEV)).contiguous()
    n = torch.tensor(n_list, dtype=torch.int64, device=DEV)
    seeds = torch.arange(R, dtype=torch.int64, device=DEV) + 1234
    stride = (n_max + 3) // 4 * 4
    args = (offsets, cps, phase, amp, start, end, n, seeds)

    def call(ws, what):
        out = GuardedTensor((R, stride))
        _lib.check(L.ake_synth_partials_f32(offsets.data_ptr(), cps.data_ptr(), phase.data_ptr(), amp.data_ptr(), start.data_ptr(), end.data_ptr(), 64, R,
                                            n.data_ptr(), n_max, stride, 0.01, seeds.data_ptr(), 0.9, out.t.data_ptr(), ws.data_ptr(), ws.numel(),
                                            stream()), "ake_synth_partials_f32")
        return finish([out], what)

    nbytes = int(L.ake_synth_partials_workspace_bytes(R))
    assert nbytes > 0
    return (nbytes, call), args


def test_synth_partials():
    """3 ragged recordings, noise and peak normalisation (the workspace holds the peak cells the second pass reads).  Held to the float64
    model of the synthesiser at the tolerance tests/test_gpu_synth.py uses for a normalised recording."""
    from ake_amd import synthetic
    n_list = [5003, 4096, 1777]
    (nbytes, call), (offsets, cps, phase, amp, start, end, n, seeds) = synth_call(3, n_list, 1)
    stale = [synth_call(5, [3000, 2000, 1000, 4000, 500], 2)[0], synth_call(2, [900, 1200], 3)[0]]

    def oracle(outs):
        y = outs[0].cpu().numpy().astype(np.float64)
        arrays = [t.cpu().numpy() for t in (offsets, cps, phase, amp, start, end)]
        model = lambda peak: synthetic.synth_partials_reference(*arrays, 64, n.cpu().numpy(), noise_sigma=0.01, seed=seeds.cpu().numpy(), peak=peak)
        raw, ref = model(0.0), model(0.9)
        for r, nr in enumerate(n_list):
            assert np.all(y[r, nr:] == 0.0), r
            A = float(arrays[3][5 * r:5 * r + 5].astype(np.float64).sum())
            bound = (1e-6 * A + 8e-6 * 0.01) * 0.9 / float(np.abs(raw[r, :nr]).max()) + 2.0 ** -23 * 0.9    # tests/test_gpu_synth.py::check
            e = float(np.abs(y[r, :nr] - ref[r, :nr]).max())
            print(f"  synth recording {r}: max |device - float64| = {e:.2e} (bound {bound:.2e})", end="")
            assert e <= bound, (r, e, bound)

    print()
    hold("synth_partials", nbytes, call, stale, oracle)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("big,small", [((64, 76), (3, 52)), ((2, 100), (3, 76))])
def test_module_reuses_its_workspace_across_shapes(big, small):
    """PitchClassNet caches one workspace and reuses it: net(x_big) then net(x_small) equals net(x_small) on a freshly built module."""
    gold = load_golden(FIXTURES["default"])
    xb, sb = inputs(*big, 7)
    xs, ss = inputs(*small, 8)
    used, _ = make_net(gold)
    used(xb, sb)
    got = used(xs, ss)
    fresh, _ = make_net(gold)
    same_bits(list(fresh(xs, ss)), list(got), f"net{big} then net{small} against a fresh module")


def test_estimator_reuses_its_workspace_across_clip_lengths():
    """KeyEstimator shares one workspace between requests: a long clip then a short one equals the short one on a fresh estimator."""
    gold = load_golden(FIXTURES["default"])
    long_, short = audio(4, 140 * HOP, 11), audio(3, 75 * HOP, 12)
    used = ake_amd.KeyEstimator(make_net(gold)[0], 22050, 5)
    used(long_)
    got = used(short)
    fresh = ake_amd.KeyEstimator(make_net(gold)[0], 22050, 5)
    same_bits(list(fresh(short)), list(got), "estimator: long clip then short clip against a fresh estimator")
