"""Weights whose outputs depend on the input, and the bounds a device forward is held to on them (a helper, not a conftest).

The seeded fixtures under tests/golden/ carry BatchNorm running statistics that do not match any data, and a time mean sits in front of
the outputs: their outputs are almost constant (the default fixture's key is 0.5251 for silence and for audio alike), so `rel_err`
against the output's maximum cannot see the input-dependent part.  Two remedies:

  * `calibrate`: one train-mode run of the float64 oracle on the test's own input, its batch statistics written into the running
    statistics (nothing is committed; half a second for 4 clips);
  * tests/golden/pcnet_trained.npz: 36 Adam steps of the float32 oracle loop on synthetic clips (oracle/make_trained.py).

`response` measures what the remedy is for, `bounds` derives the two bounds of a case from the reference alone:
    b32  = max(2e-5, 4 x rel_err(float32 oracle, float64 oracle))     2e-5: the project's f32x3 bound; 4: the device's f32 sums run in another
                                                                      order than PyTorch's.  The float32 oracle is taken twice, plain and with
                                                                      the three-term bf16 split that `f32x3` keeps in the last pitch-class
                                                                      stack and the heads (pcnet_oracle.f32x3_route), and the larger error
                                                                      counts: on calibrated weights that split alone is 1e-5 .. 3e-5
    bmix = 4 x rel_err(rounding model, float64 oracle)                pcnet_oracle.rounding_model on pcnet_oracle.mixed_route: the device's
                                                                      weight roundings themselves (BatchNorm folded, power-of-two scaled),
                                                                      the activation roundings another draw of the same size
A `mixed` forward is asserted against `mixed_bound = max(bmix, b32)`: it performs every float32 operation an `f32x3` forward performs and
its roundings on top, and on a route that rounds nothing (--denseblock, kernel sizes 3 and 5, clips beyond 146 frames: the f32 kernels
throughout, bmix = 0) it IS the float32 arithmetic that b32 bounds.  On the default net bmix is 5 to 100 times b32 and the maximum
changes nothing.  Two cases are thereby NOT held to the model: the configurations conv_layers=2,n_filters=2 and n_filters=3, whose only
reduced-precision stage is layer 0's f16 x 3 stack.  Their model error is 6e-8 .. 1.6e-6 and the device's 2e-7 .. 5e-6 (1.5 to 4.4 times the
model, above bmix on some outputs): float32 rounding level on both sides, which b32 bounds.
Both bounds are looser than first specified (b32 from the plain float32 oracle alone, `mixed` against bmix alone); DESIGN.md section 4.3
says what was measured.
"""
import numpy as np
import torch

from conftest import rel_err
from oracle import pcnet_oracle

OUTPUTS = ("key", "tonic", "genre")
MIN_RESPONSE = 0.05          # every case asserts this on the oracle alone; calibrated and trained weights sit at 0.14 and above


def calibrate(sd64, x, seq, **oracle_kw):
    """A copy of `sd64` whose BatchNorm running statistics are the batch statistics of `x` (momentum 1: mean and unbiased variance)."""
    sd = {k: v.clone() for k, v in sd64.items()}
    with torch.no_grad(), pcnet_oracle.record_bn_stats() as rows:
        pcnet_oracle.pcnet_forward(sd, x, seq, training=True, **oracle_kw)
    pcnet_oracle.update_running_stats(sd, rows, momentum=1.0, backward_ran=False)
    return sd


def response(sd64, x, seq, ref=None, **oracle_kw):
    """max|ref - ref(zeros)| / max|ref| per output: how much of the output's size the input decides."""
    with torch.no_grad():
        if ref is None:
            ref = pcnet_oracle.pcnet_forward(sd64, x, seq, **oracle_kw)
        silent = pcnet_oracle.pcnet_forward(sd64, torch.zeros_like(x), seq, **oracle_kw)
    return [float((a - b).abs().max()) / max(float(a.abs().max()), 1e-300) for a, b in zip(ref, silent)]


def route_kw(oracle_kw, frames, keep_taps=False):
    """The arguments of pcnet_oracle.mixed_route for a forward that the oracle runs with `oracle_kw`."""
    kw = {k: oracle_kw[k] for k in ("kernel_size", "head_layers", "time_pool_size") if k in oracle_kw}
    return dict(kw, frames=frames, local=oracle_kw.get("local_window") is not None, keep_taps=keep_taps)


def model_forward(sd, x, seq, keep_taps=False, precision="mixed", **oracle_kw):
    """The oracle, in the dtype of `sd` and `x`, under the rounding model of the route this net takes at this frame count in `precision`
    -> (outputs, route)."""
    build = pcnet_oracle.mixed_route if precision == "mixed" else pcnet_oracle.f32x3_route
    route = build(sd, **route_kw(oracle_kw, x.shape[3], keep_taps))
    with torch.no_grad(), pcnet_oracle.rounding_model(route, sd) as rm:
        out = pcnet_oracle.pcnet_forward(sd, x, seq, **oracle_kw)
    assert sorted(set(rm.used)) == sorted(route), (sorted(set(rm.used)), sorted(route))      # the route names no conv the forward does not run
    return out, route


class Bounds:
    """Per output: ref (float64); e32 / e32x3 / emodel: rel_err of the float32 oracle, of the float32 oracle with f32x3's split operands and
    of the float64 oracle under the `mixed` rounding model; b32, bmix, mixed_bound; route: the `mixed` route."""

    def __init__(self, ref, e32, e32x3, emodel, route):
        self.ref, self.e32, self.e32x3, self.emodel, self.route = ref, e32, e32x3, emodel, route
        self.b32 = [max(2e-5, 4 * max(a, b)) for a, b in zip(e32, e32x3)]
        self.bmix = [4 * e for e in emodel]
        self.mixed_bound = [max(a, b) for a, b in zip(self.bmix, self.b32)]

    def bound(self, precision):
        return self.mixed_bound if precision == "mixed" else self.b32

    def rows(self):
        return "  ".join(f"{n}: f32 {a:.1e} f32x3 {x:.1e} model {b:.1e} -> b32 {c:.1e} bmix {d:.1e}"
                         for n, a, x, b, c, d in zip(OUTPUTS, self.e32, self.e32x3, self.emodel, self.b32, self.bmix))


def bounds(sd, x, seq, keep_taps=False, **oracle_kw):
    """The two reference-derived bounds for the picked clips `x` (float64, (B, 1, P, T)) of one case; `sd` in any float dtype."""
    sd64 = pcnet_oracle.to_dtype(sd, torch.float64)
    sd32 = pcnet_oracle.to_dtype(sd64, torch.float32)
    x = x.double()
    with torch.no_grad():
        ref = pcnet_oracle.pcnet_forward(sd64, x, seq, **oracle_kw)
        got32 = pcnet_oracle.pcnet_forward(sd32, x.float(), seq, **oracle_kw)
    got32x3, _ = model_forward(sd32, x.float(), seq, keep_taps, "f32x3", **oracle_kw)
    model, route = model_forward(sd64, x, seq, keep_taps, "mixed", **oracle_kw)
    err = lambda outs: [rel_err(a, b) for a, b in zip(outs, ref)]
    return Bounds(ref, err(got32), err(got32x3), err(model), route)


def assert_responds(sd64, x, seq, ref=None, what="", **oracle_kw):
    """The condition that keeps a later fixture from turning a case blind again."""
    r = response(sd64, x, seq, ref, **oracle_kw)
    assert min(r) >= MIN_RESPONSE, f"{what}: response / max per output {['%.1e' % v for v in r]} is below {MIN_RESPONSE}: the weights do not see the input"
    return r


# ---- the trained fixture -------------------------------------------------------------------------------------------------------------------

TRAINED_SEQ = [76, 70, 61, 50, 76, 76, 40, 33]
TRAINED_FIRST_CLIP = 200


def trained_mel(indices, dtype=torch.float64):
    """The log-CQT (cqt_oracle, float64) of the synthetic clips `indices`: (B, 1, 288, 76)."""
    from ake_amd import synthetic
    from oracle import cqt_oracle
    ys, _ = synthetic.make_batch(indices)
    cq = cqt_oracle.FastDirectCQT(synthetic.SR, cqt_oracle.hop_for(synthetic.SR), dtype=torch.float64)
    return torch.as_tensor(cq(ys))[:, None].to(dtype)


# ---- faults planted in the oracle (the teeth) ----------------------------------------------------------------------------------------------

def planted_faults(sd64, x, seq, **oracle_kw):
    """name -> outputs of the float64 oracle with one fault planted: a weight tensor off by 2^-8, a dropped corner tap, the input one frame
    late, two clips swapped."""
    fwd = lambda s, xx: pcnet_oracle.pcnet_forward(s, xx, seq, **oracle_kw)
    out = {}
    with torch.no_grad():
        s = dict(sd64)
        s["model.0.pool_semi.weight"] = sd64["model.0.pool_semi.weight"] * (1 + 2.0 ** -8)
        out["layer 0 semitone conv x (1 + 2^-8)"] = fwd(s, x)
        s = dict(sd64)
        w = sd64["model.1.p2p.layer.0.weight"].clone()
        w[..., 0, 0] = 0
        s["model.1.p2p.layer.0.weight"] = w
        out["corner tap of the first pitch conv dropped"] = fwd(s, x)
        out["mel one frame late"] = fwd(sd64, torch.cat([torch.zeros_like(x[..., :1]), x[..., :-1]], -1))
        perm = list(range(x.shape[0]))
        perm[1], perm[2] = perm[2], perm[1]
        out["clips 1 and 2 swapped"] = fwd(sd64, x[perm])
    return out


def cqt_gain_fault(x, gain=1.01):
    """The log-CQT of magnitudes `gain` times too large."""
    return torch.log1p(gain * torch.expm1(x))


def np_outputs(outs):
    return [np.asarray(o.detach().cpu(), dtype=np.float64) for o in outs]


# ---- the nets of the suite, on the CPU -----------------------------------------------------------------------------------------------------

FIXTURES = {"default": ("pcnet_default.npz", {}), "resblock": ("pcnet_resblock_T28.npz", {}), "pc2p_mem": ("pcnet_pc2pmem_T40.npz", {}),
            "p2pc_conv": ("pcnet_p2pcconv_T40.npz", {}), "stay_sixth": ("pcnet_staysixth_T40.npz", {}), "denseblock": ("pcnet_denseblock_T40.npz", {}),
            "k3": ("pcnet_k3_T40.npz", dict(kernel_size=3)), "k5": ("pcnet_k5_T40.npz", dict(kernel_size=5))}
CONFIGS = [dict(num_layers=1), dict(num_layers=3), dict(head_layers=1), dict(head_layers=3), dict(conv_layers=2, n_filters=2), dict(n_filters=3),
           dict(max_pool=True), dict(time_pool_size=4)]          # tests/test_gpu_pcnet.py::test_other_configurations_against_oracle


def config_name(cfg):
    return ",".join(f"{k}={v}" for k, v in cfg.items())


def config_net(cfg):
    """The seeded net of test_other_configurations_against_oracle for `cfg` -> (module on the CPU, opt, float64 state_dict, oracle keywords,
    frames of its existing shape)."""
    from argparse import Namespace
    import ake_amd
    cfg = dict(cfg)
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5)
    num_layers = cfg.pop("num_layers", 2)
    for k, v in cfg.items():
        setattr(opt, k, v)
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
    kw = dict(head_layers=opt.head_layers, time_pool_size=opt.time_pool_size, max_pool=opt.max_pool)
    T = 120 if (num_layers == 3 or opt.time_pool_size == 4 or opt.head_layers == 3) else 52
    return net, opt, sd64, kw, T


def rand_input(B, T, seed):
    """x = rand * 2.5 (float64) and a seq_length in [T - 20, T] with the first clip full."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 1, 288, T), generator=g, dtype=torch.float64) * 2.5
    seq = torch.cat([torch.tensor([T]), torch.randint(T - 20, T + 1, (B - 1,), generator=g)])
    return x, seq


# ---- the tracked recording -----------------------------------------------------------------------------------------------------------------

TRACK_CLIPS = (200, 205)          # two 15-second segments in different keys: 30 s, 151 frames, 4 windows of 76 frames at stride 25
TRACK_WF, TRACK_SF = 76, 25


def track_recording():
    """(1, n) float32: the two-segment recording the end-to-end track test decodes."""
    from ake_amd import synthetic
    return np.concatenate([synthetic.make_clip(i)[0] for i in TRACK_CLIPS])[None].astype(np.float32)


def windows_of(mel, wf=TRACK_WF, sf=TRACK_SF):
    """(P, T) -> the sliding windows (W, 1, P, wf)."""
    return mel.unfold(1, wf, sf).permute(1, 0, 2).contiguous()[:, None]


def decode_is_certain(key, tonic, bound_key, bound_tonic):
    """Per window: does the oracle's decode (metrics.decode_keys: first-maximum cosine over the signature table, first maximum of the
    tonic logits) survive any error within the output bounds?  Its top two scores must differ by more than twice what the bound allows:
    tonic logits move by at most bound_tonic * max|tonic|; a cosine against a unit table row moves by at most the change of the
    normalised key vector, 2 |dk| / |k| with |dk| <= sqrt(12) * bound_key * max|key|.  Duplicate table rows (equal cosines, the first
    wins on either side) do not count as a second candidate."""
    from ake_amd import metrics
    table = metrics._device_table(key.device, key.dtype)
    sims = (key[:, None, :] * table[None]).sum(2) / (key.norm(dim=1, keepdim=True).clamp_min(1e-8) * table.norm(dim=1, keepdim=True).clamp_min(1e-8).T)
    best = sims.max(dim=1, keepdim=True).values
    rows = table[sims.argmax(dim=1)]                                                  # the winning row; its duplicates are no rivals
    rival = torch.where((table[None] == rows[:, None]).all(dim=2), torch.full_like(sims, -2.0), sims).max(dim=1).values
    dcos = 2 * (12 ** 0.5) * bound_key * float(key.abs().max()) / key.norm(dim=1)
    t2 = tonic.topk(2, dim=1).values
    return ((best[:, 0] - rival) > 2 * dcos) & ((t2[:, 0] - t2[:, 1]) > 2 * bound_tonic * float(tonic.abs().max()))
