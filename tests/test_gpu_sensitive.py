"""PARITY (GPU): the inference forward on weights whose outputs depend on the input, every route, both precisions.

Every other eval-mode parity test compares outputs on seeded-random weights, whose outputs are almost constant (tests/sensitive.py,
tests/test_sensitive_host.py): a fault in the front end, in the plumbing between the stages or in a convolution of the first layers moves
them by less than TOL.  Here the weights respond -- the default fixture with running statistics calibrated on the first 4 clips of each
case's own input (x = rand * 2.5), and the
trained fixture tests/golden/pcnet_trained.npz on the log-CQT of synthetic clips -- and the bounds come from the reference alone
(sensitive.bounds): `f32x3` is held to b32, `mixed` to the rounding model of the route the forward takes (bmix; b32 where that is larger).
On the trained fixture `mixed` is also held to BASELINE.json's 1e-3.  Measured on an MI355X: profiles/sensitive_parity.md (the device's
`mixed` error is 0.75 .. 1.42 times the model's on the default net, and equal to it to two digits where the weight roundings dominate).

Every case first asserts on the oracle alone that each output's response is at least 0.05 of its maximum, proves its route from the
kernel timer and the tap answers the way tests/test_gpu_workspace.py does, and holds the restatement of the route that the rounding
model is built on (pcnet_oracle.mixed_route) to the same evidence.  The oracle runs on at most 4 picked clips: the first, the last, and
those on either side of a chunk boundary.

Weights, inputs and references live in the module-scoped `store` fixture and are shared by the two precisions of a case.
"""
import json
from argparse import Namespace

import pytest
import torch

import ake_amd
import sensitive
from ake_amd import _lib
from conftest import golden_state_dict, load_golden, rel_err
from oracle import pcnet_oracle
from sensitive import OUTPUTS
from test_gpu_workspace import P2P_KEY, forward_call, n_cus, persistent_batch, tap_answer
from ws_guard import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 1e-3                     # BASELINE.json: `mixed` against the float64 reference
PRECISIONS = ("mixed", "f32x3")
FUSED_HEADS = "heads_fused_kernel"
TWO_LAUNCH_HEADS = {"conv_pc_bf16_kernel/head", "conv_head1_bf16_kernel"}
GENERIC = {"conv_mfma_kernel/p2p", "conv_mfma_kernel/pc2pc", "conv_mfma_kernel/head", "conv_mfma_kernel/genre_head", "head_pool_kernel"}   # the time-tiled f32 kernels
LOCAL_WINDOW = 38                 # frames * loc_window_size - head_layers * (kernel_size - 1) of the default options (tests/golden/pcnet_local_T120.npz)


@pytest.fixture(scope="module")
def store():
    """Everything a case shares with the other precision and with other cases: weights, device nets, inputs, references."""
    d = {}
    yield d
    d.clear()


def memo(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


# ---- weights and nets --------------------------------------------------------------------------------------------------------------------

def default_weights(store, wname, cal=None):
    """-> (float32 state_dict the device loads, the same numbers as float64 for the oracle, opt as JSON).  calibrated: `cal` = (x, seq,
    oracle keywords), the first clips of the case's own input, whose batch statistics become the running statistics."""
    if wname == "trained":
        def make():
            gold = load_golden("pcnet_trained.npz")
            sd32 = golden_state_dict(gold)
            return sd32, pcnet_oracle.to_dtype(sd32, torch.float64), str(gold["opt"])
        return memo(store, ("weights", wname), make)
    gold = load_golden("pcnet_default.npz")
    x, seq, kw = cal
    sd32 = pcnet_oracle.to_dtype(sensitive.calibrate(golden_state_dict(gold, torch.float64), x.double(), seq, **kw), torch.float32)
    return sd32, pcnet_oracle.to_dtype(sd32, torch.float64), str(gold["opt"])


def build_net(sd32, opt_json, **opt_kw):
    opt = Namespace(**json.loads(opt_json))
    for k, v in opt_kw.items():
        setattr(opt, k, v)
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    keep = set(net.state_dict())
    net.load_state_dict({k: v for k, v in sd32.items() if k in keep}, strict=True)
    net = net.to(DEV).eval()
    net.prepare()
    return net


NET_KW = {"nogenre": dict(genre=False), "local": dict(local=True)}


def default_net(store, wname, precision, kind):
    """The trained fixture's net (one per precision and kind for the whole module)."""
    sd32, _, opt_json = default_weights(store, wname)
    return memo(store, ("net", wname, precision, kind), lambda: build_net(sd32, opt_json, precision=precision, **NET_KW.get(kind, {})))


def case_weights_and_net(store, wname, precision, kind, x, seq, kw):
    """-> (float64 state_dict, net) of a case.  calibrated: the weights are calibrated on the first 4 clips of the case's input, so they
    belong to the case; the two precisions of a case run one after the other and share them, the case before is dropped."""
    if wname == "trained":
        return default_weights(store, wname)[1], default_net(store, wname, precision, kind)
    key = (kind, tuple(x.shape), seq is None)
    if store.get("calibrated-case", (None,))[0] != key:
        store["calibrated-case"] = (key, default_weights(store, wname, (x[:4], None if seq is None else seq[:4], kw)), {})
    _, (sd32, sd64, opt_json), nets = store["calibrated-case"]
    if precision not in nets:
        nets[precision] = build_net(sd32, opt_json, precision=precision, **NET_KW.get(kind, {}))
    return sd64, nets[precision]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------

def seq_lengths(B, T, seed):
    g = torch.Generator().manual_seed(7000 + 131 * seed + 7 * B + T)
    return torch.cat([torch.tensor([T]), torch.randint(26, T + 1, (B - 1,), generator=g)]) if T > 26 else torch.full((B,), T)


def case_input(store, wname, B, T, seed):
    """-> (x float32 on the CPU (B, 1, 288, T), seq_length).  calibrated: rand * 2.5.  trained: the log-CQT of 16 synthetic clips from
    index 200 on; clip b is base clip b % 16 rolled by b // 16 semitones, cropped to T frames or continued with the clips behind it."""
    def make():
        if wname != "trained":
            g = torch.Generator().manual_seed(5000 + 131 * seed + 7 * B + T)
            return torch.rand((B, 1, 288, T), generator=g) * 2.5, seq_lengths(B, T, seed)
        base = memo(store, "trained-base", lambda: sensitive.trained_mel(range(200, 216), torch.float32)[:, 0])       # (16, 288, 76)
        rows = []
        for b in range(B):
            parts, k = [], 0
            while sum(p.shape[1] for p in parts) < T:
                parts.append(base[(b + k) % 16])
                k += 1
            rows.append(torch.roll(torch.cat(parts, dim=1)[:, :T], 3 * ((b // 16) % 12), dims=0))
        return torch.stack(rows)[:, None].contiguous(), seq_lengths(B, T, seed)
    return memo(store, ("input", wname, B, T, seed), make)


def reference(store, key, sd64, x, seq, idx, keep_taps=False, **oracle_kw):
    """sensitive.Bounds on the picked clips, after the response condition on the oracle alone."""
    def make():
        xs = x[idx].double()
        ss = None if seq is None else seq[idx]
        b = sensitive.bounds(sd64, xs, ss, keep_taps=keep_taps, **oracle_kw)
        b.response = sensitive.assert_responds(sd64, xs, ss, b.ref, what=str(key), **oracle_kw)
        return b
    return memo(store, ("reference",) + tuple(key), make)


# ---- running a case ------------------------------------------------------------------------------------------------------------------------

def run_timed(nbytes, call):
    """One run on a workspace of 0x77 bytes between guards, under the kernel timer -> (outputs, {kernel label: (ms, launches)})."""
    g = Guarded(nbytes, 0x77)
    _lib.prof_results()
    _lib.prof_enable("", True)
    try:
        outs = call(g.view, "sensitive")
        names = _lib.prof_results()
    finally:
        _lib.prof_enable("", False)
    g.check("sensitive: workspace")
    return outs, names


def hold_route_model(route, names, l0_in_lds, semi_fused, what):
    """pcnet_oracle.mixed_route against what the `mixed` forward launched: the kernel timer's labels and the tap answers."""
    has = lambda *labels: any(n in names for n in labels)
    want = {"pitch convs on f16": (any(".p2p.layer." in k for k in route), has(P2P_KEY)),
            "last pitch-class stack on bf16": (any(".pc2pc.layer." in k and not k.startswith("model.0.") and v == "bf16x3" for k, v in route.items()),
                                               has("pc2pc_fused_kernel", "conv_pc_bf16_kernel/pc2pc")),
            "first head conv on bf16": ("key_classifier.0.conv2d.weight" in route, has(FUSED_HEADS, "conv_pc_bf16_kernel/head")),
            "last head conv on bf16": ("key_classifier.3.conv2d.weight" in route, has(FUSED_HEADS, "conv_head1_bf16_kernel")),
            "semitone conv fused (f16)": (any(k.endswith("pool_semi.weight") for k in route), semi_fused)}
    if l0_in_lds is not None:
        want["layer 0 on f16 x 3 MFMA"] = (any(k.startswith("model.0.pc2pc.") for k in route), l0_in_lds)
    wrong = {k: v for k, v in want.items() if v[0] != v[1]}
    assert not wrong, f"{what}: the route restatement (model, device) disagrees: {wrong}; launched {sorted(names)}"


def compare(outs, b, idx, precision, what, budget=None):
    """Device outputs on the picked clips against the float64 reference, per output, at the precision's bound."""
    bound = b.bound(precision)
    errs = [rel_err(a[idx].cpu().reshape(r.shape), r) for a, r in zip(outs, b.ref)]
    print(f"  SENSITIVE {what} | {precision} | " + " | ".join(
        f"{n} resp {rs:.2f} f32 {e32:.1e} f32x3 {ex:.1e} model {em:.1e} dev {e:.1e} bound {bd:.1e}"
        for n, rs, e32, ex, em, e, bd in zip(OUTPUTS, b.response, b.e32, b.e32x3, b.emodel, errs, bound)))
    bad = [(n, e, bd) for n, e, bd in zip(OUTPUTS, errs, bound) if not e < bd]
    assert not bad, f"{what} {precision}: (output, device rel_err, bound) {bad}; b32 {b.b32}, bmix {b.bmix}"
    if budget is not None:
        assert max(errs) < budget, (what, precision, errs)
    return errs


# ---- a. the default net --------------------------------------------------------------------------------------------------------------------

HEAD_CASES = [f"heads{form}-{B}x{T}" for form in ("", "2") for B in (1, 3) for T in (80, 52, 28)]
CASES = ["3x76", "3x76-noseq", "2x100", "1x27", "3x77", "persistent", "persistent-frames-major", "one-launch", "257x40", "288x76", "keep-taps",
         "1x500", "1x1501", "nogenre", "local-2x120", "local-1x1500"] + HEAD_CASES


def case_shape(case, Bp):
    if case.startswith("heads"):
        B, T = case.split("-")[1].split("x")
        return int(B), int(T)
    return {"3x76": (3, 76), "3x76-noseq": (3, 76), "2x100": (2, 100), "1x27": (1, 27), "3x77": (3, 77), "persistent": (Bp, 76),
            "persistent-frames-major": (Bp, 76), "one-launch": (n_cus(), 76), "257x40": (257, 40), "288x76": (288, 76), "keep-taps": (3, 76),
            "1x500": (1, 500), "1x1501": (1, 1501), "nogenre": (3, 76), "local-2x120": (2, 120), "local-1x1500": (1, 1500)}[case]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("wname", ["calibrated", "trained"])
def test_default_net(store, wname, case, precision):
    """Per-tile 3 x 76 with and without seq_length; per-stage layer 0 (2 x 100); odd lengths; the persistent pitch convs through the plain
    and the frames-major entry; the one-launch stack; a chunk plus a one-clip remainder (257 x 40) and a 32-clip remainder (288 x 76);
    keep_taps; the time-tiled heads (1 x 500, 1 x 1501); the fused heads and, under keep_taps, their two-launch form at B 1 and 3,
    T 80, 52 and 28; without the genre head; --local at 2 x 120 and 1 x 1500."""
    L = _lib.lib()
    kind = "nogenre" if case == "nogenre" else "local" if case.startswith("local") else "default"
    local = kind == "local"
    keep = case == "keep-taps" or case.startswith("heads2")
    B, T = case_shape(case, persistent_batch(default_net(store, "trained", "mixed", "default")))       # (the route does not depend on the weights)
    x, seq = case_input(store, wname, B, T, 1)
    if case == "3x76-noseq" or local:
        seq = None
    idx = {"257x40": [0, 255, 256], "288x76": [0, 255, 256, 287]}.get(case, list(range(B)) if B <= 4 else sorted({0, B // 2, B - 1}))
    kw = dict(local_window=LOCAL_WINDOW) if local else {}
    sd64, net = case_weights_and_net(store, wname, precision, kind, x, seq, kw)
    assert not local or net.local_window == LOCAL_WINDOW
    if kind == "nogenre":
        sd64 = {k: v for k, v in sd64.items() if not k.startswith("genre_classifier")}
    b = reference(store, (wname, case), sd64, x, seq, idx, keep_taps=keep, **kw)
    xd, sq = x.to(DEV), None if seq is None else seq.to(DEV)
    was = L.ake_debug_keep_taps(1) if keep else None
    try:
        if case == "persistent-frames-major":
            nbytes, call = forward_call(net, xd[:, 0].transpose(1, 2).contiguous(), B, T, sq, "ake_pcnet_forward_frames_major_f32")
            if precision == "f32x3":                                  # only the f16 pitch convs' loader transposes: the entry refuses, it does not fall back
                assert L.ake_pcnet_accepts_frames_major(net.handle, B, T) == 0
                with pytest.raises(_lib.AkeError, match="does not take the frames-major input"):
                    call(Guarded(nbytes, 0x77).view, "frames-major under f32x3")
                return
        else:
            nbytes, call = forward_call(net, xd, B, T, sq, "ake_pcnet_forward_local_f32" if local else "ake_pcnet_forward_f32")
        outs, names = run_timed(nbytes, call)
        launches = names.get(P2P_KEY, (0.0, 0))[1]
        accepts = 0 if local else L.ake_pcnet_accepts_frames_major(net.handle, B, T)
        (l0_rc, l0_msg), (p8_rc, p8_msg), (up_rc, up_msg) = (tap_answer(net, nm, min(B, 256), T) for nm in
                                                             ("model.0.pc2pc.layer.2", "model.1.p2p.layer.8", "model.1.up_sixth_a"))
    finally:
        if was is not None:
            L.ake_debug_keep_taps(was)
    print(f"\n  {wname} {case} {precision}: {B} x {T}, {launches} launch(es) booked as {P2P_KEY}, frames-major {accepts}, layer 0 stack "
          f"{'in LDS' if l0_rc else 'written'}, last pitch conv {'fused' if p8_rc else 'written'}, up_sixth {'f16 words' if up_rc else 'f32'}; "
          f"launched {sorted(names)}")
    if precision == "mixed":
        if case in ("3x76", "3x76-noseq", "nogenre"):
            assert launches == 3 and accepts == 0, (launches, accepts)
            assert l0_rc and "stays in LDS (layer 0 runs as one launch)" in l0_msg, l0_msg
            assert p8_rc and "fused with the semitone conv" in p8_msg, p8_msg
        if case == "2x100":
            assert accepts == 0 and l0_rc == 0 and up_rc == 0, (accepts, l0_msg, up_msg)
        if case in ("1x27", "3x77"):                                  # odd frame counts: the tiled pitch conv writes the pitch tensor, the semitone conv runs on its own in f32
            assert accepts == 0 and launches == 3 and p8_rc == 0, (accepts, launches, p8_msg)
            assert {"semi_fold_kernel/L1+", "conv_pc_bf16_kernel/pc2pc"} | TWO_LAUNCH_HEADS <= set(names), sorted(names)
        if case.startswith("persistent"):
            assert accepts == 1 and up_rc and "held as f16 words" in up_msg, (accepts, up_msg)
        if case == "one-launch":
            assert launches == 1, launches
        if case in ("257x40", "288x76"):
            assert launches in (4, 6), launches                       # two chunks: one or three launches, then the remainder's three
        if case == "keep-taps":
            assert launches == 3 and p8_rc == 0 and l0_rc == 0, (launches, p8_msg, l0_msg)
        if case in ("1x500", "1x1501"):                               # beyond the f16 pitch convs and the bf16 heads: the time-tiled generic kernels
            assert launches == 0 and FUSED_HEADS not in names and not (TWO_LAUNCH_HEADS & set(names)), sorted(names)
            assert GENERIC <= set(names), sorted(names)
        if case.startswith("heads-"):
            assert FUSED_HEADS in names and not (TWO_LAUNCH_HEADS & set(names)), sorted(names)
        if case.startswith("heads2-"):
            assert TWO_LAUNCH_HEADS <= set(names) and FUSED_HEADS not in names, sorted(names)
        if local:
            assert "local_pool_kernel" in names, sorted(names)
        if case == "local-1x1500":
            assert (GENERIC - {"head_pool_kernel"}) <= set(names), sorted(names)
        # under keep_taps the layer-0 tap is written whatever the form: its form is then not visible from outside
        hold_route_model(b.route, names, None if keep else bool(l0_rc), bool(p8_rc) and "fused with the semitone conv" in p8_msg, f"{wname} {case}")
    compare(outs, b, idx, precision, f"{wname} {case}", BUDGET if (wname == "trained" and precision == "mixed") else None)
    if case == "persistent-frames-major":                             # the same bits as the plain entry on the transposed tensor
        nb, plain = forward_call(net, xd, B, T, sq)
        for a, c in zip(run_timed(nb, plain)[0], outs):
            assert torch.equal(a, c)


# ---- b. variants and configurations, calibrated ----------------------------------------------------------------------------------------------

VARIANT_SHAPES = {"resblock": [(3, 52)], "pc2p_mem": [(3, 52), (20, 76)], "p2pc_conv": [(3, 52), (5, 76)], "stay_sixth": [(3, 52), (64, 76)],
                  "denseblock": [(3, 52), (5, 76)], "denseblock-default-widths": [(3, 52)], "k3": [(3, 52), (24, 76)], "k5": [(3, 52), (24, 76)]}


def dense_default_widths():
    """The default widths (n_filters = 4, conv_layers = 3) of test_gpu_pcnet.test_denseblock_against_reference_fixture."""
    opt = Namespace(genre=True, denseblock=True, octaves=8, num_layers=2, kernel_size=7)
    torch.manual_seed(7)
    big = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
    gb = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for name, p in big.named_parameters():
            if p.dim() == 1 and ("norm" in name or "_b." in name or name.split(".")[-2].isdigit()):
                p.copy_(torch.rand(p.shape, generator=gb) + 0.5 if name.endswith("weight") else torch.randn(p.shape, generator=gb) * 0.1)
    return {k: v.detach().clone() for k, v in big.state_dict().items()}, json.dumps(vars(opt))


def variant(store, name, x, seq):
    """-> (calibrated float32 state_dict, float64, opt JSON, oracle keywords) of a variant fixture or a seeded configuration, its running
    statistics calibrated on the first 4 clips of the case's input (x, seq)."""
    def make():
        if name in sensitive.FIXTURES:
            fname, kw = sensitive.FIXTURES[name]
            gold = load_golden(fname)
            sd64, opt_json = golden_state_dict(gold, torch.float64), str(gold["opt"])
        elif name == "denseblock-default-widths":
            sd, opt_json = dense_default_widths()
            sd64, kw = pcnet_oracle.to_dtype(sd, torch.float64), {}
        else:
            cfg = next(c for c in sensitive.CONFIGS if sensitive.config_name(c) == name)
            _, opt, sd64, kw, _ = sensitive.config_net(cfg)
            opt_json = json.dumps(dict(vars(opt), octaves=8, num_layers=cfg.get("num_layers", 2), kernel_size=7))
        sd32 = pcnet_oracle.to_dtype(sensitive.calibrate(sd64, x[:4].double(), seq[:4], **kw), torch.float32)
        return sd32, pcnet_oracle.to_dtype(sd32, torch.float64), opt_json, kw
    return memo(store, ("variant", name, tuple(x.shape)), make)


VARIANT_CASES = [(n, B, T) for n, shapes in VARIANT_SHAPES.items() for B, T in shapes] + \
                [(sensitive.config_name(c), 3, 120 if (c.get("num_layers") == 3 or c.get("time_pool_size") == 4 or c.get("head_layers") == 3) else 52)
                 for c in sensitive.CONFIGS]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,B,T", VARIANT_CASES)
def test_variants_and_configurations(store, name, B, T, precision):
    """The architecture variants from their fixtures and the eight seeded configurations of test_other_configurations_against_oracle, all
    with calibrated running statistics: at 3 x 52 (the configurations at their existing shapes) and at the larger batch their existing
    tests use, three picks.  The rounding model takes the rounded convolutions from the route THIS net gets."""
    x, seq = case_input(store, "calibrated", B, T, 3)
    sd32, sd64, opt_json, kw = variant(store, name, x, seq)
    net = memo(store, ("variant-net", name, B, T, precision), lambda: build_net(sd32, opt_json, precision=precision))
    idx = list(range(B)) if B <= 4 else sorted({0, B // 2, B - 1})
    b = reference(store, ("variant", name, B, T), sd64, x, seq, idx, **kw)
    nbytes, call = forward_call(net, x.to(DEV), B, T, seq.to(DEV))
    outs, names = run_timed(nbytes, call)
    print(f"\n  {name} {B} x {T} {precision}: rounded by the model {sorted(b.route.items())}; launched {sorted(names)}")
    if precision == "mixed":
        (l0_rc, _), (p8_rc, p8_msg) = (tap_answer(net, nm, B, T) for nm in ("model.0.pc2pc.layer.2", "model.1.p2p.layer.8"))
        l0 = bool(l0_rc) if "layer0_fused_kernel" in names else False
        hold_route_model(b.route, names, l0, bool(p8_rc) and "fused with the semitone conv" in p8_msg, f"{name} {B} x {T}")
    compare(outs, b, idx, precision, f"{name} {B}x{T}")


# ---- c. end to end through KeyEstimator, the trained fixture -----------------------------------------------------------------------------

SR, HOP = 22050, 4410
ENTRIES = ["equal", "ragged", "pcm16", "frames-major", "48k-stereo", "frames0"]


def estimator(store, precision, frames=5):
    net = default_net(store, "trained", precision, "default")
    return memo(store, ("estimator", precision, frames), lambda: ake_amd.KeyEstimator(net, SR, frames, **({} if frames else dict(window_size=592))))


def oracle_cqt(y, hop=HOP, frames=None):
    """cqt_oracle's log-CQT of one clip (float64, (288, 1 + len(y) // hop)), zero-padded to `frames` frames."""
    import numpy as np
    from oracle import cqt_oracle
    m = cqt_oracle.FastDirectCQT(SR, hop, dtype=torch.float64)(np.asarray(y, np.float32)[None])[0]
    return m if frames is None else torch.nn.functional.pad(m, (0, frames - m.shape[1]))


def entry_case(store, entry, est):
    """-> (run(est) -> outputs, device mel (B, 288, T) of the estimator's own CQT call, the oracle's mel, seq_length or None, picks)."""
    import numpy as np
    from ake_amd import synthetic
    from ake_amd.cqt import hop_for_window
    from oracle import resample_oracle
    n = synthetic.N_SAMPLES
    if entry in ("equal", "ragged", "pcm16"):
        y = memo(store, "audio3", lambda: synthetic.make_batch(range(200, 203))[0])
        lens = [n, n - 3 * HOP - 17, n - 11 * HOP] if entry == "ragged" else [n] * 3
        src = torch.from_numpy(y).to(DEV)
        if entry == "pcm16":
            src = torch.round(src * 32767).to(torch.int16).contiguous()
        lengths = torch.tensor(lens, dtype=torch.int64, device=DEV) if entry == "ragged" else None
        host = src.cpu().float() / 32768 if entry == "pcm16" else torch.from_numpy(y)
        ref_mel = memo(store, ("oracle-mel", entry), lambda: torch.stack([oracle_cqt(host[i, :k].numpy(), frames=76) for i, k in enumerate(lens)]))
        return (lambda e: e(src, lengths)), est.plan.logmag(src, lengths=lengths), ref_mel, torch.tensor([1 + k // HOP for k in lens]), [0, 1, 2]
    if entry == "frames-major":
        Bp = persistent_batch(default_net(store, "trained", "mixed", "default"))      # (an f32x3 net runs the same batch through the plain CQT layout)
        y = memo(store, ("audio", Bp), lambda: synthetic.make_batch(range(200, 200 + Bp))[0])
        src = torch.from_numpy(y).to(DEV)
        idx = sorted({0, Bp // 2, Bp - 1})
        ref_mel = memo(store, ("oracle-mel", entry, Bp), lambda: torch.stack([oracle_cqt(y[i]) for i in idx]))
        return (lambda e: e(src)), est.plan.logmag(src)[idx], ref_mel, torch.full((3,), 76), idx
    if entry == "48k-stereo":
        def make():
            a = np.stack([np.stack([synthetic.make_clip(200 + b, 48000 * 15, 48000)[0], synthetic.make_clip(210 + b, 48000 * 15, 48000)[0]]) for b in range(2)])
            mono = np.stack([resample_oracle.prepare(a[b], 48000, SR, 0) for b in range(2)])
            return a.astype(np.float32), torch.stack([oracle_cqt(m) for m in mono])
        a, ref_mel = memo(store, "audio48", make)
        src = torch.from_numpy(a).to(DEV)
        mono_dev, _ = ake_amd.Resampler(48000, SR, DEV)(src, channel=0)
        T = ref_mel.shape[2]
        return (lambda e: e(src, rate=48000, channel=0)), est.plan.logmag(mono_dev), ref_mel, torch.full((2,), T), [0, 1]
    assert entry == "frames0"
    clips = memo(store, "songs", lambda: [synthetic.make_clip(200, 20 * SR)[0], synthetic.make_clip(201, 31 * SR)[0]])
    rows = np.zeros((2, len(clips[1])), np.float32)
    for i, c in enumerate(clips):
        rows[i, :len(c)] = c
    src, lens = torch.from_numpy(rows).to(DEV), torch.tensor([len(c) for c in clips], dtype=torch.int64, device=DEV)
    hops = hop_for_window(lens, 592).to(torch.int32)
    ref_mel = memo(store, ("oracle-mel", entry), lambda: torch.stack([oracle_cqt(c, len(c) // 592 + 1, 592) for c in clips]))
    return (lambda e: e(src, lens)), est.plan.logmag_hops(src, hops, lens, out_frames=592), ref_mel, None, [0, 1]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_end_to_end_entries(store, entry, precision):
    """KeyEstimator on synthetic clips from index 200 on: equal-length, ragged and 16-bit PCM audio, a batch that takes the frames-major
    pipeline, 48 kHz stereo through the resampler, whole songs (--frames 0).  Two assertions, so that no new number is needed: the
    entry's outputs against the oracle net on the DEVICE'S OWN CQT (the estimator's CQT call on the same audio) are within the bounds of
    (a) -- plumbing and net; the oracle net on the device's CQT against the oracle net on cqt_oracle's CQT is below 1e-3 -- the front end
    as the net sees it."""
    est = estimator(store, precision, 0 if entry == "frames0" else 5)
    _, sd64, _ = default_weights(store, "trained")
    run, mel_dev, mel_ref, seq, idx = entry_case(store, entry, est)
    if entry == "frames-major":
        assert _lib.lib().ake_pcnet_accepts_frames_major(est.net.handle, persistent_batch(default_net(store, "trained", "mixed", "default")), 76) \
            == (1 if precision == "mixed" else 0)
    outs = run(est)
    torch.cuda.synchronize()
    x = mel_dev[:, None].cpu().float()
    assert x.shape[1:] == (1, 288, mel_ref.shape[2]) and x.shape[0] == len(idx), (x.shape, mel_ref.shape)
    # (the mel is the same tensor for both precisions of an entry: the CQT does not depend on the net's precision)
    b = reference(store, ("entry", entry), sd64, x, seq, list(range(len(idx))))
    print()
    compare(outs, b, idx, precision, f"end-to-end {entry}", BUDGET if precision == "mixed" else None)
    with torch.no_grad():
        front = pcnet_oracle.pcnet_forward(sd64, mel_ref[:, None], seq)
    e = [rel_err(a, r) for a, r in zip(b.ref, front)]
    print(f"  SENSITIVE-CQT end-to-end {entry} | oracle net on the device's CQT against the oracle net on cqt_oracle's: " + " ".join(f"{n} {v:.1e}" for n, v in zip(OUTPUTS, e)))
    assert max(e) < 1e-3, (entry, e)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_end_to_end_track(store, precision):
    """KeyEstimator.track on one two-segment recording (30 s, 4 windows): the windows' outputs under the same two assertions as the
    entries above, and the decoded key ids equal the oracle's decode wherever that decode has a margin of more than twice the output
    bound (sensitive.decode_is_certain); at most 5 % of the windows may lack it (tests/test_sensitive_host.py holds the recording to
    that on the oracle alone)."""
    from ake_amd import metrics
    from oracle import cqt_oracle
    est = estimator(store, precision)
    _, sd64, _ = default_weights(store, "trained")
    y = memo(store, "track-audio", sensitive.track_recording)
    src = torch.from_numpy(y).to(DEV)
    tr = est.track(src)
    torch.cuda.synchronize()
    W = int(tr.counts[0])
    win = sensitive.windows_of(est.plan.logmag(src)[0].cpu().float())
    assert W == win.shape[0] == 4 and tr.window_frames == sensitive.TRACK_WF and tr.stride_frames == sensitive.TRACK_SF
    seq = torch.full((W,), sensitive.TRACK_WF)
    b = reference(store, ("track",), sd64, win, seq, list(range(W)))
    print()
    compare([tr.key[0], tr.tonic[0], tr.genre[0]], b, list(range(W)), precision, "end-to-end track", BUDGET if precision == "mixed" else None)
    ref_win = memo(store, "track-oracle-windows",
                   lambda: sensitive.windows_of(cqt_oracle.FastDirectCQT(SR, HOP, dtype=torch.float64)(y)[0]))
    with torch.no_grad():
        front = pcnet_oracle.pcnet_forward(sd64, ref_win, seq)
    e = [rel_err(a, r) for a, r in zip(b.ref, front)]
    print("  SENSITIVE-CQT end-to-end track | oracle net on the device's CQT against the oracle net on cqt_oracle's: " + " ".join(f"{n} {v:.1e}" for n, v in zip(OUTPUTS, e)))
    assert max(e) < 1e-3, e
    bound = b.bound(precision)
    sure = sensitive.decode_is_certain(b.ref[0], b.ref[1], bound[0], bound[1])
    want = metrics.decode_keys(b.ref[0], b.ref[1])[0]
    got = tr.key_id[0, :W].cpu()
    print(f"  key ids: device {got.tolist()}, oracle {want.tolist()}, certain {sure.tolist()}")
    assert int((~sure).sum()) <= 0.05 * W and torch.equal(got[sure], want[sure])
