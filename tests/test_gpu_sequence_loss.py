"""GPU: the sequence loss -- ake_key_sequence_loss_f32 against metrics.key_sequence_loss in float64 on the device's own float32 inputs,
ake_amd.key_sequence_loss as an autograd function, KeyEstimator.training_windows(sequence_windows=K) and PitchClassNet.general_step on its
batches.

The bound on every compared tensor X, per tensor for the loss and d_trans and per window row for d_key, d_tonic and d_emis, comes from
the models alone:

    |X_kernel - X_64| <= max(4 * max|X_32 - X_64|, 2^-20 * max|X_64|)

with X_32 metrics.key_sequence_loss in float32 on the CPU on the same inputs: what the same formulas cost in float32, times 4 for the
kernels' fast exp / log and fixed summation order (the posterior tests found the kernels' error to match the float32 host model's own),
and a floor of two float32 ulps of the row's largest value.

Measured on an MI355X (profiles/track_sequence.md has the table): the worst error / bound over all cases is 0.06 for the loss, 0.07 for
d_key, 0.06 for d_tonic and d_emis and 0.16 for d_trans.  The entry computes the emissions, the chains and the gradient in double and
rounds once: a first build on the tracker's float32 chains was as exact as the float32 host model over whole tensors but missed this
bound in single rows by up to 2.05 x (float32 log-scores carry a posterior only to |log-odds| * 2^-24, which is the floor at 16)."""
import functools
import json
import math
from argparse import Namespace

import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict
from test_gpu_windows import run_loss
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, WF = 4410, 76
NAMES = ("loss", "d_key", "d_tonic", "d_trans", "d_emis")


def default_trans(stride=5.0):
    return metrics.key_transition_log(stay=math.exp(-stride / 60.0)).float()


def device_loss(key, tonic, labels, A, counts=None, prior=None, weight=1.0, trans=True, emis=True, poison=0xAB):
    """ake_key_sequence_loss_f32 on float32 tensors given on the CPU -> dict on the CPU.  The outputs are guarded tensors pre-filled with
    0xFF bytes and the workspace is guarded and poisoned: what the kernels do not write shows, and so does what they write elsewhere."""
    L = _lib.lib()
    R, W, _ = key.shape
    k_d, t_d, A_d = key.to(DEV).contiguous(), tonic.to(DEV).contiguous(), A.to(DEV).contiguous()
    assert k_d.dtype == t_d.dtype == A_d.dtype == torch.float32
    l_d = labels.to(device=DEV, dtype=torch.int32).contiguous()
    c_d = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    p_d = None if prior is None else prior.to(DEV).contiguous()
    nbytes = L.ake_key_sequence_loss_workspace_bytes(R, W)
    assert nbytes >= 6 * R * W * 24 * (8 + 4)
    ws, ws_check = guarded(nbytes, poison)
    out = {"scalars": GuardedTensor((4,)), "d_key": GuardedTensor((R, W, 12)), "d_tonic": GuardedTensor((R, W, 12)),
           "d_trans": GuardedTensor((24, 24)) if trans else None, "d_emis": GuardedTensor((R, W, 24)) if emis else None}
    ptr = lambda t: None if t is None else (t.t if isinstance(t, GuardedTensor) else t).data_ptr()       # noqa: E731
    _lib.check(L.ake_key_sequence_loss_f32(k_d.data_ptr(), t_d.data_ptr(), l_d.data_ptr(), R, W, ptr(c_d), A_d.data_ptr(), ptr(p_d), float(weight),
                                           ptr(out["scalars"]), ptr(out["d_key"]), ptr(out["d_tonic"]), ptr(out["d_trans"]), ptr(out["d_emis"]),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "ake_key_sequence_loss_f32")
    torch.cuda.synchronize()
    ws_check("ake_key_sequence_loss_f32 workspace")
    for name, g in out.items():
        if g is not None:
            g.check(name)
    res = {k: None if g is None else g.t.cpu().clone() for k, g in out.items()}
    res["loss"], res["loglik"], res["loglik_clamped"], res["labelled"] = res["scalars"].unbind(0)
    return res


def inputs(R, W, seed, tonic_scale=3.0):
    g = torch.Generator().manual_seed(seed)
    key = torch.rand((R, W, 12), generator=g) * 0.98 + 0.01
    tonic = torch.randn((R, W, 12), generator=g) * tonic_scale
    labels = torch.randint(0, 24, (R, W), generator=g)
    drop = torch.rand((R, W), generator=g)
    labels[drop < 0.2] = -1                                                               # unlabelled windows, three spellings of them
    labels[(drop >= 0.2) & (drop < 0.25)] = 24
    labels[(drop >= 0.25) & (drop < 0.3)] = -7
    return key, tonic, labels, g


SHAPES = {(1, 1): None, (3, 9): [9, 5, 1], (5, 40): [40, 0, 17, 40, 8], (2, 17): None, (1, 300): None}
# (1, 300) crosses the chains' 8-step prefetch and the 256-window chunk of the back-pointers' neighbours; (5, 40) holds a count of 0


@functools.lru_cache(maxsize=None)
def case(R, W, with_prior):
    """One case with its two models, computed once: the prior cases also take signature_weight 0.5 and a transition with -1e4 cells."""
    key, tonic, labels, g = inputs(R, W, 1000 * R + W)
    if (R, W) == (1, 1):
        labels[0, 0] = 5
    A = default_trans()
    prior, weight = None, 1.0
    if with_prior:
        prior, weight = torch.randn(24, generator=g), 0.5
        A = A.clone()
        forbidden = ((3, 17), (17, 3), (0, 5), (20, 8))
        for i, j in forbidden:
            A[i, j] = -1e4
        # no labelled path takes a forbidden move (the second window of such a pair is left unlabelled): a path through a -1e4 cell puts
        # both log-likelihoods at a magnitude whose float32 ulp is 1e-3, where no model of the rounding says anything about the loss
        for r in range(R):
            for w in range(1, W):
                if (int(labels[r, w - 1]), int(labels[r, w])) in forbidden:
                    labels[r, w] = -1
    counts = SHAPES[(R, W)]
    f64 = lambda t: None if t is None else t.double()                                     # noqa: E731
    want = metrics.key_sequence_loss(f64(key), f64(tonic), labels, f64(A), counts, weight, f64(prior))
    host32 = metrics.key_sequence_loss(key, tonic, labels, A, counts, weight, prior)
    return (key, tonic, labels, A, counts, prior, weight), want, host32


def ratios(got, want, host32):
    """For each compared tensor the worst error / bound (<= 1 passes), the worst error and the float32 host model's worst error."""
    out = {}
    for name in NAMES:
        if got.get(name) is None:
            continue
        x, x64, x32 = got[name].double(), want[name], host32[name].double()
        per_row = name in ("d_key", "d_tonic", "d_emis")
        amax = (lambda t: t.abs().amax(dim=-1)) if per_row else (lambda t: t.abs().max())
        err, bound = amax(x - x64), torch.maximum(4.0 * amax(x32 - x64), 2.0 ** -20 * amax(x64))
        assert bool(torch.isfinite(x).all()), name
        # (a bound of 0 -- rows behind the counts, d_trans of single windows -- asks for exact zeros)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        out[name] = (float(ratio.max()), float(err.max()), float(amax(x32 - x64).max()), bool((err <= bound).all()))
    return out


def report(tag, r):
    print(f"{tag}: " + "; ".join(f"{k} error/bound {v[0]:.3f} (error {v[1]:.2e}, float32 host model {v[2]:.2e})" for k, v in r.items()))


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("R,W", list(SHAPES))
def test_kernel_against_the_float64_model(R, W, with_prior):
    """The bound of the module docstring on every tensor."""
    args, want, host32 = case(R, W, with_prior)
    got = device_loss(*args)
    r = ratios(got, want, host32)
    report(f"sequence loss R={R} W={W} prior={with_prior}", r)
    counts = SHAPES[(R, W)] or [W] * R
    live = torch.arange(W)[None, :] < torch.tensor(counts)[:, None]
    for name in ("d_key", "d_tonic", "d_emis"):
        assert bool((got[name][~live] == 0).all()), name                                 # zeros behind the counts, over the 0xFF fill
    assert float(got["labelled"]) == float(want["labelled"]) > 0
    assert float(got["loss"]) >= 0.0
    for name, x64 in (("loglik", want["loglik"]), ("loglik_clamped", want["loglik_clamped"])):
        assert abs(float(got[name]) - float(x64)) <= 2e-6 * max(1.0, abs(float(x64))), name
    assert all(v[3] for v in r.values()), {k: v for k, v in r.items() if not v[3]}


def test_null_outputs_and_bit_identical_reruns():
    args, _, _ = case(5, 40, True)
    full = device_loss(*args)
    again = device_loss(*args, poison=0x00)                                              # a second run, another workspace content
    for name in ("scalars", "d_key", "d_tonic", "d_trans", "d_emis"):
        assert torch.equal(full[name], again[name]), name
    bare = device_loss(*args, trans=False, emis=False)
    assert bare["d_trans"] is None and bare["d_emis"] is None
    for name in ("scalars", "d_key", "d_tonic"):
        assert torch.equal(full[name], bare[name]), name
    key, tonic, labels, A, counts, prior, weight = args
    clamped = device_loss(key, tonic, labels, A, [99, -3, 17, 40, 8], prior, weight)       # counts are clamped to 0..W
    for name in ("scalars", "d_key", "d_tonic", "d_trans", "d_emis"):
        assert torch.equal(full[name], clamped[name]), name
    a23, _, _ = case(2, 17, False)
    null_counts = device_loss(*a23)
    given = device_loss(a23[0], a23[1], a23[2], a23[3], [17, 17], a23[5], a23[6])
    for name in ("scalars", "d_key", "d_tonic", "d_trans", "d_emis"):
        assert torch.equal(null_counts[name], given[name]), name


def test_saturated_rows():
    """Memberships of exactly 0 and 1, a subnormal one and 1e-30, tonic logits of +-40: finite everywhere, a zero derivative where the
    clamp or the subnormal rule applies, and the same bound -- in a case of its own, so that the 1 / p magnitudes loosen no other."""
    key, tonic, labels, _ = inputs(2, 6, 77)
    p = torch.tensor([0.0, 1.0, 1e-45, 1e-30], dtype=torch.float32)
    key[0, 1, :4], key[1, 2, 4:8], key[1, 4, 8:] = p, p, p
    key[0, 3] = (key[0, 3] > 0.5).float()
    tonic[0, 1, 0], tonic[0, 1, 5], tonic[1, 2, 2], tonic[1, 5, 7] = 40.0, -40.0, -40.0, 40.0
    labels[0, 1], labels[1, 2], labels[1, 4], labels[0, 3] = 3, 14, -1, 9
    A = default_trans()
    want = metrics.key_sequence_loss(key.double(), tonic.double(), labels, A.double())
    host32 = metrics.key_sequence_loss(key, tonic, labels, A)
    got = device_loss(key, tonic, labels, A)
    r = ratios(got, want, host32)
    report("sequence loss, saturated rows", r)
    for r_, w, j0 in ((0, 1, 0), (1, 2, 4), (1, 4, 8)):
        assert abs(float(got["d_key"][r_, w, j0 + 3])) > 1e18                                   # p = 1e-30: the 1 / p term is there
        assert abs(float(got["d_key"][r_, w, j0 + 2])) < 1.0 and abs(float(got["d_key"][r_, w, j0])) < 1.0      # p = 1e-45 and 0: it is not
    assert all(v[3] for v in r.values()), {k: v for k, v in r.items() if not v[3]}


def test_nothing_labelled_gives_exact_zeros():
    key, tonic, labels, _ = inputs(2, 9, 78)
    for lab, counts in ((torch.full_like(labels, -1), [9, 4]), (labels, [0, 0])):
        got = device_loss(key, tonic, lab, default_trans(), counts)
        assert got["scalars"].tolist() == [0.0, 0.0, 0.0, 0.0]
        for name in ("d_key", "d_tonic", "d_trans", "d_emis"):
            assert bool((got[name] == 0).all()), name


def test_errors_of_the_entry_point():
    L = _lib.lib()
    key, tonic = torch.full((2, 5, 12), 0.5, device=DEV), torch.zeros((2, 5, 12), device=DEV)
    labels = torch.zeros((2, 5), dtype=torch.int32, device=DEV)
    A = default_trans().to(DEV)
    scal, dk, dt = torch.empty(4, device=DEV), torch.empty((2, 5, 12), device=DEV), torch.empty((2, 5, 12), device=DEV)
    nbytes = L.ake_key_sequence_loss_workspace_bytes(2, 5)
    assert nbytes > 0 and L.ake_key_sequence_loss_workspace_bytes(0, 5) == 0 and L.ake_key_sequence_loss_workspace_bytes(2, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call(R=2, W=5, ws_bytes=nbytes, **null):
        p = lambda name, t: None if null.get(name) else t.data_ptr()                       # noqa: E731
        return L.ake_key_sequence_loss_f32(p("key", key), p("tonic", tonic), p("labels", labels), R, W, None, p("trans", A), None, 1.0,
                                           p("scalars", scal), p("d_key", dk), p("d_tonic", dt), None, None, ws.data_ptr(), ws_bytes, None)

    assert call(ws_bytes=nbytes - 1) == -4                                                # AKE_ERR_WORKSPACE
    assert b"workspace" in L.ake_last_error()
    assert call(R=0) == -1 and call(W=0) == -1 and call(R=-2) == -1                       # AKE_ERR_INVALID
    for name in ("key", "tonic", "labels", "trans", "scalars", "d_key", "d_tonic"):
        assert call(**{name: True}) == -1, name
    assert call() == 0
    torch.cuda.synchronize()


# ---- the autograd function ----

def test_backward_hands_out_the_entrys_gradients_times_the_upstream_scalar():
    args, _, _ = case(3, 9, True)
    key, tonic, labels, A, counts, prior, weight = args
    entry = device_loss(*args)
    k, t, a = key.to(DEV).requires_grad_(), tonic.to(DEV).requires_grad_(), A.to(DEV).requires_grad_()
    loss = ake_amd.key_sequence_loss(k, t, labels.to(DEV), a, counts=counts, signature_weight=weight, log_prior=prior)
    assert loss.shape == () and loss.dtype == torch.float32 and torch.equal(loss.detach().cpu(), entry["loss"])
    (2.5 * loss).backward()
    assert torch.equal(k.grad.cpu(), 2.5 * entry["d_key"]) and torch.equal(t.grad.cpu(), 2.5 * entry["d_tonic"])
    assert torch.equal(a.grad.cpu(), 2.5 * entry["d_trans"])                             # a log_trans leaf receives d_trans
    # a transition that asks for no gradient: the same loss and head gradients, float64 heads get float64 gradients of the same values
    k64, t64 = key.double().to(DEV).requires_grad_(), tonic.double().to(DEV).requires_grad_()
    loss64 = ake_amd.key_sequence_loss(k64, t64, labels.to(DEV), A.to(DEV), counts=counts, signature_weight=weight, log_prior=prior)
    loss64.backward()
    assert loss64.dtype == torch.float64 and float(loss64) == float(entry["loss"])
    assert k64.grad.dtype == torch.float64 and torch.equal(k64.grad.cpu(), entry["d_key"].double())
    assert torch.equal(t64.grad.cpu(), entry["d_tonic"].double())
    with pytest.raises(ValueError, match="labels"):
        ake_amd.key_sequence_loss(k, t, labels[:, :3].to(DEV), a)
    with pytest.raises(ValueError, match="log_trans"):
        ake_amd.key_sequence_loss(k, t, labels.to(DEV), a[:12])


# ---- end to end: sequence batches and general_step ----

SECONDS = (60.0, 52.0, 45.0)
K, STRIDE_S, SF = 4, 5.0, 25


def make_net(gold, **opt_kw):
    opt = Namespace(**{**json.loads(str(gold["opt"])), **opt_kw})
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return net.to(DEV)


@pytest.fixture(scope="module")
def recordings():
    """Three modulating recordings of 60 / 52 / 45 s (ragged), their annotations and lengths, on the device."""
    audio, ann, lengths = synthetic.make_modulating_batch_device([0, 1, 2], SECONDS, DEV, min_seconds=8.0, mean_seconds=15.0)
    torch.cuda.synchronize()
    return audio, ann, lengths


@pytest.fixture(scope="module")
def estimator(gold_default):
    return ake_amd.KeyEstimator(make_net(gold_default), 22050, 5)


def test_sequence_batches_end_to_end(estimator, recordings):
    audio, ann, lengths = recordings
    frames = [1 + int(n) // HOP for n in lengths.tolist()]
    mel_all = estimator.plan.logmag(audio, lengths=lengths)
    tw = estimator.training_windows(audio, ann, lengths=lengths, batch_size=2, batches_per_epoch=3, seed=5, sequence_windows=K, stride_seconds=STRIDE_S)
    assert tw.sequence_windows == K and tw.stride_frames == SF and len(tw) == 3
    prefix = metrics.window_prefix(frames, WF + (K - 1) * SF)
    A = metrics.key_transition_log(stay=math.exp(-SF * HOP / 22050 / 60.0)).float()
    epochs = [list(tw), list(tw)]
    assert tw.epoch == 2
    B = 2 * K
    for e, batches in enumerate(epochs):
        for i, batch in enumerate(batches):
            assert batch["sequence_shape"] == (2, K) and batch["mel"].shape == (B, 1, 288, WF)
            assert set(batch) == {"mel", "key_labels", "tonic_labels", "key_signature_id", "genre", "seq_length", "sample_weight", "recording",
                                  "start_frame", "sequence_shape", "key_id", "log_trans"}
            rec, st = metrics.sequence_windows(prefix, 5, e, 2 * i, 2, K, SF)
            assert batch["recording"].tolist() == rec and batch["start_frame"].tolist() == st
            assert batch["recording"].dtype == batch["start_frame"].dtype == batch["key_id"].dtype == torch.int32 and batch["key_id"].shape == (B,)
            for b in range(B):                                                           # rows are slices of the plan's own transform
                assert st[b] + WF <= frames[rec[b]] and torch.equal(batch["mel"][b, 0], mel_all[rec[b], :, st[b]:st[b] + WF])
            want = metrics.window_labels(ann.seg_start.cpu(), ann.seg_key.cpu(), ann.seg_count.cpu(), rec, st, HOP, WF)
            for k in ("key_labels", "tonic_labels", "key_signature_id", "seq_length", "sample_weight"):
                assert torch.equal(batch[k].cpu(), want[k]), k
            assert torch.equal(batch["key_id"].cpu(), torch.where(want["sample_weight"] > 0, want["truth"], torch.full_like(want["truth"], -1)))
            assert batch["log_trans"].shape == (24, 24) and torch.equal(batch["log_trans"].cpu(), A)
    assert [b["start_frame"].tolist() for b in epochs[0]] != [b["start_frame"].tolist() for b in epochs[1]]
    # a user transition is passed through as it is; min_purity turns impure windows into unlabelled ones
    mine = torch.nn.Parameter(A.clone().to(DEV))
    strict = estimator.training_windows(audio, ann, lengths=lengths, batch_size=4, batches_per_epoch=2, seed=5, sequence_windows=K, stride_seconds=STRIDE_S,
                                        transition=mine, min_purity=1.0)
    ids, weights = [], []
    for batch in strict:
        assert batch["log_trans"] is mine
        ids.append(batch["key_id"].cpu()), weights.append(batch["sample_weight"].cpu())
    ids, weights = torch.cat(ids), torch.cat(weights)
    assert bool((ids[weights == 0] == -1).all()) and bool((ids[weights > 0] >= 0).all()) and 0 < int((weights == 0).sum()) < len(ids)
    # refusals; and without sequence_windows the grid mode of today
    with pytest.raises(ValueError, match="sequence_windows"):
        estimator.training_windows(audio, ann, lengths=lengths, sequence_windows=1, stride_seconds=STRIDE_S)
    with pytest.raises(ValueError, match="stride"):
        estimator.training_windows(audio, ann, lengths=lengths, sequence_windows=K)
    with pytest.raises(ValueError, match="sequence"):
        estimator.training_windows(audio, ann, lengths=lengths, sequence_windows=12, stride_seconds=STRIDE_S)
    with pytest.raises(ValueError, match="transition"):
        estimator.training_windows(audio, ann, lengths=lengths, sequence_windows=K, stride_seconds=STRIDE_S, transition=torch.zeros(24))
    grid = next(iter(estimator.training_windows(audio, ann, lengths=lengths, batch_size=8, stride_seconds=STRIDE_S)))
    assert "sequence_shape" not in grid and "key_id" not in grid and grid["start_frame"].tolist() == [w * SF for w in range(8)]


def test_general_step_adds_the_weighted_sequence_loss(gold_default, estimator, recordings):
    audio, ann, lengths = recordings
    tw = estimator.training_windows(audio, ann, lengths=lengths, batch_size=2, batches_per_epoch=1, seed=3, sequence_windows=K, stride_seconds=STRIDE_S)
    batch = next(iter(tw))
    net = make_net(gold_default, sequence_weight=0.7, signature_weight=0.5).eval()
    with torch.no_grad():
        out = net(batch["mel"], batch["seq_length"])
        case_ = (out[0], out[1], out[2], batch["key_labels"], batch["tonic_labels"], batch["genre"], batch["key_signature_id"])
        windows = run_loss(case_, batch["sample_weight"], (1.0, 1.0, 0.1), grads=False)[0]
        alone = ake_amd.key_sequence_loss(out[0].view(2, K, 12), out[1].view(2, K, 12), batch["key_id"].view(2, K), batch["log_trans"], signature_weight=0.5)
        vals = torch.stack(net.general_step(batch, 0, "val")).cpu()
        assert torch.equal(net.last_sequence_loss.cpu(), alone.cpu()) and float(alone) > 0
        assert torch.equal(vals[1:], windows[1:])                                        # the nine metrics keep their order and values
        assert torch.equal(vals[0], windows[0] + 0.7 * alone.cpu())
        # a batch without sequence_shape returns the bits it returns today: the weighted entry's
        plain = {k: v for k, v in batch.items() if k not in ("sequence_shape", "key_id", "log_trans")}
        assert torch.equal(torch.stack(net.general_step(plain, 0, "val")).cpu(), windows)
    # the sequence term's gradient reaches the parameters
    grads = []
    for weight in (0.0, 1.0):
        net = make_net(gold_default, sequence_weight=weight).train()
        net.general_step(batch, 0, "train")[0].backward()
        grads.append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu())
    assert bool(torch.isfinite(grads[1]).all()) and not torch.equal(grads[0], grads[1])
    local = Namespace(**{**json.loads(str(gold_default["opt"])), "local": True, "genre": False})
    with pytest.raises(ValueError, match="--local"):
        ake_amd.PitchClassNet(288, 12, local.num_layers, local.kernel_size, local).general_step(batch, 0, "train")


class Watched:
    """An iterable that hands a TrackWindows' batches on and notes the net's sequence loss after every step."""

    def __init__(self, tw, net, log):
        self.tw, self.net, self.log = tw, net, log

    def __len__(self):
        return len(self.tw)

    def __iter__(self):
        for batch in self.tw:
            yield batch
            self.log.append(self.net.last_sequence_loss)


def test_fit_is_reproducible_and_lowers_the_sequence_loss(gold_default, estimator, recordings):
    audio, ann, lengths = recordings

    def fit(sequence_weight):
        net = make_net(gold_default, sequence_weight=sequence_weight)
        tw = estimator.training_windows(audio, ann, lengths=lengths, batch_size=2, batches_per_epoch=6, seed=5, sequence_windows=K, stride_seconds=STRIDE_S)
        log = []
        trainer = ake_amd.Trainer(max_epochs=2, accumulate_grad_batches=1)
        trainer.fit(net, train_dataloaders=Watched(tw, net, log))
        torch.cuda.synchronize()
        assert tw.epoch == 2 and len(trainer.train_losses) == 12 and len(log) == 12
        return net.flat_parameters()[0].clone().cpu(), trainer.train_losses, [float(v) for v in log]

    (w1, l1, s1), (w2, l2, s2), (w0, l0, _) = fit(1.0), fit(1.0), fit(0.0)
    assert torch.equal(w1, w2) and l1 == l2 and s1 == s2                                 # to the bit
    assert not torch.equal(w1, w0) and l1 != l0
    assert bool(torch.isfinite(w1).all()) and all(math.isfinite(v) for v in l1 + s1)
    first, last = sum(s1[:4]) / 4, sum(s1[-4:]) / 4
    print(f"sequence loss over 12 steps: {[round(v, 4) for v in s1]}; first third {first:.4f}, last third {last:.4f}")
    assert last < first
