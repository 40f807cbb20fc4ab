"""GPU: training windows of annotated recordings -- the draw (ake_draw_windows_i32), the gather with labels and weights
(ake_window_batch_f32), the weighted fused loss (ake_general_step_weighted_f32) and KeyEstimator.training_windows end to end -- against
the host models in ake_amd.metrics.  The draw, the gather and the labels are exact (torch.equal); the loss is held to the tolerance
tests/test_gpu_loss.py holds ake_general_step_f32 to.  No accuracy is asserted anywhere: the net has seeded weights, not trained ones."""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict
from test_windows_host import BIG_PREFIX, FRAMES, HOP, WF, annotations, loss_case, purity_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the draw ----

def device_draw(prefix, seed, epoch, first_slot, batch):
    rec, start = ake_amd.draw_windows(torch.tensor(prefix, dtype=torch.int64, device=DEV), seed, epoch, first_slot, batch)
    torch.cuda.synchronize()
    assert rec.dtype == torch.int32 and start.dtype == torch.int32
    return rec.cpu().tolist(), start.cpu().tolist()


@pytest.mark.parametrize("prefix,seed,epoch,first_slot,batch", [
    (metrics.window_prefix(FRAMES, WF), 1234, 0, 0, 1),
    (metrics.window_prefix(FRAMES, WF), 1234, 0, 0, 8),
    (metrics.window_prefix(FRAMES, WF), 2 ** 40 + 5, 3, 8, 300),         # more than one block; the seed's high word
    (metrics.window_prefix((1500,), WF), 7, 1, 0, 64),                   # R = 1
    (metrics.window_prefix(FRAMES, WF), 7, 2 ** 32 - 1, 2 ** 32 + 11, 64),   # first_slot beyond 2^32
    ([0, 0, 1, 1], 1, 0, 0, 16),                                         # N = 1, empty recordings on both sides
    (BIG_PREFIX, 3, 0, 0, 64),                                           # N = 2^33 + 7: indices above 2^32 (a prefix alone: nothing is gathered)
])
def test_draw_equals_the_host_model(prefix, seed, epoch, first_slot, batch):
    rec, start, index = metrics.draw_windows(prefix, seed, epoch, first_slot, batch)
    if prefix[-1] > 2 ** 33:
        assert max(index) > 2 ** 32
    assert device_draw(prefix, seed, epoch, first_slot, batch) == (rec, start)


# ---- the gather, the labels and the weights, straight through the C ABI with every output poisoned ----

def raw_batch(mel, fm, rec, start, wf, hop=HOP, ann=None, min_purity=0.0, uniform=False, gather=True):
    """-> dict of CPU tensors; mel (R, P, T) or (R, T, P) with fm.  Outputs are filled with NaN / -77 before the launch."""
    R = mel.shape[0] if mel is not None else ann[0].shape[0]
    T, P = ((mel.shape[1], mel.shape[2]) if fm else (mel.shape[2], mel.shape[1])) if mel is not None else (10 ** 6, 1)
    B = len(rec)
    rec_d, start_d = (torch.as_tensor(t).to(device=DEV, dtype=torch.int32).contiguous() for t in (rec, start))
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out = {"mel": nan(B, 1, P, wf)} if gather else {}
    a = [None] * 3
    if ann is not None:
        a = [t.to(device=DEV, dtype=dt).contiguous() for t, dt in zip(ann, (torch.int64, torch.int32, torch.int32))]
        out.update(key_labels=nan(B, 12), tonic_labels=nan(B, 12), key_signature_id=nan(B, 24),
                   seq_length=torch.full((B,), -77, dtype=torch.int64, device=DEV), sample_weight=nan(B))
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().ake_window_batch_f32(p(mel), int(fm), R, T, P, wf, hop, rec_d.data_ptr(), start_d.data_ptr(), B, p(a[0]), p(a[1]), p(a[2]),
                                               a[0].shape[1] if ann is not None else 0, min_purity, int(uniform), p(out.get("mel")),
                                               *(p(out.get(k)) for k in ("key_labels", "tonic_labels", "key_signature_id", "seq_length", "sample_weight")),
                                               torch.cuda.current_stream().cuda_stream), "ake_window_batch_f32")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.fixture(scope="module")
def sources():
    """(R, P, T) transforms of random numbers: 3 recordings of 126 frames (25 s at 5 frames per second), 288 and 36 bins."""
    g = torch.Generator().manual_seed(5)
    return {P: torch.rand((3, P, 126), generator=g) for P in (288, 36)}


@pytest.mark.parametrize("fm", [False, True])
@pytest.mark.parametrize("P,wf", [(288, 76), (36, 5)])
@pytest.mark.parametrize("B", [1, 300])
def test_gather_equals_slicing(sources, fm, P, wf, B):
    src = sources[P]
    T = src.shape[2]
    g = torch.Generator().manual_seed(B + P)
    rec = torch.randint(0, 3, (B,), generator=g)
    start = torch.randint(0, T - wf + 1, (B,), generator=g)
    start[0] = T - wf                                                    # the last start there is
    if B > 1:
        start[1], rec[2], start[2] = 0, rec[0], start[0]                 # the first, and a repeated entry
    dev_src = (src.transpose(1, 2) if fm else src).contiguous().to(DEV)
    got = raw_batch(dev_src, fm, rec, start, wf)["mel"]
    want = src[rec[:, None, None], torch.arange(P)[None, :, None], (start[:, None] + torch.arange(wf)[None, :])[:, None, :]][:, None]
    assert got.shape == (B, 1, P, wf) and torch.equal(got, want)


def label_names():
    return ("key_labels", "tonic_labels", "key_signature_id", "seq_length", "sample_weight")


def test_labels_equal_the_host_model_on_the_purity_cases():
    ann, rec, st = purity_cases()
    at = float(metrics.window_labels(*ann, rec, st, HOP, WF)["purity"][0])
    above = float(np.nextafter(np.float32(at), np.float32(1)))
    for kw in ({}, {"min_purity": at}, {"min_purity": above}, {"min_purity": 0.5, "uniform": True}, {"uniform": True}):
        want = metrics.window_labels(*ann, rec, st, HOP, WF, **kw)
        got = raw_batch(None, False, rec, st, WF, ann=ann, gather=False, **kw)              # labels only
        assert set(got) == set(label_names())
        for name in label_names():
            assert got[name].dtype == want[name].dtype and torch.equal(got[name], want[name]), (kw, name)
    # windows further into the recordings, a one-frame window and an odd hop
    rec2, st2 = torch.tensor([0, 1, 2, 3, 7, 7]), torch.tensor([WF, 40, 1, 75, 10, 38])
    for hop, wf in ((HOP, WF), (441, 1), (4411, 6)):
        want = metrics.window_labels(*ann, rec2, st2, hop, wf)
        got = raw_batch(None, False, rec2, st2, wf, hop=hop, ann=ann, gather=False)
        assert all(torch.equal(got[n], want[n]) for n in label_names()), (hop, wf)


def test_labels_on_modulating_recordings_with_and_without_the_gather(sources):
    """A random list of 300 windows over the annotations of three 25 s modulating recordings (more windows than a block has threads),
    gathered and labelled in one launch: the same labels as the labels-only launch, the same windows as the gather-only launch."""
    _, segments = synthetic.modulating_batch_arrays([0, 1, 2], 25.0, min_seconds=5.0, mean_seconds=8.0)
    ann = annotations(segments)
    assert int(ann[2].max()) >= 3
    src = sources[36]
    g = torch.Generator().manual_seed(9)
    rec, st = torch.randint(0, 3, (300,), generator=g), torch.randint(0, 126 - WF + 1, (300,), generator=g)
    want = metrics.window_labels(*ann, rec, st, HOP, WF)
    assert 0 < int((want["purity"] == 1).sum()) < 300 and float(want["sample_weight"].min()) < 1
    both = raw_batch(src.to(DEV), False, rec, st, WF, ann=ann)
    only_labels = raw_batch(None, False, rec, st, WF, ann=ann, gather=False)
    only_mel = raw_batch(src.to(DEV), False, rec, st, WF)
    assert set(only_mel) == {"mel"} and torch.equal(both["mel"], only_mel["mel"])
    for name in label_names():
        assert torch.equal(both[name], want[name]) and torch.equal(only_labels[name], want[name]), name
    # the wrapper gives the same batch
    wrapped = ake_amd.window_batch(src.to(DEV), rec.to(DEV, torch.int32), st.to(DEV, torch.int32), WF, HOP,
                                   ake_amd.KeyAnnotations(*ann, 22050))
    assert all(torch.equal(wrapped[k].cpu(), both[k]) for k in both)


def test_list_entries_out_of_range_are_read_clamped(sources):
    """The list lives in device memory, where the host cannot check it: whatever it holds, every load stays inside the transform (the
    results for such entries are unspecified; here they are the clamped window's)."""
    src = sources[36]
    ann = annotations([[(0, 3)], [(0, 4)], [(0, 5)]])
    rec, st = torch.tensor([-5, 9, 1, 2]), torch.tensor([3, -1, 10 ** 6, 2 ** 31 - 1])
    got = raw_batch(src.to(DEV), False, rec, st, 5, ann=ann)
    want = torch.stack([src[0, :, 3:8], src[2, :, 0:5], src[1, :, 121:126], src[2, :, 121:126]])[:, None]
    assert torch.equal(got["mel"], want) and got["key_signature_id"].argmax(1).tolist() == [3, 5, 4, 5]


# ---- the weighted loss ----

def run_loss(case, w, weights=(1.0, 0.7, 0.1), use_cos=False, grads=True, weighted=True):
    """ake_general_step_weighted_f32 (or ake_general_step_f32) straight through the C ABI, outputs poisoned -> (scalars, d_key, d_tonic, d_genre)."""
    L = _lib.lib()
    key, tonic, gen, kl, tl, gl, sig = (None if t is None else t.float().to(DEV).contiguous() for t in case)
    B = key.shape[0]
    wd = None if w is None else torch.as_tensor(w).float().to(DEV).contiguous()
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    scal = nan(10)
    dk, dt, dg = (nan(B, 12), nan(B, 12), nan(B, 11) if gen is not None else None) if grads else (None, None, None)
    p = lambda t: None if t is None else t.data_ptr()
    head = (p(key), p(tonic), p(gen), p(kl), p(tl), 0, p(gl), 0, p(sig), 0, B, weights[0], weights[1], weights[2], int(use_cos))
    if weighted:
        _lib.check(L.ake_general_step_weighted_f32(*head, p(wd), p(scal), p(dk), p(dt), p(dg), None), "ake_general_step_weighted_f32")
    else:
        _lib.check(L.ake_general_step_f32(*head, p(scal), p(dk), p(dt), p(dg), None), "ake_general_step_f32")
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (scal, dk, dt, dg))


def f32_values(case):
    """The case as the kernel sees it: float32 values, in float64."""
    return [None if t is None else t.float().double() for t in case[:3]] + list(case[3:])


@pytest.mark.parametrize("B,genre,use_cos", [(1, True, False), (8, True, True), (300, False, False), (37, True, True), (8, False, True)])
def test_weighted_loss_against_the_float64_model(B, genre, use_cos):
    case = loss_case(B, 20 + B, genre)
    g = torch.Generator().manual_seed(B)
    w = torch.rand(B, generator=g) + 0.05
    if B > 1:
        w[torch.randperm(B, generator=g)[:max(1, B // 4)]] = 0            # weights with zeros
    weights = (1.0, 0.7, 0.1)
    scal, dk, dt, dg = run_loss(case, w, weights, use_cos)
    ref, (gk, gt, gg) = metrics.weighted_general_step(*f32_values(case), w.double(), weights, use_cos, grads=True)
    ref = [float(v) for v in ref]
    print("loss", float(scal[0]), ref[0], "metrics", scal[1:].tolist(), ref[1:])
    assert abs(float(scal[0]) - ref[0]) < 2e-6 * max(1.0, abs(ref[0]))
    assert np.allclose(scal[1:].numpy(), np.array(ref[1:], np.float32), atol=1e-6)
    assert float((dk.double() - gk).abs().max()) < 2e-6 * max(1e-3, float(gk.abs().max()))
    assert float((dt.double() - gt).abs().max()) < 2e-6 * max(1e-3, float(gt.abs().max()))
    if genre:
        assert float((dg.double() - gg).abs().max()) < 2e-6 * max(1e-3, float(gg.abs().max()))
    assert float(dk[w == 0].abs().sum()) == 0 and float(dt[w == 0].abs().sum()) == 0
    again = run_loss(case, w, weights, use_cos)                          # bit-reproducible
    assert all(torch.equal(a, b) for a, b in zip((scal, dk, dt) + ((dg,) if genre else ()), again))
    # without the gradient buffers: the same scalars
    assert torch.equal(run_loss(case, w, weights, use_cos, grads=False)[0], scal)


@pytest.mark.parametrize("B,genre,use_cos", [(8, True, True), (300, False, False)])
def test_null_weights_are_the_unweighted_entry_bit_for_bit(B, genre, use_cos):
    case = loss_case(B, 40 + B, genre)
    a = run_loss(case, None, use_cos=use_cos)
    b = run_loss(case, None, use_cos=use_cos, weighted=False)
    assert all(x is None and y is None or torch.equal(x, y) for x, y in zip(a, b)) and bool(torch.isfinite(a[0]).all())


def test_rows_without_weight_count_for_nothing():
    case = list(loss_case(16, 2))
    w = torch.rand(16, generator=torch.Generator().manual_seed(3))
    dead = [1, 4, 9]
    w[dead] = 0
    base = run_loss(case, w, use_cos=True)
    other = [t.clone() for t in case]
    other[0][[1, 4]] = torch.tensor([0.0, 1.0] * 6, dtype=torch.float64)       # key outputs exactly 0 and 1
    other[0][9] = float("nan")
    other[1][dead] = 1e30
    other[2][9] = float("inf")
    other[3][dead] = 1 - other[3][dead]
    other[4][dead], other[5][dead], other[6][dead] = 0, 1, 0
    got = run_loss(other, w, use_cos=True)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert all(torch.equal(a, b) for a, b in zip(base, got))
    assert all(float(t[dead].abs().sum()) == 0 for t in got[1:])
    zero = run_loss(other, torch.zeros(16), use_cos=True)                      # Wsum = 0: exact zeros everywhere
    assert all(float(t.abs().sum()) == 0 and bool(torch.isfinite(t).all()) for t in zero)


# ---- end to end ----

SECONDS = (25.0, 22.0, 18.0)


def make_net(gold):
    opt = Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return net.to(DEV)


@pytest.fixture(scope="module")
def recordings():
    """Three modulating recordings of 25 / 22 / 18 s (ragged), their annotations and lengths, on the device."""
    audio, ann, lengths = synthetic.make_modulating_batch_device([0, 1, 2], SECONDS, DEV, min_seconds=5.0, mean_seconds=8.0)
    torch.cuda.synchronize()
    return audio, ann, lengths


@pytest.fixture(scope="module")
def estimator(gold_default):
    return ake_amd.KeyEstimator(make_net(gold_default), 22050, 5)


def check_batch(batch, B, mel_all, ann, frames, uniform=False):
    """Shapes, dtypes and contents of one batch against the plan's own transform and the host label model."""
    shapes = {"mel": (B, 1, 288, WF), "key_labels": (B, 12), "tonic_labels": (B, 12), "key_signature_id": (B, 24), "genre": (B, 11),
              "seq_length": (B,), "sample_weight": (B,), "recording": (B,), "start_frame": (B,)}
    assert set(batch) == set(shapes)
    for k, shape in shapes.items():
        want = torch.int64 if k == "seq_length" else torch.int32 if k in ("recording", "start_frame") else torch.float32
        assert tuple(batch[k].shape) == shape and batch[k].dtype == want and batch[k].device.type == "cuda", k
    rec, st = batch["recording"].cpu().long(), batch["start_frame"].cpu().long()
    assert all(0 <= s <= frames[r] - WF for r, s in zip(rec.tolist(), st.tolist()))
    for b in range(B):
        assert torch.equal(batch["mel"][b, 0], mel_all[rec[b], :, st[b]:st[b] + WF])
    want = metrics.window_labels(ann.seg_start.cpu(), ann.seg_key.cpu(), ann.seg_count.cpu(), rec, st, HOP, WF, uniform=uniform)
    for k in ("key_labels", "tonic_labels", "key_signature_id", "seq_length", "sample_weight"):
        assert torch.equal(batch[k].cpu(), want[k]), k
    assert float(batch["genre"].abs().sum()) == 0


def test_random_windows_end_to_end(estimator, recordings):
    audio, ann, lengths = recordings
    frames = [1 + int(n) // HOP for n in lengths.tolist()]
    mel_all = estimator.plan.logmag(audio, lengths=lengths)
    tw = estimator.training_windows(audio, ann, lengths=lengths, batch_size=8, batches_per_epoch=3, seed=5)
    assert isinstance(tw, ake_amd.TrackWindows) and len(tw) == 3 and tw.window_frames == WF
    epochs = [list(tw), list(tw)]                                        # every completed iteration advances the epoch
    assert tw.epoch == 2 and all(len(e) == 3 for e in epochs)
    for e, batches in enumerate(epochs):
        prefix = metrics.window_prefix(frames, WF)
        for i, batch in enumerate(batches):
            check_batch(batch, 8, mel_all, ann, frames)
            rec, st, _ = metrics.draw_windows(prefix, 5, e, 8 * i, 8)
            assert batch["recording"].tolist() == rec and batch["start_frame"].tolist() == st
    key = lambda batches: [b["recording"].tolist() + b["start_frame"].tolist() for b in batches]
    assert key(epochs[0]) != key(epochs[1])                              # epoch 0 and epoch 1 draw different windows
    tw.set_epoch(0)
    again = list(tw)
    assert key(again) == key(epochs[0]) and all(torch.equal(a["mel"], b["mel"]) for a, b in zip(again, epochs[0]))
    # the default epoch covers the recordings once at a stride of one window: 1 + 1 + 1 windows of 76 frames in 126 / 111 / 91 frames
    assert len(estimator.training_windows(audio, ann, lengths=lengths, batch_size=2)) == 2
    # the same recordings as 16-bit PCM: the windows of the PCM transform; uniform weights
    pcm = torch.round(audio * 32767).to(torch.int16)
    tw16 = estimator.training_windows(pcm, ann, lengths=lengths, batch_size=8, batches_per_epoch=1, seed=5, weighting="uniform")
    batch16 = next(iter(tw16))
    check_batch(batch16, 8, estimator.plan.logmag(pcm, lengths=lengths), ann, frames, uniform=True)
    assert batch16["start_frame"].tolist() == epochs[0][0]["start_frame"].tolist()


def test_grid_windows_are_the_tracks_own(estimator, recordings):
    audio, ann, lengths = recordings
    track = estimator.track(audio, lengths=lengths, window_seconds=15.0, stride_seconds=1.0)
    truth = track.score(ann).truth.cpu()
    counts = track.counts.tolist()
    tw = estimator.training_windows(audio, ann, lengths=lengths, batch_size=8, stride_seconds=1.0)
    batches = list(tw)
    assert len(tw) == len(batches) == -(-sum(counts) // 8) and [b["mel"].shape[0] for b in batches[:-1]] == [8] * (len(batches) - 1)
    assert batches[-1]["mel"].shape[0] == sum(counts) - 8 * (len(batches) - 1)
    rec = torch.cat([b["recording"] for b in batches]).tolist()
    st = torch.cat([b["start_frame"] for b in batches]).tolist()
    assert list(zip(rec, st)) == [(r, w * track.stride_frames) for r in range(3) for w in range(counts[r])]
    sig = torch.cat([b["key_signature_id"] for b in batches]).cpu()
    got = torch.where(sig.sum(dim=1) == 1, sig.argmax(dim=1), torch.full((len(rec),), -1)).tolist()
    assert got == [int(truth[r, w]) for r in range(3) for w in range(counts[r])]
    mel_all = estimator.plan.logmag(audio, lengths=lengths)
    check_batch(batches[0], 8, mel_all, ann, [1 + int(n) // HOP for n in lengths.tolist()])
    assert tw.epoch == 0                                                 # a grid has no epochs


def test_fit_is_reproducible_and_follows_the_seed(gold_default, estimator, recordings):
    audio, ann, lengths = recordings

    def fit(seed):
        net = make_net(gold_default)
        tw = estimator.training_windows(audio, ann, lengths=lengths, batch_size=8, batches_per_epoch=3, seed=seed)
        trainer = ake_amd.Trainer(max_epochs=2, accumulate_grad_batches=1)
        trainer.fit(net, train_dataloaders=tw)
        torch.cuda.synchronize()
        assert tw.epoch == 2 and len(trainer.train_losses) == 6
        return net.flat_parameters()[0].clone().cpu(), trainer.train_losses

    (w1, l1), (w2, l2), (w3, l3) = fit(5), fit(5), fit(6)
    assert torch.equal(w1, w2) and l1 == l2
    assert not torch.equal(w1, w3) and bool(torch.isfinite(w1).all()) and all(np.isfinite(l1))
    # step 0's loss is the weighted model on the net's own outputs
    net = make_net(gold_default).train()
    batch = next(iter(estimator.training_windows(audio, ann, lengths=lengths, batch_size=8, batches_per_epoch=3, seed=5)))
    with torch.no_grad():
        out = net(batch["mel"], batch["seq_length"])
    ref = metrics.weighted_general_step(*(t.double().cpu() for t in out), batch["key_labels"].cpu(), batch["tonic_labels"].cpu(), batch["genre"].cpu(),
                                        batch["key_signature_id"].cpu(), batch["sample_weight"].double().cpu(), (1.0, 1.0, 0.1), False)
    print("step 0 loss", l1[0], float(ref[0]))
    assert abs(l1[0] - float(ref[0])) < 2e-6 * max(1.0, abs(float(ref[0])))


def test_general_step_with_and_without_sample_weight(gold_default, estimator, recordings):
    audio, ann, lengths = recordings
    batch = next(iter(estimator.training_windows(audio, ann, lengths=lengths, batch_size=8, batches_per_epoch=1, seed=1)))
    assert 0 < float(batch["sample_weight"].min()) < 1                   # some window straddles a key change
    net = make_net(gold_default).eval()
    with torch.no_grad():
        out = net(batch["mel"], batch["seq_length"])
        case = (out[0], out[1], out[2], batch["key_labels"], batch["tonic_labels"], batch["genre"], batch["key_signature_id"])
        # without sample_weight: today's path, ake_general_step_f32 on the net's own outputs, bit for bit
        plain = {k: v for k, v in batch.items() if k != "sample_weight"}
        vals = torch.stack(net.general_step(plain, 0, "val")).cpu()
        assert torch.equal(vals, run_loss(case, None, (1.0, 1.0, 0.1), grads=False, weighted=False)[0])
        # with it: the weighted entry
        weighted = torch.stack(net.general_step(batch, 0, "val")).cpu()
        assert torch.equal(weighted, run_loss(case, batch["sample_weight"], (1.0, 1.0, 0.1), grads=False)[0])
        assert not torch.equal(weighted, vals)
    # the torch-op path computes the same formulas, and the same parameter gradients
    res = []
    for fused in (True, False):
        net = make_net(gold_default).train()
        net.fused_loss = fused
        vals = net.general_step(batch, 0, "train")
        assert ("FusedGeneralStep" in type(vals[0].grad_fn.next_functions[0][0]).__name__) == fused
        vals[0].backward()
        res.append(([float(v.detach()) for v in vals], torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()))
    (va, ga), (vb, gb) = res
    assert np.allclose(va, vb, rtol=2e-6, atol=1e-7), (va, vb)
    assert float((ga - gb).abs().max()) < 1e-5 * float(gb.abs().max())


def test_training_windows_refuses_what_it_cannot_do(estimator, recordings):
    audio, ann, lengths = recordings
    two = ake_amd.KeyAnnotations(ann.seg_start[:2], ann.seg_key[:2], ann.seg_count[:2], ann.sample_rate)
    with pytest.raises(ValueError, match="recordings"):
        estimator.training_windows(audio, two, lengths=lengths)
    other_rate = ake_amd.KeyAnnotations(ann.seg_start, ann.seg_key, ann.seg_count, 44100)
    with pytest.raises(ValueError, match="44100"):
        estimator.training_windows(audio, other_rate, lengths=lengths)
    with pytest.raises(ValueError, match="one window"):
        estimator.training_windows(audio[:, :22050 * 10], ann)
    with pytest.raises(ValueError, match="weighting"):
        estimator.training_windows(audio, ann, lengths=lengths, weighting="none")

    def bare(frames=5, wrap_mode="dataset_max", local=False):
        est = ake_amd.KeyEstimator.__new__(ake_amd.KeyEstimator)
        est.frames, est.wrap_mode, est.sample_rate = frames, wrap_mode, 22050
        est.net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True, local=local, frames=5, loc_window_size=10))
        return est

    for match, est in (("frames=0", bare(frames=0)), ("true_end", bare(wrap_mode="true_end")), ("--local", bare(local=True))):
        with pytest.raises(ValueError, match=match):
            est.training_windows(audio, ann, lengths=lengths)
