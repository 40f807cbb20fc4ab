"""PARITY (GPU): the whole-song data mode (--frames 0, KeyDataset.py:478-509, 212-215, 257-262): every clip with its own hop
``n // window_size + 1`` (ake_cqt_logmag_hops_f32), the KeyDataset items, KeyEstimator, the backward and training on them.

The CQT is specified by the build's direct-form oracle (oracle/cqt_oracle.py; FastDirectCQT is its dense-matmul evaluation,
checked against cqt_logmag in tests/test_oracle_cqt.py), evaluated at each clip's hop.  Parity with librosa stays unpinned."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, synthetic
from ake_amd.KeyDataset import cqt_features
from ake_amd.cqt import get_any_hop_plan, hop_for_window
from ake_amd.lightning_shim import Trainer
from conftest import golden_state_dict, rel_err
from oracle import cqt_oracle, loss_oracle, pcnet_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
TOL = 5e-4


def oracle_mel(y, sr, hop, n_bins=288):
    """Direct-form log-CQT of one clip at its own hop, float64 (n_bins, 1 + len(y) // hop)."""
    return cqt_oracle.FastDirectCQT(sr, hop, n_bins, dtype=torch.float64)(np.asarray(y, np.float32)[None])[0].numpy()


def ragged(clips):
    n_max = max(len(c) for c in clips)
    rows = np.zeros((len(clips), n_max), np.float32)
    for i, c in enumerate(clips):
        rows[i, :len(c)] = c
    return torch.from_numpy(rows).to(DEV), torch.tensor([len(c) for c in clips], dtype=torch.int64, device=DEV)


def mixed_clips(seconds, sr, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i, s in enumerate(seconds):
        n = int(round(s * sr))
        out.append(synthetic.make_clip(i, n, sr)[0] if i % 2 == 0 else rng.normal(0, 0.3, n).astype(np.float32))   # key clips + white noise
    return out


def check_against_oracle(plan, clips, sr, n_bins, out_frames=592, window=592):
    audio, lens = ragged(clips)
    hops = hop_for_window(lens, window).to(torch.int32)
    got = plan.logmag_hops(audio, hops, lens, out_frames=out_frames).cpu().numpy()
    assert got.shape == (len(clips), n_bins, out_frames)
    errs = []
    for i, y in enumerate(clips):
        hop = len(y) // window + 1
        T = 1 + len(y) // hop
        assert int(hops[i]) == hop and T <= window
        errs.append(rel_err(got[i, :, :T], oracle_mel(y, sr, hop, n_bins)))
        assert np.all(got[i, :, T:] == 0), i
    print("\nper-clip hop CQT rel err vs direct form:", ["%.1e" % e for e in errs])
    assert max(errs) < TOL, errs


def test_ragged_per_clip_hops_against_direct_form():
    clips = mixed_clips([0.3, 2.0, 4.7, 9.0, 15.0], SR)
    assert [len(c) // 592 + 1 for c in clips] == [12, 75, 176, 336, 559]
    check_against_oracle(get_any_hop_plan(SR, 288, device=DEV), clips, SR, 288)


def test_per_clip_hops_at_44k_and_with_seven_octaves():
    check_against_oracle(get_any_hop_plan(44100, 288, device=DEV), mixed_clips([1.0, 5.5, 12.0], 44100, seed=1), 44100, 288)
    check_against_oracle(get_any_hop_plan(SR, 252, device=DEV), mixed_clips([0.7, 6.0, 10.0], SR, seed=2), SR, 252)


@pytest.mark.parametrize("batch,hop", [(256, 4410), (16, 2205)])
def test_uniform_hops_bit_identical_to_the_fixed_hop_path(batch, hop):
    """The cascade's values do not depend on the hop, the hop-1 plan's phase tables are the fixed-hop plan's for every phase that plan
    has, and the row-list bank runs the same MFMA sequence per row: equal hops give the fixed-hop engine-3 output bit for bit."""
    audio, _ = synthetic.make_batch_device(range(batch), torch.device(DEV))
    fixed = ake_amd.CQTPlan(SR, hop, 288, 36, device=DEV)
    ref = fixed.logmag(audio)
    T = ref.shape[2]
    hops = torch.full((batch,), hop, dtype=torch.int32, device=DEV)
    got = get_any_hop_plan(SR, 288, device=DEV).logmag_hops(audio, hops, out_frames=T)
    assert torch.equal(got, ref)


def test_abi_refusals():
    L = _lib.lib()
    audio = torch.zeros((2, 30000), device=DEV)
    hops = torch.full((2,), 51, dtype=torch.int32, device=DEV)
    out = torch.empty((2, 288, 592), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(plan, ws_bytes=None, hop_ptr=hops.data_ptr()):
        need = plan.workspace_bytes_hops(2, 30000, 592)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        return L.ake_cqt_logmag_hops_f32(plan.handle, audio.data_ptr(), 2, 30000, 30000, None, hop_ptr, out.data_ptr(), 592,
                                         ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, stream)

    assert call(ake_amd.CQTPlan(SR, 4410, 288, 36, device=DEV)) == -1                 # even hop: no table for every phase
    assert call(ake_amd.CQTPlan(SR, 1, 288, 36, device=DEV, engine=1)) == -5          # engines 1 and 5 are not extended
    assert b"engine 3" in L.ake_last_error()
    assert call(ake_amd.CQTPlan(SR, 1, 288, 36, device=DEV, engine=5)) == -5
    plan = get_any_hop_plan(SR, 288, device=DEV)
    assert call(plan, hop_ptr=None) == -1
    assert call(plan, ws_bytes=plan.workspace_bytes_hops(2, 30000, 592) - 256) == -4
    assert L.ake_cqt_workspace_bytes_hops(ake_amd.CQTPlan(SR, 1, 288, 36, device=DEV, engine=1).handle, 2, 30000, 592) == 0
    assert call(plan) == 0
    torch.cuda.synchronize()


def frames0_opt(**kw):
    o = dict(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=0, window_size=592, octaves=8,
             key_weight=1.0, tonic_weight=1.0, genre_weight=0.1, use_cos=False, no_ckpt=True, local=False, only_semitones=False,
             multi_scale=False, lr=1e-3, gamma=0.96, acc_grad=1, reg=0)
    o.update(kw)
    return Namespace(**o)


def default_net(gold, opt):
    n = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
    n.load_state_dict(golden_state_dict(gold), strict=True)
    return n.to(DEV)


def test_keydataset_items_and_validate(gold_default):
    opt = frames0_opt()
    ds = ake_amd.KeyDataset(True, opt)
    ds.import_data(ake_amd.SyntheticSineMixLoader(5, n_samples=SR * 4),
                   ake_amd.SyntheticSineMixLoader(3, first=100, n_samples=SR * 7, name="Synthetic long"), shuffle=False)
    assert len(ds) == 8
    for idx, n, clip_id in ((0, SR * 4, 0), (7, SR * 7, 102)):
        item = ds[idx]
        assert set(item) == {"mel", "key_labels", "tonic_labels", "key_signature_id", "genre"}      # KeyDataset.py:257-262
        assert item["mel"].shape == (1, 288, 592) and item["mel"].dtype == torch.float64
        hop = n // 592 + 1
        T = 1 + n // hop
        assert rel_err(item["mel"][0, :, :T].numpy(), oracle_mel(synthetic.make_clip(clip_id, n)[0], SR, hop)) < TOL
        assert torch.all(item["mel"][:, :, T:] == 0)
    net = default_net(gold_default, opt).eval()
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)
    res = Trainer().validate(net, dataloaders=loader)[0]
    assert set(res) >= {"val_loss", "val_mirex_score", "val_accuracy", "val_accuracy_tonic", "val_accuracy_genre"}
    batch = next(iter(loader))
    assert batch["mel"].shape == (4, 1, 288, 592)
    out = net(batch["mel"].to(DEV), None)
    step = net.validation_step({k: v.to(DEV) for k, v in batch.items()}, 0)
    loss = loss_oracle.general_step_loss(out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), batch["key_labels"].numpy(),
                                         batch["tonic_labels"].numpy(), batch["genre"].numpy())
    assert abs(float(step["val_loss"]) - loss) < 1e-5
    assert abs(float(net.test_step({k: v.to(DEV) for k, v in batch.items()}, 0)["test_loss"]) - loss) < 1e-5


def test_key_estimator_whole_songs_end_to_end(gold_default):
    net = default_net(gold_default, frames0_opt()).eval()
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(net, SR, frames=0, wrap_mode="true_end")
    est = ake_amd.KeyEstimator(net, SR, frames=0, window_size=592)
    clips = mixed_clips([3.0, 8.5, 20.0, 31.0], SR, seed=3)
    audio, lens = ragged(clips)
    got = est(audio, lens)
    mel = np.zeros((len(clips), 1, 288, 592))
    for i, y in enumerate(clips):
        m = oracle_mel(y, SR, len(y) // 592 + 1)
        mel[i, 0, :, :m.shape[1]] = m
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), torch.from_numpy(mel), None)
    errs = [rel_err(a.cpu(), b) for a, b in zip(got, ref)]
    print("\nKeyEstimator(frames=0) rel err (key, tonic, genre) vs float64 oracle chain:", ["%.1e" % e for e in errs])
    assert max(errs) < 1e-3, errs
    # the same through the composed Python layers: CQT at the clips' own hops, then the net with seq_length None
    mel_d = cqt_features(audio, SR, frames0_opt(), lengths=lens.cpu())
    for a, b in zip(got, net(mel_d[:, None], None)):
        assert torch.equal(a, b)
    # equal-length clips without `lengths`: every clip's hop from n
    k1 = est(audio[:2, :len(clips[0])])[0]
    k2 = est(audio[:2, :len(clips[0])], torch.full((2,), len(clips[0]), dtype=torch.int64, device=DEV))[0]
    assert torch.equal(k1, k2)


def grad_rows(gold, frames, seed):
    from test_gpu_backward import grad_errors, loss_fn, reference_grads
    sd32 = golden_state_dict(gold)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((2, 1, 288, frames), generator=g) * 2.5
    labels = ((torch.rand((2, 12), generator=g) > 0.5).float(), torch.tensor([3, 7]), torch.tensor([1, 9]), torch.tensor([True, True]))
    loss_ref, ref = reference_grads(sd32, x, None, labels)
    net = default_net(gold, frames0_opt()).train()
    out = net(x.to(DEV), None)
    loss = loss_fn(out[0], out[1], out[2], *(t.to(DEV) for t in labels))
    assert abs(float(loss.detach()) - loss_ref) < 2e-5 * max(1.0, abs(loss_ref))
    loss.backward()
    rows = grad_errors(net, ref)
    print("\n%d frames, seed %d: gradient rel err worst %.1e (%s), median %.1e" % (frames, seed, rows[0][0], rows[0][1], rows[len(rows) // 2][0]))
    return rows


def test_long_map_gradients_against_float64_autograd(gold_default):
    """The backward of maps longer than the LDS slices of two kernels, with no seq_length, against float64 autograd through the oracle: the
    pool_semi weight gradient in time tiles (more than 318 frames) and the heads' data gradient on the generic kernel (more than 164 head
    frames, i.e. 340 + input frames).  360 frames take both; seed 12 is clear of LeakyReLU decisions that flip between f32 and f64 (median
    5e-6 measured).  Long maps see more such flips: 300 frames, where neither new path runs, measured medians of 2e-3 .. 3e-3, so 592 frames
    are held to the kinked bounds of tests/test_gpu_backward.py's uncurated test."""
    rows = grad_rows(gold_default, 360, 12)
    assert rows[len(rows) // 2][0] < 1e-4, rows[len(rows) // 2]
    assert rows[0][0] < 5e-2, rows[:5]
    for seed in (11, 12):
        rows = grad_rows(gold_default, 592, seed)
        assert rows[0][0] < 1e-1 and rows[len(rows) // 2][0] < 2e-2, rows[:3]


def fit_once(gold, opt, ds, seed):
    torch.manual_seed(seed)
    net = default_net(gold, opt)
    trainer = Trainer(max_epochs=1, accumulate_grad_batches=1)
    trainer.fit(net, train_dataloaders=torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True))
    return net, trainer


def test_training_on_whole_songs(gold_default):
    """Trainer.fit, one epoch of 8 ragged whole songs at batch 4 (general_step -> forward(mel, None) -> the training autograd node ->
    the fused loss -> backward -> FusedAdam); train-mode outputs of a batch against the oracle; a second run from the same seed is bit-equal."""
    opt = frames0_opt()
    clips = mixed_clips([2.0, 3.5, 5.0, 6.5, 8.0, 9.5, 11.0, 12.5], SR, seed=4)
    ds = ake_amd.KeyDataset(True, opt)
    ds.import_data(ake_amd.WaveformLoader("ragged", clips, list(range(8)), SR, genres=list(range(8))), shuffle=False)
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)))
    assert set(batch) == {"mel", "key_labels", "tonic_labels", "key_signature_id", "genre"} and batch["mel"].shape == (4, 1, 288, 592)
    probe = default_net(gold_default, opt).train()
    with torch.no_grad():
        got = probe(batch["mel"].to(DEV), None)
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), batch["mel"].double(), None, training=True)
    errs = [rel_err(a.cpu(), b) for a, b in zip(got, ref)]
    print("\ntrain-mode rel err (key, tonic, genre) vs float64 oracle:", ["%.1e" % e for e in errs])
    assert max(errs) < 1e-3, errs
    sd0 = {k: v.detach().cpu().clone() for k, v in default_net(gold_default, opt).state_dict().items()}
    net, trainer = fit_once(gold_default, opt, ds, seed=7)
    print("whole-song training losses:", trainer.train_losses)
    assert len(trainer.train_losses) == 2 and all(np.isfinite(trainer.train_losses))
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    moved = max(float((sd[k] - sd0[k]).abs().max()) for k in sd if k.endswith(".weight"))
    assert moved > 1e-4, moved
    net2, trainer2 = fit_once(gold_default, opt, ds, seed=7)
    assert trainer2.train_losses == trainer.train_losses
    for k, v in net2.state_dict().items():
        assert torch.equal(v.detach().cpu(), sd[k]), k
