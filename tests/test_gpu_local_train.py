"""GPU: --local training through the drop-in classes -- general_step's fused --local loss against its torch-op loop, and KeyDataset
(opt.local) -> PitchClassNet -> Trainer.fit / validate end to end."""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ake_amd
from ake_amd import synthetic
from ake_amd.lightning_shim import Trainer
from conftest import golden_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAL_KEYS = ("val_loss", "val_accuracy", "val_mirex_score", "val_correct", "val_fifths", "val_relative", "val_parallel", "val_other",
            "val_accuracy_tonic", "val_accuracy_genre")


def local_opt(gold, **kw):
    opt = Namespace(**json.loads(str(gold["opt"])))
    opt.local, opt.genre = True, False
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def local_batch(B, T, seq, seed, R=None):
    """A --local batch as KeyDataset makes it: labels per frame for each clip's seq - 49 frames, zero rows behind them, R rows."""
    R = R or T
    g = torch.Generator().manual_seed(seed)
    kid = torch.randint(0, 24, (B, R), generator=g)
    labels = {"key_labels": ake_amd.KEY_SIGNATURE_MAP[kid % 21].clone(), "tonic_labels": F.one_hot(kid % 12, 12).float(),
              "key_signature_id": F.one_hot(kid, 24).float()}
    for i, s in enumerate(seq):
        for t in labels.values():
            t[i, s - 49:] = 0
    return {"mel": (torch.rand((B, 1, 288, T), generator=g) * 2.5).to(DEV), "seq_length": torch.tensor(seq), **labels}


@pytest.mark.parametrize("seq,T", [([120, 110, 60], 120), ([300, 52, 301, 170], 301)])
def test_fused_local_step_matches_the_loop(gold_default, seq, T):
    opt = local_opt(gold_default)
    batch = local_batch(len(seq), T, seq, seed=len(seq))
    res = []
    for fused in (True, False):
        net = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
        net.load_state_dict({k: v for k, v in golden_state_dict(gold_default).items() if not k.startswith("genre_classifier")}, strict=True)
        net = net.to(DEV).train()
        net.fused_loss = fused
        d = net.training_step(batch, 0)
        node = type(d["loss"].grad_fn.next_functions[0][0]).__name__ if d["loss"].grad_fn.next_functions else ""
        assert ("FusedGeneralStepLocal" in node) == fused, node
        d["loss"].backward()
        vals = [float(d["loss"].detach())] + [float(d["train_" + n].detach()) for n in net._NAMES]
        res.append((vals, torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()))
    (va, ga), (vb, gb) = res
    assert np.allclose(va, vb, rtol=1e-6, atol=1e-6), (va, vb)
    assert float((ga - gb).abs().max()) < 1e-5 * float(gb.abs().max())


def test_fused_local_step_refuses_more_frames_than_the_outputs(gold_default):
    opt = local_opt(gold_default)
    net = ake_amd.PitchClassNet(288, 12, 2, 7, opt).to(DEV).train()
    batch = local_batch(2, 100, [100, 80], seed=1)
    batch["seq_length"] = torch.tensor([101, 80])                       # n = 53 > T' = 100 - 49 = 51
    with pytest.raises(ValueError, match="more than the 51 output frames"):
        net.training_step(batch, 0)


def local_dataset(opt):
    sr = synthetic.SR
    waves = [synthetic.make_clip(i, int(sec * sr), sr)[0] for i, sec in enumerate((12, 20, 31))]
    ds = ake_amd.KeyDataset(False, opt)
    ds.import_data(ake_amd.WaveformLoader("clips", waves, [3, 14, 20], sr), shuffle=False)
    return ds


def fit_once(opt, ds, seed):
    torch.manual_seed(seed)
    net = ake_amd.PitchClassNet(288, 12, 2, 7, opt, batch_size=3, train_set=ds, val_set=ds).to(DEV)
    trainer = Trainer(max_epochs=2).fit(net)
    return net, trainer


def test_local_dataset_trains_end_to_end(gold_default):
    """Clips of 12, 20 and 31 s (T = 61, 101, 156 CQT frames, so 12, 52 and 107 labelled frames behind a 50-frame window) in one
    ragged batch per epoch, the reference's default learning rate (3e-4): the loss falls; a second seeded run gives bit-identical
    weights."""
    opt = local_opt(gold_default)
    ds = local_dataset(opt)
    assert [ds[i]["seq_length"] for i in range(len(ds))] == [61, 101, 156]
    assert ds[0]["key_labels"].shape == (156, 12) and ds[0]["mel"].shape == (1, 288, 156)
    net, trainer = fit_once(opt, ds, seed=0)
    losses = trainer.train_losses
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert len(trainer.val_results) == 2 and set(trainer.val_results[-1]) == set(VAL_KEYS)
    res = Trainer().validate(net)[0]
    assert set(res) == set(VAL_KEYS) and all(np.isfinite(list(res.values()))), res
    assert res == trainer.val_results[-1]
    net2, trainer2 = fit_once(opt, ds, seed=0)
    assert trainer2.train_losses == losses
    for (k, a), b in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(a, b), k                                          # two seeded runs: bit-identical weights
