"""CPU restatement of a short ``Trainer.fit`` on the reference module.

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``): the oracle forward in train mode with torch's running-statistics update, the
``general_step`` loss with autograd (pinned on ``loss_oracle``), ``torch.optim.Adam``.  Used by tests/test_gpu_training.py (the curve a
device fit is held to) and by oracle/make_trained.py (the recipe of tests/golden/pcnet_trained.npz).
"""
import torch

from . import loss_oracle, pcnet_oracle


def torch_loss(out, b):
    """models.py:878-893 with autograd (the numpy loss_oracle pins its value below)."""
    F = torch.nn.functional
    loss = F.binary_cross_entropy(out[0], b["key_labels"].to(out[0].dtype)) + F.cross_entropy(out[1], b["tonic_labels"].argmax(1))
    gl = b["genre"].long()
    mask = gl.sum(1) == 1
    if mask.sum() != 0:
        loss = loss + 0.1 * F.cross_entropy(out[2][mask], gl.argmax(1)[mask])
    return loss


def oracle_fit(sd32, opt, batches, acc, steps, lr=3e-4, gamma=0.96, dtype=torch.float64):
    """float64 restatement of Trainer.fit on the reference module within ONE epoch: oracle forward (train-mode BN + torch's running-statistics
    update), general_step loss (loss_oracle), torch.optim.Adam at a constant `lr`: no ExponentialLR step is applied, the loop restates the
    steps in front of the scheduler's first one.  `opt` and `gamma` are not read; they stay in the signature for the callers that
    pass them.  `acc`: accumulate_grad_batches; `steps`: optimizer steps after which the loop ends.
    dtype=torch.float32: the same loop as stock float32 PyTorch on the CPU would run it (the band a float32 run occupies around the float64 curve)."""
    sd = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and "num_batches" not in k
              else v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in sd32.items()}
    params = [v for v in sd.values() if torch.is_tensor(v) and v.requires_grad]
    optim = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999))
    losses = []
    done = 0
    for i, b in enumerate(batches):
        with pcnet_oracle.record_bn_stats() as rows:
            out = pcnet_oracle.pcnet_forward(sd, b["mel"].to(dtype), b["seq_length"], training=True)
        pcnet_oracle.update_running_stats(sd, rows)
        loss = torch_loss(out, b)
        if i == 0 and dtype == torch.float64:
            pinned = loss_oracle.general_step_loss(out[0].detach().numpy(), out[1].detach().numpy(), out[2].detach().numpy(),
                                                   b["key_labels"].numpy(), b["tonic_labels"].numpy(), b["genre"].numpy())
            assert abs(float(loss.detach()) - float(pinned)) < 1e-12
        (loss / acc).backward()
        losses.append(float(loss.detach()))
        if (i + 1) % acc == 0 or i + 1 == len(batches):
            optim.step(); optim.zero_grad(); done += 1
            if done >= steps:
                break
    return losses, sd
