"""PARITY (GPU) at the sizes that are BENCHMARKED: the training step of `bench.py --train` / BASELINE configs[3]
runs 256 clips x 76 frames per rank -- 7 424 row tiles on 256 persistent workgroups, hundreds of weight-gradient partials, BatchNorm sums
over 5.6 M values per channel -- while every other gradient test uses 1..6 clips (one tile per workgroup).  Here:

  * gradients of the default net at 32 clips x 76 frames (29 x 32 = 928 tiles: 3-4 tiles per workgroup of conv_p2p_f16x3_kernel, its
    double-buffer swap / pending-store hand-over / statistics flush; 32..64 partials in wgrad_partial_reduce_kernel) against float64
    autograd through the pinned oracle -- the kink-robust statement of tests/test_gpu_backward.py;
  * the same at 256 clips (the benchmark's per-rank shard) -- one seed, float64 autograd of the whole batch on the host (about a minute);
  * the train-mode forward at 256 clips: outputs AND every BatchNorm's batch mean / variance against the float64 oracle forward;
  * gradients are homogeneous in the loss scale: a loss times 2^-10 must give the same gradients times 2^-10 (the f16 hi / lo
    data-gradient operands once lost their low bits for |dz| below f16's normal range).
"""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ake_amd
from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# model.0.pool_semi_b.weight: see tests/test_gpu_backward.py.  The last biases of the tonic / genre heads: the softmax gradient sums to zero over
# the classes and the bias reaches every class alike, so their gradient is an exactly cancelling sum (|ref| ~ 1e-8 next to 1e-1).
# model.0.pool_semi_b.bias: the same BatchNorm's other cancelling sum (2e-5 between 512 and 256 clips where its weight shows 5e-4)
ILL_CONDITIONED = {"model.0.pool_semi_b.weight": 2e-3, "model.0.pool_semi_b.bias": 2e-4, "tonic_classifier.3.conv2d.bias": 2e-3,
                   "genre_classifier.3.bias": 2e-3}


def big_case(batch, frames, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand((batch, 1, 288, frames), generator=g) * 2.5
    seq = frames - torch.randint(0, 20, (batch,), generator=g)
    seq[0] = frames
    key_labels = (torch.rand((batch, 12), generator=g) > 0.5).float()
    tonic_idx = torch.randint(0, 12, (batch,), generator=g)
    genre_idx = torch.randint(0, 11, (batch,), generator=g)
    genre_mask = torch.rand((batch,), generator=g) > 0.25
    genre_mask[0] = True
    return x, seq, (key_labels, tonic_idx, genre_idx, genre_mask)


def loss_fn(key, tonic, genre, key_labels, tonic_idx, genre_idx, genre_mask):
    loss = F.binary_cross_entropy(key, key_labels.to(key.dtype)) + F.cross_entropy(tonic, tonic_idx)     # models.py:878-889
    return loss + 0.1 * F.cross_entropy(genre[genre_mask], genre_idx[genre_mask])                         # models.py:881-893


def oracle_grads(sd32, x, seq, labels):
    sd = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
          for k, v in sd32.items()}
    out = pcnet_oracle.pcnet_forward(sd, x.double(), seq, training=True)
    loss = loss_fn(out[0], out[1], out[2], *labels)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad}


def fresh_net(gold_default):
    opt = Namespace(**json.loads(str(gold_default["opt"])))
    net = ake_amd.PitchClassNet(288, 12, 2, 7, opt)
    sd32 = golden_state_dict(gold_default)
    net.load_state_dict(sd32, strict=True)
    return net.to(DEV).train(), sd32


def device_grads(net, x, seq, labels, scale=1.0):
    for p in net.parameters():
        p.grad = None
    out = net(x.to(DEV), seq.to(DEV))
    loss = loss_fn(out[0], out[1], out[2], *(t.to(DEV) for t in labels))
    (loss * scale).backward()
    return float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in net.named_parameters()}


def error_rows(got, ref):
    """[(max|g - ref| / max(max|ref|, floor), name, max|ref|, unfloored ratio)], worst first; floor = 1e-4 of the step's largest gradient
    (a tensor four orders below it is a cancelling sum whose absolute accuracy the others set, tests/test_gpu_backward.py)."""
    floor = 1e-4 * max(float(ref[n].abs().max()) for n in got)
    rows = []
    for n, g in got.items():
        r = ref[n]
        m = float(r.abs().max())
        if n.endswith(".bias") and m < 1e-9:          # a convolution bias in front of a BatchNorm: exactly zero gradient
            assert float(g.abs().max()) < 1e-6, n
            continue
        d = float((g - r).abs().max())
        rows.append((d / max(m, floor, 1e-7), n, m, d / max(m, 1e-30)))
    rows.sort(reverse=True)
    return rows


def report(tag, rows):
    print(f"\n{tag}: worst {rows[0][0]:.2e} ({rows[0][1]}), median {rows[len(rows) // 2][0]:.2e}, "
          f"worst unfloored {max(r[3] for r in rows):.2e}")


F32_BAND = (5e-2, 1e-2)     # (worst tensor, median tensor): what float32 PyTorch on the CPU itself shows against float64 at these sizes, see below
TOP = ("key_classifier.3.conv2d.weight", "tonic_classifier.3.conv2d.weight", "genre_classifier.3.weight")    # nothing above them can flip


def test_gradients_at_32_clips(gold_default):
    """Four data seeds at 32 x 76 against float64 autograd.

    At this size no float32 run is tight in every tensor: of the 2.4e7 LeakyReLU / max decisions of a step a handful sit within 1e-6 of the
    kink and go the other way than in the float64 forward, and because a gradient tensor is a cancelling sum over N ~ 1e6 positions ONE
    flipped position moves it by ~N^-1/2 = 1e-3 of its size -- and every tensor upstream of it.  Stock float32 PyTorch on the CPU, same
    batches, against the same float64 gradients: worst tensor 4.6e-3 .. 3.0e-2, MEDIAN tensor 1.0e-3 .. 3.6e-3 on each of seeds 0-3
    (256 clips: 5.2e-3 / 2.1e-3).  So against float64 the statement is: every seed inside that band; the tensors no flip can reach tight
    on every seed; and a seed whose flips sit low in the net (seed 0: median 5e-6) shows most tensors tight.  The flip-free statements at
    these sizes are the replication identities below (device against device) and tests/test_gpu_backward_decisions.py (these four batches
    against float64 autograd at the device's own decisions, every tensor to 2e-5)."""
    net, sd32 = fresh_net(gold_default)
    medians = []
    for seed in range(4):
        x, seq, labels = big_case(32, 76, seed)
        loss_ref, ref = oracle_grads(sd32, x, seq, labels)
        loss, got = device_grads(net, x, seq, labels)
        assert abs(loss - loss_ref) < 2e-5 * max(1.0, abs(loss_ref)), (seed, loss, loss_ref)
        rows = error_rows(got, ref)
        report(f"32 clips, seed {seed}", rows)
        assert rows[0][0] < F32_BAND[0] and rows[len(rows) // 2][0] < F32_BAND[1], (seed, rows[:4])
        # no tensor is "effectively unchecked" (ADVICE r2): relative to its OWN largest entry every gradient tensor is right to 10 %
        assert max(r[3] for r in rows if r[1] not in ILL_CONDITIONED) < 1e-1, (seed, sorted(rows, key=lambda r: -r[3])[:4])
        by_name = {n: e for e, n, _, _ in rows}
        for n in TOP:
            assert by_name[n] < 3e-5, (seed, n, by_name[n])
        medians.append(rows[len(rows) // 2][0])
    assert min(medians) < 3e-5, medians


def replicate(x, seq, labels, copies, seed):
    """`copies` copies of every clip, in a random order: the batch statistics of every BatchNorm, the per-clip activations and the (mean)
    losses are those of the small batch, so the loss is the same FUNCTION of the weights and the gradients are equal."""
    perm = torch.randperm(x.shape[0] * copies, generator=torch.Generator().manual_seed(seed))
    rep = lambda t: t.repeat((copies,) + (1,) * (t.dim() - 1))[perm]
    return rep(x), rep(seq), tuple(rep(t) for t in labels)


def test_64_clips_equal_the_replicated_32(gold_default):
    """Two shuffled copies of a 32-clip batch (64 x 76: 1 856 row tiles, 7 per persistent workgroup; twice the weight-gradient partials,
    other workgroup shapes in the weight-gradient kernels) give the 32-clip gradients: every tensor to 1e-5 (measured 2e-7 .. 3e-6)."""
    net, _ = fresh_net(gold_default)
    x, seq, labels = big_case(32, 76, 0)
    loss32, g32 = device_grads(net, x, seq, labels)
    loss64, g64 = device_grads(net, *replicate(x, seq, labels, 2, 5))
    assert abs(loss64 - loss32) < 2e-6 * max(1.0, abs(loss32)), (loss64, loss32)
    rows = error_rows(g64, g32)
    report("64 = 2 x 32 clips against 32 clips (device both)", rows)
    bad = [(e, n) for e, n, _, _ in rows if e > ILL_CONDITIONED.get(n, 1e-5)]
    assert not bad, bad[:6]


def test_bench_shard_gradients_against_the_replicated_32_clips(gold_default):
    """256 clips x 76 frames = 8 shuffled copies of a 32-clip batch against the 32-clip gradients (same loss function of the weights).  From
    256 clips on (one per CU) the generic convolution kernel picks other tilings (whole-clip time tiles, other input-channel chunks), whose
    outputs differ from the small-batch tilings' in the last bit (deterministically: two runs of either are bit-identical) -- enough to flip
    a handful of the 4e7 decisions, ~1e-3 each (module docstring).  So this link of the chain is a BAND statement; the flip-free statements
    on either side of it are test_64_clips_equal_the_replicated_32 (small-batch tilings, several tiles per persistent workgroup) and
    test_512_clips_equal_the_replicated_256 (large-batch tilings)."""
    net, _ = fresh_net(gold_default)
    for seed in range(3):
        x, seq, labels = big_case(32, 76, seed)
        loss32, g32 = device_grads(net, x, seq, labels)
        loss256, g256 = device_grads(net, *replicate(x, seq, labels, 8, 5 + seed))
        assert abs(loss256 - loss32) < 2e-6 * max(1.0, abs(loss32)), (loss256, loss32)
        rows = error_rows(g256, g32)
        report(f"256 = 8 x 32 clips against 32 clips (device both), seed {seed}", rows)
        assert rows[0][0] < F32_BAND[0] and rows[len(rows) // 2][0] < F32_BAND[1], (seed, rows[:5])
        by_name = {n: e for e, n, _, _ in rows}
        for n in TOP:
            assert by_name[n] < 1e-5, (seed, n, by_name[n])


def test_512_clips_equal_the_replicated_256(gold_default):
    """The benchmarked shard's kernels, flip-free: 512 = 2 shuffled copies of a 256-clip batch of distinct clips give the 256-clip gradients
    in every tensor to 1e-5.  Both sides run the large-batch tilings (7 424 / 14 848 row tiles on 256 persistent workgroups: 29 / 58 per
    workgroup -- prefetch, buffer swap, pending stores, statistics flush; 512 / 1 024 ordered weight-gradient partials; 72 rows per
    workgroup in the pitch weight gradient; BatchNorm sums over 5.6 / 11 M values per channel; dz around 1e-7 / 5e-8 in the f16 hi / lo
    data-gradient operands), so the BatchNorm tables are the same bits and no decision flips."""
    net, _ = fresh_net(gold_default)
    x, seq, labels = big_case(256, 76, 11)
    loss256, g256 = device_grads(net, x, seq, labels)
    loss512, g512 = device_grads(net, *replicate(x, seq, labels, 2, 3))
    assert abs(loss512 - loss256) < 2e-6 * max(1.0, abs(loss256)), (loss512, loss256)
    rows = error_rows(g512, g256)
    report("512 = 2 x 256 clips against 256 clips (device both)", rows)
    bad = [(e, n) for e, n, _, _ in rows if e > ILL_CONDITIONED.get(n, 1e-5)]
    assert not bad, bad[:6]


def test_gradients_at_the_bench_shard(gold_default):
    """256 clips x 76 frames of DISTINCT data -- the per-rank batch of `bench.py --train` and of BASELINE configs[3] -- against float64
    autograd of the whole batch (about a minute on the host).  Inside the float32 band (float32 PyTorch on the CPU, this batch: worst
    5.2e-3, median 2.1e-3 against the same float64 gradients); the tensors nothing can flip above -- the heads' last convolutions -- tight.
    The flip-free statement about this very step is tests/test_gpu_backward_decisions.py::test_the_bench_shard_is_tight: the same device
    gradients against float64 at the device's own decisions, every tensor to 2e-5."""
    import device_decisions
    run = device_decisions.bench_shard_run(gold_default)      # the device step, shared with tests/test_gpu_backward_decisions.py
    sd32, x, seq, labels, loss, got = (run[k] for k in ("sd32", "x", "seq", "labels", "loss", "got"))
    loss_ref, ref = oracle_grads(sd32, x, seq, labels)
    assert abs(loss - loss_ref) < 2e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    rows = error_rows(got, ref)
    report("256 clips", rows)
    assert rows[0][0] < F32_BAND[0] and rows[len(rows) // 2][0] < F32_BAND[1], rows[:4]
    assert max(r[3] for r in rows if r[1] not in ILL_CONDITIONED) < 1e-1, sorted(rows, key=lambda r: -r[3])[:4]
    by_name = {n: e for e, n, _, _ in rows}
    for n in TOP:
        assert by_name[n] < 3e-5, (n, by_name[n])


def test_gradients_scale_with_the_loss(gold_default):
    """grad(2^-10 loss) == 2^-10 grad(loss): a power-of-two factor is exact in every float operation of the backward pass, so the two
    differ only where an operand's absolute size matters -- the 2^-40 resolution of the fixed-point sums (1e-12) and, before the fix, the
    f16 hi / lo planes of dz.  At 32 x 76 the unscaled dz are already ~1e-5; times 2^-10 they are where 256 clips and genre_weight put them."""
    net, _ = fresh_net(gold_default)
    x, seq, labels = big_case(32, 76, 1)
    _, g1 = device_grads(net, x, seq, labels)
    _, g2 = device_grads(net, x, seq, labels, scale=2.0 ** -10)
    floor = 1e-4 * max(float(g.abs().max()) for g in g1.values())      # (the tonic head's last bias: sum of softmax - onehot, zero to rounding)
    errs = sorted(((float((g2[n] * 1024.0 - g1[n]).abs().max()) / max(float(g1[n].abs().max()), floor), n) for n in g1), reverse=True)
    print(f"\nloss-scale homogeneity: worst {errs[0][0]:.2e} ({errs[0][1]}), median {errs[len(errs) // 2][0]:.2e}")
    bad = [(e, n) for e, n in errs if e > ILL_CONDITIONED.get(n, 1e-4)]
    assert not bad and errs[len(errs) // 2][0] < 1e-5, errs[:5]


def test_train_forward_and_batch_statistics_at_the_bench_batch(gold_default):
    """Train-mode forward of 256 x 76: the three outputs and EVERY BatchNorm's batch mean / biased variance (recovered from the running
    statistics the step leaves: running = 0.9 old + 0.1 batch) against the float64 oracle forward of the same batch."""
    net, sd32 = fresh_net(gold_default)
    with torch.no_grad():       # running statistics zeroed: after ONE train-mode forward they are 0.1 x the batch statistics to f32 rounding
        for m in net.modules():  # (recovering them from 0.9 old + 0.1 batch loses 10 x 6e-8 of the OLD value: 6e-5 of a small variance)
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.zero_(); m.running_var.zero_()
    sd32 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x, seq, _ = big_case(256, 76, 3)
    sd64 = pcnet_oracle.to_dtype(sd32, torch.float64)
    with torch.no_grad(), pcnet_oracle.record_bn_stats() as rows:
        ref = pcnet_oracle.pcnet_forward(sd64, x.double(), seq, training=True)
    with torch.no_grad():
        got = net(x.to(DEV), seq.to(DEV))
    for a, b, name in zip(got, ref, ("key", "tonic", "genre")):
        assert rel_err(a.cpu(), b) < 2e-4, (name, rel_err(a.cpu(), b))
    new = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    assert len(rows) == sum(1 for k in sd32 if k.endswith("running_mean"))
    worst_m = worst_v = 0.0
    for prefix, mean, var, count in rows:
        m_dev = (new[prefix + "running_mean"] - 0.9 * sd64[prefix + "running_mean"]) / 0.1
        v_dev = (new[prefix + "running_var"] - 0.9 * sd64[prefix + "running_var"]) / 0.1 * (count - 1) / count
        std = var.sqrt()
        em = float(((m_dev - mean).abs() / (std + 1e-6)).max())          # the mean in units of the channel's standard deviation
        ev = float(((v_dev - var).abs() / (var + 1e-12)).max())
        worst_m, worst_v = max(worst_m, em), max(worst_v, ev)
        assert em < 5e-6 and ev < 5e-6, (prefix, em, ev)
        assert int(new[prefix + "num_batches_tracked"]) == int(sd32[prefix + "num_batches_tracked"]) + 1
    print(f"\nbatch statistics at 256 clips: mean {worst_m:.2e} sigma, variance {worst_v:.2e} relative")
