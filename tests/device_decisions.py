"""Test helper (not product code): the decisions of the device's train-mode forward, restated on the host side from what the backward
kernels themselves read, and a float64 oracle step that is told to take them.

The device keeps no masks or indices.  Its backward kernels re-derive every decision from the raw convolution output z and the per-channel
(scale, shift, slope) table of the BatchNorm behind it (`affine_act`, csrc/pcnet_kernels.h):
    y = fmaf(z, scale, shift);  a = y > 0 ? y : y * slope
    LeakyReLU:            the sign y > 0                              (act_bwd_stats_kernel, bn_bwd_apply_kernel, the weight gradients' loads)
    octave fold:          the first maximum of a over the octaves     (fold_bwd_kernel, `if (v > bv)`)
    time pool (1, tp):    the first maximum of a inside each window   (time_pool_bwd_kernel, the same rule)
Both inputs sit in the training workspace between the forward and the backward: `net.tap("train:raw/<bn>")`, `net.tap("train:aff/<bn>")`.
Here the same is computed with torch on the GPU: z * scale is exact in float64 (two float32 factors), so float32(float64(z) * scale + shift)
is the fused multiply-add up to a double rounding; y * slope is one float32 product as on the device; torch's argmax returns the first
maximum.  A float64 oracle run under `pcnet_oracle.forced_decisions` with these decisions is a smooth function of the weights around the
device's operating point: against it the device's gradients must be tight at every batch size and seed."""
import torch

import test_gpu_backward as tb
from conftest import rel_err
from oracle import pcnet_oracle

DEV = "cuda:0"


def bn_sites(sd):
    """state_dict prefixes ("model.1.p2p.layer.4.") of every BatchNorm, in state_dict order."""
    return [k[:-len("running_mean")] for k in sd if k.endswith("running_mean")]


class DeviceDecisions:
    """Reads (z, aff) of every BatchNorm site from the workspace of `net`'s last train-mode forward -- call BEFORE the backward -- and keeps,
    on the GPU: pre[site] = y (float32), sign[site] = y > 0, and the pool winners under the oracle's site names.  Calling the object with a
    site name returns the decision (the provider of forced_decisions)."""

    def __init__(self, net, time_pool_size=2):
        sd = net.state_dict()
        self.pre, self.decision = {}, {}
        winners = {}                          # BatchNorm site whose activation is pooled -> (the pool's site name, kind)
        i = 0
        while f"model.{i}.pool_semi_b.running_mean" in sd:
            winners[f"model.{i}.pool_semi_b."] = (f"model.{i}.pool", "octave")
            for stack, pool in (("p2p", "time_pool_p"), ("pc2pc", "time_pool_pc")) if i >= 1 else ():
                j = 0
                while f"model.{i}.{stack}.layer.{3 * (j + 1) + 1}.running_mean" in sd:
                    j += 1
                winners[f"model.{i}.{stack}.layer.{3 * j + 1}."] = (f"model.{i}.{pool}", "time")
            i += 1
        for site in bn_sites(sd):
            z = net.tap("train:raw/" + site)
            aff = net.tap("train:aff/" + site).double()
            assert aff.shape == (z.shape[1], 3), (site, aff.shape, z.shape)
            y = (z.double() * aff[:, 0].view(1, -1, 1, 1) + aff[:, 1].view(1, -1, 1, 1)).float()
            self.pre[site] = y
            self.decision[site] = y > 0
            if site not in winners:
                continue
            a = torch.where(y > 0, y, y * aff[:, 2].float().view(1, -1, 1, 1))
            B, C, H, T = a.shape
            name, kind = winners[site]
            if kind == "octave":                                                  # row = octave * 12 + pitch class
                assert H % 12 == 0
                self.decision[name] = a.reshape(B, C, H // 12, 12, T).argmax(dim=2).to(torch.uint8)
            else:
                tp = time_pool_size
                self.decision[name] = a[..., :T // tp * tp].reshape(B, C, H, T // tp, tp).argmax(dim=-1).to(torch.uint8)
        self.parity = {}

    def __call__(self, site):
        d = self.decision.get(site)
        return None if d is None else d.cpu()

    def observe(self, site, x):
        """forced_decisions' observer: forward parity of the device's pre-activation against the oracle's BatchNorm output at the same site."""
        if site in self.pre:
            self.parity[site] = rel_err(self.pre[site].cpu(), x)


def forced_reference(sd32, x, seq, labels, dec, genre=True, kernel_size=7):
    """(loss, {name: gradient}, context) of the float64 oracle step that takes the decisions of `dec` (a DeviceDecisions)."""
    sd = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
          for k, v in sd32.items()}
    with pcnet_oracle.forced_decisions(dec, keep_own=False, observe=dec.observe) as ctx:
        out = pcnet_oracle.pcnet_forward(sd, x.double(), seq, training=True, kernel_size=kernel_size, genre=genre)
    loss = tb.loss_fn(out[0], out[1], out[2] if genre else None, *labels)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad}, ctx


def device_step(net, x, seq, labels, genre=True):
    """One train-mode forward + backward of `net`; the decisions are read in between.  -> (loss, {name: gradient (cpu, float64)}, DeviceDecisions)"""
    for p in net.parameters():
        p.grad = None
    out = net(x.to(DEV), seq.to(DEV))
    dec = DeviceDecisions(net)
    loss = tb.loss_fn(out[0], out[1], out[2] if genre else None, *(t.to(DEV) if t is not None else None for t in labels))
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in net.named_parameters()}, dec


def grad_rows(got, ref):
    """test_gpu_backward.grad_errors on two dictionaries: [(max|g - ref| / max|ref|, name, max|ref|)], worst first, with its rules unchanged --
    a convolution bias in front of a BatchNorm has an exactly-zero gradient and the device must return (near) zero; only the FLOORED tensors
    are measured against 1e-4 of the step's largest gradient instead of their own size."""
    floor = 1e-4 * max(float(ref[n].abs().max()) for n in got)
    rows = []
    for name, g in got.items():
        r = ref[name]
        if name.endswith(".bias") and float(r.abs().max()) < 1e-9:
            assert float(g.abs().max()) < 1e-6, name
            continue
        scale = max(float(r.abs().max()), floor if name in tb.FLOORED else 0.0, 1e-7)
        rows.append((float((g - r).abs().max()) / scale, name, float(r.abs().max())))
    rows.sort(reverse=True)
    return rows


PARITY_TOL = 1e-4     # the suite's forward tolerance (the train-mode forward tests use 2e-4 at the outputs)
FLIP_CAP = 1e-5       # of the decisions of a case; float32 torch on the CPU shows 0.4e-6 .. 1e-6 against its own float64
GRAD_TOL = 2e-5       # the suite's tight bound (test_gpu_backward.test_default_net_gradients_tight)


def check_against_forced(tag, sd32, x, seq, labels, loss, got, dec, ill, genre=True, kernel_size=7, named=None, cancelling=()):
    """The three statements of tests/test_gpu_backward_decisions.py for one device step; prints the figures before it asserts.
    `ill`: the project's ILL_CONDITIONED list; `named`: further bounds by tensor name (each with its reason at the call); `cancelling`:
    tensors whose exact gradient is zero, held as test_gpu_backward.cancelling_ok holds them -- |error| < 1e-5 of the step's LARGEST
    gradient -- instead of against their own size."""
    loss_ref, ref, ctx = forced_reference(sd32, x, seq, labels, dec, genre=genre, kernel_size=kernel_size)
    rows = grad_rows(got, ref)
    worst_site = max(dec.parity, key=dec.parity.get)
    print(f"\n{tag}: forward parity worst {dec.parity[worst_site]:.2e} ({worst_site}); {ctx.total_flips} of {ctx.total_decisions} decisions forced "
          f"against the oracle's own; gradients worst {rows[0][0]:.2e} ({rows[0][1]}), median {rows[len(rows) // 2][0]:.2e}; "
          f"loss {loss:.8f} against {loss_ref:.8f}")
    for e, n, m in rows[:4]:
        print(f"      {e:9.2e}  max|ref| {m:9.2e}  {n}")
    # 1. forward parity per site (every BatchNorm of the net was visited by the oracle and read from the device)
    assert set(dec.parity) == set(dec.pre) and set(ctx.counts) == set(dec.decision), set(ctx.counts) ^ set(dec.decision)
    bad = {s: e for s, e in dec.parity.items() if not e < PARITY_TOL}
    assert not bad, bad
    # 2. flip cap
    assert ctx.total_flips <= FLIP_CAP * ctx.total_decisions, (ctx.total_flips, ctx.total_decisions, {s: f for s, f in ctx.flips.items() if f})
    # 3. loss and gradients
    assert abs(loss - loss_ref) < 2e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    bound = dict(ill, **(named or {}))
    bad = [(e, n) for e, n, _ in rows if n not in cancelling and not e <= bound.get(n, GRAD_TOL)]
    assert not bad, bad[:6]
    gmax = max(float(ref[n].abs().max()) for n in got)
    bad = [(n, float((got[n] - ref[n]).abs().max()), gmax) for n in cancelling if not float((got[n] - ref[n]).abs().max()) < 1e-5 * gmax]
    assert not bad, bad
    return rows, ctx


_BENCH_SHARD = {}


def bench_shard_run(gold_default):
    """The device step of the benchmark's per-rank batch (256 clips x 76 frames, big_case seed 7), run once for
    test_gpu_train_scale.test_gradients_at_the_bench_shard (free float64 reference) and the forced-decision case of
    tests/test_gpu_backward_decisions.py: -> dict(sd32, x, seq, labels, loss, got, dec)."""
    if not _BENCH_SHARD:
        import test_gpu_train_scale as ts
        net, sd32 = ts.fresh_net(gold_default)
        x, seq, labels = ts.big_case(256, 76, 7)
        loss, got, dec = device_step(net, x, seq, labels)
        _BENCH_SHARD.update(sd32=sd32, x=x, seq=seq, labels=labels, loss=loss, got=got, dec=dec)
    return _BENCH_SHARD
