"""CPU restatement of ``PitchClassNet.forward`` (default architecture family).

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).  Stock torch CPU ops,
any float dtype (float64 is the reference's dtype, ``models.py:199,237,739``).

Every function cites the reference lines it restates (``/root/reference``).
The restatement is purely functional: it consumes a reference-format
``state_dict`` (key names of SURVEY.md section 8b) and never builds modules, so
it shares no code path with the product's drop-in class.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.01   # nn.LeakyReLU() default, models.py:197,234,315
BN_EPS = 1e-5        # nn.BatchNorm2d default, models.py:196,233,314


_BN_SINK = None      # set by record_bn_stats(): list of (prefix, batch mean, biased batch var, elements per channel)


class record_bn_stats:
    """Context manager: collect the batch statistics of every train-mode BatchNorm the forward visits, so that a caller
    can restate nn.BatchNorm2d's side effect (``running <- 0.9*running + 0.1*(mean, unbiased var)``, torch defaults; the
    reference never overrides momentum, models.py:196,233,314)."""

    def __enter__(self):
        global _BN_SINK
        self.rows = _BN_SINK = []
        return self.rows

    def __exit__(self, *exc):
        global _BN_SINK
        _BN_SINK = None


def update_running_stats(sd, rows, momentum=0.1, backward_ran=True):
    """Apply torch's train-mode running-statistics update to ``sd`` in place for the rows of ``record_bn_stats``.

    ``backward_ran``: the reference checkpoints norm1 + conv1 of every dense layer (``cp.checkpoint``, models.py:484-489, 553), so a
    training step's BACKWARD runs those BatchNorms a second time in train mode: they blend the same batch statistics twice and count two
    batches per step (pinned by tests/golden/pcnet_denseblock_train_T40.npz)."""
    with torch.no_grad():
        for prefix, mean, var, count in rows:
            unbiased = var * count / max(count - 1, 1)
            for _ in range(2 if backward_ran and ".denselayer" in prefix and prefix.endswith(".norm1.") else 1):
                sd[prefix + "running_mean"].mul_(1 - momentum).add_(momentum * mean.detach().to(sd[prefix + "running_mean"].dtype))
                sd[prefix + "running_var"].mul_(1 - momentum).add_(momentum * unbiased.detach().to(sd[prefix + "running_var"].dtype))
                key = prefix + "num_batches_tracked"
                if key in sd:
                    sd[key] += 1


def _bn(x, sd, prefix, training=False, stats=None):
    """BatchNorm2d, eval mode = running stats (models.py:196 etc.).

    ``training=True`` restates train-mode normalisation (batch statistics,
    biased variance) as ``equivariance_test.py:178`` runs the net; running
    buffers are not updated here (see ``record_bn_stats`` / ``update_running_stats``).
    """
    w, b = sd[prefix + "weight"], sd[prefix + "bias"]
    if training:
        mean = x.mean(dim=(0, 2, 3))
        var = x.var(dim=(0, 2, 3), unbiased=False)
        if _BN_SINK is not None:
            _BN_SINK.append((prefix, mean, var, x.numel() // x.shape[1]))
    else:
        mean, var = sd[prefix + "running_mean"], sd[prefix + "running_var"]
    if stats is not None:
        stats[prefix] = (mean, var)
    scale = w / torch.sqrt(var + BN_EPS)
    return (x - mean[None, :, None, None]) * scale[None, :, None, None] + b[None, :, None, None]


_DECISIONS = None    # set by forced_decisions(): the active context


class forced_decisions:
    """Context manager: take every DECISION of the forward -- the sign of each LeakyReLU pre-activation, the winning octave of each
    Pitch2PitchClassPool, the winning frame of each time-pool window -- from ``provider`` instead of from the oracle's own values.  With
    the decisions fixed the forward is a smooth (piecewise-linear pieces glued by the BatchNorm statistics) function of the weights, so
    a float64 run that is told the decisions of a float32 run has that run's gradients to rounding, whereas a free float64 run differs
    by 1e-3 .. 3e-2 wherever one pre-activation within 1e-6 of zero goes the other way.

    Sites are named by reference module path, as ``taps``:
      * ``<bn prefix>`` (e.g. ``model.1.p2p.layer.4.``) for every LeakyReLU(BatchNorm(.)): a boolean tensor of the activation's shape,
        True where the positive branch is taken, ``y = where(mask, z, slope * z)``;
      * ``model.i.pool``: the octave index (int64) per (clip, channel, pitch class, frame);
      * ``model.i.time_pool_p`` / ``model.i.time_pool_pc``: the index inside each window (int64) per (clip, channel, row, pooled frame).
    ``provider`` is a mapping or a callable ``site -> tensor``; a site it does not know (KeyError / None) keeps the oracle's own
    decision.  ``provider=None`` forces nothing and only records.  After the forward ``own[site]`` holds the oracle's own decision (the
    first maximum for the pools, as ``nn.MaxPool2d``), ``flips[site]`` the number of forced decisions that differ from it and
    ``counts[site]`` the number of decisions; ``keep_own=False`` keeps the counts only.  ``observe(site, x)`` (optional) is called with
    the detached tensor each decision is taken on -- the BatchNorm output in front of a LeakyReLU, the windows of a pool -- before the
    provider is asked, so that a caller can compare the forward per site.

    Default family only (num_layers, n_filters, conv_layers, kernel_size, head_layers, genre, mean head pooling): the architecture
    variants, --local and max_pool raise NotImplementedError under the context.  Without the context nothing changes."""

    def __init__(self, provider=None, keep_own=True, observe=None):
        self.provider, self.keep_own, self.observe = provider, keep_own, observe
        self.own, self.flips, self.counts = {}, {}, {}

    def __enter__(self):
        global _DECISIONS
        assert _DECISIONS is None, "forced_decisions does not nest"
        _DECISIONS = self
        return self

    def __exit__(self, *exc):
        global _DECISIONS
        _DECISIONS = None

    def decide(self, site, own, x):
        """The decision to apply at ``site`` given the oracle's own (taken on ``x``); records both."""
        assert site not in self.counts, f"decision site {site!r} visited twice"
        if self.observe is not None:
            self.observe(site, x)
        forced = None
        if self.provider is not None:
            try:
                forced = self.provider(site) if callable(self.provider) else self.provider[site]
            except KeyError:
                forced = None
        self.counts[site] = own.numel()
        if forced is None:
            self.flips[site] = 0
        else:
            forced = forced.to(device=own.device, dtype=own.dtype)
            if forced.shape != own.shape:
                raise ValueError(f"forced_decisions: {site!r} wants shape {tuple(own.shape)}, the provider gave {tuple(forced.shape)}")
            self.flips[site] = int((forced != own).sum())
        if self.keep_own:
            self.own[site] = own
        return own if forced is None else forced

    @property
    def total_flips(self):
        return sum(self.flips.values())

    @property
    def total_decisions(self):
        return sum(self.counts.values())


def _no_forcing(what):
    if _DECISIONS is not None:
        raise NotImplementedError(f"forced_decisions covers the default architecture family only: {what} is not supported")


def _lrelu(x, site=None):
    """LeakyReLU behind the BatchNorm ``site`` (its state_dict prefix): the one place where a sign decision is taken."""
    if _DECISIONS is None:
        return F.leaky_relu(x, LRELU_SLOPE)
    if site is None:
        _no_forcing("an activation without a site name")
    mask = _DECISIONS.decide(site, (x > 0).detach(), x.detach())
    return torch.where(mask, x, LRELU_SLOPE * x)


def _act_bn(x, sd, prefix, training):
    return _lrelu(_bn(x, sd, prefix, training), prefix)


def _time_pool(x, size, site):
    """F.max_pool2d(x, (1, size)) (models.py:395-396); under forced_decisions the winner of each window comes from the provider."""
    if _DECISIONS is None:
        return F.max_pool2d(x, (1, size))
    B, C, H, T = x.shape
    w = x[..., :T // size * size].reshape(B, C, H, T // size, size)
    idx = _DECISIONS.decide(site, w.detach().argmax(dim=-1), w.detach())
    return w.gather(-1, idx.unsqueeze(-1)).squeeze(-1)


_ROUNDING = None     # set by rounding_model(): the active context

F16_MAX = 65504.0


def _f16(t):
    """Round to IEEE half and back (the device converts with saturation, MODE.FP16_OVFL: clamp first)."""
    return t.clamp(-F16_MAX, F16_MAX).to(torch.float16).to(t.dtype)


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _split(t, fmt):
    """(hi, lo) of the device's two-term operand split: f16 hi = rn(t), lo = rn((t - hi) * 2^11) / 2^11 (kP2pLoScale); bf16 hi = rn(t),
    lo = rn(t - hi) (bf16_bits, round to nearest even)."""
    if fmt == "f16":
        hi = _f16(t)
        return hi, _f16((t - hi) * 2048.0) / 2048.0
    hi = _bf16(t)
    return hi, _bf16(t - hi)


def _weight_scale(w):
    """f16_weight_scale per output channel: the power of two s with s * max|w| in [2^13, 2^14) (1 for an all-zero channel)."""
    wmax = w.detach().abs().amax(dim=tuple(range(1, w.dim())), keepdim=True)
    _, e = torch.frexp(wmax)
    s = torch.ldexp(torch.ones_like(wmax), (14 - e).clamp(max=100))
    return torch.where(wmax > 0, s, torch.ones_like(s))


class rounding_model:
    """Context manager: the float64 forward with the operand roundings of the device's ``mixed`` precision, and
    nothing else of it -- every sum, bias, BatchNorm, activation and pool stays in the dtype of the run.  ``route`` maps the state_dict
    key of a convolution's weight to how the device multiplies it (``mixed_route`` builds it for a net and a shape):
      * ``"f16"``: one product of f16 operands.  The activation is rounded to f16; the weight is scaled by its output channel's power of
        two (``f16_weight_scale``), rounded to f16 and scaled back (pack_p2p_f16_kernel, pack_semi_f16_kernel);
      * ``"f16+split0"``: the same, but input channel 0 (the log-CQT in front of a stack's first pitch conv, kP2pSplit0) is multiplied
        f32-equivalently: x w ~ xh wh + xl wh + xh wl;
      * ``"f16x3"``: both operands split into f16 hi + lo (weights scaled as above), three products (layer0_mfma_kernel);
      * ``"bf16x3"``: both operands split into bf16 hi + lo, three products (conv_pc_bf16_kernel, pc2pc_fused_kernel, the head kernels).
    A convolution the route does not name is left alone.  The device rounds the weight AFTER folding the BatchNorm that follows into it
    (fold_pack; "BatchNorm already folded" in the pack kernels): with ``sd`` given, the model does the same -- it rounds
    ``w * gamma / sqrt(running_var + eps)`` per output channel and divides the factor out again, so that its weight roundings are the
    device's own and only the activation roundings are another draw.  Without ``sd`` the weight is rounded as it stands in the
    state_dict.  ``used`` collects the sites that were rounded.  Without the context nothing changes, to the bit."""

    def __init__(self, route, sd=None):
        self.route = dict(route)
        for site, mode in self.route.items():
            assert mode in ("f16", "f16+split0", "f16x3", "bf16x3"), (site, mode)
        self.used = []
        self.fold = {}
        for site in (self.route if sd is not None else ()):
            base = site[:-len(".conv2d.weight")] if site.endswith(".conv2d.weight") else site[:-len(".weight")]
            head, _, last = base.rpartition(".")
            bn = f"{head}.{int(last) + 1}." if last.isdigit() else base + "_b."
            if bn + "running_var" in sd:
                f = (sd[bn + "weight"] / torch.sqrt(sd[bn + "running_var"] + BN_EPS)).detach()
                self.fold[site] = torch.where(f == 0, torch.ones_like(f), f)

    def __enter__(self):
        global _ROUNDING
        assert _ROUNDING is None, "rounding_model does not nest"
        _ROUNDING = self
        return self

    def __exit__(self, *exc):
        global _ROUNDING
        _ROUNDING = None


def _conv(site, x, w, bias, fn):
    """``fn(x, w, bias)`` -- a convolution, bilinear in (x, w) -- as the active rounding_model multiplies the site ``site``."""
    mode = None if _ROUNDING is None else _ROUNDING.route.get(site)
    if mode is None:
        return fn(x, w, bias)
    _ROUNDING.used.append(site)
    if site in _ROUNDING.fold:         # round the weight as the device holds it: with the BatchNorm behind the convolution folded in
        f = _ROUNDING.fold[site].to(w.dtype).reshape(-1, *([1] * (w.dim() - 1)))
        inner = fn
        w, fn = w * f, lambda x_, w_, b_: inner(x_, w_ / f, b_)
    if mode == "bf16x3":
        (xh, xl), (wh, wl) = _split(x, "bf16"), _split(w, "bf16")
        return fn(xh, wh, bias) + fn(xl, wh, None) + fn(xh, wl, None)
    s = _weight_scale(w)
    if mode == "f16x3":
        (xh, xl), (wh, wl) = _split(x, "f16"), _split(w * s, "f16")
        return fn(xh, wh / s, bias) + fn(xl, wh / s, None) + fn(xh, wl / s, None)
    y = fn(_f16(x), _f16(w * s) / s, bias)
    if mode == "f16+split0":      # slot 5: channel 0's weight again, meets the activation's low half; slot 6: the weight's low half, meets the high half
        (xh, xl), (wh, wl) = _split(x[:, :1], "f16"), _split(w[:, :1] * s, "f16")
        only0 = lambda t, like: torch.cat([t, torch.zeros_like(like[:, 1:])], dim=1)
        y = y + fn(only0(xl, x), only0(wh / s, w), None) + fn(only0(xh, x), only0(wl / s, w), None)
    return y


def _p2p_ps_rows_semi(H, T):
    """p2p_ps_rows(H, T, semi = true) of csrc/pcnet.hip with 8 waves: the rows of a tile of the persistent pitch conv that also runs the
    semitone conv, 0 where the shape does not qualify (odd frame counts among them)."""
    if T < 2 or T & 1:
        return 0
    J = T // 2
    Tp = 2 * J + 16                                                       # p2p_pitch
    plane_of = lambda R: ((R + 6) * Tp + 63) // 64 * 64
    lds_of = lambda R: (2 * plane_of(R) + 2 * 8 * 3 * 16 * 2) * 16        # kP2pMT = 3
    R = max(1, min(H, 8 * 3 * 16 // J)) // 3 * 3
    while R >= 3 and (lds_of(R) > 156 * 1024 or plane_of(R) // 64 > 8 * 3):   # kP2pPieces = 3
        R -= 3
    if R < 3 or H < R + 6 or H % 3 or (H // 3) % 12:
        return 0
    return R


def mixed_route(sd, frames, kernel_size=7, head_layers=2, time_pool_size=2, local=False, keep_taps=False, pitches=None):
    """Which convolutions the device's ``mixed`` inference forward multiplies in reduced precision for THIS net at THIS frame count, as
    ``rounding_model`` wants them: a restatement of the arithmetic side of ``build_route()`` (csrc/pcnet_plan.h) and of the eligibility rules
    of ``rebuild_bf16_frags()``.  Which launch form runs a stage (per tile, persistent, one launch, fused heads) does not change what is
    rounded -- those forms are bit-identical to one another -- so batch size and CU count do not enter.  tests/test_gpu_sensitive.py holds
    this restatement to the kernel timer's labels of the forward it models.

    default net, 76 frames: layer 0's stack f16 x 3; the pitch convs and the semitone conv behind them one f16 product (the log-CQT
    channel of the first f32-equivalent); the last pitch-class stack and both convs of every head bf16 x 3."""
    route = {}
    L = 0
    while f"model.{L}.pc2pc.layer.0.conv2d.weight" in sd or f"model.{L}.pc2pc.layer.0.denselayer1.norm1.weight" in sd:
        L += 1
    dense = "model.0.pc2pc.layer.0.denselayer1.norm1.weight" in sd
    res = "model.0.pc2pc.layer.3.b1.weight" in sd
    p2pc_conv = "model.0.pool.conv.weight" in sd
    stay = L > 1 and "model.1.up_sixth.weight" not in sd
    if dense or L < 1:
        return route                                                  # --denseblock: conv_mfma_kernel (f32) throughout, generic heads (final_ch != 16)
    tp = 1 if local else time_pool_size
    conv_layers = _count(sd, "model.0.pc2pc.layer.", ".conv2d.weight") if not res else None
    NF = sd["model.0.pc2pc.layer.0.conv2d.weight"].shape[0]
    P = pitches if pitches is not None else 288
    Tl = [frames if i < 2 else None for i in range(L)]
    for i in range(2, L):
        Tl[i] = Tl[i - 1] // tp
    Tf = Tl[L - 1] // tp if L > 1 else frames

    def shape(key):
        return tuple(sd[key].shape)

    # ---- layer 0 (layer0_plan): the one-launch MFMA form multiplies its 12 x 7 stack f16 x 3; every other form is exact f32 ----
    if L > 1 and not res and not p2pc_conv and not stay and 2 <= NF <= 4 and 1 <= conv_layers <= 4 and kernel_size == 7 and P % 36 == 0:
        T0 = Tl[0]
        ok = shape("model.0.pool_semi.weight")[:2] == (1, 1)
        for j in range(conv_layers):
            ok = ok and shape(f"model.0.pc2pc.layer.{3*j}.conv2d.weight") == (NF, 1 if j == 0 else NF, 12, 7)
        RP, RPp = 4 * ((T0 + 3) // 4) + 8, (T0 + 9) // 2 * 2
        lds_v = (9 * 12 * RP + P * T0) * 4
        lds_m = (4 * 12 * RP + 2 * 12 * RPp * 4 + P * T0) * 4
        if ok and lds_v <= 150 * 1024 and (P * T0) % 4 == 0 and lds_m <= 150 * 1024:
            for j in range(conv_layers):
                route[f"model.0.pc2pc.layer.{3*j}.conv2d.weight"] = "f16x3"

    # ---- pitch stacks of the layers >= 1 (p2p_uses_f16, p2p_fuses_semi) ----
    Pi = P // 3 if stay else P
    for i in range(1, L):
        if res:
            break
        keys = [f"model.{i}.p2p.layer.{3*j}.weight" for j in range(conv_layers)]
        f16 = conv_layers >= 2 and Tl[i] <= 146 and all(k in sd and shape(k)[0] == 8 and shape(k)[1] <= 8 and shape(k)[2:] == (7, 7) for k in keys)
        if not f16:
            continue
        for j, k in enumerate(keys):
            route[k] = "f16+split0" if shape(k)[1] <= 5 else "f16"       # kP2pSplit0 (only a stack's first conv is that narrow)
        semi = f"model.{i}.pool_semi.weight"
        if (not keep_taps and not p2pc_conv and not stay and i == L - 1 and semi in sd and shape(semi) == (8, 8, 3, 3)
                and _p2p_ps_rows_semi(Pi, Tl[i]) > 0):
            route[semi] = "f16"

    # ---- the last layer's pitch-class stack (pc2pc_uses_bf16; the fused form is the same arithmetic) ----
    i = L - 1
    if not res and L > 1:
        keys = [f"model.{i}.pc2pc.layer.{3*j}.conv2d.weight" for j in range(conv_layers)]
        if Tl[i] <= 120 and all(shape(k)[0] == 16 and shape(k)[1] <= 16 and shape(k)[2:] == (12, 7) for k in keys):
            for k in keys:
                route[k] = "bf16x3"
    elif not res and L == 1:
        keys = [f"model.0.pc2pc.layer.{3*j}.conv2d.weight" for j in range(conv_layers)]
        if Tl[0] <= 120 and all(shape(k)[0] == 16 and shape(k)[1] <= 16 and shape(k)[2:] == (12, 7) for k in keys):
            for k in keys:
                route[k] = "bf16x3"

    # ---- heads (HeadForm) ----
    def eligible0(k):      # pc_bf16_eligible
        return k in sd and shape(k)[2] in (12, 1) and shape(k)[3] == 7 and shape(k)[1] <= 16 and shape(k)[0] in (16, 32)

    def eligible1(k):      # the 32 -> 1 last convolution of a two-conv head
        return k in sd and shape(k)[2] in (12, 2) and shape(k)[3] == 7 and shape(k)[0] == 1 and shape(k)[1] == 32

    k0, t0 = "key_classifier.0.conv2d.weight", "tonic_classifier.0.conv2d.weight"
    final_ch = shape(k0)[1]
    if not (L > 1 and final_ch == 16 and head_layers >= 2 and eligible0(k0) and eligible0(t0) and Tf <= 120):
        return route
    route[k0] = route[t0] = "bf16x3"                                  # Bf16First
    k1, t1 = "key_classifier.3.conv2d.weight", "tonic_classifier.3.conv2d.weight"
    T2 = Tf - 2 * (kernel_size - 1)
    if not (head_layers == 2 and eligible1(k1) and eligible1(t1) and T2 > 0 and (12 * ((T2 + 15) // 16) + 15) // 16 <= 4):
        return route
    route[k1] = route[t1] = "bf16x3"                                  # Head1 / Fused
    g0, g1 = "genre_classifier.0.weight", "genre_classifier.3.weight"
    if eligible0(g0) and eligible1(g1) and shape(g0)[2] == 1 and shape(g1)[2] == 2:
        route[g0] = route[g1] = "bf16x3"
    return route


def f32x3_route(sd, frames, **kw):
    """The same for the ``f32x3`` precision: the last pitch-class stack and the heads keep their three-term bf16
    split, the pitch convs run on three f16 products (f32-equivalent to 2^-22; named here wherever ``mixed`` runs them on f16, which is
    a superset of where ``conv_p2p_f16x3_kernel`` takes them -- the others are exact f32), layer 0 and the semitone convs are exact f32."""
    return {k: ("bf16x3" if v == "bf16x3" else "f16x3") for k, v in mixed_route(sd, frames, **kw).items() if v == "bf16x3" or ".p2p.layer." in k}


def equiv_pc_conv(x, weight, bias, same: bool, site=None):
    """EquivariantPitchClassConvolutionSimple.forward, models.py:36-47.

    Wrap the first 11 pitch-class rows below the 12 (``x_wrap``, :45) and run a
    plain Conv2d with a (12, kd) kernel; zero 'same' padding in time only (:28).
    """
    pcs = weight.shape[2]
    assert x.shape[2] == pcs                                   # models.py:44
    x_wrap = torch.cat([x, x[:, :, 0:pcs - 1, :]], dim=2)      # models.py:45
    kd = weight.shape[3]
    return _conv(site, x_wrap, weight, bias, lambda x_, w_, b_: F.conv2d(x_, w_, b_, padding=(0, kd // 2 if same else 0)))


def pitch2pitchclass_pool(x, pitch_classes: int = 12, site=None):
    """Pitch2PitchClassPool.forward, models.py:95-106 (ctor :84-92).

    Dilated max-pool over octaves; -inf rows are appended only when the row
    count is not a multiple of 12.
    """
    rows = x.shape[2]
    ks = math.ceil(rows / pitch_classes)
    pad = ks * pitch_classes - rows
    if pad:
        filler = torch.full((x.shape[0], x.shape[1], pad, x.shape[3]), float("-inf"), dtype=x.dtype)
        x = torch.cat([x, filler], dim=2)
    if _DECISIONS is not None:      # row = octave * 12 + pitch class: the window of pitch class p is x[:, :, p::12]
        if site is None:
            _no_forcing("an octave pool without a site name")
        o = x.reshape(x.shape[0], x.shape[1], ks, pitch_classes, x.shape[3])
        idx = _DECISIONS.decide(site, o.detach().argmax(dim=2), o.detach())
        return o.gather(2, idx.unsqueeze(2)).squeeze(2)
    return F.max_pool2d(x, (ks, 1), (1, 1), dilation=(pitch_classes, 1))


def pitch2pitchclass_conv(x, sd, prefix, training=False):
    """Pitch2PitchClassConv.forward, models.py:108-133 (--p2pc_conv): the octave fold as a learned convolution -- kernel
    (ceil(pitches_in / 12), 1) with dilation (12, 1) over the channels, then BatchNorm + LeakyReLU -- instead of the max."""
    _no_forcing("--p2pc_conv")
    w = sd[prefix + "conv.weight"]
    pad = w.shape[2] * 12 - x.shape[2]                       # rows of padding_value appended (:130-131); 0 for whole octaves
    if pad:
        x = torch.cat([x, torch.full((x.shape[0], x.shape[1], pad, x.shape[3]), float("-inf"), dtype=x.dtype)], dim=2)
    y = F.conv2d(x, w, sd[prefix + "conv.bias"], dilation=(12, 1))
    return _act_bn(y, sd, prefix + "bn.", training)


def pitchclass2pitch(x, target_rows: int):
    """PitchClass2Pitch.forward, models.py:140-143: tile rows, crop."""
    reps = math.ceil(target_rows / x.shape[2])
    return x.repeat(1, 1, reps, 1)[:, :, 0:target_rows, :]


def _circular_conv(x, weight, bias, stride, pad_hw, site=None):
    """nn.Conv2d(..., padding=pad_hw, padding_mode='circular') (models.py:230,313)."""
    ph, pw = pad_hw
    x = F.pad(x, (pw, pw, ph, ph), mode="circular")
    return _conv(site, x, weight, bias, lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=stride))


def _count(sd, prefix, suffix):
    """Number of conv blocks in an nn.Sequential(conv, bn, act, conv, bn, act, ...)."""
    n = 0
    while f"{prefix}{3 * n}{suffix}" in sd:
        n += 1
    return n


def _res_blocks(x, sd, prefix, conv, training, taps):
    """--resblock (models.py:181-187 / :218-224): after the first conv + BN + LeakyReLU the Sequential holds ``conv_layers`` blocks
    at indices 3, 4, ...; a block is x -> act2(x + b2(conv2(act1(b1(conv1(x)))))) (ResBlock / ResBlockEquivariant, models.py:402-454).
    ``conv(x, block_prefix + "conv1")`` applies the stack's convolution type."""
    _no_forcing("--resblock")
    idx = 3
    while f"{prefix}layer.{idx}.b1.weight" in sd:
        bp = f"{prefix}layer.{idx}."
        h = _act_bn(conv(x, bp + "conv1"), sd, bp + "b1.", training)
        x = _lrelu(x + _bn(conv(h, bp + "conv2"), sd, bp + "b2.", training))
        if taps is not None:
            taps[f"{prefix}layer.{idx}"] = x
        idx += 1
    return x


def _dense_block(x, sd, prefix, conv, training, taps):
    """--denseblock (DenseBlock / DenseBlockEquivariant, models.py:584-648; layers _DenseLayer / _DenseLayerEquivariant, :456-582):
    every layer reads the concatenation of the block input and all earlier layers' outputs,
        new = conv2(relu(norm2(conv1(leaky_relu(norm1(cat))))))          (:473-476, 516-517 / :536-539, 579-580)
    (pre-activation BatchNorm; relu1 is a LeakyReLU, relu2 a plain ReLU; conv1 is the 1-wide bottleneck), and the block returns the
    concatenation of everything (:614 / :647).  drop_rate is 0.0 at both call sites (:189, 226).  ``conv(x, key_prefix, same)``
    applies the stack's convolution type."""
    _no_forcing("--denseblock")
    feats = [x]
    j = 1
    while f"{prefix}denselayer{j}.norm1.weight" in sd:
        lp = f"{prefix}denselayer{j}."
        cat = torch.cat(feats, dim=1)
        h = conv(_act_bn(cat, sd, lp + "norm1.", training), lp + "conv1")
        new = conv(F.relu(_bn(h, sd, lp + "norm2.", training)), lp + "conv2")
        feats.append(new)
        if taps is not None:
            taps[f"{prefix}denselayer{j}"] = new
        j += 1
    return torch.cat(feats, dim=1)


def pc2pc_stack(pc, sd, prefix, training=False, taps=None):
    """PitchClass2PitchClass default branch, models.py:190-197, 201-203; --resblock branch :181-187; --denseblock branch :188-189."""
    if f"{prefix}layer.0.denselayer1.norm1.weight" in sd:
        # conv1: EquivariantPitchClassConvolutionSimple with kernel_depth 1 (12 x 1, no time padding needed), conv2: 12 x k, same padding
        return _dense_block(pc, sd, prefix + "layer.0.", lambda x, q: equiv_pc_conv(x, sd[q + ".conv2d.weight"], sd[q + ".conv2d.bias"], same=True),
                            training, taps)
    if f"{prefix}layer.3.b1.weight" in sd:
        pc = equiv_pc_conv(pc, sd[prefix + "layer.0.conv2d.weight"], sd[prefix + "layer.0.conv2d.bias"], same=True)
        pc = _act_bn(pc, sd, prefix + "layer.1.", training)
        return _res_blocks(pc, sd, prefix, lambda x, q: equiv_pc_conv(x, sd[q + ".conv2d.weight"], sd[q + ".conv2d.bias"], same=True),
                           training, taps)
    n = _count(sd, prefix + "layer.", ".conv2d.weight")
    for i in range(n):
        pc = equiv_pc_conv(pc, sd[f"{prefix}layer.{3*i}.conv2d.weight"], sd[f"{prefix}layer.{3*i}.conv2d.bias"], same=True,
                           site=f"{prefix}layer.{3*i}.conv2d.weight")
        pc = _act_bn(pc, sd, f"{prefix}layer.{3*i+1}.", training)
        if taps is not None:
            taps[f"{prefix}layer.{3*i+2}"] = pc
    return pc


def p2p_stack(p, sd, prefix, training=False, taps=None):
    """Pitch2Pitch default branch, models.py:227-234, 239-243: circular on both axes; --resblock branch :218-224; --denseblock
    branch :225-226 (plain nn.Conv2d without bias: 1 x 1, then k x k with ZERO padding k // 2 on both axes, :464, 468)."""
    if f"{prefix}layer.0.denselayer1.norm1.weight" in sd:
        return _dense_block(p, sd, prefix + "layer.0.", lambda x, q: F.conv2d(x, sd[q + ".weight"], None, padding=sd[q + ".weight"].shape[2] // 2),
                            training, taps)
    if f"{prefix}layer.3.b1.weight" in sd:
        circ = lambda x, q: _circular_conv(x, sd[q + ".weight"], sd[q + ".bias"], (1, 1), (sd[q + ".weight"].shape[2] // 2,) * 2)
        p = _act_bn(circ(p, prefix + "layer.0"), sd, prefix + "layer.1.", training)
        return _res_blocks(p, sd, prefix, circ, training, taps)
    n = _count(sd, prefix + "layer.", ".weight")
    for i in range(n):
        w = sd[f"{prefix}layer.{3*i}.weight"]
        k = w.shape[2]
        p = _circular_conv(p, w, sd[f"{prefix}layer.{3*i}.bias"], (1, 1), (k // 2, k // 2), site=f"{prefix}layer.{3*i}.weight")
        p = _act_bn(p, sd, f"{prefix}layer.{3*i+1}.", training)
        if taps is not None:
            taps[f"{prefix}layer.{3*i+2}"] = p
    return p


def semitone_pool(p, sd, prefix, training=False):
    """pool_semi + BN + LeakyReLU, models.py:313-315 / :337-339, used :361-363, :386-388.

    3x3 conv, stride (3,1), circular padding (0,1): three third-semitone bins ->
    one semitone, time wraps.
    """
    x = _circular_conv(p, sd[prefix + "pool_semi.weight"], sd[prefix + "pool_semi.bias"], (3, 1), (0, 1), site=prefix + "pool_semi.weight")
    return _act_bn(x, sd, prefix + "pool_semi_b.", training)


def pitchclass2pitch_memory(p, p_sixth):
    """PitchClass2Pitch_MemoryVariant.forward, models.py:145-166 (--pc2p_mem): instead of concatenating the repeated third-semitone
    map, ADD it to the pitch stream -- after summing groups of its channels down to the stream's channel count.  The reference
    reshapes the P pitch rows to (36, P / 36), so row r receives third-semitone index r // (P / 36) (eight CONSECUTIVE rows share
    one), not r % 36 as the repeat of the default path does; kept as it is."""
    _no_forcing("--pc2p_mem")
    B, C, P, T = p.shape
    s = p_sixth.reshape(B, C, p_sixth.shape[1] // C, p_sixth.shape[2], T).sum(dim=2)          # (B, C, 36, T)
    k = s.shape[2]
    return (p.reshape(B, C, k, P // k, T) + s.reshape(B, C, k, 1, T)).reshape(B, C, P, T)


def forward_features(sd, mel, time_pool_size=2, training=False, taps=None):
    """nn.Sequential of PitchClassNetLayer.forward, models.py:352-399 (default flags; --pc2p_mem when the first pitch conv of a
    layer takes only the pitch stream's channels)."""
    num_layers = 0
    while (f"model.{num_layers}.pc2pc.layer.0.conv2d.weight" in sd       # (pool_semi is absent from --stay_sixth layers >= 1)
           or f"model.{num_layers}.pc2pc.layer.0.denselayer1.norm1.weight" in sd):
        num_layers += 1
    p, pc = mel, None
    pitches = mel.shape[2]
    # --stay_sixth (models.py:322-323, 336, 366-367, 371, 385): the pitch stream continues at semitone resolution -- layer 0's semitone
    # map replaces the CQT as the stream, later layers have neither up_sixth nor pool_semi and repeat the 12 pitch-class rows directly
    stay = num_layers > 1 and "model.1.up_sixth.weight" not in sd
    for i in range(num_layers):
        pre = f"model.{i}."
        if i == 0:
            p_semi = semitone_pool(p, sd, pre, training)            # :361-363
            if stay:
                p = p_semi                                          # :366-367
            pc = (pitch2pitchclass_conv(p_semi, sd, pre + "pool.", training) if pre + "pool.conv.weight" in sd
                  else pitch2pitchclass_pool(p_semi, site=pre + "pool"))   # :368 (p stays raw, :366-367)
            if taps is not None:
                taps[pre + "pool"] = pc
            pc = pc2pc_stack(pc, sd, pre + "pc2pc.", training, taps)  # :369
        elif stay:
            _no_forcing("--stay_sixth")
            p = torch.cat([p, pitchclass2pitch(pc, p.shape[2])], dim=1)   # :379-383 with up = PitchClass2Pitch(pitches // 3)
            p = p2p_stack(p, sd, pre + "p2p.", training, taps)      # :384
            pc2 = (pitch2pitchclass_conv(p, sd, pre + "pool.", training) if pre + "pool.conv.weight" in sd
                   else pitch2pitchclass_pool(p))                   # :391
            if taps is not None:
                taps[pre + "pool"] = pc2
            pc = torch.cat([pc, pc2], dim=1)                        # :392
            pc = pc2pc_stack(pc, sd, pre + "pc2pc.", training, taps)  # :393
            p = F.max_pool2d(p, (1, time_pool_size))                # :395
            pc = F.max_pool2d(pc, (1, time_pool_size))              # :396
            if taps is not None:
                taps[pre + "time_pool_pc"] = pc
        else:
            p_sixth = F.conv_transpose2d(pc, sd[pre + "up_sixth.weight"], sd[pre + "up_sixth.bias"], stride=(3, 1))  # :372
            p_sixth = _act_bn(p_sixth, sd, pre + "up_sixth_b.", training)         # :373-374
            if taps is not None:
                taps[pre + "up_sixth_a"] = p_sixth
            if pre + "p2p.layer.0.weight" in sd and sd[pre + "p2p.layer.0.weight"].shape[1] == p.shape[1]:       # --pc2p_mem: :376-377, no concat (:382)
                p = pitchclass2pitch_memory(p, p_sixth)
            else:
                p2 = pitchclass2pitch(p_sixth, pitches)             # :378
                p = torch.cat([p, p2], dim=1)                       # :383
            p = p2p_stack(p, sd, pre + "p2p.", training, taps)      # :384
            pc2 = semitone_pool(p, sd, pre, training)               # :386-388
            pc2 = (pitch2pitchclass_conv(pc2, sd, pre + "pool.", training) if pre + "pool.conv.weight" in sd
                   else pitch2pitchclass_pool(pc2, site=pre + "pool"))   # :389
            if taps is not None:
                taps[pre + "pool"] = pc2
            pc = torch.cat([pc, pc2], dim=1)                        # :392
            pc = pc2pc_stack(pc, sd, pre + "pc2pc.", training, taps)  # :393
            p = _time_pool(p, time_pool_size, pre + "time_pool_p")      # :395
            pc = _time_pool(pc, time_pool_size, pre + "time_pool_pc")   # :396
            if taps is not None:
                taps[pre + "time_pool_pc"] = pc
    return p, pc, num_layers


def _equiv_head(pc, sd, name, training=False):
    """tonic/key classifier Sequential, models.py:716-731, applied :750-751."""
    n_hidden = _count(sd, name + ".", ".conv2d.weight")
    # hidden blocks sit at indices 0,3,6..; the last conv (no BN) closes the Sequential
    idx = 0
    x = pc
    while f"{name}.{idx}.conv2d.weight" in sd:
        x = equiv_pc_conv(x, sd[f"{name}.{idx}.conv2d.weight"], sd[f"{name}.{idx}.conv2d.bias"], same=False, site=f"{name}.{idx}.conv2d.weight")
        if f"{name}.{idx+1}.weight" in sd:       # BN follows -> hidden block
            x = _act_bn(x, sd, f"{name}.{idx+1}.", training)
            idx += 3
        else:
            break
    return x


def _genre_head(pc, sd, training=False):
    """genre classifier: plain Conv2d (1,k) [+BN+LReLU] ..., Conv2d (2,k); models.py:724,733."""
    idx = 0
    x = pc
    while f"genre_classifier.{idx}.weight" in sd and sd[f"genre_classifier.{idx}.weight"].dim() == 4:
        x = _conv(f"genre_classifier.{idx}.weight", x, sd[f"genre_classifier.{idx}.weight"], sd[f"genre_classifier.{idx}.bias"], F.conv2d)
        if f"genre_classifier.{idx+1}.running_mean" in sd:
            x = _act_bn(x, sd, f"genre_classifier.{idx+1}.", training)
            idx += 3
        else:
            break
    return x


def pcnet_forward(sd: Dict[str, torch.Tensor], mel: torch.Tensor, seq_length: Optional[torch.Tensor],
                  kernel_size: int = 7, head_layers: int = 2, time_pool_size: int = 2,
                  genre: Optional[bool] = None, max_pool: bool = False, training: bool = False,
                  taps: Optional[dict] = None, local_window: Optional[int] = None) -> Tuple[torch.Tensor, ...]:
    """PitchClassNet.forward, models.py:747-817.

    Returns ``(key_out, tonic_out[, genre_out])`` exactly as the reference:
    sigmoid on key only (:802), 2-tuple when there is no genre head (:815).

    ``local_window`` = ``opt.frames * opt.loc_window_size - head_layers * (kernel_size - 1)`` selects ``--local``
    (models.py:720-722, 805-810): the key / tonic heads end in ``MaxPool2d((1, W), stride=1)`` and the maps are returned per
    frame -- *reshaped*, not transposed, to ``(B, T', 12)`` (the reference's ``reshape``, kept as it is), genre ``(B, Tm, 11)``.
    """
    if genre is None:
        genre = "genre_classifier.0.weight" in sd
    if max_pool:
        _no_forcing("max_pool")
    if local_window is not None:
        _no_forcing("--local")
        time_pool_size = 1                                                           # :348, :394 -- no time pooling with --local
    p, pc, num_layers = forward_features(sd, mel, time_pool_size, training, taps)   # :749
    tonic = _equiv_head(pc, sd, "tonic_classifier", training)                        # :750
    key = _equiv_head(pc, sd, "key_classifier", training)                            # :751
    gen = _genre_head(pc, sd, training) if genre else None                           # :753
    if taps is not None:
        taps["tonic_map"], taps["key_map"] = tonic, key
        if genre:
            taps["genre_map"] = gen
    if local_window is not None:                                                     # :720-722, :805-810
        tonic = F.max_pool2d(tonic, kernel_size=(1, local_window), stride=1)
        key = F.max_pool2d(key, kernel_size=(1, local_window), stride=1)
        tonic_out = tonic.reshape(tonic.shape[0], tonic.shape[3], tonic.shape[2])
        key_out = torch.sigmoid(key.reshape(key.shape[0], key.shape[3], key.shape[2]))
        if genre:
            return key_out, tonic_out, gen.reshape(gen.shape[0], gen.shape[3], gen.shape[2])
        return key_out, tonic_out

    def pool_all(x):
        return x.max(dim=-1).values if max_pool else x.mean(dim=-1)

    if seq_length is not None:
        # :757-760 -- floor per layer, then subtract the heads' valid-conv shrink
        actual = seq_length.reshape(-1).to(torch.float64)
        for _ in range(num_layers - 1):
            actual = torch.floor(actual / time_pool_size)
        actual = actual.to(torch.int32) - (kernel_size - 1) * head_layers
        if actual.numel() == 1 and tonic.shape[0] > 1:
            actual = actual.expand(tonic.shape[0])

        def pool_masked(x):
            rows = []
            for j in range(x.shape[0]):
                seg = x[j, :, :, : int(actual[j])]
                # :764-785 -- quirk kept: with max_pool only sample 0 takes the max
                if max_pool and j == 0:
                    rows.append(seg.max(dim=-1).values)
                else:
                    rows.append(seg.mean(dim=-1))
            return torch.stack(rows, 0)

        tonic_out, key_out = pool_masked(tonic), pool_masked(key)
        genre_out = pool_masked(gen) if genre else None
    else:                                                                            # :786-797
        tonic_out, key_out = pool_all(tonic), pool_all(key)
        genre_out = pool_all(gen) if genre else None

    tonic_out = tonic_out.flatten(1)                                                 # :800
    key_out = torch.sigmoid(key_out.flatten(1))                                      # :801-802
    if genre:
        return key_out, tonic_out, genre_out.flatten(1)                              # :813
    return key_out, tonic_out                                                        # :815


def to_dtype(sd, dtype):
    """Cast the float entries of a state_dict (``num_batches_tracked`` stays int64)."""
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
