"""The sequence loss as an autograd function (``ake_amd.key_sequence_loss``): on the device one call of ``ake_key_sequence_loss_f32``, which
leaves the loss and its gradients with respect to the two heads' outputs and the transition; off it the same formulas in torch ops
(``metrics.key_sequence_loss``).  Either way the backward is the closed form, not autograd's: where ``nn.BCELoss``'s clamp is active the
chain rule through ``log`` gives 0 * inf.
"""
from __future__ import annotations

import torch

from . import _lib, metrics


def _aligned(t):
    """float32, contiguous and 16-byte aligned (the kernels move rows as 16-byte pieces)."""
    t = t.detach().float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _KeySequenceLoss(torch.autograd.Function):
    """forward -> the scalar loss; the gradients are computed with it and kept, and backward multiplies them by the incoming scalar, as
    ``_FusedGeneralStep`` does."""

    @staticmethod
    def forward(ctx, key, tonic, log_trans, labels, counts, signature_weight, log_prior):
        if key.dim() != 3 or key.shape[2] != 12 or tonic.shape != key.shape:
            raise ValueError(f"key_sequence_loss: key and tonic must be (R, W, 12), got {tuple(key.shape)} and {tuple(tonic.shape)}")
        R, W, _ = key.shape
        if tuple(labels.shape) != (R, W):
            raise ValueError(f"key_sequence_loss: labels must be ({R}, {W}), got {tuple(labels.shape)}")
        if tuple(log_trans.shape) != (24, 24):
            raise ValueError("key_sequence_loss: log_trans must be a (24, 24) tensor of log-probabilities, from key i (row) to key j")
        need_trans = ctx.needs_input_grad[2]
        ctx.out_dtype, ctx.trans_dtype, ctx.trans_device = key.dtype, log_trans.dtype, log_trans.device
        if not (key.is_cuda and key.dtype in (torch.float32, torch.float64)):
            out = metrics.key_sequence_loss(key.detach(), tonic.detach(), labels, log_trans, counts, signature_weight, log_prior)
            ctx.d_key, ctx.d_tonic, ctx.d_trans = out["d_key"], out["d_tonic"], out["d_trans"] if need_trans else None
            return out["loss"]
        if R < 1 or W < 1:
            raise ValueError(f"key_sequence_loss: no windows ({R} recordings of {W})")
        dev = key.device
        k32, t32 = _aligned(key), _aligned(tonic)
        lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        cnt = None if counts is None else torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
        if cnt is not None and cnt.shape != (R,):
            raise ValueError(f"key_sequence_loss: counts must be ({R},), got {tuple(cnt.shape)}")
        A = log_trans.detach().to(device=dev, dtype=torch.float32).contiguous()
        prior = None if log_prior is None else torch.as_tensor(log_prior).detach().to(device=dev, dtype=torch.float32).reshape(24).contiguous()
        L = _lib.lib()
        nbytes = L.ake_key_sequence_loss_workspace_bytes(R, W)
        if nbytes == 0:
            _lib.check(-1, "ake_key_sequence_loss_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        scal = torch.empty(4, dtype=torch.float32, device=dev)
        grads = torch.empty((2, R, W, 12), dtype=torch.float32, device=dev)
        d_trans = torch.empty((24, 24), dtype=torch.float32, device=dev) if need_trans else None
        ptr = lambda t: t.data_ptr() if t is not None else None                          # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(L.ake_key_sequence_loss_f32(k32.data_ptr(), t32.data_ptr(), lab.data_ptr(), R, W, ptr(cnt), A.data_ptr(), ptr(prior),
                                                   float(signature_weight), scal.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(),
                                                   ptr(d_trans), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                       "ake_key_sequence_loss_f32")
        ctx.d_key, ctx.d_tonic, ctx.d_trans = grads[0], grads[1], d_trans
        return scal[0].to(key.dtype)

    @staticmethod
    def backward(ctx, g):
        d_key = (ctx.d_key * g).to(ctx.out_dtype) if ctx.needs_input_grad[0] else None
        d_tonic = (ctx.d_tonic * g).to(ctx.out_dtype) if ctx.needs_input_grad[1] else None
        d_trans = (ctx.d_trans * g).to(device=ctx.trans_device, dtype=ctx.trans_dtype) if ctx.d_trans is not None else None
        return d_key, d_tonic, d_trans, None, None, None, None


def key_sequence_loss(key, tonic, labels, log_trans, counts=None, signature_weight=1.0, log_prior=None):
    """The sequence loss of (R, W, 12) ``key`` (sigmoid memberships) and ``tonic`` (logits) -> a scalar that carries gradients for
    ``key``, ``tonic`` and -- where it requires grad -- ``log_trans``.

    The conditional log-likelihood of the labelled windows in a linear-chain CRF whose unary scores are the tracker's own emissions
    (``metrics.key_emissions`` with ``signature_weight``) and whose chain is the smoother's (``log_trans`` (24, 24), ``log_prior``,
    ``counts``, as ``metrics.key_posteriors`` takes them); ``labels`` (R, W) integers, a key 0..23 or anything else for an unlabelled
    window, which is marginalised.  Formulas: ``metrics.key_sequence_loss``.  On CUDA float32 / float64 tensors this is one call of
    ``ake_key_sequence_loss_f32`` on the current stream (4 launches, 6 with a transition that requires grad; nothing waits for the
    device); elsewhere the model in torch ops.  ``log_prior`` gets no gradient."""
    labels = torch.as_tensor(labels)
    log_trans = torch.as_tensor(log_trans)
    return _KeySequenceLoss.apply(key, tonic, log_trans, labels, counts, float(signature_weight), log_prior)
