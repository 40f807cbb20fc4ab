"""Tuning on the device: how far recordings sit from A4 = 440 Hz, and the varispeed resampler that puts them back.

Not part of the reference: it pins librosa 0.9.2, whose ``cqt`` runs at ``tuning=0.0``, and its net collapses each semitone's three bins
as they come, so a recording that is 35 cents sharp lands one full bin off.  Host wrappers of ``ake_tuning_estimate_f32``
(csrc/tuning.hip) and ``ake_retune_f32`` / ``ake_retune_pcm16_f32`` (csrc/audio.hip); the float64 models are
``metrics.estimate_tuning`` and ``metrics.retune_reference``.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib, metrics


def _need_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise _lib.AkeError(f"{what} needs its input on a HIP device; there is no CPU fallback (the float64 model is in ake_amd.metrics)")


def estimate_tuning(logmag: torch.Tensor, counts: torch.Tensor | None = None, min_strength: float = 0.0, frames_major: bool = False,
                    workspace: torch.Tensor | None = None):
    """The detuning of B recordings from their log-CQT on the device -> ``(cents, strength)``, float32 (B,).

    ``logmag`` (B, n_bins, T) float32 as ``CQTPlan.logmag`` returns it, or (B, T, n_bins) with ``frames_major=True``; ``n_bins`` must be
    a multiple of 3 (3 bins per semitone, in-tune notes on bins ``k = 0 (mod 3)``), else ``ValueError``.  ``counts`` (B,): frames of every
    recording; not needed behind a ragged transform, whose zeros behind a recording's end add nothing.  ``cents`` in (-50, 50], positive
    = sharp; ``strength`` in [0, 1]; rows with ``strength < min_strength`` report 0 cents (decided on the device); a silent row gives
    (0, 0).  Definition: ``metrics.estimate_tuning``.  Two launches on the current stream, no host synchronisation.  ``workspace``: a
    uint8 device tensor to use instead of a fresh one (``ake_tuning_workspace_bytes``)."""
    _need_device(logmag, "estimate_tuning")
    if logmag.dim() != 3:
        raise ValueError(f"estimate_tuning: logmag must be (B, n_bins, T), got {tuple(logmag.shape)}")
    mel = logmag.to(torch.float32).contiguous()
    B, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    if P % metrics.TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"estimate_tuning: {P} bins are no multiple of 3 (3 bins per semitone)")
    dev = mel.device
    cents = torch.empty((B,), dtype=torch.float32, device=dev)
    strength = torch.empty((B,), dtype=torch.float32, device=dev)
    if B == 0:
        return cents, strength
    if T == 0:
        return cents.zero_(), strength.zero_()
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
        assert counts.shape == (B,)
    L = _lib.lib()
    nbytes = int(L.ake_tuning_workspace_bytes(B, T))
    if nbytes == 0:
        _lib.check(-1, "ake_tuning_workspace_bytes")
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.ake_tuning_estimate_f32(mel.data_ptr(), 1 if frames_major else 0, B, P, T, counts.data_ptr() if counts is not None else None,
                                             float(min_strength), cents.data_ptr(), strength.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream), "ake_tuning_estimate_f32")
    return cents, strength


def retune_out_len(n: int) -> int:
    """Width of the buffer ``retune`` returns for rows of ``n`` samples: ``floor(n * 2 ** (50 / 1200)) + 1`` (``ake_retune_out_len``)."""
    return int(_lib.lib().ake_retune_out_len(int(n)))


def retune(audio: torch.Tensor, cents, lengths: torch.Tensor | None = None):
    """Undo a detuning of ``cents`` by varispeed resampling on the device -> ``(audio (B, retune_out_len(n)) float32, lengths (B,) int64)``.

    ``audio`` (B, n) float32, or int16 = 16-bit PCM (``pcm16_to_float``), read in place with the float route's results bit for bit.
    ``cents``: one number or a (B,) tensor (float32 on the device: ``estimate_tuning``'s output goes straight in; nothing is read back).
    Row i is resampled by ``rho_i = 2 ** (cents_i / 1200)`` to ``floor(lengths[i] * rho_i)`` samples -- a sharp recording comes out longer
    and lower -- with a 64-tap Kaiser-windowed sinc (``metrics.retune_reference``); zeros follow a row's end.  A row with 0 cents is
    copied bit for bit.  Content above 0.94 of the Nyquist frequency is discarded.  One launch on the current stream."""
    _need_device(audio, "retune")
    if audio.dim() != 2:
        raise ValueError(f"retune: audio must be (B, n), got {tuple(audio.shape)}")
    pcm = audio.dtype == torch.int16
    if not pcm:
        audio = audio.to(torch.float32)
    if audio.stride(1) != 1 or (audio.shape[0] > 1 and audio.stride(0) < audio.shape[1]):
        audio = audio.contiguous()
    dev = audio.device
    B, n = audio.shape
    L = _lib.lib()
    width = retune_out_len(n)
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    len_out = torch.empty((B,), dtype=torch.int64, device=dev)
    if B == 0 or n == 0:
        return out.zero_(), len_out.zero_()
    if isinstance(cents, torch.Tensor):
        cents = cents.to(device=dev, dtype=torch.float32).reshape(-1)
        cents = (cents.expand(B) if cents.numel() == 1 else cents).contiguous()
    else:
        cents = torch.full((B,), float(cents), dtype=torch.float32, device=dev)
    if cents.shape != (B,):
        raise ValueError(f"retune: {B} rows but {cents.numel()} tunings")
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
        assert lengths.shape == (B,)
    fn, name = (L.ake_retune_pcm16_f32, "ake_retune_pcm16_f32") if pcm else (L.ake_retune_f32, "ake_retune_f32")
    with torch.cuda.device(dev):
        _lib.check(fn(audio.data_ptr(), B, n, audio.stride(0) if B > 1 else max(n, 1), lengths.data_ptr() if lengths is not None else None,
                      cents.data_ptr(), out.data_ptr(), out.stride(0), len_out.data_ptr(), torch.cuda.current_stream().cuda_stream), name)
    return out, len_out
