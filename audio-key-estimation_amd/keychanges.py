"""Key changes to the frame on the device: where, between two windows of a key track that carry different keys, the key changes.

Not part of the reference, which names one key per clip.  Host wrapper of ``ake_key_changes_f32`` (csrc/changes.hip); the float64
model and the definition is ``metrics.key_changes``.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib, metrics
from .keyprofile import device_profiles


def check_span(stride_frames: int, slack_frames: int):
    """``ValueError`` for a span the kernel does not hold (``stride_frames + 2 * slack_frames > metrics.KEY_CHANGES_MAX_SPAN``)."""
    if stride_frames + 2 * slack_frames > metrics.KEY_CHANGES_MAX_SPAN:
        raise ValueError(f"key_changes: a span of stride_frames {stride_frames} + 2 * slack_frames {slack_frames} frames exceeds "
                         f"{metrics.KEY_CHANGES_MAX_SPAN}, the longest the kernel holds")


def key_changes(logmag: torch.Tensor, labels: torch.Tensor, window_frames: int, stride_frames: int, counts: torch.Tensor | None = None,
                window_counts: torch.Tensor | None = None, slack_frames: int | None = None, profiles="krumhansl", compression: str = "log",
                frames_major: bool = False):
    """Where the key changes between two windows of a key track, to the frame, on the device -> ``(change_frame int32 (R, W-1),
    gain (R, W-1), contrast (R, W-1))``, the last two float32.  Definition: ``metrics.key_changes``, whose arguments these are (it
    returns a fourth tensor for tests, which the kernel does not compute).

    ``logmag`` (R, n_bins, T) float32 as ``CQTPlan.logmag`` returns it, or (R, T, n_bins) with ``frames_major=True``; ``n_bins`` must be a
    multiple of 3.  ``labels`` integer (R, W): a key 0..23 per window (``KeyTrack.key_id`` or ``smooth_key_id``), anything else is no
    key.  ``counts`` (R,): frames of every recording (default T); ``window_counts`` (R,): its windows (default: what its frames hold).
    ``slack_frames`` (default ``stride_frames``): how far beyond the two windows' centres the change is looked for;
    ``stride_frames + 2 * slack_frames`` may not exceed 1024 (``ValueError``).  Where two neighbouring windows carry the same key, or
    one carries none, ``change_frame`` is -1 and the other two 0.  One launch on the current stream, no workspace, no host
    synchronisation."""
    if not logmag.is_cuda:
        raise _lib.AkeError("key_changes needs its input on a HIP device; there is no CPU fallback (the float64 model is in ake_amd.metrics)")
    if logmag.dim() != 3:
        raise ValueError(f"key_changes: logmag must be (R, n_bins, T), got {tuple(logmag.shape)}")
    mel = logmag.to(torch.float32).contiguous()
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    if P % metrics.TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"key_changes: {P} bins are no multiple of 3 (3 bins per semitone)")
    mode = metrics._profile_compression(compression)
    wf, sf = int(window_frames), int(stride_frames)
    if wf < 1 or sf < 1:
        raise ValueError("key_changes: window_frames and stride_frames must be >= 1")
    slack = sf if slack_frames is None else int(slack_frames)
    if slack < 0:
        raise ValueError("key_changes: slack_frames must be >= 0")
    check_span(sf, slack)
    dev = mel.device
    labels = torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()
    if labels.dim() != 2 or labels.shape[0] != R:
        raise ValueError(f"key_changes: labels must be (R, W) with R = {R}, got {tuple(labels.shape)}")
    as_counts = lambda t: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.int32).reshape(R).contiguous()
    return _launch(mel, frames_major, as_counts(counts), labels, as_counts(window_counts), wf, sf, slack, device_profiles(profiles, dev), mode)


def _launch(mel, frames_major, counts, labels, window_counts, wf, sf, slack, prof, mode):
    """``ake_key_changes_f32`` on checked arguments: ``mel`` float32 contiguous on the device, ``labels`` int32 (R, W) contiguous and
    ``counts`` / ``window_counts`` int32 (R,) there or None, ``prof`` float32 (2, 12) there, ``mode`` 0..2."""
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    W = labels.shape[1]
    dev = mel.device
    B = max(W - 1, 0)
    frame = torch.empty((R, B), dtype=torch.int32, device=dev)
    gain, contrast = torch.empty((R, B), dtype=torch.float32, device=dev), torch.empty((R, B), dtype=torch.float32, device=dev)
    if R == 0 or B == 0:
        return frame, gain, contrast
    if T == 0:                                                       # no frames: no recording holds a window
        return frame.fill_(-1), gain.zero_(), contrast.zero_()
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ake_key_changes_f32(mel.data_ptr(), 1 if frames_major else 0, R, P, T, ptr(counts), labels.data_ptr(), W,
                                                  ptr(window_counts), wf, sf, slack, prof.data_ptr(), mode, frame.data_ptr(),
                                                  gain.data_ptr(), contrast.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "ake_key_changes_f32")
    return frame, gain, contrast
