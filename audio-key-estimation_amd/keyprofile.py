"""Key-profile emissions on the device: a key track without a trained net (Krumhansl-Schmuckler).

Not part of the reference, which has no method that runs without a checkpoint.  Host wrapper of ``ake_profile_emissions_f32``
(csrc/profile.hip); the float64 model is ``metrics.profile_emissions``.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib, metrics

_tables = {}


def device_profiles(profiles, device):
    """``profiles`` (a name of ``metrics.KEY_PROFILES`` or a (2, 12) tensor) checked -> float32 (2, 12) on ``device``, as the kernel reads
    it.  The built-in tables are uploaded once per device; a tensor is checked on the host (24 numbers) every call."""
    if isinstance(profiles, str):
        key = (profiles, str(device))
        if key not in _tables:
            _tables[key] = metrics.key_profile_table(profiles).to(device=device, dtype=torch.float32).contiguous()
        return _tables[key]
    return metrics.key_profile_table(profiles).to(device=device, dtype=torch.float32).contiguous()


def profile_windows(frames: int, window_frames: int, stride_frames: int) -> int:
    """W of ``profile_emissions`` on ``frames`` frames (``ake_profile_windows``): ``pipeline.track_counts``, or 1 in the whole-clip mode."""
    return int(_lib.lib().ake_profile_windows(int(frames), int(window_frames), int(stride_frames)))


def profile_emissions(logmag: torch.Tensor, window_frames: int, stride_frames: int, counts: torch.Tensor | None = None,
                      frames_major: bool = False, profiles="krumhansl", compression: str = "log", sharpness: float = 10.0,
                      workspace: torch.Tensor | None = None, cents=None):
    """Key emissions without a net, on the device -> ``(chroma (R, W, 12), emissions (R, W, 24), key_id int32 (R, W), confidence (R, W))``,
    float32: every window's chroma correlated with the 24 rotations of a minor and a major key profile.  Definition:
    ``metrics.profile_emissions``, whose arguments these are.

    ``logmag`` (R, n_bins, T) float32 as ``CQTPlan.logmag`` returns it, or (R, T, n_bins) with ``frames_major=True``; ``n_bins`` must be a
    multiple of 3, else ``ValueError``.  ``counts`` (R,): frames of every recording (default T).  ``window_frames = 0``: one window over
    every recording's own frames.  ``profiles``: a name of ``KEY_PROFILES`` or a (2, 12) tensor, rows minor and major, tonic first; the
    kernel reads it rounded to float32.  ``sharpness = 10.0`` and ``compression = "log"`` are starting values that nobody has measured
    against annotated music (``profiles/key_profiles.md`` scores them and their neighbours on synthesised recordings).  The emissions go
    into ``ake_viterbi_keys_f32`` and ``ake_key_posteriors_f32`` as the net's do.  Two launches on the current stream, no host
    synchronisation.  ``workspace``: a uint8 device tensor to use instead of a fresh one (``ake_profile_workspace_bytes``).

    ``cents`` (default None: the launches and bits above) selects the tuned chroma, ``ake_profile_emissions_tuned_f32``: the emissions of
    recordings that sit ``cents`` off A4 = 440 Hz from this one transform, without retuning the audio.  One number, or a tensor (R,) or
    (R, W) -- ``estimate_tuning``'s cents or ``tuning_track``'s curve go straight in, nothing is read back; a (R, W) tensor may be a
    view with a row stride beyond W.  The kernel reads float32, NaN as 0, beyond +-50 as +-50.  ``n_bins`` must then be a multiple of 36,
    and the workspace holds ``ake_profile_tuned_workspace_bytes``.  Two launches, ``profile_fold_kernel`` and
    ``profile_tuned_score_kernel``."""
    if not logmag.is_cuda:
        raise _lib.AkeError("profile_emissions needs its input on a HIP device; there is no CPU fallback (the float64 model is in ake_amd.metrics)")
    if logmag.dim() != 3:
        raise ValueError(f"profile_emissions: logmag must be (R, n_bins, T), got {tuple(logmag.shape)}")
    mel = logmag.to(torch.float32).contiguous()
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    if P % metrics.TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"profile_emissions: {P} bins are no multiple of 3 (3 bins per semitone)")
    if cents is not None and P % metrics.FOLDED_BINS != 0:
        raise ValueError(f"profile_emissions: the tuned chroma (cents) needs whole octaves, and {P} bins are no multiple of 36")
    mode = metrics._profile_compression(compression)
    sharpness = float(sharpness)
    if not sharpness > 0.0:
        raise ValueError("profile_emissions: sharpness must be positive")
    wf, sf = int(window_frames), int(stride_frames)
    if wf < 0 or sf < 1:
        raise ValueError("profile_emissions: window_frames must be >= 0 (0: the whole clip) and stride_frames >= 1")
    dev = mel.device
    prof = device_profiles(profiles, dev)
    W = (1 if wf == 0 else 0) if T == 0 else profile_windows(T, wf, sf)
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
        assert counts.shape == (R,)
    if cents is not None:
        cents = device_cents(cents, R, W, dev)
    return _launch(mel, frames_major, counts, wf, sf, W, prof, mode, sharpness, workspace, cents)


def device_cents(cents, R, W, device):
    """``cents`` of the tuned chroma (a number, or a tensor (R,) or (R, W)) checked -> a float32 tensor on ``device``, (R,) or (R, W)
    with unit stride along the windows, as ``_launch`` hands it to the kernel.  A float32 device tensor is taken as it is."""
    if not isinstance(cents, torch.Tensor):
        return torch.full((R,), float(cents), dtype=torch.float32, device=device)
    c = cents.detach().to(device=device, dtype=torch.float32)
    if c.dim() == 0:
        return c.reshape(1).expand(R).contiguous()
    if not (tuple(c.shape) == (R,) or tuple(c.shape) == (R, W)):
        raise ValueError(f"profile_emissions: cents must be a number, ({R},) or ({R}, {W}), got {tuple(c.shape)}")
    if c.dim() == 2 and W > 0 and (c.stride(1) != 1 or (R > 1 and c.stride(0) < W)):
        c = c.contiguous()
    return c


def _launch(mel, frames_major, counts, wf, sf, W, prof, mode, sharpness, workspace=None, cents=None):
    """``ake_profile_emissions_f32`` on checked arguments: ``mel`` float32 contiguous on the device, ``counts`` int32 (R,) there or None,
    ``prof`` float32 (2, 12) there, ``mode`` 0..2, ``W`` = ``profile_windows``.  ``cents`` (``device_cents``): the tuned entry,
    ``ake_profile_emissions_tuned_f32``, instead."""
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    dev = mel.device
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    chroma, emissions, key_id, conf = f32(R, W, 12), f32(R, W, 24), torch.empty((R, W), dtype=torch.int32, device=dev), f32(R, W)
    if R == 0 or W == 0:
        return chroma, emissions, key_id, conf
    if T == 0:                                                       # the whole-clip mode on no frames: every recording is silent
        return chroma.zero_(), emissions.zero_(), key_id.fill_(-1), conf.zero_()
    L = _lib.lib()
    if cents is not None:
        nbytes = int(L.ake_profile_tuned_workspace_bytes(R, T))
        if nbytes == 0:
            _lib.check(-1, "ake_profile_tuned_workspace_bytes")
        ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rec_stride, win_stride = (cents.stride(0) if R > 1 else 0, 0) if cents.dim() == 1 else (cents.stride(0) if R > 1 else W, 1)
        with torch.cuda.device(dev):
            _lib.check(L.ake_profile_emissions_tuned_f32(mel.data_ptr(), 1 if frames_major else 0, R, P, T,
                                                         counts.data_ptr() if counts is not None else None, wf, sf, W, prof.data_ptr(), mode,
                                                         sharpness, cents.data_ptr(), rec_stride, win_stride, chroma.data_ptr(),
                                                         emissions.data_ptr(), key_id.data_ptr(), conf.data_ptr(), ws.data_ptr(), ws.numel(),
                                                         torch.cuda.current_stream().cuda_stream), "ake_profile_emissions_tuned_f32")
        return chroma, emissions, key_id, conf
    nbytes = int(L.ake_profile_workspace_bytes(R, T))
    if nbytes == 0:
        _lib.check(-1, "ake_profile_workspace_bytes")
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.ake_profile_emissions_f32(mel.data_ptr(), 1 if frames_major else 0, R, P, T, counts.data_ptr() if counts is not None else None,
                                               wf, sf, W, prof.data_ptr(), mode, sharpness, chroma.data_ptr(), emissions.data_ptr(),
                                               key_id.data_ptr(), conf.data_ptr(), ws.data_ptr(), ws.numel(),
                                               torch.cuda.current_stream().cuda_stream), "ake_profile_emissions_f32")
    return chroma, emissions, key_id, conf


def fit_key_profiles(chroma, key_id, weight=None):
    """``metrics.fit_key_profiles``: key profiles from labelled chroma -> (2, 12) float64 on the inputs' device, which
    ``profile_emissions(profiles=...)`` and ``KeyEstimator.track(method="profile", profiles=...)`` take."""
    return metrics.fit_key_profiles(chroma, key_id, weight)
