"""Tuning on the device: how far recordings sit from A4 = 440 Hz, and the varispeed resampler that puts them back.

Not part of the reference: it pins librosa 0.9.2, whose ``cqt`` runs at ``tuning=0.0``, and its net collapses each semitone's three bins
as they come, so a recording that is 35 cents sharp lands one full bin off.  Host wrappers of ``ake_tuning_estimate_f32``
(csrc/tuning.hip) and ``ake_retune_f32`` / ``ake_retune_pcm16_f32`` (csrc/audio.hip); the float64 models are
``metrics.estimate_tuning`` and ``metrics.retune_reference``.  For a tuning that drifts within a recording: ``tuning_track``
(``ake_tuning_track_f32``) and ``retune_curve`` / ``retune_curve_positions`` (``ake_retune_curve_f32`` / ``_pcm16_f32`` /
``ake_retune_curve_positions``), with the models ``metrics.tuning_track`` and ``metrics.retune_curve_reference``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

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


def tuning_track(logmag: torch.Tensor, window_frames: int, stride_frames: int, counts: torch.Tensor | None = None,
                 min_strength: float = 0.0, frames_major: bool = False, workspace: torch.Tensor | None = None):
    """The detuning of B recordings over time, for a tuning that drifts -> ``(cents_raw, strength, curve, window_counts)``: float32
    (B, W) three times and int32 (B,), on the device (``ake_tuning_track_f32``; ``metrics.tuning_track`` is the definition).

    ``logmag``, ``counts``, ``frames_major`` and ``workspace`` (``ake_tuning_track_workspace_bytes``) as in ``estimate_tuning``.  Windows of
    ``window_frames`` frames, ``stride_frames`` apart; ``W = metrics.tuning_track_windows(T, ...)`` is computed from the shape, so nothing is
    read back.  ``cents_raw`` and ``strength`` are every window's estimate; ``curve`` is what ``retune_curve`` follows: windows weaker
    than ``min_strength`` hold the last strong value, the sequence is unwrapped across the +-50 seam and clamped to +-50.  Three launches
    on the current stream."""
    _need_device(logmag, "tuning_track")
    if logmag.dim() != 3:
        raise ValueError(f"tuning_track: logmag must be (B, n_bins, T), got {tuple(logmag.shape)}")
    mel = logmag.to(torch.float32).contiguous()
    B, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    if P % metrics.TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"tuning_track: {P} bins are no multiple of 3 (3 bins per semitone)")
    wf, sf = int(window_frames), int(stride_frames)
    W = metrics.tuning_track_windows(T, wf, sf)
    dev = mel.device
    cents, strength, curve = (torch.empty((B, W), dtype=torch.float32, device=dev) for _ in range(3))
    n_win = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0 or T == 0:
        return cents, strength, curve, n_win.zero_()
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
        assert counts.shape == (B,)
    L = _lib.lib()
    nbytes = int(L.ake_tuning_track_workspace_bytes(B, T, wf, sf))
    if nbytes == 0:
        _lib.check(-1, "ake_tuning_track_workspace_bytes")
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.ake_tuning_track_f32(mel.data_ptr(), 1 if frames_major else 0, B, P, T, counts.data_ptr() if counts is not None else None,
                                          wf, sf, float(min_strength), cents.data_ptr(), strength.data_ptr(), curve.data_ptr(), n_win.data_ptr(),
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "ake_tuning_track_f32")
    return cents, strength, curve, n_win


def _curve_on_device(cents, B, dev, what):
    """``cents`` (K,) or (B, K) -> float32 (B, K) on ``dev`` with unit stride along the knots."""
    if not isinstance(cents, torch.Tensor):
        cents = torch.as_tensor(cents, dtype=torch.float32)
    cents = cents.to(device=dev, dtype=torch.float32)
    if cents.dim() == 1:
        cents = cents[None]
    if cents.dim() != 2 or cents.shape[1] < 1:
        raise ValueError(f"{what}: a curve is (K,) or (B, K) with K >= 1, got {tuple(cents.shape)}")
    if cents.shape[0] == 1 and B != 1:
        cents = cents.expand(B, -1)
    if cents.shape[0] != B:
        raise ValueError(f"{what}: {B} rows but {cents.shape[0]} curves")
    return cents.contiguous()


def _curve_workspace(L, B, K, dev):
    nbytes = int(L.ake_retune_curve_workspace_bytes(B, K))
    if nbytes == 0:
        _lib.check(-1, "ake_retune_curve_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def retune_curve(audio: torch.Tensor, cents, knot_first: int, knot_step: int, lengths: torch.Tensor | None = None):
    """``retune`` along a tuning curve -> ``(audio (B, retune_out_len(n)) float32, lengths (B,) int64)``.

    ``audio`` and ``lengths`` as in ``retune``.  ``cents`` (B, K) or (K,) float32 (``tuning_track``'s ``curve`` goes straight in; nothing
    is read back): knot i sits at input sample ``knot_first + i * knot_step`` (``knot_first >= 0``, ``knot_step >= 64``); the ratio is
    ``2 ** (cents / 1200)`` at the knots, linear in the input position between them and constant outside
    (``metrics.retune_curve_reference``).  A row whose cents are all 0 is copied bit for bit.  Two launches on the current stream."""
    _need_device(audio, "retune_curve")
    if audio.dim() != 2:
        raise ValueError(f"retune_curve: audio must be (B, n), got {tuple(audio.shape)}")
    pcm = audio.dtype == torch.int16
    if not pcm:
        audio = audio.to(torch.float32)
    if audio.stride(1) != 1 or (audio.shape[0] > 1 and audio.stride(0) < audio.shape[1]):
        audio = audio.contiguous()
    dev = audio.device
    B, n = audio.shape
    if int(knot_first) < 0 or int(knot_step) < 64:
        raise ValueError(f"retune_curve: knot_first {knot_first} must be >= 0 and knot_step {knot_step} >= 64 samples")
    L = _lib.lib()
    width = retune_out_len(n)
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    len_out = torch.empty((B,), dtype=torch.int64, device=dev)
    if B == 0 or n == 0:
        return out.zero_(), len_out.zero_()
    cents = _curve_on_device(cents, B, dev, "retune_curve")
    K = cents.shape[1]
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
        assert lengths.shape == (B,)
    ws = _curve_workspace(L, B, K, dev)
    fn, name = (L.ake_retune_curve_pcm16_f32, "ake_retune_curve_pcm16_f32") if pcm else (L.ake_retune_curve_f32, "ake_retune_curve_f32")
    with torch.cuda.device(dev):
        _lib.check(fn(audio.data_ptr(), B, n, audio.stride(0) if B > 1 else max(n, 1), lengths.data_ptr() if lengths is not None else None,
                      cents.data_ptr(), K, cents.stride(0), int(knot_first), int(knot_step), out.data_ptr(), out.stride(0), len_out.data_ptr(),
                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), name)
    return out, len_out


def retune_curve_positions(out_index: torch.Tensor, cents, knot_first: int, knot_step: int):
    """Where the outputs ``out_index`` (B, m) or (m,) int64 of ``retune_curve`` read their input -> float64 positions in samples, of the
    same shape, by the device function the resampler uses (``ake_retune_curve_positions``; ``metrics.retune_curve_positions``)."""
    idx = torch.as_tensor(out_index)
    _need_device(idx, "retune_curve_positions")
    single = idx.dim() == 1
    idx = (idx[None] if single else idx).to(torch.int64).contiguous()
    if idx.dim() != 2:
        raise ValueError(f"retune_curve_positions: out_index must be (m,) or (B, m), got {tuple(out_index.shape)}")
    if int(knot_first) < 0 or int(knot_step) < 64:
        raise ValueError(f"retune_curve_positions: knot_first {knot_first} must be >= 0 and knot_step {knot_step} >= 64 samples")
    B, m = idx.shape
    dev = idx.device
    pos = torch.empty((B, m), dtype=torch.float64, device=dev)
    if B == 0 or m == 0:
        return pos[0] if single else pos
    cents = _curve_on_device(cents, B, dev, "retune_curve_positions")
    K = cents.shape[1]
    L = _lib.lib()
    ws = _curve_workspace(L, B, K, dev)
    with torch.cuda.device(dev):
        _lib.check(L.ake_retune_curve_positions(cents.data_ptr(), B, K, cents.stride(0), int(knot_first), int(knot_step), idx.data_ptr(), m,
                                                pos.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                   "ake_retune_curve_positions")
    return pos[0] if single else pos


class StreamRetuner:
    """``retune`` on audio that arrives in chunks: R recordings in lockstep, all retuned by the one ``cents``.

    ``push(chunk)`` takes the next m samples of every recording -- (R, m) float32, or int16 = 16-bit PCM (``pcm16_to_float``); any m >= 0;
    the format may change from push to push -- and returns the (R, k) float32 outputs that chunk made final; ``finish()`` returns the
    rest.  Joined, the pieces are ``retune(whole, cents)[0][:, :floor(n * rho)]`` on the joined chunks, bit for bit, however the audio was
    cut (``ake_stream_retune_f32``; host model ``metrics.stream_retune``).  An output is final once the last of its 64 taps has arrived,
    so the outputs trail the input by 32 samples.

    ``cents``: one number within +-50 (all recordings share it: recordings with ratios of their own would finish different numbers of
    samples per push).  ``rho`` is the ratio as the device computes it, read back once, here (``ake_retune_ratio``): the offline kernel's
    own double, which the host's ``2 ** (cents / 1200)`` may miss by a last place.  With ``cents == 0`` the stream is a copy, as it is
    offline.  The carried state (64 float32 a recording) is sized here; a push allocates only what it returns, reads nothing back from the
    device and runs on the current stream.  A chunk longer than ``max_chunk_samples`` (default: no limit) goes in several pieces, joined
    by one ``torch.cat``."""

    def __init__(self, cents, recordings: int, device=None, max_chunk_samples: int | None = None):
        if not torch.cuda.is_available():
            raise _lib.AkeError("the retuner needs a HIP device; there is no CPU fallback (the float64 model is metrics.stream_retune)")
        self.R = int(recordings)
        if not 1 <= self.R <= 65535:
            raise ValueError(f"StreamRetuner: recordings must lie in 1..65535, got {recordings}")
        if isinstance(cents, torch.Tensor):
            if cents.numel() != 1:
                raise ValueError("StreamRetuner: one number of cents for all recordings (they advance in lockstep)")
            cents = cents.item()
        if not abs(float(cents)) <= metrics.RETUNE_MAX_CENTS:
            raise ValueError(f"StreamRetuner: {cents} cents; a detuning lies within +-{metrics.RETUNE_MAX_CENTS:g} cents")
        self.max_chunk = None if max_chunk_samples is None else int(max_chunk_samples)
        if self.max_chunk is not None and self.max_chunk < 1:
            raise ValueError("StreamRetuner: max_chunk_samples must be at least 1")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.cents = C.c_float(float(cents)).value                   # what the kernel is given: float32
        L = _lib.lib()
        rho = C.c_double(0.0)
        with torch.cuda.device(self.device):
            _lib.check(L.ake_retune_ratio(self.cents, C.byref(rho), torch.cuda.current_stream().cuda_stream), "ake_retune_ratio")
        self.rho = rho.value
        self.state = torch.empty(int(L.ake_stream_retune_state_bytes(self.R)), dtype=torch.uint8, device=self.device)
        self.n = 0                                                   # inputs so far: the device keeps no count
        self.finished = False

    def out_count(self, n_in: int, finished: bool = False) -> int:
        """Outputs that are final after ``n_in`` inputs (``metrics.retune_final`` with this stream's ``rho``)."""
        return int(_lib.lib().ake_stream_retune_out_count(self.cents, self.rho, int(n_in), int(finished)))

    def _checked(self, chunk):
        if not isinstance(chunk, torch.Tensor) or chunk.dtype not in (torch.float32, torch.int16):
            raise ValueError("StreamRetuner.push: a chunk is a float32 or int16 (16-bit PCM) tensor")
        if chunk.dim() != 2 or chunk.shape[0] != self.R:
            raise ValueError(f"StreamRetuner.push: a chunk is (R, m) with R = {self.R}, got {tuple(chunk.shape)}")
        chunk = chunk.to(self.device)
        if chunk.stride(1) != 1 and chunk.shape[1] > 1:
            chunk = chunk.contiguous()
        return chunk

    def _piece(self, chunk, finishing, out=None):
        """One call of the entry point: ``chunk`` (R, m) as ``_checked`` leaves it, or None -> the (R, k) outputs, written to the front
        of ``out`` (R, >= k) when that is given."""
        L = _lib.lib()
        m = 0 if chunk is None else int(chunk.shape[1])
        k = self.out_count(self.n + m, finishing) - self.out_count(self.n)
        if out is None:
            out = torch.empty((self.R, k), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.shape[0] == self.R and out.shape[1] >= k and (out.stride(1) == 1 or out.shape[1] <= 1)
        k_out = C.c_int64(-1)
        fn, name = ((L.ake_stream_retune_pcm16_f32, "ake_stream_retune_pcm16_f32") if m and chunk.dtype == torch.int16
                    else (L.ake_stream_retune_f32, "ake_stream_retune_f32"))
        with torch.cuda.device(self.device):
            _lib.check(fn(chunk.data_ptr() if m else None, self.R, m, (chunk.stride(0) if self.R > 1 else m) if m else 0, self.cents, self.rho,
                          self.n, int(finishing), self.state.data_ptr(), self.state.numel(), out.data_ptr() if k else None,
                          max(out.stride(0), k), C.byref(k_out), torch.cuda.current_stream().cuda_stream), name)
        assert k_out.value == k
        self.n += m
        return out[:, :k]

    @torch.no_grad()
    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise ValueError("StreamRetuner.push: the stream has been finished")
        chunk = self._checked(chunk)
        m = chunk.shape[1]
        if self.max_chunk is None or m <= self.max_chunk:
            return self._piece(chunk, False)
        return torch.cat([self._piece(chunk[:, a:a + self.max_chunk], False) for a in range(0, m, self.max_chunk)], dim=1)

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """The recordings end here: the outputs whose taps reach behind the end, which see zeros there, as the offline ones do."""
        if self.finished:
            raise ValueError("StreamRetuner.finish: the stream has been finished")
        out = self._piece(None, True)
        self.finished = True
        return out
