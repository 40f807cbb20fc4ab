"""Training batches cut from annotated recordings on the device (``KeyEstimator.training_windows`` -> ``TrackWindows``).

One CQT per recording is made once and kept on the device, as ``KeyEstimator.track`` makes it; every batch is then two launches with no
host round trip: ``ake_draw_windows_i32`` (window positions from a counter-based generator) and ``ake_window_batch_f32`` (the windows
gathered from the cached transform, with their labels and a weight per window from the ``KeyAnnotations``).  The batches follow
``KeyDataset``'s contract plus ``sample_weight``, which ``PitchClassNet.general_step`` hands to the weighted loss
(``ake_general_step_weighted_f32``).  Host models: ``metrics.draw_windows``, ``metrics.window_labels``, ``metrics.weighted_general_step``.
"""
from __future__ import annotations

import torch

from . import _lib, metrics
from .pipeline import KeyAnnotations

_U64 = 0xFFFFFFFFFFFFFFFF


def draw_windows(prefix: torch.Tensor, seed: int, epoch: int, first_slot: int, batch: int):
    """``batch`` window positions on the device -> ``(recording, start)`` int32 (batch,): ``ake_draw_windows_i32``.

    ``prefix`` int64 (R + 1,) on the device: ``metrics.window_prefix`` of the recordings' frame counts, with ``prefix[R] > 0`` (the
    caller's contract: the kernel cannot report it).  Slot ``first_slot + b`` of ``(seed, epoch)`` always draws the same window, however
    the slots are split into calls.  ``metrics.draw_windows`` is the same arithmetic in Python ints."""
    dev = prefix.device
    if prefix.dtype != torch.int64 or prefix.dim() != 1 or prefix.numel() < 2 or not prefix.is_contiguous():
        raise ValueError("draw_windows: prefix must be a contiguous int64 (R + 1,) tensor")
    recording = torch.empty(int(batch), dtype=torch.int32, device=dev)
    start = torch.empty(int(batch), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ake_draw_windows_i32(prefix.data_ptr(), prefix.numel() - 1, int(seed) & _U64, int(epoch) & 0xFFFFFFFF, int(first_slot),
                                                   int(batch), recording.data_ptr(), start.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "ake_draw_windows_i32")
    return recording, start


def window_batch(mel, recording, start, window_frames, hop, annotations=None, frames_major=False, min_purity=0.0, uniform=False):
    """The windows ``(recording[b], start[b])`` of the cached transforms ``mel`` -> dict, one launch (``ake_window_batch_f32``).

    ``mel`` float32 (R, P, T), or (R, T, P) with ``frames_major``; ``recording`` / ``start`` int32 (B,) on the device.  Always:
    ``mel`` (B, 1, P, window_frames).  ``annotations`` (``KeyAnnotations``, in samples at the transform's rate): ``key_labels`` (B, 12),
    ``tonic_labels`` (B, 12), ``key_signature_id`` (B, 24), ``seq_length`` int64 (B,) and ``sample_weight`` (B,) as
    ``metrics.window_labels`` states them.  List entries outside their range are read clamped into it."""
    dev = mel.device
    if mel.dtype != torch.float32 or mel.dim() != 3 or not mel.is_contiguous():
        raise ValueError("window_batch: mel must be a contiguous float32 (R, P, T) or (R, T, P) tensor")
    R = mel.shape[0]
    T, P = (mel.shape[1], mel.shape[2]) if frames_major else (mel.shape[2], mel.shape[1])
    wf, B = int(window_frames), recording.numel()
    for t in (recording, start):
        if t.dtype != torch.int32 or t.device != dev or t.shape != (B,) or not t.is_contiguous():
            raise ValueError("window_batch: recording and start must be contiguous int32 (B,) tensors on mel's device")
    out = {"mel": torch.empty((B, 1, P, wf), dtype=torch.float32, device=dev)}
    ann = (None,) * 3
    labels = (None,) * 5
    S = 0
    if annotations is not None:
        if annotations.seg_start.shape[0] != R:
            raise ValueError(f"window_batch: {R} transforms, but annotations of {annotations.seg_start.shape[0]} recordings")
        ann = (annotations.seg_start.to(device=dev, dtype=torch.int64).contiguous(), annotations.seg_key.to(device=dev, dtype=torch.int32).contiguous(),
               annotations.seg_count.to(device=dev, dtype=torch.int32).contiguous())
        S = ann[0].shape[1]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        labels = (f32(B, 12), f32(B, 12), f32(B, 24), torch.empty(B, dtype=torch.int64, device=dev), f32(B))
        out.update(zip(("key_labels", "tonic_labels", "key_signature_id", "seq_length", "sample_weight"), labels))
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ake_window_batch_f32(mel.data_ptr(), int(bool(frames_major)), R, T, P, wf, int(hop), recording.data_ptr(), start.data_ptr(), B,
                                                   ptr(ann[0]), ptr(ann[1]), ptr(ann[2]), S, float(min_purity), int(bool(uniform)), out["mel"].data_ptr(),
                                                   *(ptr(t) for t in labels), torch.cuda.current_stream().cuda_stream), "ake_window_batch_f32")
    return out


class TrackWindows:
    """An iterable of training batches over annotated recordings (``KeyEstimator.training_windows`` builds it); it has ``__len__`` and
    ``__iter__``, so ``Trainer.fit(net, train_dataloaders=tw)`` takes it as it takes a ``DataLoader``.

    Every batch is a dict on the device in ``KeyDataset``'s contract: ``mel`` (B, 1, P, window_frames) float32, ``key_labels`` (B, 12),
    ``tonic_labels`` (B, 12), ``key_signature_id`` (B, 24), ``genre`` (B, ``genre_classes``) zeros (no window carries a genre label),
    ``seq_length`` (B,) int64 = ``window_frames``; plus ``sample_weight`` (B,) float32 and, to say where the window lies,
    ``recording`` and ``start_frame`` (B,) int32.  The ``genre`` tensor is shared between the batches: read it, do not write it.

    Random mode (``stride_frames=None``): every batch is ``batch_size`` windows drawn uniformly from all start frames of all recordings
    that hold one window (``metrics.draw_windows``), ``batches_per_epoch`` batches an epoch (default: as many as cover the recordings
    once at a stride of one window).  Slot ``i * batch_size + b`` of ``(seed, epoch)`` is window b of batch i, so the same ``(seed,
    epoch)`` yields the same batches; every completed iteration advances ``epoch`` by one and ``set_epoch`` sets it.

    Grid mode (``stride_frames`` given), for validation: ``KeyEstimator.track``'s own windows at that stride, in order, recording by
    recording; the last batch may be short.

    Sequence mode (``sequence_windows=K`` with ``stride_frames``), for the sequence loss (``ake_amd.key_sequence_loss``): every batch is
    ``batch_size`` sequences of K consecutive ``track`` windows, ``stride_frames`` apart, so ``B = batch_size * K`` rows ordered
    ``[sequence][window]``.  The sequence starts are drawn as random mode draws windows, over the recordings that hold one whole sequence
    (``metrics.window_prefix(frames, window_frames + (K - 1) * stride_frames)``): slot ``i * batch_size + s`` of ``(seed, epoch)`` is
    sequence s of batch i (``metrics.sequence_windows``).  The batch carries three more entries: ``sequence_shape = (batch_size, K)``,
    ``key_id`` int32 (B,) -- the window's key where ``sample_weight > 0``, else -1, an unlabelled window to the loss -- and ``log_trans``,
    the (24, 24) transition the sequences are scored under, the tensor given here as it is.

    ``weighting``: ``"purity"`` weighs a window by the share of its samples that carry its label, ``"uniform"`` by 1; either way 0 for an
    unlabelled window and for ``purity < min_purity``.  Iterating launches kernels and allocates outputs, and waits for nothing.  Under
    data-parallel training every rank's loss is normalised by the weights of its own batch."""

    def __init__(self, mel, frames, annotations, hop, window_frames, batch_size=8, batches_per_epoch=None, stride_frames=None, seed=0,
                 weighting="purity", min_purity=0.0, genre_classes=11, sequence_windows=None, log_trans=None):
        if weighting not in ("purity", "uniform"):
            raise ValueError("weighting must be 'purity' or 'uniform'")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if not 0.0 <= float(min_purity) <= 1.0:
            raise ValueError("min_purity must lie in 0..1")
        dev = mel.device
        self.mel = mel                                                   # (R, P, T), as CQTPlan.logmag leaves it
        # on the device in the kernel's dtypes once, so that no batch converts or copies them
        self.annotations = KeyAnnotations(annotations.seg_start.to(device=dev, dtype=torch.int64).contiguous(),
                                          annotations.seg_key.to(device=dev, dtype=torch.int32).contiguous(),
                                          annotations.seg_count.to(device=dev, dtype=torch.int32).contiguous(), annotations.sample_rate)
        self.frames = [int(t) for t in frames]
        if len(self.frames) != mel.shape[0] or annotations.seg_start.shape[0] != mel.shape[0]:
            raise ValueError(f"TrackWindows: {mel.shape[0]} transforms, {len(self.frames)} frame counts, annotations of "
                             f"{annotations.seg_start.shape[0]} recordings")
        self.hop, self.window_frames, self.batch_size = int(hop), int(window_frames), int(batch_size)
        self.seed, self.epoch = int(seed), 0
        self.weighting, self.min_purity = weighting, float(min_purity)
        self.stride_frames = None if stride_frames is None else int(stride_frames)
        wf = self.window_frames
        self._genre = {}
        self._genre_classes = int(genre_classes)
        count = lambda t, sf: 0 if t < wf else (t - wf) // sf + 1                                   # pipeline.track_counts
        self.sequence_windows = None if sequence_windows is None else int(sequence_windows)
        self.log_trans = log_trans
        if self.sequence_windows is not None:
            K = self.sequence_windows
            if K < 2:
                raise ValueError("sequence_windows must be at least 2 (one window is what random mode draws)")
            if self.stride_frames is None or self.stride_frames < 1:
                raise ValueError("sequence_windows needs a stride of at least one frame between a sequence's windows (stride_seconds)")
            if not isinstance(log_trans, torch.Tensor) or tuple(log_trans.shape) != (24, 24):
                raise ValueError("sequence_windows needs log_trans, a (24, 24) tensor of log-probabilities, from key i (row) to key j")
            prefix = metrics.window_prefix(self.frames, wf + (K - 1) * self.stride_frames)
            if prefix[-1] <= 0:
                raise ValueError(f"training_windows: no recording is as long as one sequence of {K} windows")
            self._prefix = torch.tensor(prefix, dtype=torch.int64, device=dev)
            self._offsets = torch.arange(K, dtype=torch.int32, device=dev) * self.stride_frames
            grid = sum(count(t, self.stride_frames) for t in self.frames)
            self.batches_per_epoch = -(-grid // (self.batch_size * K)) if batches_per_epoch is None else int(batches_per_epoch)
            if self.batches_per_epoch < 1:
                raise ValueError("batches_per_epoch must be at least 1")
        elif self.stride_frames is None:
            prefix = metrics.window_prefix(self.frames, wf)
            if prefix[-1] <= 0:
                raise ValueError("training_windows: no recording is as long as one window")
            self._prefix = torch.tensor(prefix, dtype=torch.int64, device=dev)
            grid = sum(count(t, wf) for t in self.frames)
            self.batches_per_epoch = -(-grid // self.batch_size) if batches_per_epoch is None else int(batches_per_epoch)
            if self.batches_per_epoch < 1:
                raise ValueError("batches_per_epoch must be at least 1")
        else:
            if self.stride_frames < 1:
                raise ValueError("stride_frames must be at least 1")
            rec = [r for r, t in enumerate(self.frames) for _ in range(count(t, self.stride_frames))]
            start = [w * self.stride_frames for t in self.frames for w in range(count(t, self.stride_frames))]
            if not rec:
                raise ValueError("training_windows: no recording is as long as one window")
            self._recording = torch.tensor(rec, dtype=torch.int32, device=dev)
            self._start = torch.tensor(start, dtype=torch.int32, device=dev)
            self.batches_per_epoch = -(-len(rec) // self.batch_size)

    def __len__(self):
        return self.batches_per_epoch

    def set_epoch(self, epoch: int):
        """The epoch the next iteration draws (random mode)."""
        self.epoch = int(epoch)

    def _batch(self, recording, start):
        out = window_batch(self.mel, recording, start, self.window_frames, self.hop, self.annotations, min_purity=self.min_purity,
                           uniform=self.weighting == "uniform")
        B = recording.numel()
        if B not in self._genre:
            self._genre[B] = torch.zeros((B, self._genre_classes), dtype=torch.float32, device=self.mel.device)
        out["genre"], out["recording"], out["start_frame"] = self._genre[B], recording, start
        return out

    def _sequences(self, epoch, i):
        """Batch i of ``epoch`` in sequence mode: the drawn starts expanded to K windows each, two torch ops on the device."""
        B, K = self.batch_size, self.sequence_windows
        recording, start = draw_windows(self._prefix, self.seed, epoch, i * B, B)
        out = self._batch(recording[:, None].expand(B, K).reshape(-1), (start[:, None] + self._offsets[None, :]).reshape(-1))
        out["sequence_shape"] = (B, K)
        key = out["key_signature_id"].argmax(dim=1).to(torch.int32)
        out["key_id"] = torch.where(out["sample_weight"] > 0, key, torch.full_like(key, -1))
        out["log_trans"] = self.log_trans
        return out

    def __iter__(self):
        B = self.batch_size
        if self.sequence_windows is not None:
            epoch = self.epoch
            for i in range(self.batches_per_epoch):
                yield self._sequences(epoch, i)
            self.epoch = epoch + 1
            return
        if self.stride_frames is not None:
            for i in range(self.batches_per_epoch):
                yield self._batch(self._recording[i * B:(i + 1) * B], self._start[i * B:(i + 1) * B])
            return
        epoch = self.epoch
        for i in range(self.batches_per_epoch):
            yield self._batch(*draw_windows(self._prefix, self.seed, epoch, i * B, B))
        self.epoch = epoch + 1
