"""Audio that starts in host memory: ``HostFeeder`` uploads batch k + 1 while the estimator computes batch k.

Decoders and WAV files deliver 16-bit PCM in host memory, and the host link carries far fewer clips a second than the device computes.
What the library can do about it is move few bytes (int16 goes over the link as int16 and is read in place by the PCM kernels) and hide
the copies under the compute (a copy stream of its own, double-buffered).  One Python thread, no extra process.
"""
from __future__ import annotations

from collections import deque

import torch

from .pipeline import KeyEstimator

_ROW = 4                                                             # row stride of the staging and device buffers: a multiple of 4 samples


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _rows_of(x: torch.Tensor):
    """A CPU batch as the rows of its own storage -> ``(rows (B, r), rebuild)``; ``rebuild`` turns a (B, r) tensor that holds the same
    rows anywhere else back into the batch's shape.  Mono (B, n), planar (B, C, n) and interleaved storage (B, n, C) handed over as
    ``buf.transpose(1, 2)`` keep their layout, so every upload is one straight copy; anything else is made planar first."""
    if x.dim() == 2:
        if x.stride(1) != 1 and x.shape[1] > 1:
            x = x.contiguous()
        return x, lambda rows: rows
    if x.dim() != 3:
        raise ValueError(f"HostFeeder: a batch is (B, n) or (B, C, n), got {tuple(x.shape)}")
    B, Cn, n = x.shape
    if x.transpose(1, 2).is_contiguous():                            # interleaved storage
        return x.transpose(1, 2).reshape(B, n * Cn), lambda rows: rows.unflatten(1, (n, Cn)).transpose(1, 2)
    return x.contiguous().reshape(B, Cn * n), lambda rows: rows.unflatten(1, (Cn, n))


class HostFeeder:
    """``feeder = HostFeeder(estimator, depth=2, **call_kwargs)``; ``for result in feeder(batches): ...``

    ``batches``: an iterable of CPU tensors or ``(tensor, lengths)`` pairs -- int16 (16-bit PCM) or float32, (B, n) or (B, C, n), any
    mix, any sizes.  ``call_kwargs``: ``rate`` and ``channel`` of ``KeyEstimator.__call__``, or ``track=True`` and ``track()``'s
    arguments.  Yields every batch's result, in order, exactly what ``estimator(batch.to(device), lengths, **call_kwargs)`` returns, with
    at most ``depth`` batches in flight: batch k is yielded once batch k + depth - 1 has been issued.

    The feeder owns ``depth`` pinned staging buffers, ``depth`` device buffers (row stride a multiple of 4 samples, so int16 rows are
    4-byte aligned; both grow to the largest batch seen) and one copy stream.  A batch is copied into a staging buffer on the host,
    uploaded on the copy stream and computed on the caller's current stream, which waits for that upload alone.  An input that is
    already pinned is uploaded from where it lies (keep it unchanged until its result has been yielded).  Events guard the reuse: a
    staging buffer is not overwritten before its upload has finished (the host waits), a device buffer not before the compute that read
    it has finished (the copy stream waits).  A yielded result is safe to read on the caller's current stream (an estimator with
    ``streams`` > 1 is joined)."""

    def __init__(self, estimator: KeyEstimator, depth: int = 2, **call_kwargs):
        if int(depth) < 1:
            raise ValueError("HostFeeder: depth must be at least 1")
        self.estimator, self.depth = estimator, int(depth)
        self.device = estimator.device
        self._track = bool(call_kwargs.pop("track", False))
        self._kwargs = call_kwargs
        self._copy_stream = None
        self._slots = [{"pinned": None, "dev": None, "uploaded": None, "consumed": None, "keep": None} for _ in range(self.depth)]
        self._turn = 0

    def _buffers(self, slot, nbytes, staged):
        if staged and (slot["pinned"] is None or slot["pinned"].numel() < nbytes):
            slot["pinned"] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        if slot["dev"] is None or slot["dev"].numel() < nbytes:
            slot["dev"] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            slot["dev"].record_stream(self._copy_stream)             # written on the copy stream, whatever stream allocated it
            # The allocator hands out memory that is free in the order of the CURRENT stream: kernels already queued there (an earlier
            # batch's compute, on temporaries it has since released) may still be using these bytes.  The copy stream is not in that
            # order, so it waits for what is queued now before it writes here.  Only when a buffer grows.
            self._copy_stream.wait_stream(torch.cuda.current_stream(self.device))

    def _submit(self, item):
        x, lengths = item if isinstance(item, (tuple, list)) else (item, None)
        if not isinstance(x, torch.Tensor) or x.device.type != "cpu":
            raise ValueError("HostFeeder: batches are CPU tensors (audio that is already on the device goes to the estimator directly)")
        if x.dtype not in (torch.int16, torch.float32):
            raise ValueError(f"HostFeeder: batches are int16 (16-bit PCM) or float32, got {x.dtype}")
        rows, rebuild = _rows_of(x)
        B, r = rows.shape
        S, item_bytes = _round_up(r, _ROW), x.element_size()
        nbytes = B * S * item_bytes
        slot = self._slots[self._turn]
        self._turn = (self._turn + 1) % self.depth
        cur = torch.cuda.current_stream(self.device)
        staged = not rows.is_pinned()
        self._buffers(slot, nbytes, staged)
        dev_rows = slot["dev"][:nbytes].view(x.dtype).view(B, S)
        if staged:
            if slot["uploaded"] is not None:
                slot["uploaded"].synchronize()                       # the staging buffer's last upload has left it
            host_rows = slot["pinned"][:nbytes].view(x.dtype).view(B, S)
            host_rows[:, :r].copy_(rows)
        with torch.cuda.stream(self._copy_stream):
            if slot["consumed"] is not None:
                self._copy_stream.wait_event(slot["consumed"])      # the compute that read the device buffer last
            if staged:
                dev_rows.copy_(host_rows, non_blocking=True)         # one contiguous transfer (the pad samples travel along; never read as audio)
            else:
                dev_rows[:, :r].copy_(rows, non_blocking=True)
            if lengths is not None:
                lengths = torch.as_tensor(lengths).to(torch.int64).to(self.device, non_blocking=True)
                lengths.record_stream(cur)
            slot["uploaded"] = torch.cuda.Event()
            slot["uploaded"].record(self._copy_stream)
        slot["keep"] = None if staged else rows                      # a pinned input stays alive until its slot's next upload
        cur.wait_event(slot["uploaded"])
        audio = rebuild(dev_rows[:, :r])
        est = self.estimator
        out = est.track(audio, lengths=lengths, **self._kwargs) if self._track else est(audio, lengths=lengths, **self._kwargs)
        est.join()
        slot["consumed"] = torch.cuda.Event()
        slot["consumed"].record(cur)
        return out

    def __call__(self, batches):
        pending = deque()
        for item in batches:
            with torch.cuda.device(self.device):
                if self._copy_stream is None:
                    self._copy_stream = torch.cuda.Stream(self.device)
                pending.append(self._submit(item))
            if len(pending) == self.depth:
                yield pending.popleft()
        while pending:
            yield pending.popleft()
