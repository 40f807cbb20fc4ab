"""Device-side audio preparation in front of the CQT: channel selection / mono mix-down and polyphase resampling.

Not part of the reference, which takes channel 0 of ``torchaudio.load``'s output at the file's own sample rate
(KeyDataset.py:479-485): ``prepare(..., channel=0)`` on audio that already has the target rate is exactly that.  The rest is for
serving pipelines that hold decoded multi-channel audio of mixed rates on the GPU and want one CQT plan.
Host wrapper of ``ake_resample_f32`` (csrc/audio.hip) = ``scipy.signal.resample_poly`` with its default filter.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def pcm16_to_float(x: torch.Tensor) -> torch.Tensor:
    """What a 16-bit PCM sample means everywhere in this package: ``x.to(float32) * 2**-15`` (exact for every int16; -32768 -> -1.0),
    the float ``torchaudio.load`` returns for the same file.  int16 audio handed to the device entry points gives the results of the
    float32 route on this tensor, bit for bit, without the tensor being written."""
    return x.to(torch.float32) * 2.0 ** -15


def pcm16_rows(audio: torch.Tensor, device):
    """(B, n) int16 -> ``(tensor on device, row stride in samples)`` as the PCM kernels read it in place: unit sample stride, a 4-byte
    aligned base and an even row stride (they load whole 4-byte words).  A tensor that violates this -- a contiguous (B, n) with odd
    n does -- is copied into an even-stride buffer: the only case where PCM costs a pass."""
    assert audio.dtype == torch.int16 and audio.dim() == 2
    audio = audio.to(device=device)
    B, n = audio.shape
    stride = audio.stride(0) if B > 1 else n + (n & 1)              # (one row: its stride is never used as one)
    if audio.stride(1) == 1 and stride >= n and stride % 2 == 0 and audio.data_ptr() % 4 == 0:
        return audio, stride
    buf = torch.empty((B, n + (n & 1)), dtype=torch.int16, device=device)
    buf[:, :n].copy_(audio)                                          # (the pad sample of an odd n is never the clip's: the kernel zeroes it)
    return buf[:, :n], buf.stride(0)


class Resampler:
    """``rate_in`` -> ``rate_out`` polyphase filter on one device; reusable across calls."""

    def __init__(self, rate_in: int, rate_out: int, device=None):
        if not torch.cuda.is_available():
            raise _lib.AkeError("the resampler needs a HIP device; there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ake_resampler_create(self.rate_in, self.rate_out, C.byref(self._h)), "ake_resampler_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().ake_resampler_destroy(self._h)
                self._h = None
        except Exception:      # noqa: BLE001
            pass

    def out_len(self, n_in: int) -> int:
        return int(_lib.lib().ake_resampler_out_len(self._h, int(n_in)))

    def __call__(self, audio: torch.Tensor, channel: int = 0, lengths: torch.Tensor | None = None):
        """audio (B, C, n) or (B, n) float32 -> (mono (B, n_out) float32, lengths_out (B,) int64).  int16 audio is 16-bit PCM
        (``pcm16_to_float``) and is read in place whatever its strides -- planar (B, C, n) storage, or interleaved (B, n, C) storage
        handed over as the view ``buf.transpose(1, 2)`` -- with the float route's results on the converted tensor, bit for bit.

        ``channel`` >= 0 selects that channel (0 = the reference's ``waveform[0]``), -1 takes the mean over the channels.
        ``lengths`` (B,) int64: ragged batch, clip i holds ``lengths[i] <= n`` samples; its output is zero behind its own end."""
        if audio.dim() == 2:
            audio = audio[:, None, :]
        pcm = audio.dtype == torch.int16
        audio = audio.to(device=self.device) if pcm else audio.to(device=self.device, dtype=torch.float32)
        if not pcm and audio.stride(-1) != 1:
            audio = audio.contiguous()
        B, Cn, n = audio.shape
        n_out = self.out_len(n)
        out = torch.empty((B, n_out), dtype=torch.float32, device=self.device)
        len_out = torch.empty((B,), dtype=torch.int64, device=self.device)
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
            assert lengths.shape == (B,)
        if pcm:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().ake_resample_pcm16_f32(self._h, audio.data_ptr(), B, Cn, n, audio.stride(0), audio.stride(1), audio.stride(2),
                                                             int(channel), lengths.data_ptr() if lengths is not None else None, out.data_ptr(),
                                                             out.stride(0), len_out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                           "ake_resample_pcm16_f32")
            return out, len_out
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ake_resample_f32(self._h, audio.data_ptr(), B, Cn, n, audio.stride(0), audio.stride(1), int(channel),
                                                   lengths.data_ptr() if lengths is not None else None, out.data_ptr(), out.stride(0),
                                                   len_out.data_ptr(), torch.cuda.current_stream().cuda_stream), "ake_resample_f32")
        return out, len_out


_resamplers = {}


def get_resampler(rate_in, rate_out, device=None) -> Resampler:
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(rate_in), int(rate_out), str(dev))
    if key not in _resamplers:
        _resamplers[key] = Resampler(rate_in, rate_out, dev)
    return _resamplers[key]


class StreamResampler:
    """``Resampler`` on audio that arrives in chunks: R recordings in lockstep, ``channels`` channels each, ``rate_in`` -> ``rate_out``.

    ``push(chunk)`` takes the next m samples of every recording -- (R, C, m), or (R, m) when there is one channel; float32, or int16 =
    16-bit PCM (``pcm16_to_float``); any m >= 0 -- and returns the (R, k) float32 outputs that chunk made final; ``finish()`` returns the
    rest.  Joined, the pieces are ``Resampler(rate_in, rate_out)(whole, channel)`` on the joined chunks, bit for bit, however the audio
    was cut (``ake_stream_resample_f32``; host model ``metrics.stream_resample``).  An output is final once the last input under the
    filter has arrived, so the outputs trail the input by ``half / up`` samples (about 0.45 ms of audio at 44.1 or 48 kHz).

    int16 chunks are read in place whatever their strides: interleaved (R, m, C) storage is handed over as ``buf.transpose(1, 2)``.
    float32 chunks are made contiguous in the last dimension, as ``Resampler`` does.  ``channel`` >= 0 takes that channel, -1 the mean.
    The carried state (a few dozen float32 a recording) is sized here; a push allocates only what it returns, reads nothing back from the
    device and runs on the current stream.  A chunk longer than ``max_chunk_samples`` (default 10 s) goes in several pieces, joined by
    one ``torch.cat``."""

    def __init__(self, rate_in: int, rate_out: int, recordings: int, channels: int = 1, channel: int = 0, device=None,
                 max_chunk_samples: int | None = None):
        self.R, self.C, self.channel = int(recordings), int(channels), int(channel)
        if not 1 <= self.R <= 65535:
            raise ValueError(f"StreamResampler: recordings must lie in 1..65535, got {recordings}")
        if self.C < 1 or not -1 <= self.channel < self.C:
            raise ValueError(f"StreamResampler: channel {channel} of {channels} channels")
        self.resampler = get_resampler(rate_in, rate_out, device)
        self.device = self.resampler.device
        self.rate_in, self.rate_out = self.resampler.rate_in, self.resampler.rate_out
        self.max_chunk = 10 * self.rate_in if max_chunk_samples is None else int(max_chunk_samples)
        if self.max_chunk < 1:
            raise ValueError("StreamResampler: max_chunk_samples must be at least 1")
        nbytes = int(_lib.lib().ake_stream_resample_state_bytes(self.resampler._h, self.R))
        if nbytes == 0:
            _lib.check(-1, "ake_stream_resample_state_bytes")
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.n = 0                                                   # inputs so far: the device keeps no count
        self.finished = False

    def out_count(self, n_in: int, finished: bool = False) -> int:
        """Outputs that are final after ``n_in`` inputs (``stream.resampled_final``)."""
        return int(_lib.lib().ake_stream_resample_out_count(self.resampler._h, int(n_in), int(finished)))

    def _checked(self, chunk):
        if not isinstance(chunk, torch.Tensor) or chunk.dtype not in (torch.float32, torch.int16):
            raise ValueError("StreamResampler.push: a chunk is a float32 or int16 (16-bit PCM) tensor")
        if chunk.dim() == 2 and self.C == 1:
            chunk = chunk[:, None, :]
        if chunk.dim() != 3 or chunk.shape[0] != self.R or chunk.shape[1] != self.C:
            raise ValueError(f"StreamResampler.push: a chunk is (R, C, m) with R = {self.R}, C = {self.C}"
                             + (" or (R, m)" if self.C == 1 else "") + f", got {tuple(chunk.shape)}")
        chunk = chunk.to(self.device)
        if chunk.dtype == torch.float32 and chunk.stride(2) != 1 and chunk.shape[2] > 1:
            chunk = chunk.contiguous()
        return chunk

    def _piece(self, chunk, finishing, out=None):
        """One call of the entry point: ``chunk`` (R, C, m) as ``_checked`` leaves it, or None -> the (R, k) outputs, written to the
        front of ``out`` (R, >= k) when that is given."""
        L = _lib.lib()
        m = 0 if chunk is None else int(chunk.shape[2])
        k = self.out_count(self.n + m, finishing) - self.out_count(self.n)
        if out is None:
            out = torch.empty((self.R, k), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.shape[0] == self.R and out.shape[1] >= k and (out.stride(1) == 1 or out.shape[1] <= 1)
        k_out = C.c_int64(-1)
        ptr = chunk.data_ptr() if m else None
        strides = chunk.stride() if m else (0, 0, 1)
        args = (self.channel, self.n, int(finishing), self.state.data_ptr(), self.state.numel(), out.data_ptr() if k else None,
                max(out.stride(0), k), C.byref(k_out))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            if m and chunk.dtype == torch.int16:
                _lib.check(L.ake_stream_resample_pcm16_f32(self.resampler._h, ptr, self.R, self.C, m, strides[0], strides[1], strides[2], *args,
                                                           stream), "ake_stream_resample_pcm16_f32")
            else:
                _lib.check(L.ake_stream_resample_f32(self.resampler._h, ptr, self.R, self.C, m, strides[0], strides[1], *args, stream),
                           "ake_stream_resample_f32")
        assert k_out.value == k
        self.n += m
        return out[:, :k]

    @torch.no_grad()
    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise ValueError("StreamResampler.push: the stream has been finished")
        chunk = self._checked(chunk)
        m = chunk.shape[2]
        if m <= self.max_chunk:
            return self._piece(chunk, False)
        return torch.cat([self._piece(chunk[:, :, a:a + self.max_chunk], False) for a in range(0, m, self.max_chunk)], dim=1)

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """The recordings end here: the outputs whose filter reaches behind the end, which see nothing there, as the offline ones do."""
        if self.finished:
            raise ValueError("StreamResampler.finish: the stream has been finished")
        out = self._piece(None, True)
        self.finished = True
        return out


def prepare(audio: torch.Tensor, rate_in: int, rate_out: int, channel: int = 0, lengths=None, device=None):
    """One call: (B, C, n) at ``rate_in`` -> mono (B, n_out) at ``rate_out`` + per-clip lengths, on the GPU."""
    dev = device if device is not None else (audio.device if audio.is_cuda else None)
    return get_resampler(rate_in, rate_out, dev)(audio, channel=channel, lengths=lengths)
