"""Key tracking on audio as it arrives: ``KeyEstimator.stream`` -> ``KeyStream``.

A stream takes the audio of R recordings in chunks, all R in lockstep, and emits ``KeyEstimator.track``'s windows exactly once each, as
soon as every frame of a window is final; a smoother with carried state (``ake_key_stream_step_f32``, host model
``metrics.key_stream``) adds the filtered key scores and a fixed-lag Viterbi path, and on request the fixed-lag posteriors and the
running log-likelihood (``ake_key_stream_posteriors_f32``, host model ``metrics.key_stream_posteriors``).  Every count is known on the host from the number of
samples pushed: a push reads nothing back from the device and waits for nothing.  Chunks in a source format (another rate, several
channels) first pass ``audio.StreamResampler``, the polyphase resampler with a carried tail (``resampled_final`` below), whose output is
the offline resampler's on the whole audio to the bit; everything here then counts samples at the estimator's rate.

``method="profile"`` streams need no net (``KeyEstimator(None, ...)``): in place of the frame cache and the net's workspace they carry a
ring of per-frame chroma, 12 doubles a frame, which ``ake_stream_frame_stats_f32`` fills from every push's new frames and
``ake_stream_profile_emissions_f32`` scores the newly complete windows from (host model ``metrics.stream_profile``, ring capacity
``metrics.stream_profile_ring_frames``).  ``tuning_meter=True`` carries ``estimate_tuning``'s three sums in the same state and the same
launch (``metrics.stream_tuning``) and reports the detuning of the audio so far with every update.  ``retune_cents=c`` puts
``tuning.StreamRetuner`` behind the resampler and in front of the history: the offline varispeed filter with a carried ring of 64 inputs
(``retune_final`` below; ``ake_stream_retune_f32``, host model ``metrics.stream_retune``), whose output is ``retune``'s on the whole audio
to the bit.  Everything here then counts retuned samples; only ``StreamUpdate.times`` are divided by ``rho`` again, and the meter reports
the detuning that is left.  ``refine=True`` places every key change to the frame inside the stream, as ``track(refine=True)`` does
offline: ``ake_stream_key_changes_f32`` reads the chroma ring (a ``"net"`` stream keeps one for it) and a carried ring of labels, and
computes the boundaries a push made final -- ``metrics.stream_changes_ready`` on the host's counts; host model
``metrics.stream_key_changes`` -- into ``StreamUpdate.change_frame`` and its kin: joined, ``ake_amd.key_changes`` on the stream's own
frames and labels to the bit.  Not built: automatic retuning inside a stream (the number of cents is the caller's: taking it from the
stream's own meter needs a read-back or a ratio that changes in mid-stream), chunk lengths that differ between recordings, a weighting
of the bins.

The geometry, as pure host functions (``H`` = ``ake_cqt_plan_half_support``: frame t depends on samples ``[t*hop - H, t*hop + H]``):

- ``final_frames``: with N samples received, frame t is final iff ``t*hop + H <= N - 1``; at the end all ``1 + N // hop`` frames are.
- ``windows_ready``: ``track_counts`` of the final frames -- window w covers frames ``[w*sf, w*sf + wf)``.
- ``transform_start``: new final frames come from re-transforming ``[s0, N)`` of a float32 audio history with the offline entry
  points; ``s0`` is the largest multiple of ``hop`` at or below ``first_needed_frame*hop - H`` (0 at the start of the stream, whose
  frames then see the zeros in front of sample 0 that ``track``'s see).  ``s0`` is NOT held to a multiple of ``2**(octaves - 1)``: that
  would make the decimation grids of the streamed and the offline transform coincide, but with hop 4410 the two conditions meet only
  every 64 hops (12.8 s), which a push would have to re-transform.  Streamed frames therefore equal offline frames to the transform's
  own accuracy (its float64 oracle bound), not to the bit; ``profiles/track_stream.md`` has the measured difference.
"""
from __future__ import annotations

from dataclasses import dataclass

import ctypes as C

import torch

from . import _lib, metrics
from .audio import StreamResampler
from .tuning import StreamRetuner
from .pipeline import track_counts, track_stride_frames, track_window_frames


def final_frames(n_samples: int, hop: int, half_support: int, finished: bool = False) -> int:
    """Frames of the transform that are final after ``n_samples`` samples: frame t is final iff ``t*hop + H <= n_samples - 1``; at the
    end of the recording (``finished``) all ``1 + n_samples // hop`` are, seeing zeros behind the end as ``track``'s frames do."""
    n_samples, hop, half_support = int(n_samples), int(hop), int(half_support)
    if finished:
        return 1 + n_samples // hop
    return 0 if n_samples - 1 - half_support < 0 else (n_samples - 1 - half_support) // hop + 1


def windows_ready(frames: int, window_frames: int, stride_frames: int) -> int:
    """Windows all of whose frames lie among the first ``frames`` final frames (``track_counts``)."""
    return track_counts(int(frames), int(window_frames), int(stride_frames))


def transform_start(first_frame: int, hop: int, half_support: int) -> int:
    """``s0``: the sample a re-transform starts at so that frame ``first_frame`` and everything behind it see their whole support --
    the largest multiple of ``hop`` at or below ``first_frame*hop - H``, never below 0."""
    first_frame, hop, half_support = int(first_frame), int(hop), int(half_support)
    return max(0, (first_frame * hop - half_support) // hop) * hop


smooth_count = metrics.key_stream_count      # (windows_before, k, lag, flush) -> (first smoothed window, k_out)

# a stream opened with source_rate / source_channels resamples in front of its history (ake_stream_resample_f32): the geometry
resampled_final = metrics.resampled_final            # (n_in, up, down, half, finished=False) -> outputs that are final
resample_first_input = metrics.resample_first_input  # (k, up, down, half) -> the first input output k reads
resample_tail = metrics.resample_tail                # (n_in, up, down, half) -> inputs still to be held, <= 2*half // up

# a stream opened with retune_cents retunes behind that, in front of its history (ake_stream_retune_f32): the geometry
retune_final = metrics.retune_final                  # (n_in, rho, finished=False) -> outputs that are final
retune_tail = metrics.retune_tail                    # (n_in, rho) -> inputs still to be held, <= 63


@dataclass
class StreamUpdate:
    """What one ``KeyStream.push`` (or ``finish``) emits: ``windows`` = k new windows from ``first_window`` on.

    ``key`` (R, k, 12), ``tonic`` (R, k, 12), ``genre`` (R, k, 11) or None, ``key_id``, ``signature_id``, ``tonic_id`` int32 (R, k) and
    ``confidence`` (R, k): as ``KeyTrack`` names them (``signature_id`` is ``KeyTrack.sig``).  ``times`` (k,) float64 on the host: window
    centres in seconds, as ``KeyTrack.times``.  A smooth stream adds ``emissions`` (R, k, 24), ``filtered`` (R, k, 24) -- the normalised
    log forward scores: ``exp`` is the probability of each key given the audio so far -- and the fixed-lag path ``smooth_key_id`` int32
    (R, k2) for the k2 windows from ``smooth_first_window`` on that have left the lag; None on a stream without a smoother.  A stream
    opened with ``posteriors=True`` adds ``posteriors`` (R, k2, 24) and ``smooth_confidence`` (R, k2) for those k2 windows -- the
    probability of each key given the audio up to ``lag_windows`` windows later, and its entry at ``smooth_key_id`` -- and
    ``log_likelihood`` (R, k), the running log-score after each new window; None otherwise.

    On a ``method="profile"`` stream the fields hold what ``KeyTrack`` documents for that method: ``key`` is the window's chroma,
    ``tonic`` the larger of each tonic's two emissions, ``genre`` None, ``confidence`` the winning correlation, and ``emissions`` is
    always there, also with ``smooth=False``.  A stream opened with ``tuning_meter=True`` adds ``tuning_cents`` and ``tuning_strength``,
    float32 (R,): the detuning estimate over every final frame so far (zeros before the first frame); None otherwise.

    A stream opened with ``retune_cents`` carries that number (float32-rounded, as the kernel reads it) in ``retune_cents``; its ``times``
    are divided by ``rho``, so they are seconds of the recording as it was pushed, not of its retuned copy, and its meter reports the
    detuning that is left.  None on a stream opened without the keyword.

    A stream opened with ``refine=True`` adds where the key changes, to the frame, for the b boundaries from ``change_first_boundary``
    on that this update made final (boundary w lies between the windows w and w + 1; ``metrics.stream_changes_ready``):
    ``change_frame`` int32 (R, b), the frame of the stream -- not of the push -- from which the key of window w + 1 holds, or -1 where
    the two windows do not carry two different keys, ``change_gain`` and ``change_contrast`` (R, b) as ``KeyTrack`` names them, and
    ``change_times`` float64 (R, b), ``change_frame * hop / sample_rate`` in seconds of the recording as it was pushed (divided by
    ``rho`` under ``retune_cents``; negative where ``change_frame`` is -1).  None on a stream opened without the keyword."""
    first_window: int
    windows: int
    key: torch.Tensor
    tonic: torch.Tensor
    genre: torch.Tensor | None
    key_id: torch.Tensor
    signature_id: torch.Tensor
    tonic_id: torch.Tensor
    confidence: torch.Tensor
    times: torch.Tensor
    emissions: torch.Tensor | None = None
    filtered: torch.Tensor | None = None
    smooth_first_window: int | None = None
    smooth_key_id: torch.Tensor | None = None
    posteriors: torch.Tensor | None = None
    smooth_confidence: torch.Tensor | None = None
    log_likelihood: torch.Tensor | None = None
    tuning_cents: torch.Tensor | None = None
    tuning_strength: torch.Tensor | None = None
    retune_cents: float | None = None
    change_first_boundary: int | None = None
    change_frame: torch.Tensor | None = None
    change_gain: torch.Tensor | None = None
    change_contrast: torch.Tensor | None = None
    change_times: torch.Tensor | None = None

    @staticmethod
    def concat(parts):
        """One update out of the consecutive updates of a push that was cut into pieces (the tuning meter's value: the last piece's)."""
        if len(parts) == 1:
            return parts[0]
        cat = lambda name: None if getattr(parts[0], name) is None else torch.cat([getattr(p, name) for p in parts], dim=1)
        return StreamUpdate(parts[0].first_window, sum(p.windows for p in parts), cat("key"), cat("tonic"), cat("genre"), cat("key_id"),
                            cat("signature_id"), cat("tonic_id"), cat("confidence"), torch.cat([p.times for p in parts]), cat("emissions"),
                            cat("filtered"), parts[0].smooth_first_window, cat("smooth_key_id"), cat("posteriors"), cat("smooth_confidence"),
                            cat("log_likelihood"), parts[-1].tuning_cents, parts[-1].tuning_strength, parts[0].retune_cents,
                            parts[0].change_first_boundary, cat("change_frame"), cat("change_gain"), cat("change_contrast"), cat("change_times"))


class KeyStream:
    """``KeyEstimator.stream(...)``: see there.  ``push(chunk)`` and ``finish()`` return a ``StreamUpdate``.

    Everything a push needs between calls is sized here, from R, the window geometry, ``lag_windows`` and ``max_chunk_samples``: the
    audio history (float32, ``2*H + hop + max_chunk_samples`` samples a recording), the transform's output and workspace, the two
    halves of the frame cache, the net's workspace, the smoother's state and, with ``posteriors``, the posteriors' state.  A
    ``method="profile"`` stream has neither frame cache nor net workspace: in their place stands the state of
    ``ake_stream_frame_stats_f32``, a ring of ``window_frames + max_mel`` rows of per-frame chroma (96 bytes a frame) and three sums for
    the tuning meter.  ``refine=True`` lengthens that ring to the larger of the two rules (``metrics.stream_profile_ring_frames``,
    ``metrics.stream_changes_ring_frames``; a ``"net"`` stream then has the ring too) and adds a ring of labels
    (``metrics.stream_changes_labels_carried`` + a piece's new ones).  After the first push a push allocates only the tensors
    it returns (a chunk longer than ``max_chunk_samples`` is pushed as several pieces, whose updates are joined by one ``torch.cat``
    each).  ``push`` runs on the current stream.

    With ``source_rate`` / ``source_channels`` a ``StreamResampler`` stands in front of the history: a push first resamples its chunk
    (``max_chunk_samples`` source samples at a time) into a buffer sized here, and what that made final goes the way of a mono chunk.
    With ``retune_cents`` a ``StreamRetuner`` stands behind it (or alone): what it makes final of a mono piece, in a second buffer sized
    here, is what the history gets, and ``max_chunk_samples`` counts the samples in front of it."""

    resampler = None                                                 # the StreamResampler of a stream with a source format
    retuner = None                                                   # the StreamRetuner of a stream with retune_cents

    def __init__(self, est, recordings, window_seconds=15.0, stride_seconds=5.0, smooth=True, lag_windows=6, mean_key_seconds=60.0,
                 transition=None, log_prior=None, signature_weight=1.0, keep_frames=False, max_chunk_samples=None, posteriors=False,
                 source_rate=None, source_channels=None, channel=0, method="net", profiles="krumhansl", compression="log",
                 profile_sharpness=10.0, tuning_meter=False, tuning_min_strength=0.0, retune_cents=None, refine=False,
                 refine_slack_seconds=None):
        R = int(recordings)
        if R < 1:
            raise ValueError("stream: recordings must be at least 1")
        lag = int(lag_windows)
        if not 0 <= lag <= 255:
            raise ValueError(f"stream: lag_windows must lie in 0..255, got {lag_windows}")
        if method not in ("net", "profile"):
            raise ValueError('stream: method must be "net" or "profile"')
        self.profile = method == "profile"
        if self.profile:
            est._refuse_unprofilable('stream(method="profile")')
            if float(signature_weight) != 1.0:
                raise ValueError('stream(method="profile"): signature_weight weighs the net\'s key head, which this method does not run; leave it at 1')
            self.mode = metrics._profile_compression(compression)
            self.sharpness = float(profile_sharpness)
            if not self.sharpness > 0.0:
                raise ValueError('stream(method="profile"): profile_sharpness must be positive')
        else:
            est._need_net('KeyEstimator.stream(method="net")')
            est._refuse_untrackable()
        self.refine = bool(refine)
        if self.refine and not self.profile:                         # (the chroma the boundaries are placed by: compression as for the profile method)
            self.mode = metrics._profile_compression(compression)
        self.meter, self.min_strength = bool(tuning_meter), float(tuning_min_strength)
        if self.meter and self.min_strength != self.min_strength:
            raise ValueError("stream: tuning_min_strength is NaN")
        if posteriors and not smooth:
            raise ValueError("stream: posteriors=True needs smooth=True (the posteriors are the smoother's)")
        self.est, self.R, self.lag, self.smooth, self.posteriors = est, R, lag, bool(smooth), bool(posteriors)
        dev = self.device = est.device
        L = _lib.lib()
        plan, net = est.plan, est.net
        if not self.profile:
            net._sync_weights(dev, for_eval=True)
        hop = self.hop = int(plan.hop_length)
        self.wf = track_window_frames(int(round(window_seconds * est.sample_rate)), hop)
        self.sf = track_stride_frames(stride_seconds, est.frames)
        self.H = int(L.ake_cqt_plan_half_support(plan.handle))
        if self.H < 0:
            _lib.check(-1, "ake_cqt_plan_half_support")
        # ---- the source: chunks at another rate or with several channels pass a resampler with carried state first ----
        rate_in = est.sample_rate if source_rate is None else int(source_rate)
        channels = 1 if source_channels is None else int(source_channels)
        if rate_in < 1 or channels < 1 or not -1 <= int(channel) < channels:
            raise ValueError(f"stream: source_rate {source_rate}, source_channels {source_channels}, channel {channel}")
        self.resampler = None
        if rate_in != est.sample_rate or channels > 1:
            # max_chunk_samples counts source samples; the history takes what a piece of that many can make final (no more than
            # ceil(m*up / down)), or what finish() adds behind the last piece (fewer than (half + 1) / down + 2)
            src_max = 10 * rate_in if max_chunk_samples is None else int(max_chunk_samples)
            if src_max < 1:
                raise ValueError("stream: max_chunk_samples must be at least 1")
            up, down, half = metrics.resample_ratio(rate_in, est.sample_rate)
            self.resampler = StreamResampler(rate_in, est.sample_rate, R, channels, int(channel), dev, src_max)
            max_chunk_samples = max(resampled_final(src_max, up, down, half, True), (half + 1) // down + 2)
            self.resampled = torch.empty((R, max_chunk_samples), dtype=torch.float32, device=dev)
        # ---- the retuner: behind the resampler, in front of the history; everything from here on counts retuned samples ----
        self.retuner, self.retune_cents, self.rho = None, None, 1.0
        if retune_cents is not None:
            if isinstance(retune_cents, (bool, str, torch.Tensor)) or not abs(float(retune_cents)) <= metrics.RETUNE_MAX_CENTS:
                raise ValueError(f"stream: retune_cents is one number within +-{metrics.RETUNE_MAX_CENTS:g} cents for all recordings (they "
                                 f"advance in lockstep), got {retune_cents!r}")
            self.retune_cents = float(retune_cents)
        if self.retune_cents:                                        # (None and 0: the stream as it is without a retuner)
            est._refuse_unretunable("stream(retune_cents=...)")
            in_max = 10 * est.sample_rate if max_chunk_samples is None else int(max_chunk_samples)      # what a piece hands the retuner at most
            if in_max < 1:
                raise ValueError("stream: max_chunk_samples must be at least 1")
            self.retuner = StreamRetuner(self.retune_cents, R, dev, in_max)
            self.retune_cents, self.rho = self.retuner.cents, self.retuner.rho
            # m inputs make at most m*rho + 2 outputs final (each of the two counts lies within one of its real value), finish() at
            # most Z*rho + 1 more
            max_chunk_samples = metrics.retune_out_len(in_max) + 2 * metrics.RETUNE_ZEROS
            self.retuned = torch.empty((R, max_chunk_samples), dtype=torch.float32, device=dev)
        self.max_chunk =10 * est.sample_rate if max_chunk_samples is None else int(max_chunk_samples)
        if self.max_chunk < 1:
            raise ValueError("stream: max_chunk_samples must be at least 1")
        self.signature_weight = float(signature_weight)
        self.trans = est._transition(self.sf, mean_key_seconds, transition) if self.smooth else None
        self.prior = None
        if self.smooth and log_prior is not None:
            prior = torch.as_tensor(log_prior).detach()
            if tuple(prior.shape) != (24,):
                raise ValueError("stream: log_prior must hold 24 log-probabilities")
            metrics._check_finite("log_prior", prior)
            self.prior = prior.to(device=dev, dtype=torch.float32).contiguous()
        self.P = int(plan.n_bins)
        self.fm = bool(L.ake_cqt_frames_major_supported(plan.handle))
        # what the stream has seen: samples, final frames, emitted windows -- host integers all
        self.N = self.F = self.W = 0
        self.s0 = 0                                                  # the history's first sample
        self.finished = False
        fed = self.resampler is not None or self.retuner is not None
        self.dtype = torch.float32 if fed else None                  # (what the history is fed: the resampler's or the retuner's output)
        # the history holds [s0, N): at most 2H + hop samples survive a push (frame F is not final, so N <= F*hop + H, and
        # s0 > F*hop - H - hop), and a piece adds at most max_chunk
        self.hist_cap = (2 * self.H + hop + self.max_chunk + 3) // 4 * 4
        self.max_mel = 1 + self.hist_cap // hop                      # frames of the longest re-transform
        self.cache_cap = self.wf + self.max_mel                      # fewer than wf frames survive a push
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self.hist = f32(R, self.hist_cap)
        self.mel = f32(R * self.P * self.max_mel)
        self.cache = None if self.profile else [f32(R * self.P * self.cache_cap), f32(R * self.P * self.cache_cap)]
        # which half is current, the stream's frame it begins at (W * sf: ahead of F when the stride skips frames) and the frames it holds
        self.cache_at, self.cache_start, self.cache_frames = 0, 0, 0
        with torch.cuda.device(dev):
            cqt_bytes = max(int(L.ake_cqt_workspace_bytes(plan.handle, R, n)) for n in (self.hist_cap, self.hist_cap // 2, hop))
            net_bytes = None if self.profile else max(int(L.ake_pcnet_forward_windows_workspace_bytes(net.handle, R, t, self.wf, self.sf))
                                                      for t in (self.cache_cap, self.wf))
        if cqt_bytes == 0 or net_bytes == 0:
            _lib.check(-1, "stream: workspace query")
        self.cqt_ws = torch.empty(cqt_bytes, dtype=torch.uint8, device=dev)
        self.net_ws = None if self.profile else torch.empty(net_bytes, dtype=torch.uint8, device=dev)
        # ---- the profile method's chroma ring and the tuning meter's sums (ake_stream_frame_stats_f32): a piece brings at most max_mel frames
        # refine=True: the boundaries are placed from the same ring (ake_stream_key_changes_f32), which then holds the larger of the two
        # rules' rows; the labels trail the windows by the lag where the smoother decides them
        self.slack = None
        if self.refine:
            self.slack = self.sf if refine_slack_seconds is None else int(round(float(refine_slack_seconds) * est.frames))
            if self.slack < 0:
                raise ValueError("stream(refine=True): refine_slack_seconds must not be negative")
            from . import keychanges
            keychanges.check_span(self.sf, self.slack)
        self.stats_parts = (1 if self.profile or self.refine else 0) | (2 if self.meter else 0)
        self.stats_state = self.tuning = None
        if self.stats_parts:
            self.ring_frames = max(metrics.stream_profile_ring_frames(self.wf, self.max_mel) if self.profile else 1,
                                   metrics.stream_changes_ring_frames(self.wf, self.sf, self.slack, lag if self.smooth else 0, self.max_mel)
                                   if self.refine else 1)
            nbytes = int(L.ake_stream_profile_state_bytes(R, self.ring_frames))
            if nbytes == 0:
                _lib.check(-1, "ake_stream_profile_state_bytes")
            self.stats_state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if self.meter:
            self.tuning = (torch.zeros(R, dtype=torch.float32, device=dev), torch.zeros(R, dtype=torch.float32, device=dev))
        if self.profile or self.refine:
            from . import keyprofile
            self.prof = keyprofile.device_profiles(profiles, dev)
        if self.profile:
            self.key_sig = est._key_sig_table(dev)
        # the labels of the windows a boundary still needs, int32 (R, label_ring): those carried between pieces and a piece's new ones
        # (at most one per stride of new frames, and the lag's at the flush), so the slots a piece reads and writes cannot meet
        self.L = self.B = 0                                          # decided labels, final boundaries -- host integers
        self.label_state = None
        if self.refine:
            self.label_ring = metrics.stream_changes_labels_carried(self.wf, self.sf, self.slack) + (self.max_mel + self.sf - 1) // self.sf + lag
            nbytes = int(L.ake_stream_key_changes_state_bytes(R, self.label_ring))
            if nbytes == 0:
                _lib.check(-1, "ake_stream_key_changes_state_bytes")
            self.label_state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.state = None
        if self.smooth:
            self.state = torch.empty(max(int(L.ake_key_stream_state_bytes(R, lag)), 16), dtype=torch.uint8, device=dev)
        self.post_state = None
        if self.posteriors:
            self.post_state = torch.empty(int(L.ake_key_stream_posteriors_state_bytes(R, lag)), dtype=torch.uint8, device=dev)
        self.keep_frames = bool(keep_frames)
        self._frames = [] if keep_frames else None

    @property
    def frames(self):
        """``keep_frames=True``: every final frame so far, (R, P, T) float32 (for tests and debugging)."""
        if self._frames is None:
            raise ValueError("KeyStream.frames: the stream was opened without keep_frames=True")
        if not self._frames:
            return torch.empty((self.R, self.P, 0), dtype=torch.float32, device=self.device)
        if len(self._frames) > 1:
            self._frames = [torch.cat(self._frames, dim=2)]
        return self._frames[0]

    @torch.no_grad()
    def push(self, chunk: torch.Tensor) -> StreamUpdate:
        """(R, m) float32 or int16 (16-bit PCM, sample / 32768) at the estimator's rate, any m >= 0 -> ``StreamUpdate``.  A stream
        opened with ``source_rate`` / ``source_channels`` takes (R, C, m) chunks at that rate instead ((R, m) with one channel; int16 with
        any strides, so interleaved storage goes in as ``buf.transpose(1, 2)``): they pass the carried resampler, and what that makes
        final goes the way of a mono chunk.  On a stream opened with ``retune_cents`` the mono audio then passes the carried retuner, which
        takes float32 and int16 chunks in any order."""
        if self.finished:
            raise ValueError("KeyStream.push: the stream has been finished")
        if self.resampler is not None:
            self._sync_weights()
            chunk = self.resampler._checked(chunk)
            step = self.resampler.max_chunk
            return StreamUpdate.concat([self._through(self.resampler._piece(chunk[:, :, a:a + step], False, out=self.resampled))
                                        for a in range(0, max(chunk.shape[2], 1), step)])
        if not isinstance(chunk, torch.Tensor) or chunk.dim() != 2 or chunk.shape[0] != self.R:
            raise ValueError(f"KeyStream.push: a chunk is (R, m) with R = {self.R}: mono audio at the estimator's rate (open the stream "
                             "with source_rate / source_channels for anything else: it then resamples and picks channels with carried state)")
        if chunk.dtype not in (torch.float32, torch.int16):
            raise ValueError("KeyStream.push: a chunk is float32 or int16 (16-bit PCM)")
        if self.retuner is not None:                                 # (the history is fed float32 whatever arrives)
            self._sync_weights()
            chunk = self.retuner._checked(chunk)
            step = self.retuner.max_chunk
            return StreamUpdate.concat([self._through(chunk[:, a:a + step]) for a in range(0, max(chunk.shape[1], 1), step)])
        if self.dtype is None:
            self.dtype = chunk.dtype
        elif chunk.dtype != self.dtype:
            raise ValueError(f"KeyStream.push: this stream takes {self.dtype} chunks, got {chunk.dtype}")
        self._sync_weights()
        chunk = chunk.to(self.device)
        if chunk.stride(1) != 1 and chunk.shape[1] > 1:
            chunk = chunk.contiguous()
        m = chunk.shape[1]
        if m <= self.max_chunk:
            return self._piece(chunk, False)
        return StreamUpdate.concat([self._piece(chunk[:, a:a + self.max_chunk], False) for a in range(0, m, self.max_chunk)])

    def _through(self, mono):
        """A mono piece at the estimator's rate -> its update, by way of the retuner where the stream has one."""
        if self.retuner is not None:
            mono = self.retuner._piece(mono, False, out=self.retuned)
        return self._piece(mono, False)

    def _sync_weights(self):
        if not self.profile:
            self.est.net._sync_weights(self.device, for_eval=True)

    @torch.no_grad()
    def finish(self) -> StreamUpdate:
        """The recording ends here: the rest of the windows (every frame is final now, seeing zeros behind the end as ``track``'s do)
        and the rest of the smoothed path."""
        if self.finished:
            raise ValueError("KeyStream.finish: the stream has been finished")
        parts = []
        if self.resampler is not None:                               # first what the resampler still held back
            rest = self.resampler._piece(None, True, out=self.resampled)
            self.resampler.finished = True
            if rest.shape[1]:
                parts.append(self._through(rest))
        if self.retuner is not None:                                 # then what the retuner still held back
            rest = self.retuner._piece(None, True, out=self.retuned)
            self.retuner.finished = True
            if rest.shape[1]:
                parts.append(self._piece(rest, False))
        parts.append(self._piece(None, True))
        self.finished = True
        return StreamUpdate.concat(parts)

    def _piece(self, chunk, finishing):
        L, dev, R, hop, P = _lib.lib(), self.device, self.R, self.hop, self.P
        m = 0 if chunk is None else int(chunk.shape[1])
        # ---- the counts of this piece, all on the host ----
        N = self.N + m
        F = final_frames(N, hop, self.H, finishing)
        s0 = transform_start(self.F, hop, self.H)                    # where the history must begin for frames F_old.. (>= self.s0)
        new_frames = F - self.F
        nw = windows_ready(F, self.wf, self.sf)
        k = nw - self.W
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            # ---- the history: [s0, N) ----
            drop, keep = s0 - self.s0, self.N - s0
            hist = L.ake_stream_history_pcm16 if self.dtype == torch.int16 else L.ake_stream_history_f32
            _lib.check(hist(self.hist.data_ptr(), R, self.hist_cap, drop, keep, chunk.data_ptr() if m else None,
                            (chunk.stride(0) if R > 1 else m) if m else 0, m, stream), "ake_stream_history")
            self.s0, self.N = s0, N
            # ---- the new final frames, from a re-transform of the history ----
            n = N - s0
            if new_frames > 0 and n > 0:
                T = 1 + n // hop
                if self.fm:
                    _lib.check(L.ake_cqt_logmag_frames_major_f32(self.est.plan.handle, self.hist.data_ptr(), R, n, self.hist_cap, self.mel.data_ptr(),
                                                                 self.cqt_ws.data_ptr(), self.cqt_ws.numel(), stream), "ake_cqt_logmag_frames_major_f32")
                else:
                    _lib.check(L.ake_cqt_logmag_f32(self.est.plan.handle, self.hist.data_ptr(), R, n, self.hist_cap, self.mel.data_ptr(), T,
                                                    self.cqt_ws.data_ptr(), self.cqt_ws.numel(), stream), "ake_cqt_logmag_f32")
                first = self.F - s0 // hop                           # the transform's frame of the stream's frame F_old
                assert 0 <= first and first + new_frames <= T
                # ---- the frame cache: what it holds, then the new frames (those no window needs left out), into the other half ----
                skip = min(new_frames, max(0, self.cache_start - self.F))
                if self.stats_parts:                                 # the chroma of every new frame into its ring row, the meter's sums
                    if self.meter:
                        self.tuning = (f32(R), f32(R))
                    _lib.check(L.ake_stream_frame_stats_f32(self.mel.data_ptr(), int(self.fm), R, P, T, first, new_frames, self.F, self.ring_frames,
                                                            self.stats_parts, self.mode if self.stats_parts & 1 else 0, self.min_strength,
                                                            self.stats_state.data_ptr(), self.stats_state.numel(),
                                                            self.tuning[0].data_ptr() if self.meter else None,
                                                            self.tuning[1].data_ptr() if self.meter else None, stream), "ake_stream_frame_stats_f32")
                if not self.profile and new_frames > skip:
                    assert self.cache_frames + new_frames - skip <= self.cache_cap
                    dst, old = self.cache[1 - self.cache_at], self.cache[self.cache_at]
                    _lib.check(L.ake_stream_frames_f32(dst.data_ptr(), old.data_ptr(), self.mel.data_ptr(), int(self.fm), R, P, self.cache_frames, 0,
                                                       self.cache_frames, T, first + skip, new_frames - skip, stream), "ake_stream_frames_f32")
                    self.cache_at, self.cache_frames = 1 - self.cache_at, self.cache_frames + new_frames - skip
                if self._frames is not None:
                    mel = self.mel[:R * P * T]
                    mel = mel.view(R, T, P).transpose(1, 2) if self.fm else mel.view(R, P, T)
                    self._frames.append(mel[:, :, first:first + new_frames].clone())
            elif new_frames > 0:                                     # finish() on a stream that never got a sample: nothing to transform
                new_frames, F, k = 0, self.F, 0
            self.F = F
            # ---- the newly complete windows: one call of the net over the cached frames ----
            key, tonic, genre = f32(R, k, 12), f32(R, k, 12), f32(R, k, 11) if not self.profile and self.est.net.genre else None
            key_id, sig, tonic_id, conf = i32(R, k), i32(R, k), i32(R, k), f32(R, k)
            times = (torch.arange(self.W, self.W + k, dtype=torch.float64) * self.sf + (self.wf - 1) / 2) * hop / self.est.sample_rate
            if self.retuner is not None:                             # seconds of the recording as it was pushed
                times = times / self.rho
            up = StreamUpdate(self.W, k, key, tonic, genre, key_id, sig, tonic_id, conf, times, retune_cents=self.retune_cents)
            if self.meter:
                up.tuning_cents, up.tuning_strength = self.tuning
            if self.profile:                                         # one launch scores the new windows from the ring
                up.emissions = f32(R, k, 24)
                _lib.check(L.ake_stream_profile_emissions_f32(self.stats_state.data_ptr(), self.stats_state.numel(), R, self.ring_frames, self.F,
                                                              self.wf, self.sf, self.W, k, self.prof.data_ptr(), self.sharpness,
                                                              self.key_sig.data_ptr(), key.data_ptr(), up.emissions.data_ptr(), key_id.data_ptr(),
                                                              conf.data_ptr(), tonic.data_ptr(), tonic_id.data_ptr(), sig.data_ptr(), stream),
                           "ake_stream_profile_emissions_f32")
            elif k > 0:
                cur = self.cache[self.cache_at]
                assert self.cache_start == self.W * self.sf and track_counts(self.cache_frames, self.wf, self.sf) == k
                _lib.check(L.ake_pcnet_forward_windows_f32(self.est.net.handle, cur.data_ptr(), int(self.fm), R, self.cache_frames, self.wf, self.sf,
                                                           key.data_ptr(), tonic.data_ptr(), genre.data_ptr() if genre is not None else None,
                                                           self.net_ws.data_ptr(), self.net_ws.numel(), stream), "ake_pcnet_forward_windows_f32")
                _lib.check(L.ake_decode_keys_f32(key.data_ptr(), tonic.data_ptr(), R * k, None, 1, key_id.data_ptr(), sig.data_ptr(),
                                                 tonic_id.data_ptr(), conf.data_ptr(), stream), "ake_decode_keys_f32")
                # the tail later windows still need slides to the front (of the other half): the cache begins at frame W * sf again
                left = max(0, self.cache_frames - k * self.sf)        # (a stride longer than a window leaves none, and skips some to come)
                dst = self.cache[1 - self.cache_at]
                _lib.check(L.ake_stream_frames_f32(dst.data_ptr(), cur.data_ptr(), None, int(self.fm), R, P, self.cache_frames,
                                                   self.cache_frames - left, left, 0, 0, 0, stream), "ake_stream_frames_f32")
                self.cache_at, self.cache_start, self.cache_frames = 1 - self.cache_at, self.cache_start + k * self.sf, left
            # ---- the smoother ----
            if self.smooth:
                first_s, k2 = smooth_count(self.W, k, self.lag, finishing)
                up.filtered = f32(R, k, 24)
                up.smooth_first_window, up.smooth_key_id = first_s, i32(R, k2)
                if not self.profile:
                    up.emissions = f32(R, k, 24)
                if k > 0 and not self.profile:
                    _lib.check(L.ake_key_emissions_f32(key.data_ptr(), tonic.data_ptr(), R * k, None, 1, self.signature_weight,
                                                       up.emissions.data_ptr(), stream), "ake_key_emissions_f32")
                if k > 0 or k2 > 0:
                    k_out = C.c_int(-1)
                    _lib.check(L.ake_key_stream_step_f32(up.emissions.data_ptr() if k else None, R, k, self.W, self.lag, int(finishing),
                                                         self.trans.data_ptr(), self.prior.data_ptr() if self.prior is not None else None,
                                                         self.state.data_ptr(), self.state.numel(), up.filtered.data_ptr() if k else None,
                                                         up.smooth_key_id.data_ptr() if k2 else None, C.byref(k_out), stream),
                               "ake_key_stream_step_f32")
                    assert k_out.value == k2
                if self.posteriors:
                    up.posteriors, up.smooth_confidence, up.log_likelihood = f32(R, k2, 24), f32(R, k2), f32(R, k)
                    if k > 0 or k2 > 0:
                        k_out = C.c_int(-1)
                        _lib.check(L.ake_key_stream_posteriors_f32(up.emissions.data_ptr() if k else None, up.filtered.data_ptr() if k else None,
                                                                   R, k, self.W, self.lag, int(finishing), self.trans.data_ptr(),
                                                                   self.prior.data_ptr() if self.prior is not None else None,
                                                                   up.smooth_key_id.data_ptr() if k2 else None, self.post_state.data_ptr(),
                                                                   self.post_state.numel(), up.posteriors.data_ptr() if k2 else None,
                                                                   up.smooth_confidence.data_ptr() if k2 else None,
                                                                   up.log_likelihood.data_ptr() if k else None, C.byref(k_out), stream),
                                   "ake_key_stream_posteriors_f32")
                        assert k_out.value == k2
            self.W += k
            # ---- the boundaries this piece made final, placed to the frame from the chroma ring ----
            if self.refine:
                labels = up.smooth_key_id if self.smooth else key_id
                k_l = labels.shape[1]
                B = metrics.stream_changes_ready(self.L + k_l, self.F, self.wf, self.sf, self.slack, finishing)
                b = B - self.B
                up.change_first_boundary, up.change_frame, up.change_gain, up.change_contrast = self.B, i32(R, b), f32(R, b), f32(R, b)
                if k_l > 0 or b > 0:
                    _lib.check(L.ake_stream_key_changes_f32(self.stats_state.data_ptr(), self.stats_state.numel(), R, self.ring_frames, self.F,
                                                            labels.data_ptr() if k_l else None, k_l, self.L, int(finishing), self.wf, self.sf,
                                                            self.slack, self.prof.data_ptr(), self.label_state.data_ptr(),
                                                            self.label_state.numel(), self.label_ring, self.B, b,
                                                            up.change_frame.data_ptr() if b else None, up.change_gain.data_ptr() if b else None,
                                                            up.change_contrast.data_ptr() if b else None, stream), "ake_stream_key_changes_f32")
                up.change_times = up.change_frame.to(torch.float64) * hop / self.est.sample_rate
                if self.retuner is not None:                         # seconds of the recording as it was pushed
                    up.change_times = up.change_times / self.rho
                self.L, self.B = self.L + k_l, B
        return up
