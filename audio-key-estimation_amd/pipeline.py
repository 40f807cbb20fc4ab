"""Whole hot path in one call: waveforms on the GPU -> (key, tonic[, genre]).

Host wrapper of ``ake_pipeline_forward_f32``: CQT, seq_length fill and the network run back
to back on one stream with no host round trip (what ``DatasetLoader.get_all`` ->
``KeyDataset.__getitem__`` -> ``PitchClassNet.forward`` do in the reference, KeyDataset.py:469-509,
242-256, models.py:846).
"""
from __future__ import annotations

from dataclasses import dataclass

import math

import torch

from . import _lib, keychanges as _keychanges, keyprofile as _keyprofile, metrics, tuning as _tuning
from .audio import get_resampler, pcm16_rows
from .cqt import WHOLE_SONG_FRAMES, CQTPlan, get_any_hop_plan, hop_for, hop_for_window
from .models import PitchClassNet


def track_window_frames(window_samples: int, hop: int) -> int:
    """Frames of one tracking window: the framing of a clip of that many samples (``ake_cqt_num_frames``)."""
    return 1 + int(window_samples) // int(hop)


def track_stride_frames(stride_seconds: float, frames: int) -> int:
    """Frames between the starts of consecutive windows (``frames`` = the estimator's frames per second)."""
    return max(1, int(round(float(stride_seconds) * frames)))


def track_counts(total_frames, window_frames: int, stride_frames: int):
    """Windows of a recording of ``total_frames`` frames (int or integer tensor): 0 if it is shorter than one window."""
    if isinstance(total_frames, torch.Tensor):
        n = torch.div(total_frames - window_frames, stride_frames, rounding_mode="floor") + 1
        return torch.where(total_frames < window_frames, torch.zeros_like(n), n)
    return 0 if total_frames < window_frames else (int(total_frames) - window_frames) // stride_frames + 1


@dataclass
class KeyAnnotations:
    """Key labels of R recordings over time, on the device: what ``KeyTrack.score`` scores a track against.

    ``seg_start`` int64 (R, S): the segments' first samples, ascending, segment 0 at sample 0; ``seg_key`` int32 (R, S): their keys in
    ``metrics.KEY_NAMES`` order, -1 for an unlabelled stretch; ``seg_count`` int32 (R,).  Behind a recording's count the starts hold
    INT64_MAX and the keys -1.  A segment lasts until the next one starts, the last one to the end of the recording."""
    seg_start: torch.Tensor
    seg_key: torch.Tensor
    seg_count: torch.Tensor
    sample_rate: int = 0

    @classmethod
    def from_segments(cls, segments, sample_rate, device="cpu"):
        """``segments``: for every recording a list of ``(start_seconds, key)``, ``key`` an id 0..23, -1 (unlabelled) or a name of
        ``metrics.KEY_NAMES`` ("A minor").  Starts become samples as ``round(start_seconds * sample_rate)``.  ``ValueError`` unless
        segment 0 starts at 0 and the starts are strictly ascending (in samples); a recording may have no segments at all."""
        rows = []
        for r, segs in enumerate(segments):
            starts, keys = [], []
            for start_s, key in segs:
                if isinstance(key, str):
                    if key not in metrics.KEY_NAMES:
                        raise ValueError(f"KeyAnnotations: recording {r}: unknown key name {key!r} (metrics.KEY_NAMES: 'C minor' .. 'B major')")
                    key = metrics.KEY_NAMES.index(key)
                key = int(key)
                if not -1 <= key < 24:
                    raise ValueError(f"KeyAnnotations: recording {r}: key id {key} is outside -1..23")
                starts.append(int(round(float(start_s) * sample_rate)))
                keys.append(key)
            if starts and starts[0] != 0:
                raise ValueError(f"KeyAnnotations: recording {r}: segment 0 must start at 0, not at sample {starts[0]}")
            if any(b <= a for a, b in zip(starts, starts[1:])):
                raise ValueError(f"KeyAnnotations: recording {r}: segment starts must be strictly ascending")
            rows.append((starts, keys))
        R, S = len(rows), max([len(st) for st, _ in rows] + [1])
        seg_start = torch.full((R, S), metrics._I64_MAX, dtype=torch.int64)
        seg_key = torch.full((R, S), -1, dtype=torch.int32)
        for r, (starts, keys) in enumerate(rows):
            seg_start[r, :len(starts)] = torch.tensor(starts, dtype=torch.int64)
            seg_key[r, :len(keys)] = torch.tensor(keys, dtype=torch.int32)
        seg_count = torch.tensor([len(st) for st, _ in rows], dtype=torch.int32)
        return cls(seg_start.to(device), seg_key.to(device), seg_count.to(device), int(sample_rate))


@dataclass
class TrackScore:
    """A track against annotations (``KeyTrack.score``); the four tensors live on the device.

    ``truth`` int32 (R, W): the annotated key of every window (-1: none); ``category`` int32 (R, W): -1 where the truth is -1, else
    0 correct, 1 fifth, 2 relative, 3 parallel, 4 other, 5 undecoded (``metrics.SCORE_CATEGORIES``); ``tally`` int32 (R, 2, 6): the
    category counts over all scored windows and over the pure ones (every annotated segment under the window carries one key);
    ``changes`` int32 (R, 2): how often the track's key changes from one window to the next, and how often the truth does."""
    truth: torch.Tensor
    category: torch.Tensor
    tally: torch.Tensor
    changes: torch.Tensor

    def _tally(self, pure):
        return self.tally[:, 1 if pure else 0].cpu().to(torch.float64)                          # (R, 6)

    def fractions(self, pure: bool = False):
        """Share of every category among the scored windows -> ``(per_recording (R, 6), pooled (6,))`` float64 on the host; NaN where
        nothing was scored.  ``pure``: over the pure windows only."""
        t = self._tally(pure)
        return t / t.sum(dim=1, keepdim=True), t.sum(dim=0) / t.sum()

    def weighted(self, pure: bool = False):
        """The MIREX-weighted score (correct 1, fifth 0.5, relative 0.3, parallel 0.2; ``metrics.SCORE_WEIGHTS``) ->
        ``(per_recording (R,), pooled float)``."""
        per, pooled = self.fractions(pure)
        w = torch.tensor(metrics.SCORE_WEIGHTS, dtype=torch.float64)
        return per @ w, float(pooled @ w)

    def flicker(self):
        """Key changes of the track per key change of the truth -> ``(per_recording (R,), pooled float)``; 1 is a track that moves as
        often as the key does (NaN or inf where the truth never moves)."""
        c = self.changes.cpu().to(torch.float64)
        tot = c.sum(dim=0)
        return c[:, 0] / c[:, 1], float(tot[0] / tot[1])


@dataclass
class _Follow:
    """``tuning="follow"`` checked: the windows of the tuning track, in frames."""
    window_frames: int
    stride_frames: int


@dataclass
class _Followed:
    """What ``tuning="follow"`` retuned by: the curve (R, W_t) on the device and where its knots sit, in input samples."""
    curve: torch.Tensor
    knot_first: int
    knot_step: int


def _mark_tuning(track, used, strength):
    """What a track was retuned by (``KeyEstimator._retuned``'s third and fourth item) -> its tuning fields."""
    if isinstance(used, _Followed):
        track.tuning_curve, track.tuning_curve_strength = used.curve, strength
        track.tuning_knot_first, track.tuning_knot_step = int(used.knot_first), int(used.knot_step)
    else:
        track.tuning_cents, track.tuning_strength = used, strength


@dataclass
class KeyTrack:
    """The key of R recordings over time (``KeyEstimator.track``), W windows each; everything but ``times`` lives on the device.

    ``key`` (R, W, 12) sigmoid pitch-class membership, ``tonic`` (R, W, 12) logits, ``genre`` (R, W, 11) or None: the net's outputs per
    window.  ``key_id``, ``sig``, ``tonic_id`` int32 (R, W) and ``confidence`` (R, W): the decode of ``metrics.decode_keys``.  ``counts``
    int32 (R,): windows of each recording; windows at index >= its count hold -1.  ``times`` (W,) float64 on the host: window centres
    in seconds.

    ``track(smooth=True)`` adds ``emissions`` (R, W, 24), every window's log-score of the 24 keys (``metrics.key_emissions``; zeros behind
    a recording's count), and ``smooth_key_id`` int32 (R, W), the Viterbi path through them (``metrics.viterbi_keys``): always a key
    0..23 below the count, -1 behind it.  Both are None otherwise.

    ``track(smooth=True, posteriors=True)`` adds the forward-backward pass over the same emissions and transition
    (``metrics.key_posteriors``): ``posteriors`` (R, W, 24), the posterior probability of every key at every window (rows below the
    count sum to 1, rows behind it are zeros); ``smooth_confidence`` (R, W), the posterior of the key ``smooth_key_id`` names (0 behind
    the count); ``log_likelihood`` (R,), the recording's log-score under the transition (the emissions are log-scores, not normalised
    likelihoods: it compares transitions on the same recording and means nothing else).  All three are None otherwise.

    ``hop``, ``window_frames``, ``stride_frames`` and ``sample_rate`` are the track's geometry in samples and frames (0 on a track
    built by hand): ``score`` needs them to place the windows on the annotations.

    ``track(tuning=...)`` adds ``tuning_cents`` (R,) float32, the detuning every recording was retuned by, and with ``tuning="auto"``
    ``tuning_strength`` (R,), how clearly it was measured (``metrics.estimate_tuning``); both are None on a plain track.  Such a track
    was made from audio whose time axis is stretched by ``rho_i = 2 ** (cents_i / 1200)``: ``times`` and the geometry are the
    retuned audio's, ``segments`` and ``score`` translate to and from the recording's own time.

    ``track(tuning="follow")`` instead adds ``tuning_curve`` and ``tuning_curve_strength`` (R, W_t) float32, the curve every recording
    was retuned along and the strength of the tuning track's windows (``metrics.tuning_track``), and ``tuning_knot_first`` /
    ``tuning_knot_step``, where the curve's knots sit in samples of the recording; ``tuning_cents`` is None on such a track.  Its time
    axis is stretched by a ratio that changes along the recording: ``segments``, ``change_points`` and ``boundary_score`` send their
    boundaries through the curve's inverse map (``ake_amd.retune_curve_positions``), ``score`` moves the annotation boundaries with the
    forward map (``metrics.curve_boundaries``).

    ``track(method="profile")`` fills the same fields without a net (``metrics.profile_emissions``): ``key`` is every window's
    sum-normalised chroma, ``emissions`` (always there) ``sharpness`` times the 24 profile correlations, ``tonic[..., t]`` the larger of
    ``emissions[..., t]`` and ``emissions[..., 12 + t]``, ``genre`` None, ``key_id`` the best-correlated key and ``confidence`` its
    correlation, ``tonic_id = key_id % 12`` and ``sig`` the first ``KEY_SIGNATURE_MAP`` row of the key's scale; a silent window holds -1
    in the three labels and zeros elsewhere.

    ``track(refine=True)`` adds where the key changes, to the frame (``metrics.key_changes``): ``change_frame`` int32 (R, W - 1), the
    frame from which the key of window w + 1 holds, where ``refined_source`` (``"smooth_key_id"`` or ``"key_id"``, the labels that were
    refined) names two different keys at the windows w and w + 1, else -1; ``change_gain`` and ``change_contrast`` (R, W - 1): what the
    frames' own scores gain over the grid's placement, and the mean per-frame advantage of each side's own key (near 0 or below: the
    labels do not fit the frames).  All four are None otherwise.  ``segments``, ``change_points`` and ``boundary_score`` read them.

    ``track(method="profile", tuning=..., tuned_chroma=True)`` sets ``tuned_chroma``: the recordings were not retuned, the class
    boundaries of the chroma were moved instead (``metrics.profile_emissions(cents=...)``).  ``tuning_cents`` then holds the cents
    every window's chroma was cut by, (R,) float32, or (R, W) with ``tuning="follow"`` (the tuning track's curve on the key track's
    windows), and ``tuning_strength`` the strength of the measurement in the same shape (None with given cents).  ``times``, the
    geometry and every boundary are in the recording's own time: nothing is translated."""
    key: torch.Tensor
    tonic: torch.Tensor
    genre: torch.Tensor | None
    key_id: torch.Tensor
    sig: torch.Tensor
    tonic_id: torch.Tensor
    confidence: torch.Tensor
    counts: torch.Tensor
    times: torch.Tensor
    window_seconds: float = 0.0
    stride_seconds: float = 0.0
    emissions: torch.Tensor | None = None
    smooth_key_id: torch.Tensor | None = None
    posteriors: torch.Tensor | None = None
    smooth_confidence: torch.Tensor | None = None
    log_likelihood: torch.Tensor | None = None
    hop: int = 0
    window_frames: int = 0
    stride_frames: int = 0
    sample_rate: int = 0
    tuning_cents: torch.Tensor | None = None
    tuning_strength: torch.Tensor | None = None
    tuning_curve: torch.Tensor | None = None
    tuning_curve_strength: torch.Tensor | None = None
    tuning_knot_first: int = 0
    tuning_knot_step: int = 0
    change_frame: torch.Tensor | None = None
    change_gain: torch.Tensor | None = None
    change_contrast: torch.Tensor | None = None
    refined_source: str | None = None
    tuned_chroma: bool = False

    @property
    def _stretch_cents(self):
        """The cents the track's time axis is stretched by: ``tuning_cents``, but None on a tuned-chroma track, whose audio nobody
        resampled."""
        return None if self.tuned_chroma else self.tuning_cents

    def _tensors(self):
        """Every device tensor of the track; the two of a smooth track, the three of its posteriors, the two of a retuned track and
        the three of a refined one only when it has them (a plain track lists what it always did)."""
        out = (self.key, self.tonic, self.genre, self.key_id, self.sig, self.tonic_id, self.confidence, self.counts)
        if self.emissions is not None or self.smooth_key_id is not None:
            out += (self.emissions, self.smooth_key_id)
            if self.posteriors is not None:
                out += (self.posteriors, self.smooth_confidence, self.log_likelihood)
        return out + tuple(t for t in (self.tuning_cents, self.tuning_strength, self.change_frame, self.change_gain, self.change_contrast,
                                       self.tuning_curve, self.tuning_curve_strength) if t is not None)

    def _curve_positions(self, k, rows=None):
        """Samples ``k`` (float64, (R, m), or (m,) of the one recording ``rows``) on the time axis of a followed track's retuned audio ->
        samples of the recording as it was handed in, through the curve's inverse map: ``ake_amd.retune_curve_positions`` (the
        retuner's own device function) at the two whole samples around ``k`` and a linear blend between them; a track that lives on the
        host (built by hand) goes through the model, ``metrics.retune_curve_positions``."""
        curve = self.tuning_curve if rows is None else self.tuning_curve[rows]
        k = torch.as_tensor(k, dtype=torch.float64, device=curve.device)
        lo = torch.floor(k)
        fn = _tuning.retune_curve_positions if curve.is_cuda else \
            (lambda i, c, first, step: metrics.retune_curve_positions(i.to(torch.float64), c, first, step))
        both = fn(torch.cat([lo, lo + 1], dim=-1).to(torch.int64), curve, self.tuning_knot_first, self.tuning_knot_step)
        a, b = both[..., :k.shape[-1]], both[..., k.shape[-1]:]
        return a + (k - lo) * (b - a)

    def _own_seconds(self, recording, seconds):
        """Seconds on the track's time axis -> seconds of recording ``recording`` as it was handed in (list -> list)."""
        if self.tuning_curve is not None:
            if not seconds:
                return []
            k = torch.tensor(seconds, dtype=torch.float64) * self.sample_rate
            return (self._curve_positions(k, recording).cpu() / self.sample_rate).tolist()
        rho = 1.0 if self._stretch_cents is None else 2.0 ** (float(self._stretch_cents[recording]) / 1200.0)
        return [t / rho for t in seconds]

    def _source(self, what, smoothed, refined):
        """``smoothed`` and ``refined`` of ``segments`` and its kin checked -> ``(labels (R, W), whether to read change_frame)``."""
        if smoothed and self.smooth_key_id is None:
            raise ValueError(f"{what}(smoothed=True): this track has no smoothed path; make it with track(..., smooth=True)")
        smoothed = bool(smoothed) or (smoothed is None and self.smooth_key_id is not None)
        has = self.change_frame is not None and self.refined_source == ("smooth_key_id" if smoothed else "key_id")
        if refined and not has:
            raise ValueError(f"{what}(refined=True): this track has no refined boundaries of its {'smooth_key_id' if smoothed else 'key_id'}; "
                             "make it with track(..., refine=True), which refines the smoothed path when there is one")
        return (self.smooth_key_id if smoothed else self.key_id), (has if refined is None else bool(refined))

    def segments(self, recording: int, smoothed: bool | None = None, confidence: bool = False, refined: bool | None = None):
        """Run-length encoding of one recording's key labels on the host -> list of ``(start_s, end_s, key_id, name)``.  A window stands
        for the stride around its centre; the first segment starts at 0 and the last ends with the last window.  ``name`` is
        ``metrics.KEY_NAMES[key_id]`` ("A minor"), or "unknown" where signature and tonic disagree (-1).

        ``smoothed``: True reads ``smooth_key_id`` (``ValueError`` if the track has none), False ``key_id``; None (default) the smoothed
        path when the track has one, ``key_id`` otherwise.

        ``confidence=True``: every tuple gets a fifth item, the mean of ``smooth_confidence`` over the segment's windows: how sure the
        smoother is of the key it names there (``ValueError`` on a track without posteriors).

        ``refined``: with True a key change lies at ``change_frame * hop / sample_rate`` instead of halfway between two window centres
        (``ValueError`` on a track without ``change_frame``, or whose ``refined_source`` is the other labels); a change to or from
        "unknown" has no refined frame and stays on the grid.  False: the grid.  None (default): refined when the track has them for the
        labels being read.  Where the search spans on either side of a short run overlap and the later change was placed before the
        earlier one (``metrics.key_changes``), the later one is read at the earlier one's frame: the run between them is empty.

        On a retuned track (``tuning_cents``) the times are divided by the recording's ``rho``: they are seconds of the recording as it
        was handed in, not of its retuned copy.  On a followed track (``tuning_curve``) they go through the curve's inverse map."""
        if confidence and self.smooth_confidence is None:
            raise ValueError("segments(confidence=True): this track has no posteriors; make it with track(..., smooth=True, posteriors=True)")
        source, refined = self._source("segments", smoothed, refined)
        n = int(self.counts[recording])
        change = self.change_frame[recording, :max(n - 1, 0)].cpu().tolist() if refined else None
        latest = -1
        for w in range(len(change or ())):                           # the spans of a short run may overlap: no segment ends before it starts
            if change[w] >= 0:
                latest = change[w] = max(change[w], latest)
        ids = source[recording, :n].cpu().tolist()
        times = self.times[:n].tolist()
        conf = self.smooth_confidence[recording, :n].cpu().tolist() if confidence else None
        half_w, half_s = self.window_seconds / 2, self.stride_seconds / 2
        if self.tuning_curve is not None:                            # a followed track: the boundaries go through the curve, all at once
            rho = 1.0
        else:
            rho = 1.0 if self._stretch_cents is None else 2.0 ** (float(self._stretch_cents[recording]) / 1200.0)
        out, a = [], 0
        for b in range(n):
            if b + 1 < n and ids[b + 1] == ids[a]:
                continue
            start = 0.0 if a == 0 else (times[a] - half_s) / rho
            end = (times[b] + (half_w if b == n - 1 else half_s)) / rho
            if refined and a > 0 and change[a - 1] >= 0:
                start = change[a - 1] * self.hop / self.sample_rate / rho
            if refined and b < n - 1 and change[b] >= 0:
                end = change[b] * self.hop / self.sample_rate / rho
            seg = (start, end, ids[a], metrics.KEY_NAMES[ids[a]] if ids[a] >= 0 else "unknown")
            out.append(seg + (sum(conf[a:b + 1]) / (b + 1 - a),) if confidence else seg)
            a = b + 1
        if self.tuning_curve is not None and out:
            own = self._own_seconds(recording, [t for seg in out for t in seg[:2]])
            out = [(own[2 * i], own[2 * i + 1]) + seg[2:] for i, seg in enumerate(out)]
        return out

    def change_points(self, recording: int):
        """The refined key changes of one recording on the host -> list of ``(time_s, from_key, to_key, gain, contrast)`` in ascending
        time: ``change_frame * hop / sample_rate`` (divided by ``rho`` on a retuned track, through the curve on a followed one, as in ``segments``), the two keys of
        ``refined_source`` around it, ``change_gain`` and ``change_contrast``.  ``ValueError`` on a track without ``refine=True``."""
        if self.change_frame is None:
            raise ValueError("change_points: this track has no refined boundaries; make it with track(..., refine=True)")
        n = int(self.counts[recording])
        ids = getattr(self, self.refined_source)[recording, :n].cpu().tolist()
        frame, gain, contrast = (t[recording, :max(n - 1, 0)].cpu().tolist() for t in (self.change_frame, self.change_gain, self.change_contrast))
        if self.tuning_curve is not None:
            at = [w for w in range(n - 1) if frame[w] >= 0]
            own = self._own_seconds(recording, [frame[w] * self.hop / self.sample_rate for w in at])
            return [(t, ids[w], ids[w + 1], gain[w], contrast[w]) for t, w in zip(own, at)]
        rho = 1.0 if self._stretch_cents is None else 2.0 ** (float(self._stretch_cents[recording]) / 1200.0)
        return [(frame[w] * self.hop / self.sample_rate / rho, ids[w], ids[w + 1], gain[w], contrast[w]) for w in range(n - 1) if frame[w] >= 0]

    def boundary_score(self, annotations: KeyAnnotations, refined: bool | None = None, tolerance_seconds: float = 1.0):
        """How far the track's key changes lie from the annotated ones -> ``{"count", "median_abs_seconds", "within_tolerance"}``: for
        every annotated key change (a segment whose key differs from the one before it, both labelled) the distance to the nearest
        predicted boundary of that recording (infinite where the track never changes); their number, the median distance in seconds
        and the share within ``tolerance_seconds`` (NaN where there is none).  The labels are the smoothed path when the track has one,
        else ``key_id``; ``refined`` picks their boundaries as in ``segments``.  Torch ops on the device; the three numbers are read at
        the end.

        On a retuned track the annotations are moved onto the retuned time axis first (``metrics.scale_boundaries``, as ``score``
        does), and every distance is divided by the recording's ``rho``: seconds of the recording as it was handed in.  On a followed
        track the predicted boundaries go back through the curve instead and meet the annotations on the recording's own axis."""
        pred, refined = self._source("boundary_score", None, refined)
        if self.hop <= 0 or self.window_frames <= 0 or self.stride_frames <= 0 or self.sample_rate <= 0:
            raise ValueError("boundary_score: this track does not know its geometry (hop, window_frames, stride_frames, sample_rate); "
                             "KeyEstimator.track fills it in")
        if annotations.sample_rate and annotations.sample_rate != self.sample_rate:
            raise ValueError(f"boundary_score: the annotations are in samples at {annotations.sample_rate} Hz, the track at {self.sample_rate} Hz")
        dev = pred.device
        R, W = pred.shape
        if annotations.seg_start.shape[0] != R:
            raise ValueError(f"boundary_score: the track has {R} recordings, the annotations {annotations.seg_start.shape[0]}")
        start = annotations.seg_start.to(device=dev, dtype=torch.int64)
        rho = torch.ones((R, 1), dtype=torch.float64, device=dev)
        if self._stretch_cents is not None:
            start = metrics.scale_boundaries(start, self._stretch_cents)
            rho = metrics.tuning_ratio(self._stretch_cents.to(dev)).reshape(R, 1)
        key = annotations.seg_key.to(device=dev, dtype=torch.int64)
        S = start.shape[1]
        count = annotations.seg_count.to(dev).to(torch.int64).reshape(R, 1).clamp(0, S)
        s_idx = torch.arange(1, S, device=dev)[None, :]
        wanted = (s_idx < count) & (key[:, 1:] >= 0) & (key[:, :-1] >= 0) & (key[:, 1:] != key[:, :-1])              # (R, S - 1)
        # the predicted boundaries in samples: the grid's halfway point, or the refined frame where there is one
        w_idx = torch.arange(max(W - 1, 0), device=dev, dtype=torch.float64)[None, :]
        at = ((w_idx * self.stride_frames + (self.window_frames - 1) / 2 + self.stride_frames / 2) * self.hop).expand(R, -1)
        if refined:
            at = torch.where(self.change_frame >= 0, self.change_frame.to(torch.float64) * self.hop, at)
        if self.tuning_curve is not None and W > 1:                  # a followed track: the predicted boundaries go back through the curve,
            at = self._curve_positions(at.contiguous())              # and meet the annotations on the recording's own axis
        moves = (pred[:, 1:] != pred[:, :-1]) & (torch.arange(1, max(W, 1), device=dev)[None, :] < self.counts.to(dev).reshape(R, 1))
        at = torch.where(moves, at, torch.full_like(at, float("inf")))
        dist = (start[:, 1:].to(torch.float64)[:, :, None] - at[:, None, :]).abs()                                  # (R, S - 1, W - 1)
        nearest = dist.amin(dim=2) if W > 1 else torch.full((R, S - 1), float("inf"), dtype=torch.float64, device=dev)
        d = (nearest / rho / self.sample_rate)[wanted].sort().values
        n = int(d.numel())
        if n == 0:
            return {"count": 0, "median_abs_seconds": float("nan"), "within_tolerance": float("nan")}
        return {"count": n, "median_abs_seconds": float((d[(n - 1) // 2] + d[n // 2]) / 2),
                "within_tolerance": float((d <= float(tolerance_seconds)).to(torch.float64).mean())}

    def score(self, annotations: KeyAnnotations, smoothed: bool | None = None) -> TrackScore:
        """Score the track against ``annotations`` on the device (``ake_track_score_i32``, one launch; ``metrics.track_score`` is its
        restatement) -> ``TrackScore``.  ``smoothed`` picks the source as in ``segments``: True ``smooth_key_id`` (``ValueError`` if the
        track has none), False ``key_id``, None the smoothed path when there is one.  The annotations are in samples at the track's
        sample rate.  ``ValueError`` on a track without its geometry (``hop``, ``window_frames``, ``stride_frames``).

        On a retuned track (``tuning_cents``) the annotation boundaries are first moved onto the retuned time axis,
        ``floor(start * rho_i)`` in float64 torch ops on the device (``metrics.scale_boundaries``); the launch is the same.  On a followed
        track (``tuning_curve``) they are moved with the curve's forward map (``metrics.curve_boundaries``)."""
        if smoothed and self.smooth_key_id is None:
            raise ValueError("score(smoothed=True): this track has no smoothed path; make it with track(..., smooth=True)")
        if self.hop <= 0 or self.window_frames <= 0 or self.stride_frames <= 0:
            raise ValueError("score: this track does not know its geometry (hop, window_frames, stride_frames); KeyEstimator.track fills it in")
        if annotations.sample_rate and self.sample_rate and annotations.sample_rate != self.sample_rate:
            raise ValueError(f"score: the annotations are in samples at {annotations.sample_rate} Hz, the track at {self.sample_rate} Hz")
        pred = self.smooth_key_id if (smoothed or (smoothed is None and self.smooth_key_id is not None)) else self.key_id
        dev = pred.device
        R, W = pred.shape
        if annotations.seg_start.shape[0] != R:
            raise ValueError(f"score: the track has {R} recordings, the annotations {annotations.seg_start.shape[0]}")
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        truth, category, tally, changes = i32(R, W), i32(R, W), i32(R, 2, 6), i32(R, 2)
        if W == 0:
            tally.zero_(); changes.zero_()
            return TrackScore(truth, category, tally, changes)
        start = annotations.seg_start.to(device=dev, dtype=torch.int64)
        if self._stretch_cents is not None:
            start = metrics.scale_boundaries(start, self._stretch_cents)
        if self.tuning_curve is not None:
            start = metrics.curve_boundaries(start, self.tuning_curve, self.tuning_knot_first, self.tuning_knot_step)
        start = start.contiguous()
        key = annotations.seg_key.to(device=dev, dtype=torch.int32).contiguous()
        count = annotations.seg_count.to(device=dev, dtype=torch.int32).contiguous()
        pred, counts = pred.contiguous(), self.counts.to(torch.int32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ake_track_score_i32(pred.data_ptr(), counts.data_ptr(), start.data_ptr(), key.data_ptr(), count.data_ptr(), R, W,
                                                      start.shape[1], self.hop, self.window_frames, self.stride_frames, truth.data_ptr(),
                                                      category.data_ptr(), tally.data_ptr(), changes.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "ake_track_score_i32")
        return TrackScore(truth, category, tally, changes)


class KeyEstimator:
    """``streams`` > 1: consecutive calls are issued round-robin on that many side streams, each with a workspace of its own, so
    that independent batches overlap on the GPU -- the CQT stage is VALU / HBM-bound, the network MFMA-bound, and one batch's CQT
    runs under another's convolutions (measured: +8..12 % clips/s at 2 streams).  The weights and CQT tables are shared (read-only
    during a forward).  Outputs of such calls belong to their side stream: call ``join()`` before the caller's stream reads them.

    ``wrap_mode``: the pitch convolutions are circular in TIME as well (models.py:221,230), and a batch is zero-padded to its
    longest clip (the reference pads to the longest clip of the whole dataset, KeyDataset.py:243-245), so a shorter clip's last
    frames wrap into padding and its outputs depend on what it was batched with.  ``"dataset_max"`` (default) is that
    behaviour, bit for bit.  ``"true_end"`` (opt-in) wraps every clip at its OWN last frame: clips are
    grouped by frame count and each group runs unpadded, so a clip's outputs are those of the clip alone.

    ``frames=0``: the reference's whole-song mode (``--frames 0 --window_size W``, KeyDataset.py:485-503, 212-215, models.py:842-847).
    Clip i is transformed at its own hop ``n_i // W + 1`` (``n_i`` = ``lengths[i]``, or n), which gives ``T_i <= W`` frames, zero-padded
    to F = 592 frames (the reference's item width; for W > 592, ``F = max(min(W, max T_i), 592)``, which reads the lengths on the host).
    The net then runs on (B, 1, n_bins, F) with ``seq_length=None``: its pooling covers all F frames, the zero tail included, as the
    reference's does.  ``wrap_mode`` has no meaning here ("true_end" is refused).

    ``tuning`` (``__call__`` and ``track``; not in the reference, which assumes A4 = 440 Hz everywhere): None (default) is the code
    path without it, untouched -- same launches, same bits.  ``"auto"`` measures every recording's detuning from one transform at the
    estimator's plan (``estimate_tuning``), resamples it by ``2 ** (cents / 1200)`` (``ake_amd.retune``, one launch) and then runs the
    call on the retuned audio with the retuned lengths: that first transform is the price of the estimate, so the call transforms
    twice.  A number or a (B,) tensor of cents skips the estimate: one transform and one extra launch.  ``min_strength``: recordings
    whose estimate is weaker keep their audio (0 cents), decided on the device.  The retuned batch is always ragged, in a buffer of
    ``ake_retune_out_len(n)`` columns (the widest a row can get), so nothing waits for the device; ``lengths``, ``rate``, ``channel``,
    int16 audio, ``streams`` > 1, ``wrap_mode="true_end"`` and ``frames=0`` work as without it.  The resampler discards content above
    0.94 of the Nyquist frequency: an estimator whose transform reaches that far refuses ``tuning`` with a ``ValueError``.

    ``tuning="follow"`` (``__call__``, ``track``, ``profile_key``) is for a tuning that drifts within a recording, a tape that changes
    speed: one transform at the estimator's plan, the estimate on sliding windows of ``tuning_window_seconds`` (default 5, rounded to
    an odd number of frames) every ``tuning_stride_seconds`` (default 1) (``tuning_track``, ``ake_amd.tuning_track``; windows weaker than
    ``min_strength`` hold the last strong value), then a resampler whose ratio is linear in the input position between the window
    centres (``ake_amd.retune_curve``, two launches), then the call on the retuned audio as with "auto".  Nothing is read back.
    Refused with a ``ValueError`` on ``frames=0`` estimators, which have a hop per clip.

    ``tuned_chroma=True`` (``track(method="profile")`` and ``profile_key``, with any ``tuning``) retunes nothing: the profile method only
    sums bins, so the one transform's chroma is cut at class boundaries moved by the cents (``track`` has the details).

    ``KeyEstimator(None, device=..., pitches=288)``: an estimator without a net, for the calls that need none --
    ``track(method="profile")``, ``stream(method="profile")``, ``profile_key`` and ``fit_key_profiles`` (and ``estimate_tuning``).
    ``__call__``, ``track(method="net")``, ``stream(method="net")`` and ``training_windows`` raise a ``ValueError`` on it.  With a net, ``device`` and ``pitches`` are the net's
    and must be left at None."""

    def __init__(self, net: PitchClassNet | None, sample_rate: int = 22050, frames: int = 5, streams: int = 1, wrap_mode: str = "dataset_max",
                 q_mode: int = 0, window_size: int = WHOLE_SONG_FRAMES, device=None, pitches: int | None = None):
        if wrap_mode not in ("dataset_max", "true_end"):
            raise ValueError("wrap_mode must be 'dataset_max' or 'true_end'")
        if frames <= 0 and wrap_mode == "true_end":
            raise ValueError("wrap_mode 'true_end' has no meaning with frames=0 (every clip is zero-padded to the same width)")
        if net is None:
            if not torch.cuda.is_available():
                raise _lib.AkeError("KeyEstimator needs a HIP device; there is no CPU fallback")
            self.net = None
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            pitches = 288 if pitches is None else int(pitches)
        else:
            if device is not None or pitches is not None:
                raise ValueError("KeyEstimator: device and pitches are the net's; give them only with net=None")
            self.net = net.eval()
            self.device = net._device()
            pitches = net.pitches
        self.sample_rate, self.wrap_mode = int(sample_rate), wrap_mode
        self.frames, self.window_size = int(frames), int(window_size)
        if self.frames <= 0:
            self.plan = get_any_hop_plan(sample_rate, pitches, 36, device=self.device, q_mode=q_mode)
        else:
            self.plan = CQTPlan(sample_rate, hop_for(sample_rate, frames), pitches, 36, q_mode=q_mode, device=self.device)   # q_mode: ake_amd.cqt.get_plan
        self.streams = max(1, int(streams))
        self._slots = [{"ws": None, "stream": None} for _ in range(self.streams)]
        self._turn = 0
        self._transitions = {}                                       # track(smooth=True): log transition matrices on the device

    def _need_net(self, what):
        if self.net is None:
            raise ValueError(f"{what} runs the net, and this estimator was built without one (KeyEstimator(None, ...)): it serves "
                             'track(method="profile"), stream(method="profile"), profile_key and fit_key_profiles')

    def join(self):
        """Make the caller's current stream wait for every call issued so far (``streams`` > 1; a no-op otherwise)."""
        if self.streams == 1:
            return
        cur = torch.cuda.current_stream(self.device)
        for slot in self._slots:
            if slot["stream"] is not None:
                cur.wait_stream(slot["stream"])

    @torch.no_grad()
    def __call__(self, audio: torch.Tensor, lengths: torch.Tensor | None = None, rate: int | None = None, channel: int = 0,
                 tuning=None, min_strength: float = 0.0, tuning_window_seconds: float = 5.0, tuning_stride_seconds: float = 1.0):
        """audio (B, n) or (B, C, n) float32 on the GPU -> tuple of (B,12), (B,12)[, (B,11)] float32 tensors.

        int16 audio is 16-bit PCM, sample / 32768 (``ake_amd.pcm16_to_float``): mono at the estimator's rate goes straight to the PCM
        pipeline entry, (B, C, n) audio of any strides (interleaved storage as ``buf.transpose(1, 2)``) or another ``rate`` through the PCM
        resampler first.  No float32 copy of the audio is written, and the results are those of the float32 route on the converted
        audio, bit for bit.  Every other dtype is converted with ``.to(float32)``, unscaled.

        ``lengths`` (B,) int64: ragged batch, row i holds ``lengths[i] <= n`` samples; every clip is pooled over its own frames
        (``seq_length`` = ``1 + lengths[i] // hop``), as a ``KeyDataset`` batch of unequal clips is (KeyDataset.py:245-256).
        ``rate``: sample rate of ``audio`` when it is not the estimator's -- it is resampled on the device first
        (``scipy.signal.resample_poly``'s filter; with ``frames=0`` each clip's hop is then taken from its resampled length); ``channel``: which channel of (B, C, n) audio to take (0 = the reference's
        ``waveform[0]``, KeyDataset.py:480) or -1 for the mean of all.  ``tuning``, ``min_strength``: see the class."""
        self._need_net("KeyEstimator.__call__")
        self.net._sync_weights(self.device, for_eval=True)
        if audio.dim() == 3 or (rate is not None and int(rate) != self.sample_rate):
            rs = get_resampler(self.sample_rate if rate is None else int(rate), self.sample_rate, self.device)
            audio, len_out = rs(audio, channel=channel, lengths=lengths)
            lengths = len_out if lengths is not None else None
        if tuning is None:
            return self._issue(self._run_wrapped, audio, lengths)
        cents = self._given_tuning(tuning, audio.shape[0], tuning_window_seconds, tuning_stride_seconds)
        return self._issue(lambda slot, a, l: self._run_wrapped(slot, *self._retuned(slot, a, l, cents, min_strength)[:2]), audio, lengths)

    def _given_tuning(self, tuning, B, window_seconds=5.0, stride_seconds=1.0, retunes=True):
        """``tuning`` of ``__call__`` / ``track`` / ``profile_key`` checked -> None for "auto", the ``_Follow`` geometry for "follow",
        else the (B,) float32 cents on the device.  ``retunes=False``: for the tuned chroma, which resamples nothing."""
        if retunes:
            self._refuse_unretunable("tuning")
        if isinstance(tuning, str):
            if tuning == "follow":
                return self._follow_geometry('tuning="follow"', window_seconds, stride_seconds)
            if tuning != "auto":
                raise ValueError('tuning must be None, "auto", "follow", a number of cents or a (B,) tensor of cents')
            return None
        if isinstance(tuning, torch.Tensor):
            cents = tuning.detach().to(device=self.device, dtype=torch.float32).reshape(-1)
            if cents.numel() != B:
                raise ValueError(f"tuning: {B} recordings but {cents.numel()} tunings")
            # what the kernel would read anyway (NaN as 0, beyond +-50 as +-50), made explicit here, on the device, so that the cents a
            # track carries are the cents its audio was resampled by
            return torch.nan_to_num(cents, nan=0.0).clamp(-metrics.RETUNE_MAX_CENTS, metrics.RETUNE_MAX_CENTS).contiguous()
        if not abs(float(tuning)) <= metrics.RETUNE_MAX_CENTS:
            raise ValueError(f"tuning: {tuning} cents; a detuning lies within +-{metrics.RETUNE_MAX_CENTS:g} cents (beyond that it is the next semitone)")
        return torch.full((B,), float(tuning), dtype=torch.float32, device=self.device)

    def _refuse_unretunable(self, what):
        """The retuner discards what lies above 0.94 of the Nyquist frequency: an estimator whose top bin lies there cannot use it."""
        top = 32.70319566257483 * 2.0 ** ((self.plan.n_bins - 1) / self.plan.bins_per_octave)           # C1, the plan's fmin
        if top >= metrics.RETUNE_CUTOFF * self.sample_rate / 2:
            raise ValueError(f"{what}: the retuner keeps {metrics.RETUNE_CUTOFF} of the Nyquist frequency, and this estimator's top bin "
                             f"({top:.0f} Hz at {self.sample_rate} Hz) lies beyond it")

    def _slot_ws(self, slot, nbytes):
        if slot["ws"] is None or slot["ws"].numel() < nbytes:
            slot["ws"] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return slot["ws"]

    def _estimate(self, slot, audio, lengths, min_strength=0.0):
        """One transform at the estimator's plan in the slot's workspace, then ``ake_tuning_estimate_f32`` in the same place (same
        stream, behind it) -> ``(cents, strength)``.  The ragged transform writes zeros behind every row's frames: no counts needed."""
        L = _lib.lib()
        audio = audio.to(self.device)
        B, n = audio.shape
        if self.frames <= 0:                                         # whole-song mode: every clip at its own hop, as the net will see it
            W = self.window_size
            # T_i <= W frames per clip.  (_run_whole_song reads the lengths on the host to trim this width for W > 592; here the
            # zero frames behind a clip add nothing to the sums, so the full W serves and nothing waits for the device)
            F = max(W, WHOLE_SONG_FRAMES)
            if lengths is None:
                hops = torch.full((B,), hop_for_window(n, W), dtype=torch.int32, device=self.device)
            else:
                lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
                hops = hop_for_window(lengths, W).to(torch.int32)
            ws = self._slot_ws(slot, max(self.plan.workspace_bytes_hops(B, n, F), int(L.ake_tuning_workspace_bytes(B, F))))
            mel = self.plan.logmag_hops(audio, hops, lengths, out_frames=F, workspace=ws)
        else:
            T = self.plan.num_frames(n)
            ws = self._slot_ws(slot, max(int(L.ake_cqt_workspace_bytes(self.plan.handle, B, n)), int(L.ake_tuning_workspace_bytes(B, T))))
            mel = self.plan.logmag(audio, lengths=lengths, workspace=ws)
        return _tuning.estimate_tuning(mel, None, min_strength, workspace=ws)

    def _follow_geometry(self, what, window_seconds, stride_seconds):
        """The windows of a tuning track -> ``_Follow``: ``window_seconds`` rounded to an odd number of frames (a window then has a frame
        at its centre, where its knot sits), ``stride_seconds`` to at least one."""
        if self.frames <= 0:
            raise ValueError(f"{what} needs a fixed frame rate: this estimator was built with frames=0, which has a hop per clip")
        wf = max(1, int(round(float(window_seconds) * self.frames)))
        return _Follow(wf + 1 - wf % 2, max(1, int(round(float(stride_seconds) * self.frames))))

    def _tuning_track(self, slot, audio, lengths, follow, min_strength):
        """One transform at the estimator's plan in the slot's workspace, then ``ake_tuning_track_f32`` in the same place (same stream,
        behind it) -> ``(cents_raw, strength, curve, window_counts)``."""
        L = _lib.lib()
        audio = audio.to(self.device)
        B, n = audio.shape
        T = self.plan.num_frames(n)
        ws = self._slot_ws(slot, max(int(L.ake_cqt_workspace_bytes(self.plan.handle, B, n)),
                                     int(L.ake_tuning_track_workspace_bytes(B, T, follow.window_frames, follow.stride_frames))))
        frames = None
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
            frames = (1 + lengths.clamp(0, n) // self.plan.hop_length).clamp(max=T).to(torch.int32)
        mel = self.plan.logmag(audio, lengths=lengths, workspace=ws)
        return _tuning.tuning_track(mel, follow.window_frames, follow.stride_frames, frames, min_strength, workspace=ws)

    def _retuned(self, slot, audio, lengths, cents, min_strength):
        """-> ``(retuned audio, retuned lengths, cents, strength)``; ``cents`` None: estimated here (``strength`` is None otherwise);
        ``cents`` a ``_Follow``: the tuning track is measured here and the audio retuned along its curve, with the knots at the window
        centres; ``cents`` then comes back as a ``_Followed`` (``strength`` is that of the windows)."""
        if isinstance(cents, _Follow):
            _, strength, curve, _ = self._tuning_track(slot, audio, lengths, cents, min_strength)
            hop = self.plan.hop_length
            first, step = (cents.window_frames - 1) // 2 * hop, cents.stride_frames * hop
            audio, lengths = _tuning.retune_curve(audio.to(self.device), curve, first, step, lengths)
            return audio, lengths, _Followed(curve, first, step), strength
        strength = None
        if cents is None:
            cents, strength = self._estimate(slot, audio, lengths, min_strength)
        audio = audio.to(self.device)
        audio, lengths = _tuning.retune(audio, cents, lengths)
        return audio, lengths, cents, strength

    @torch.no_grad()
    def estimate_tuning(self, audio: torch.Tensor, lengths: torch.Tensor | None = None, rate: int | None = None, channel: int = 0,
                        min_strength: float = 0.0):
        """How far every recording sits from A4 = 440 Hz -> ``(cents, strength)``, float32 (B,) on the device: one transform at the
        estimator's plan, in its ragged form, then ``ake_amd.estimate_tuning`` (``metrics.estimate_tuning`` is the definition).  ``audio``,
        ``lengths``, ``rate``, ``channel``, ``streams`` > 1 and ``join()`` as in ``__call__``."""
        if audio.dim() == 3 or (rate is not None and int(rate) != self.sample_rate):
            rs = get_resampler(self.sample_rate if rate is None else int(rate), self.sample_rate, self.device)
            audio, len_out = rs(audio, channel=channel, lengths=lengths)
            lengths = len_out if lengths is not None else None
        return self._issue(lambda slot, a, l: self._estimate(slot, a, l, min_strength), audio, lengths)

    @torch.no_grad()
    def tuning_track(self, audio: torch.Tensor, lengths: torch.Tensor | None = None, rate: int | None = None, channel: int = 0,
                     window_seconds: float = 5.0, stride_seconds: float = 1.0, min_strength: float = 0.0):
        """How far every recording sits from A4 = 440 Hz over time -> ``(cents_raw, strength, curve, window_counts)``, float32 (B, W)
        three times and int32 (B,) on the device: one transform at the estimator's plan, then ``ake_amd.tuning_track`` on windows of
        ``window_seconds`` (rounded to an odd number of frames) every ``stride_seconds`` (``metrics.tuning_track`` is the definition).
        It is the measurement ``tuning="follow"`` retunes by.  ``audio``, ``lengths``, ``rate``, ``channel``, ``streams`` > 1 and ``join()``
        as in ``__call__``.  Refused with a ``ValueError`` on ``frames=0`` estimators."""
        follow = self._follow_geometry("tuning_track", window_seconds, stride_seconds)
        audio, lengths = self._resampled(audio, lengths, rate, channel)
        return self._issue(lambda slot, a, l: self._tuning_track(slot, a, l, follow, min_strength), audio, lengths)

    def _issue(self, run, audio, lengths):
        """``run(slot, audio, lengths)`` on the caller's stream (``streams`` == 1) or on the next side stream in turn."""
        slot = self._slots[self._turn]
        if self.streams == 1:
            return run(slot, audio, lengths)
        self._turn = (self._turn + 1) % self.streams
        with torch.cuda.device(self.device):
            if slot["stream"] is None:
                slot["stream"] = torch.cuda.Stream(self.device)
            slot["stream"].wait_stream(torch.cuda.current_stream(self.device))      # the inputs were produced on the caller's stream
            cur = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(slot["stream"]):
                out = run(slot, audio, lengths)
            # the outputs were allocated on the side stream and will be read on the caller's: tell the allocator now (nothing to
            # remember until join(), nothing to drop when a caller never joins)
            for t in (out._tensors() if isinstance(out, KeyTrack) else out):
                if t is not None:
                    t.record_stream(cur)
            audio.record_stream(slot["stream"])
        return out

    @torch.no_grad()
    def track(self, audio: torch.Tensor, lengths: torch.Tensor | None = None, rate: int | None = None, channel: int = 0,
              window_seconds: float = 15.0, stride_seconds: float = 5.0, smooth: bool = False, mean_key_seconds: float = 60.0,
              transition: torch.Tensor | None = None, signature_weight: float = 1.0, posteriors: bool = False,
              tuning=None, min_strength: float = 0.0, method: str = "net", profiles="krumhansl", compression: str = "log",
              profile_sharpness: float = 10.0, refine: bool = False, refine_slack_seconds: float | None = None,
              tuning_window_seconds: float = 5.0, tuning_stride_seconds: float = 1.0, tuned_chroma: bool = False) -> KeyTrack:
        """The key of long recordings over time: audio (R, n) or (R, C, n) float32 on the GPU -> ``KeyTrack``.  int16 audio is 16-bit
        PCM, as in ``__call__``.

        Every recording is transformed ONCE at the estimator's hop (``T = 1 + n // hop`` frames); the net then runs on sliding windows
        of those frames -- ``window_frames = 1 + round(window_seconds * sample_rate) // hop`` frames each (76 for 15 s at 22.05 kHz and 5
        frames per second), ``stride_frames = max(1, round(stride_seconds * frames))`` apart -- exactly as on a clip of that many frames
        with ``seq_length = window_frames``, and every window's outputs are decoded to a key label on the device
        (``metrics.decode_keys``).  Recording i has ``(T_i - window_frames) // stride_frames + 1`` windows (0 if it is shorter than one).
        The one difference from cutting the audio into clips and calling the estimator on them: a frame near a window edge sees the
        recording's real neighbouring audio, where a separately transformed clip sees zero padding.

        ``lengths``, ``rate``, ``channel``, ``streams`` > 1 and ``join()`` behave as in ``__call__``.  Refused with a ``ValueError``:
        ``frames=0`` estimators (one hop per song: there are no frames to slide over), ``wrap_mode="true_end"`` (a window has no padding
        to wrap into) and ``--local`` nets (their own per-frame forward; its rows are not time frames).

        ``smooth=True`` appends two launches on the same stream and fills ``KeyTrack.emissions`` and ``KeyTrack.smooth_key_id``: every
        window's log-score of the 24 keys from the two heads (``metrics.key_emissions``: the tonic head's log-softmax plus
        ``signature_weight`` times the key head's mean Bernoulli log-likelihood of the key's scale), then a first-order Viterbi decode
        (``metrics.viterbi_keys``).  The path always names a key: a tonic that does not fit the signature scores low instead of decoding
        to -1.  ``transition``: a (24, 24) log matrix, from key i (row) to key j, all finite (write a forbidden transition as a large
        negative number).  Default: ``metrics.key_transition_log(stay=exp(-stride / mean_key_seconds))`` with ``stride`` the track's
        actual stride in seconds, so the amount of smoothing does not depend on the stride chosen.  The default of 60 s is a starting
        value; how it and its neighbours score against ground truth on synthesised modulating recordings is in
        ``profiles/track_accuracy.md`` (``KeyTrack.score``).  Nothing else of the track changes with ``smooth``.

        ``posteriors=True`` (with ``smooth=True``; a ``ValueError`` without it) appends the forward-backward pass over the same
        emissions and transition, two more launches on the same stream, and fills ``KeyTrack.posteriors``, ``smooth_confidence`` and
        ``log_likelihood`` (``metrics.key_posteriors``).  Nothing else of the track changes with it.  ``ake_amd.fit_key_transition``
        fits a ``transition`` to smooth tracks' own emissions; the same table scores it.

        ``tuning``, ``min_strength``: see the class.  The track is then that of the retuned audio -- its ``times`` and geometry are the
        retuned time axis -- and carries ``tuning_cents`` (and ``tuning_strength`` with "auto"), by which ``KeyTrack.segments`` and
        ``KeyTrack.score`` translate to and from the recording's own time.  With ``tuning="follow"`` (``tuning_window_seconds``,
        ``tuning_stride_seconds``: see the class) it carries ``tuning_curve`` and its kin instead, and they translate through the curve.

        ``method``: ``"net"`` (default) is all of the above.  ``"profile"`` needs no net: the same one transform per recording, then
        ``ake_amd.profile_emissions`` on the same windows (two launches, no net launch) with ``profiles`` (a name of
        ``metrics.KEY_PROFILES`` or a (2, 12) tensor, as ``fit_key_profiles`` returns it), ``compression`` and ``profile_sharpness``; what
        the ``KeyTrack`` then holds is in its docstring.  ``emissions`` is always filled; ``smooth`` and ``posteriors`` append the same
        Viterbi and forward-backward launches to it.  ``signature_weight`` has no meaning there and must be left at 1.  ``lengths``,
        ``rate``, ``channel``, int16 audio, ``tuning`` and ``streams`` > 1 work as with the net; ``frames=0`` estimators and ``--local``
        nets are refused.  ``profile_sharpness = 10`` and ``compression = "log"`` are unmeasured starting values
        (``profiles/key_profiles.md``).

        ``refine=True`` (both methods) places every key change to the frame: one more launch (``ake_amd.key_changes``;
        ``metrics.key_changes`` is the definition) on ``smooth_key_id`` with ``smooth=True``, else on ``key_id``, with the call's
        ``profiles`` and ``compression``, and the change is looked for ``refine_slack_seconds`` (default: the stride) beyond the two
        windows' centres.  It fills ``KeyTrack.change_frame``, ``change_gain``, ``change_contrast`` and ``refined_source``, which
        ``KeyTrack.segments``, ``change_points`` and ``boundary_score`` read; nothing else of the track changes with it.  The profile
        method reads the log-CQT it already holds.  The net method transforms the audio once more for it: the fused track call keeps
        its own transform inside its workspace and does not expose it.  How far the boundaries then lie from the
        truth on synthesised recordings is in ``profiles/track_refine.md``.

        ``tuned_chroma=True`` (``method="profile"`` with a ``tuning``; default False: everything above, same launches, same bits) meets
        the detuning without retuning the audio: ONE transform, then the chroma's class boundaries are moved by the cents and split
        the bin each crosses (``ake_amd.profile_emissions(cents=...)``; ``metrics.profile_emissions`` is the definition) -- no resampling
        pass, no second transform, and every time of the track stays in the recording's own clock.  ``tuning="auto"``:
        ``ake_amd.estimate_tuning`` on that transform (``min_strength`` as above), one value per recording.  A number or a (R,) tensor of
        cents: used as given.  ``tuning="follow"``: ``ake_amd.tuning_track`` on the key track's own windows (``window_frames``,
        ``stride_frames``), whose ``curve`` row gives every window its cents, held weak windows, unwrap and clamp included;
        ``tuning_window_seconds`` and ``tuning_stride_seconds`` are not read in this mode.  ``KeyTrack.tuning_cents`` and
        ``tuning_strength`` are filled and ``KeyTrack.tuned_chroma`` is set.  The smoother, the posteriors, ``score`` and
        ``fit_key_transition`` take the emissions as before.  Refused with a ``ValueError``: ``method="net"`` (the net needs retuned
        audio), ``tuning=None``, ``refine=True`` (the change-point kernel reads the uniform per-frame chroma) and a plan whose bins are
        not a multiple of 36.  The estimator's top bin may lie anywhere: nothing is resampled."""
        if posteriors and not smooth:
            raise ValueError("track(posteriors=True) needs smooth=True: the posteriors belong to the smoothed track's emissions and transition")
        if tuned_chroma and method == "net":
            raise ValueError('track(tuned_chroma=True): only method="profile" sums bins; the net needs retuned audio (leave tuned_chroma at False)')
        if method == "profile":
            return self._track_profile(audio, lengths, rate, channel, window_seconds, stride_seconds, smooth, mean_key_seconds, transition,
                                       signature_weight, posteriors, tuning, min_strength, profiles, compression, profile_sharpness,
                                       refine, refine_slack_seconds, tuning_window_seconds, tuning_stride_seconds, bool(tuned_chroma))
        if method != "net":
            raise ValueError('track: method must be "net" or "profile"')
        self._need_net('KeyEstimator.track(method="net")')
        self._refuse_untrackable()
        self.net._sync_weights(self.device, for_eval=True)
        if audio.dim() == 3 or (rate is not None and int(rate) != self.sample_rate):
            rs = get_resampler(self.sample_rate if rate is None else int(rate), self.sample_rate, self.device)
            audio, len_out = rs(audio, channel=channel, lengths=lengths)
            lengths = len_out if lengths is not None else None
        wf = track_window_frames(int(round(window_seconds * self.sample_rate)), self.plan.hop_length)
        sf = track_stride_frames(stride_seconds, self.frames)
        # (made on the caller's stream, which every side stream waits for before it runs the call)
        smoothing = (self._transition(sf, mean_key_seconds, transition), float(signature_weight), bool(posteriors)) if smooth else None
        refining = self._refining(sf, refine_slack_seconds, profiles, compression) if refine else None
        if tuning is None and refining is None:
            return self._issue(lambda slot, a, l: self._run_track(slot, a, l, wf, sf, smoothing), audio, lengths)
        cents = None if tuning is None else self._given_tuning(tuning, audio.shape[0], tuning_window_seconds, tuning_stride_seconds)

        def run(slot, a, l):
            used = strength = None
            if tuning is not None:
                a, l, used, strength = self._retuned(slot, a, l, cents, min_strength)
            track = self._run_track(slot, a, l, wf, sf, smoothing)
            _mark_tuning(track, used, strength)
            if refining is not None:                                 # the fused call's transform stays in its workspace: one more
                mel, frames = self._profile_logmag(slot, a, l)[:2] if track.key_id.shape[1] > 1 else (None, None)
                self._refine(track, mel, frames, refining)
            return track
        return self._issue(run, audio, lengths)

    def _refining(self, sf, slack_seconds, profiles, compression):
        """``track(refine=True)``'s arguments checked -> ``(slack_frames, the profile table on the device, compression 0..2)`` (made on
        the caller's stream, which every side stream waits for)."""
        slack = sf if slack_seconds is None else int(round(float(slack_seconds) * self.frames))
        if slack < 0:
            raise ValueError("track(refine=True): refine_slack_seconds must not be negative")
        _keychanges.check_span(sf, slack)
        return slack, _keyprofile.device_profiles(profiles, self.device), metrics._profile_compression(compression)

    def _refine(self, track, mel, frames, refining):
        """``ake_key_changes_f32`` on the track's labels (the smoothed path when it has one) and the log-CQT ``mel`` (R, P, T) with
        ``frames`` int32 (R,) or None; ``mel`` None: the track has no pair of windows."""
        slack, prof, mode = refining
        track.refined_source = "smooth_key_id" if track.smooth_key_id is not None else "key_id"
        labels = getattr(track, track.refined_source)
        if mel is None:
            R, B = labels.shape[0], max(labels.shape[1] - 1, 0)
            track.change_frame = torch.empty((R, B), dtype=torch.int32, device=self.device)
            track.change_gain, track.change_contrast = (torch.empty((R, B), dtype=torch.float32, device=self.device) for _ in range(2))
            return
        if self.streams > 1:                                         # (a user's table is a fresh tensor of the caller's stream)
            prof.record_stream(torch.cuda.current_stream(self.device))
        track.change_frame, track.change_gain, track.change_contrast = _keychanges._launch(
            mel, False, frames, labels.contiguous(), track.counts, track.window_frames, track.stride_frames, slack, prof, mode)

    def stream(self, recordings: int, window_seconds: float = 15.0, stride_seconds: float = 5.0, smooth: bool = True, lag_windows: int = 6,
               mean_key_seconds: float = 60.0, transition: torch.Tensor | None = None, log_prior: torch.Tensor | None = None,
               signature_weight: float = 1.0, keep_frames: bool = False, max_chunk_samples: int | None = None, rate: int | None = None,
               tuning=None, posteriors: bool = False, source_rate: int | None = None, source_channels: int | None = None, channel: int = 0,
               method: str = "net", profiles="krumhansl", compression: str = "log", profile_sharpness: float = 10.0,
               tuning_meter: bool = False, tuning_min_strength: float = 0.0, retune_cents: float | None = None, refine: bool = False,
               refine_slack_seconds: float | None = None):
        """Track keys on audio as it arrives -> ``ake_amd.KeyStream``: ``push(chunk)`` takes the next (R, m) samples of all
        ``recordings`` = R recordings at once (float32, or int16 = 16-bit PCM; any m >= 0, the same m for every recording) and returns
        a ``StreamUpdate`` with the windows that chunk completed; ``finish()`` ends the recordings and returns the rest.

        ``source_rate`` / ``source_channels`` / ``channel``: what arrives is at ``source_rate`` Hz with ``source_channels`` channels --
        chunks are then (R, C, m) ((R, m) with one channel), float32 or int16 with any strides (interleaved (R, m, C) storage goes in as
        ``buf.transpose(1, 2)``) -- and passes an ``ake_amd.StreamResampler`` in front of the history: ``channel`` >= 0 takes that
        channel, -1 the mean, and the polyphase filter carries its last few dozen inputs from push to push, so the stream sees
        ``prepare_audio(whole, source_rate, rate, channel)`` bit for bit however the audio is cut (one or two small launches a push:
        ``ake_stream_resample_f32``).  ``max_chunk_samples`` then counts source samples, and ``finish()`` first pushes what the resampler
        held back: after N source samples the stream has emitted the windows ``track(audio, rate=source_rate, channel=channel)`` gives.
        Times stay seconds of audio.  With ``source_rate`` the estimator's (or None) and one channel nothing is added to a push.

        The windows are ``track``'s (``window_seconds``, ``stride_seconds``), each emitted exactly once, in order, as soon as all its
        frames are final: a frame of the transform depends on ``H`` = ``ake_cqt_plan_half_support`` samples to either side, so frame
        t is final once sample ``t*hop + H`` has arrived (just under 1 s behind the audio with the default plan), and at ``finish()``
        all ``1 + N // hop`` frames are.  After ``finish()`` on N samples the stream has emitted the windows ``track`` gives for them.
        New frames come from re-transforming the last ``2*H + hop`` samples and the chunk with the offline transform; they equal
        ``track``'s frames to the transform's accuracy, not to the bit (``ake_amd.stream``).  Nothing is read back from the device and
        a push waits for nothing; it runs on the current stream (the estimator's side streams are not used), and after the first push
        it allocates only the tensors it returns -- everything else is sized here, for chunks of up to ``max_chunk_samples`` (default
        10 s; a longer chunk is pushed as several pieces).

        ``smooth=True`` (default) adds, per window, ``emissions`` (``metrics.key_emissions`` with ``signature_weight``), ``filtered``
        (the normalised log forward scores: the probability of each key given the audio so far) and the fixed-lag path
        ``smooth_key_id``: window v gets its label once ``lag_windows`` more windows have been seen -- the label
        ``metrics.viterbi_keys`` gives it on the windows up to ``v + lag_windows`` -- and never changes afterwards; ``finish()``
        labels the last ``lag_windows`` windows with the Viterbi path of the whole recording (``metrics.key_stream``).
        ``lag_windows`` 0..255; 6 is an unmeasured starting value (``profiles/track_stream.md``).  ``transition`` and
        ``mean_key_seconds`` as in ``track``; ``log_prior`` (24,), default zeros.  ``keep_frames=True`` keeps every final frame in
        ``KeyStream.frames`` (R, P, T), for tests and debugging.

        ``posteriors=True`` (with ``smooth=True``) adds what ``track(smooth=True, posteriors=True)`` has offline, at the same lag as the
        path: ``posteriors`` (R, k2, 24), the probability of each key at window v given the audio up to window ``v + lag_windows`` --
        ``metrics.key_posteriors`` on that prefix, the evidence the label of v was decided on; after ``finish()`` the last
        ``lag_windows`` windows hold the offline posteriors --, ``smooth_confidence`` (R, k2), its entry at ``smooth_key_id``, and
        ``log_likelihood`` (R, k), the running log-score of the recording under the transition after each new window
        (``metrics.key_stream_posteriors``; two more launches a push, ``ake_key_stream_posteriors_f32``).

        ``method="profile"`` needs no net, so ``KeyEstimator(None, ...)`` streams: the windows are scored as
        ``track(method="profile")`` scores them, with ``profiles``, ``compression`` and ``profile_sharpness`` as there.  Such a stream keeps
        no frame cache and no net workspace but a ring of per-frame chroma, 12 doubles a frame: a push computes the chroma of every new
        frame once (``ake_stream_frame_stats_f32``) and scores the windows it completed from the ring
        (``ake_stream_profile_emissions_f32``), two launches in place of the net's; on the stream's own frames
        (``keep_frames=True``) the result is ``ake_amd.profile_emissions``' to the bit, however the audio is cut.  The ``StreamUpdate`` holds
        what ``KeyTrack`` documents for the method (``key`` the chroma, ``genre`` None), ``emissions`` always, and the smoother and
        ``posteriors`` take those emissions as they take the net's.  ``signature_weight`` must be left at 1.

        ``tuning_meter=True``, with either method, adds ``StreamUpdate.tuning_cents`` and ``.tuning_strength`` (R,): ``estimate_tuning``
        over every final frame so far, from three sums carried on the device (``metrics.stream_tuning``; ``tuning_min_strength`` as
        ``min_strength`` there).  It rides in the profile method's frame launch; on a ``"net"`` stream it is that launch with the chroma
        part off, one more launch per piece that has new frames.  The meter itself retunes nothing.

        ``retune_cents=c`` (one number within +-50, the same for all recordings) retunes the stream as ``track(tuning=c)`` retunes a
        recording: an ``ake_amd.StreamRetuner`` stands behind the optional resampler and in front of the history, the offline 64-tap
        varispeed filter carrying its last 64 inputs from push to push, so the stream sees ``ake_amd.retune(whole, c)`` bit for bit
        however the audio is cut (one or two small launches a push: ``ake_stream_retune_f32``; the ratio ``rho = 2 ** (c / 1200)`` is
        read off the device once, here, and a push still reads nothing back).  Everything downstream counts retuned samples: after N
        samples the stream has emitted the windows ``track(audio, tuning=c)`` gives.  ``StreamUpdate.times`` are divided by ``rho``, so
        they are seconds of the recording as it was pushed; ``StreamUpdate.retune_cents`` carries c; with ``tuning_meter=True`` the meter
        sees the retuned audio and reports the detuning that is left.  ``max_chunk_samples`` counts samples in front of the retuner.
        ``None`` and ``0`` leave the stream as it is without the keyword: the same launches, the same bits.  The number is the caller's:
        a stream does not retune itself from its meter, which would take a read-back or a ratio that changes in mid-stream.

        ``refine=True`` (both methods) places every key change to the frame as ``track(refine=True)`` does, inside the stream: every update
        carries the boundaries it made final -- boundary w, between the windows w and w + 1, once the label of window w + 2 is decided
        (``smooth_key_id`` with ``smooth=True``, so ``lag_windows`` later, else ``key_id``) and frame ``m_{w+1} + slack`` is final, and at
        ``finish()`` the rest (``metrics.stream_changes_ready``) -- in ``StreamUpdate.change_first_boundary``, ``change_frame`` (frames of
        the stream), ``change_gain``, ``change_contrast`` and ``change_times`` (seconds of the recording as pushed).  One more launch per
        push that brings labels (``ake_stream_key_changes_f32``; host model ``metrics.stream_key_changes``) reads the per-frame chroma
        ring of the profile method, 96 bytes a frame, never the transform; a ``"net"`` stream keeps that ring for it (the chroma part of
        ``ake_stream_frame_stats_f32``, one more launch per piece that has new frames, shared with the meter).  ``profiles`` and
        ``compression`` apply as for ``method="profile"``, ``refine_slack_seconds`` (default: the stride) as on ``track``.  On the stream's
        own frames and labels the joined fields are ``ake_amd.key_changes``' to the bit, however the audio is cut.  Labels are not
        revised from the frames, and there is one change per pair of windows.  Without it a stream is what it was: the same launches,
        the same bits.

        Refused with a ``ValueError``: ``posteriors=True`` with ``smooth=False``; a ``refine_slack_seconds`` that is negative or whose span
        ``stride + 2 * slack`` exceeds 1024 frames; what ``track`` refuses (``frames=0``, ``wrap_mode="true_end"``, ``--local`` nets), with
        ``method="net"`` an estimator without a net, ``rate`` other than the estimator's (``rate`` names the rate the stream works at; what arrives is
        ``source_rate``), multi-channel chunks on a stream opened without ``source_channels``, ``tuning``, ``lag_windows`` outside
        0..255; by ``push``: a chunk after ``finish()``, a chunk whose R (or C) differs from the stream's, on a stream without a source
        format a dtype that differs from the first chunk's; ``retune_cents`` that is no number within +-50, or on an estimator whose
        top bin lies above 0.94 of the Nyquist frequency (as ``track(tuning=...)``).  Not built: automatic retuning inside a stream
        (from its own meter), chunk lengths that differ between recordings, and a weighting of the bins in the chroma."""
        from .stream import KeyStream
        if rate is not None and int(rate) != self.sample_rate:
            raise ValueError(f"stream: rate is the rate the stream works at, the estimator's ({self.sample_rate} Hz); for chunks at "
                             f"another rate pass source_rate={int(rate)} (and source_channels), which resamples them with carried state")
        if tuning is not None:
            raise ValueError("stream: tuning (estimating and retuning as track does) is not offered inside a stream; tuning_meter=True "
                             "reports the running estimate in StreamUpdate.tuning_cents / .tuning_strength, and retune_cents=c retunes "
                             "the stream by a number of cents the caller names")
        return KeyStream(self, recordings, window_seconds, stride_seconds, smooth, lag_windows, mean_key_seconds, transition, log_prior,
                         signature_weight, keep_frames, max_chunk_samples, posteriors, source_rate, source_channels, channel, method,
                         profiles, compression, profile_sharpness, tuning_meter, tuning_min_strength, retune_cents, refine,
                         refine_slack_seconds)

    def _refuse_untrackable(self):
        """What ``track`` and ``training_windows`` cannot slide windows over."""
        if self.frames <= 0:
            raise ValueError("track() needs a fixed frame rate: this estimator was built with frames=0 (whole-song mode)")
        if self.wrap_mode == "true_end":
            raise ValueError("track() runs every window unpadded; wrap_mode 'true_end' has no meaning here: build the estimator with 'dataset_max'")
        if getattr(self.net, "local", False):
            raise ValueError("track() slides a clip-level net over the recording: a --local net is not tracked "
                             "(it has its own per-frame forward, and its rows are not time frames)")

    @torch.no_grad()
    def training_windows(self, audio: torch.Tensor, annotations: KeyAnnotations, lengths: torch.Tensor | None = None, rate: int | None = None,
                         channel: int = 0, window_seconds: float = 15.0, batch_size: int = 8, batches_per_epoch: int | None = None,
                         stride_seconds: float | None = None, seed: int = 0, weighting: str = "purity", min_purity: float = 0.0,
                         sequence_windows: int | None = None, mean_key_seconds: float = 60.0, transition: torch.Tensor | None = None):
        """Training batches cut from annotated recordings on the device -> ``ake_amd.TrackWindows``, which
        ``Trainer.fit(net, train_dataloaders=...)`` takes as it takes a ``DataLoader``.

        ``audio``, ``lengths``, ``rate`` and ``channel`` mean what they mean in ``track`` (int16 is 16-bit PCM), and the windows are
        ``track``'s: every recording is transformed ONCE at the estimator's hop, here and now, and the transform stays on the device
        (``T_i = 1 + lengths[i] // hop`` frames); a window is ``1 + round(window_seconds * sample_rate) // hop`` consecutive frames of
        it, so its edge frames have seen the neighbouring audio, as the windows ``track`` feeds the net have.  ``annotations``
        (``KeyAnnotations``, in samples at the estimator's rate) give every window its labels and its weight.

        ``stride_seconds=None``: every epoch draws ``batches_per_epoch`` batches of ``batch_size`` windows at random start frames, from
        ``seed`` and the epoch.  ``stride_seconds`` given: ``track``'s own windows at that stride, in order (for validation).
        ``weighting`` and ``min_purity``: see ``TrackWindows``.  Refused with a ``ValueError``: what ``track`` refuses, annotations of
        another number of recordings or another sample rate, and recordings none of which holds one window.  The lengths are read on
        the host once, here; iterating the result waits for nothing.

        ``sequence_windows=K`` (with ``stride_seconds``, which then is the stride inside a sequence): every batch is ``batch_size``
        sequences of K consecutive ``track`` windows at random starts, for ``PitchClassNet.general_step``'s sequence loss
        (``TrackWindows``' sequence mode has the batch's extra entries).  Its ``log_trans`` is the transition ``track(smooth=True)``
        would use at this stride with ``mean_key_seconds``, or ``transition``, a (24, 24) tensor that is passed through as it is: one
        that requires grad receives the loss's gradient and is trained by the caller's optimiser.  Refused: K < 2, a missing stride,
        and recordings none of which holds one sequence."""
        from .windows import TrackWindows
        self._need_net("KeyEstimator.training_windows")
        self._refuse_untrackable()
        if annotations.sample_rate and annotations.sample_rate != self.sample_rate:
            raise ValueError(f"training_windows: the annotations are in samples at {annotations.sample_rate} Hz, the estimator runs at {self.sample_rate} Hz")
        if annotations.seg_start.shape[0] != audio.shape[0]:
            raise ValueError(f"training_windows: {audio.shape[0]} recordings, but annotations of {annotations.seg_start.shape[0]}")
        if audio.dim() == 3 or (rate is not None and int(rate) != self.sample_rate):
            rs = get_resampler(self.sample_rate if rate is None else int(rate), self.sample_rate, self.device)
            audio, len_out = rs(audio, channel=channel, lengths=lengths)
            lengths = len_out if lengths is not None else None
        hop = self.plan.hop_length
        mel = self.plan.logmag(audio, lengths=lengths)                                       # (R, P, T), zeros behind a recording's end
        T = mel.shape[2]
        frames = [T] * mel.shape[0] if lengths is None else [min(1 + int(n) // hop, T) for n in torch.as_tensor(lengths).reshape(-1).tolist()]
        wf = track_window_frames(int(round(window_seconds * self.sample_rate)), hop)
        if T < wf:
            raise ValueError("training_windows: no recording is as long as one window")
        sf = None if stride_seconds is None else track_stride_frames(stride_seconds, self.frames)
        log_trans = None
        if sequence_windows is not None:
            if sf is None:
                raise ValueError("training_windows: sequence_windows needs stride_seconds, the stride between a sequence's windows")
            if transition is None:
                log_trans = self._transition(sf, mean_key_seconds, None)
            elif not isinstance(transition, torch.Tensor) or tuple(transition.shape) != (24, 24):
                raise ValueError("training_windows: transition must be a (24, 24) tensor of log-probabilities, from key i (row) to key j")
            else:
                log_trans = transition
        return TrackWindows(mel, frames, annotations, hop, wf, batch_size=batch_size, batches_per_epoch=batches_per_epoch, stride_frames=sf,
                            seed=seed, weighting=weighting, min_purity=min_purity, genre_classes=11 if self.net.genre else 8,
                            sequence_windows=sequence_windows, log_trans=log_trans)

    def _transition(self, sf, mean_key_seconds, transition):
        """The (24, 24) float32 log transition matrix on the device: built and validated once per (stride, mean_key_seconds) or per
        user tensor (by identity and version; the entry keeps the tensor alive), not per call."""
        cache = self.__dict__.setdefault("_transitions", {})
        if transition is None:
            mean_key_seconds = float(mean_key_seconds)
            if not mean_key_seconds > 0.0:
                raise ValueError("track(smooth=True): mean_key_seconds must be positive")
            key = (sf, mean_key_seconds)
            if key not in cache:
                stride = sf * self.plan.hop_length / self.sample_rate
                cache[key] = (None, metrics.key_transition_log(stay=math.exp(-stride / mean_key_seconds)).to(device=self.device, dtype=torch.float32))
            return cache[key][1]
        if not isinstance(transition, torch.Tensor) or tuple(transition.shape) != (24, 24):
            raise ValueError("track(smooth=True): transition must be a (24, 24) tensor of log-probabilities, from key i (row) to key j")
        key = (id(transition), transition._version)
        if key not in cache:
            metrics._check_finite("transition", transition)
            cache[key] = (transition, transition.detach().to(device=self.device, dtype=torch.float32).contiguous())
        return cache[key][1]

    def _run_track(self, slot, audio, lengths, wf, sf, smoothing=None):
        net, L, dev = self.net, _lib.lib(), self.device
        pcm = audio.dtype == torch.int16
        if pcm:
            audio, row_stride = pcm16_rows(audio, dev)
        else:
            audio = audio.to(device=dev, dtype=torch.float32)
            if audio.stride(-1) != 1:
                audio = audio.contiguous()
        R, n = audio.shape
        hop = self.plan.hop_length
        W = track_counts(1 + n // hop, wf, sf)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        key, tonic, genre = f32(R, W, 12), f32(R, W, 12), f32(R, W, 11) if net.genre else None
        key_id, sig, tonic_id, conf, counts = i32(R, W), i32(R, W), i32(R, W), f32(R, W), i32(R)
        times = (torch.arange(W, dtype=torch.float64) * sf + (wf - 1) / 2) * hop / self.sample_rate
        track = KeyTrack(key, tonic, genre, key_id, sig, tonic_id, conf, counts, times, wf * hop / self.sample_rate, sf * hop / self.sample_rate)
        track.hop, track.window_frames, track.stride_frames, track.sample_rate = int(hop), int(wf), int(sf), self.sample_rate
        if smoothing is not None:
            track.emissions, track.smooth_key_id = f32(R, W, 24), i32(R, W)
            if smoothing[2]:
                track.posteriors, track.smooth_confidence, track.log_likelihood = f32(R, W, 24), f32(R, W), f32(R)
        if W == 0:                                                   # every recording is shorter than one window
            counts.zero_()
            if track.log_likelihood is not None:
                track.log_likelihood.zero_()
            return track
        nbytes = L.ake_pipeline_track_workspace_bytes(self.plan.handle, net.handle, R, n, wf, sf)
        if nbytes == 0:
            _lib.check(-1, "ake_pipeline_track_workspace_bytes")
        if smoothing is not None:                                    # the back-pointers: after the track on the same stream, so in its workspace
            nbytes = max(int(nbytes), self._smooth_workspace_bytes(R, W, smoothing[2]))
        if slot["ws"] is None or slot["ws"].numel() < nbytes:
            slot["ws"] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        ws = slot["ws"]
        with torch.cuda.device(dev):
            outs = (key.data_ptr(), tonic.data_ptr(), genre.data_ptr() if genre is not None else None, key_id.data_ptr(), sig.data_ptr(),
                    tonic_id.data_ptr(), conf.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            if pcm:
                if lengths is not None:
                    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
                    assert lengths.shape == (R,)
                _lib.check(L.ake_pipeline_track_pcm16_f32(self.plan.handle, net.handle, audio.data_ptr(), R, n, row_stride,
                                                          lengths.data_ptr() if lengths is not None else None, wf, sf, *outs),
                           "ake_pipeline_track_pcm16_f32")
            elif lengths is None:
                _lib.check(L.ake_pipeline_track_f32(self.plan.handle, net.handle, audio.data_ptr(), R, n, audio.stride(0), wf, sf, *outs),
                           "ake_pipeline_track_f32")
            else:
                lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).contiguous()
                assert lengths.shape == (R,)
                _lib.check(L.ake_pipeline_track_ragged_f32(self.plan.handle, net.handle, audio.data_ptr(), R, n, audio.stride(0),
                                                           lengths.data_ptr(), wf, sf, *outs), "ake_pipeline_track_ragged_f32")
            if smoothing is not None:
                trans, weight, with_posteriors = smoothing
                stream = torch.cuda.current_stream().cuda_stream
                _lib.check(L.ake_key_emissions_f32(key.data_ptr(), tonic.data_ptr(), R * W, counts.data_ptr(), W, weight,
                                                   track.emissions.data_ptr(), stream), "ake_key_emissions_f32")
                self._smooth(track, trans, with_posteriors, ws, stream)
        return track

    @staticmethod
    def _smooth_workspace_bytes(R, W, with_posteriors):
        """Workspace of ``_smooth``: the Viterbi's back-pointers, then (same stream, after it, in the same place) a, b of the
        forward-backward pass."""
        L = _lib.lib()
        nbytes = L.ake_viterbi_keys_workspace_bytes(R, W)
        if nbytes == 0:
            _lib.check(-1, "ake_viterbi_keys_workspace_bytes")
        if with_posteriors:
            pbytes = L.ake_key_posteriors_workspace_bytes(R, W)
            if pbytes == 0:
                _lib.check(-1, "ake_key_posteriors_workspace_bytes")
            nbytes = max(int(nbytes), int(pbytes))
        return int(nbytes)

    @staticmethod
    def _smooth(track, trans, with_posteriors, ws, stream):
        """The Viterbi decode of ``track.emissions`` and, with ``with_posteriors``, the forward-backward pass over them, on ``stream``
        (the current device is the track's)."""
        L = _lib.lib()
        R, W = track.key_id.shape
        counts = track.counts
        _lib.check(L.ake_viterbi_keys_f32(track.emissions.data_ptr(), R, W, counts.data_ptr(), trans.data_ptr(), None,
                                          track.smooth_key_id.data_ptr(), ws.data_ptr(), ws.numel(), stream), "ake_viterbi_keys_f32")
        if with_posteriors:
            _lib.check(L.ake_key_posteriors_f32(track.emissions.data_ptr(), R, W, counts.data_ptr(), trans.data_ptr(), None,
                                                track.smooth_key_id.data_ptr(), track.posteriors.data_ptr(),
                                                track.log_likelihood.data_ptr(), None, track.smooth_confidence.data_ptr(),
                                                ws.data_ptr(), ws.numel(), stream), "ake_key_posteriors_f32")

    # ---- the profile method: key tracks without a net (csrc/profile.hip) ----

    def _refuse_unprofilable(self, what):
        if self.frames <= 0:
            raise ValueError(f"{what} needs a fixed frame rate: this estimator was built with frames=0 (whole-song mode)")
        if self.net is not None and getattr(self.net, "local", False):
            raise ValueError(f"{what}: the profile method is not offered on an estimator of a --local net; build one with KeyEstimator(None, ...)")

    def _refuse_untunable_chroma(self, what, tuning):
        if tuning is None:
            raise ValueError(f'{what} needs a tuning ("auto", "follow", a number of cents or a (B,) tensor of cents): it is the cents that '
                             f'move the chroma\'s class boundaries')
        if self.plan.n_bins % metrics.FOLDED_BINS != 0:
            raise ValueError(f"{what}: the tuned chroma folds whole octaves, and this estimator's {self.plan.n_bins} bins are no multiple of 36")

    def _tuned_cents(self, mel, frames, tuned, ws):
        """The cents of the tuned chroma, measured on the transform the chroma is cut from -> ``(cents, strength)``: (R,) twice for
        ``tuning="auto"`` (``ake_amd.estimate_tuning``; the ragged transform's zeros behind a row's frames add nothing, so no counts),
        the tuning track's ``curve`` and ``strength`` (R, W) for a ``_Follow``, on its windows; given cents as they are, with no
        strength."""
        cents, min_strength = tuned
        if isinstance(cents, _Follow):
            _, strength, curve, _ = _tuning.tuning_track(mel, cents.window_frames, cents.stride_frames, frames, min_strength, workspace=ws)
            return curve, strength
        if cents is None:
            return _tuning.estimate_tuning(mel, None, min_strength, workspace=ws)
        return cents, None

    def _resampled(self, audio, lengths, rate, channel):
        if audio.dim() == 3 or (rate is not None and int(rate) != self.sample_rate):
            rs = get_resampler(self.sample_rate if rate is None else int(rate), self.sample_rate, self.device)
            audio, len_out = rs(audio, channel=channel, lengths=lengths)
            lengths = len_out if lengths is not None else None
        return audio, lengths

    def _track_profile(self, audio, lengths, rate, channel, window_seconds, stride_seconds, smooth, mean_key_seconds, transition,
                       signature_weight, posteriors, tuning, min_strength, profiles, compression, sharpness, refine=False,
                       refine_slack_seconds=None, tuning_window_seconds=5.0, tuning_stride_seconds=1.0, tuned_chroma=False):
        self._refuse_unprofilable('track(method="profile")')
        if tuned_chroma:
            self._refuse_untunable_chroma('track(tuned_chroma=True)', tuning)
            if refine:
                raise ValueError("track(tuned_chroma=True): refine=True is not offered with it; the change-point kernel reads the uniform "
                                 "per-frame chroma")
        if float(signature_weight) != 1.0:
            raise ValueError('track(method="profile"): signature_weight weighs the net\'s key head, which this method does not run; leave it at 1')
        mode = metrics._profile_compression(compression)
        sharpness = float(sharpness)
        if not sharpness > 0.0:
            raise ValueError('track(method="profile"): profile_sharpness must be positive')
        prof = _keyprofile.device_profiles(profiles, self.device)    # (made on the caller's stream, which every side stream waits for)
        audio, lengths = self._resampled(audio, lengths, rate, channel)
        wf = track_window_frames(int(round(window_seconds * self.sample_rate)), self.plan.hop_length)
        sf = track_stride_frames(stride_seconds, self.frames)
        smoothing = (self._transition(sf, mean_key_seconds, transition), bool(posteriors)) if smooth else None
        if tuned_chroma and isinstance(tuning, str) and tuning == "follow":
            cents = _Follow(wf, sf)                                  # the tuning track runs on the key track's own windows
        else:
            cents = None if tuning is None else self._given_tuning(tuning, audio.shape[0], tuning_window_seconds, tuning_stride_seconds,
                                                                   retunes=not tuned_chroma)
        refining = (self._refining(sf, refine_slack_seconds, profiles, compression)[0], prof, mode) if refine else None

        def run(slot, a, l):
            used = strength = None
            if self.streams > 1:                                     # (a user's table is a fresh tensor of the caller's stream)
                prof.record_stream(torch.cuda.current_stream(self.device))
            if tuned_chroma:                                         # one transform; nothing is retuned
                return self._run_profile_track(slot, a, l, wf, sf, smoothing, prof, mode, sharpness, tuned=(cents, float(min_strength)))
            if tuning is not None:
                a, l, used, strength = self._retuned(slot, a, l, cents, min_strength)
            track = self._run_profile_track(slot, a, l, wf, sf, smoothing, prof, mode, sharpness, refining)
            _mark_tuning(track, used, strength)
            return track
        return self._issue(run, audio, lengths)

    def _profile_logmag(self, slot, audio, lengths, more_bytes=0):
        """One transform at the estimator's plan in the slot's workspace (sized for ``ake_profile_emissions_f32`` and ``more_bytes`` too:
        they run behind it on the same stream) -> ``(mel (R, P, T), frame counts int32 (R,) or None, workspace)``."""
        L = _lib.lib()
        if audio.dtype != torch.int16:
            audio = audio.to(device=self.device, dtype=torch.float32)
        R, n = audio.shape
        T = self.plan.num_frames(n)
        pbytes = int(L.ake_profile_workspace_bytes(R, T))
        if pbytes == 0:
            _lib.check(-1, "ake_profile_workspace_bytes")
        ws = self._slot_ws(slot, max(int(L.ake_cqt_workspace_bytes(self.plan.handle, R, n)), pbytes, int(more_bytes)))
        frames = None
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
            frames = (1 + lengths.clamp(0, n) // self.plan.hop_length).clamp(max=T).to(torch.int32)
        return self.plan.logmag(audio, lengths=lengths, workspace=ws), frames, ws

    def _tuned_bytes(self, R, T, wf, sf):
        """Workspace of the tuned chroma's launches on (R, T) frames: the tuning measurement's and ``ake_profile_emissions_tuned_f32``'s."""
        L = _lib.lib()
        nbytes = int(L.ake_profile_tuned_workspace_bytes(R, T))
        if nbytes == 0:
            _lib.check(-1, "ake_profile_tuned_workspace_bytes")
        return max(nbytes, int(L.ake_tuning_workspace_bytes(R, T)), int(L.ake_tuning_track_workspace_bytes(R, T, wf, sf)) if wf > 0 else 0)

    _sig_tables = {}

    @classmethod
    def _key_sig_table(cls, device):
        """int32 (24,) on ``device``: for every key of ``KEY_NAMES`` the first ``KEY_SIGNATURE_MAP`` row that carries its scale."""
        key = str(device)
        if key not in cls._sig_tables:
            rows = metrics.MAJOR_TONIC.tolist()
            cls._sig_tables[key] = torch.tensor([rows.index(m) for m in metrics.KEY_MAJOR_TONIC], dtype=torch.int32, device=device)
        return cls._sig_tables[key]

    def _run_profile_track(self, slot, audio, lengths, wf, sf, smoothing, prof, mode, sharpness, refining=None, tuned=None):
        dev = self.device
        R, n = audio.shape
        hop = self.plan.hop_length
        W = track_counts(1 + n // hop, wf, sf)
        times = (torch.arange(W, dtype=torch.float64) * sf + (wf - 1) / 2) * hop / self.sample_rate
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        if W == 0:                                                   # every recording is shorter than one window
            track = KeyTrack(f32(R, 0, 12), f32(R, 0, 12), None, i32(R, 0), i32(R, 0), i32(R, 0), f32(R, 0), i32(R).zero_(), times,
                             wf * hop / self.sample_rate, sf * hop / self.sample_rate, emissions=f32(R, 0, 24))
        else:
            sbytes = 0 if smoothing is None else self._smooth_workspace_bytes(R, W, smoothing[1])
            if tuned is None:
                mel, frames, ws = self._profile_logmag(slot, audio, lengths, sbytes)
                chroma, emissions, key_id, conf = _keyprofile._launch(mel, False, frames, wf, sf, W, prof, mode, sharpness, ws)
            else:                                                    # the tuned chroma: the cents from this transform, then the cut
                mel, frames, ws = self._profile_logmag(slot, audio, lengths, max(sbytes, self._tuned_bytes(R, self.plan.num_frames(n), wf, sf)))
                cents, strength = self._tuned_cents(mel, frames, tuned, ws)
                chroma, emissions, key_id, conf = _keyprofile._launch(mel, False, frames, wf, sf, W, prof, mode, sharpness, ws, cents)
            counts = torch.full((R,), W, dtype=torch.int32, device=dev) if frames is None else \
                track_counts(frames.to(torch.int64), wf, sf).to(torch.int32)
            tonic = torch.maximum(emissions[..., :12], emissions[..., 12:])
            undecided = key_id < 0
            minus = torch.full_like(key_id, -1)
            tonic_id = torch.where(undecided, minus, key_id % 12)
            sig = torch.where(undecided, minus, self._key_sig_table(dev)[key_id.clamp_min(0).to(torch.int64)])
            track = KeyTrack(chroma, tonic, None, key_id, sig, tonic_id, conf, counts, times, wf * hop / self.sample_rate,
                             sf * hop / self.sample_rate, emissions=emissions)
        track.hop, track.window_frames, track.stride_frames, track.sample_rate = int(hop), int(wf), int(sf), self.sample_rate
        if tuned is not None:
            track.tuned_chroma = True
            if W == 0:                                               # no window, no transform: given cents stay, nothing was measured
                cents, strength = (tuned[0], None) if isinstance(tuned[0], torch.Tensor) else \
                    (f32(R, 0), f32(R, 0)) if isinstance(tuned[0], _Follow) else (f32(R).zero_(), f32(R).zero_())
            track.tuning_cents, track.tuning_strength = cents, strength
        if smoothing is not None:
            track.smooth_key_id = i32(R, W)
            if smoothing[1]:
                track.posteriors, track.smooth_confidence, track.log_likelihood = f32(R, W, 24), f32(R, W), f32(R)
            if W == 0:
                if track.log_likelihood is not None:
                    track.log_likelihood.zero_()
            else:
                with torch.cuda.device(dev):
                    self._smooth(track, smoothing[0], smoothing[1], ws, torch.cuda.current_stream().cuda_stream)
        if refining is not None:                                     # on the log-CQT this track was made from
            self._refine(track, mel if W > 1 else None, frames if W > 1 else None, refining)
        return track

    @torch.no_grad()
    def profile_key(self, audio: torch.Tensor, lengths: torch.Tensor | None = None, rate: int | None = None, channel: int = 0,
                    tuning=None, min_strength: float = 0.0, profiles="krumhansl", compression: str = "log", sharpness: float = 10.0,
                    tuning_window_seconds: float = 5.0, tuning_stride_seconds: float = 1.0, tuned_chroma: bool = False):
        """One key per clip without a net -> ``(key_id int32 (B,), confidence (B,), chroma (B, 12), emissions (B, 24))`` on the device:
        one transform at the estimator's plan, then ``ake_amd.profile_emissions`` in its whole-clip mode (``window_frames=0``: every
        clip's chroma over its own ``1 + lengths[i] // hop`` frames; ``metrics.profile_emissions`` is the definition).  ``audio``,
        ``lengths``, ``rate``, ``channel``, ``tuning``, ``min_strength``, ``streams`` > 1 and ``join()`` as in ``__call__``; ``profiles``,
        ``compression`` and ``sharpness`` as in ``ake_amd.profile_emissions``.  ``key_id`` is -1 for a silent clip.  Refused with a
        ``ValueError`` on ``frames=0`` estimators.

        ``tuned_chroma=True`` (with a ``tuning``, else ``ValueError``; bins that are no multiple of 36 likewise): the clip is not
        retuned; one transform, then ``ake_amd.profile_emissions(cents=...)`` cuts the chroma by the cents (``track`` has the details).
        ``"auto"`` and ``"follow"`` both use the whole-clip estimate (``ake_amd.estimate_tuning`` with ``min_strength``), a number or a
        (B,) tensor is used as given; ``tuning_window_seconds`` and ``tuning_stride_seconds`` are not read."""
        self._refuse_unprofilable("profile_key")
        if tuned_chroma:
            self._refuse_untunable_chroma("profile_key(tuned_chroma=True)", tuning)
        mode = metrics._profile_compression(compression)
        sharpness = float(sharpness)
        if not sharpness > 0.0:
            raise ValueError("profile_key: sharpness must be positive")
        prof = _keyprofile.device_profiles(profiles, self.device)
        audio, lengths = self._resampled(audio, lengths, rate, channel)
        if tuned_chroma and isinstance(tuning, str) and tuning == "follow":
            cents = None                                             # one window, the clip: the whole-clip estimate, as "auto"
        else:
            cents = None if tuning is None else self._given_tuning(tuning, audio.shape[0], tuning_window_seconds, tuning_stride_seconds,
                                                                   retunes=not tuned_chroma)

        def run(slot, a, l):
            if self.streams > 1:
                prof.record_stream(torch.cuda.current_stream(self.device))
            if tuned_chroma:                                         # one transform; nothing is retuned
                R, n = a.shape
                mel, frames, ws = self._profile_logmag(slot, a, l, self._tuned_bytes(R, self.plan.num_frames(n), 0, 1))
                used = self._tuned_cents(mel, frames, (cents, float(min_strength)), ws)[0]
                chroma, emissions, key_id, conf = _keyprofile._launch(mel, False, frames, 0, 1, 1, prof, mode, sharpness, ws, used)
                return key_id[:, 0], conf[:, 0], chroma[:, 0], emissions[:, 0]
            if tuning is not None:
                a, l = self._retuned(slot, a, l, cents, min_strength)[:2]
            mel, frames, ws = self._profile_logmag(slot, a, l)
            chroma, emissions, key_id, conf = _keyprofile._launch(mel, False, frames, 0, 1, 1, prof, mode, sharpness, ws)
            return key_id[:, 0], conf[:, 0], chroma[:, 0], emissions[:, 0]
        return self._issue(run, audio, lengths)

    @torch.no_grad()
    def fit_key_profiles(self, audio: torch.Tensor, annotations: KeyAnnotations, lengths: torch.Tensor | None = None,
                         window_seconds: float = 15.0, stride_seconds: float = 5.0, compression: str = "log", min_purity: float = 0.0):
        """Key profiles fitted to annotated recordings -> (2, 12) float64 on the device, rows minor and major, tonic first, which goes
        straight into ``profiles=`` of ``track(method="profile")``, ``profile_key`` and ``ake_amd.profile_emissions``.

        The windows are ``track``'s grid (``window_seconds``, ``stride_seconds``) and their chroma comes from the kernel
        (``ake_amd.profile_emissions`` with ``compression``); every window's label and weight come from ``metrics.window_labels`` (the key
        at its centre, weighted by its purity; 0 below ``min_purity`` and for unlabelled windows); ``metrics.fit_key_profiles`` then takes
        the weighted mean per mode.  Silent windows count for nothing.  ``audio`` (R, n) float32 or int16 at the estimator's rate;
        ``annotations`` in samples at that rate.  ``ValueError``: annotations of another number of recordings or another rate, no
        recording as long as one window, or a mode without a labelled window.  Runs on the current stream."""
        self._refuse_unprofilable("fit_key_profiles")
        if annotations.sample_rate and annotations.sample_rate != self.sample_rate:
            raise ValueError(f"fit_key_profiles: the annotations are in samples at {annotations.sample_rate} Hz, the estimator runs at {self.sample_rate} Hz")
        if audio.dim() != 2 or annotations.seg_start.shape[0] != audio.shape[0]:
            raise ValueError(f"fit_key_profiles: audio must be (R, n) with one row per annotated recording ({annotations.seg_start.shape[0]})")
        hop = self.plan.hop_length
        wf = track_window_frames(int(round(window_seconds * self.sample_rate)), hop)
        sf = track_stride_frames(stride_seconds, self.frames)
        mel, frames, ws = self._profile_logmag({"ws": None}, audio, lengths)                 # a workspace of its own: no side stream's
        R, W = mel.shape[0], track_counts(mel.shape[2], wf, sf)
        if W == 0:
            raise ValueError("fit_key_profiles: no recording is as long as one window")
        chroma, _, key_id, _ = _keyprofile.profile_emissions(mel, wf, sf, frames, compression=compression, workspace=ws)
        dev = self.device
        lab = metrics.window_labels(annotations.seg_start.to(dev), annotations.seg_key.to(dev), annotations.seg_count.to(dev),
                                    torch.arange(R, device=dev).repeat_interleave(W), torch.arange(W, device=dev).repeat(R) * sf, hop, wf,
                                    min_purity=min_purity)
        weight = torch.where(key_id.reshape(-1) >= 0, lab["sample_weight"], torch.zeros_like(lab["sample_weight"]))
        return metrics.fit_key_profiles(chroma.reshape(-1, 12), lab["truth"], weight)

    def _run_wrapped(self, slot, audio, lengths):
        """wrap_mode "true_end": one unpadded call per distinct frame count (the clips of a group share T, so no frame is padding)."""
        if self.frames <= 0:
            return self._run_whole_song(slot, audio, lengths)
        if self.wrap_mode != "true_end" or lengths is None:
            return self._run(slot, audio, lengths)
        lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64)
        lens = lengths.cpu()                                      # (opt-in mode: grouping needs the lengths on the host)
        frames = 1 + lens // self.plan.hop_length
        B = audio.shape[0]
        outs = [torch.empty((B, w), dtype=torch.float32, device=self.device) for w in ((12, 12, 11) if self.net.genre else (12, 12))]
        for t in torch.unique(frames).tolist():
            idx = torch.nonzero(frames == t).flatten()
            n_g = int(lens[idx].max())
            # a group's clips have the same frame count but not the same sample count: lengths stay (the CQT zero-pads the tails)
            sub = audio.index_select(0, idx.to(self.device))[:, :max(n_g, 1)].contiguous()
            if self.plan.num_frames(sub.shape[1]) != t:            # n_g rounds into the next hop only if a clip does: cannot happen
                raise _lib.AkeError("true_end grouping: frame count mismatch")
            got = self._run(slot, sub, lengths[idx.to(self.device)])
            for o, g in zip(outs, got):
                o.index_copy_(0, idx.to(self.device), g)
        return tuple(outs)

    def _run(self, slot, audio, lengths):
        net, L = self.net, _lib.lib()
        pcm = audio.dtype == torch.int16
        if pcm:
            audio, row_stride = pcm16_rows(audio, self.device)
        else:
            audio = audio.to(device=self.device, dtype=torch.float32)
            if audio.stride(-1) != 1:
                audio = audio.contiguous()
        B, n = audio.shape
        nbytes = L.ake_pipeline_workspace_bytes(self.plan.handle, net.handle, B, n)
        if slot["ws"] is None or slot["ws"].numel() < nbytes:
            slot["ws"] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        ws = slot["ws"]
        key = torch.empty((B, 12), dtype=torch.float32, device=self.device)
        tonic = torch.empty((B, 12), dtype=torch.float32, device=self.device)
        genre = torch.empty((B, 11), dtype=torch.float32, device=self.device) if net.genre else None
        with torch.cuda.device(self.device):
            if pcm:
                if lengths is not None:
                    lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
                    assert lengths.shape == (B,)
                _lib.check(L.ake_pipeline_forward_pcm16_f32(self.plan.handle, net.handle, audio.data_ptr(), B, n, row_stride,
                                                            lengths.data_ptr() if lengths is not None else None,
                                                            key.data_ptr(), tonic.data_ptr(), genre.data_ptr() if genre is not None else None,
                                                            ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                           "ake_pipeline_forward_pcm16_f32")
            elif lengths is None:
                _lib.check(L.ake_pipeline_forward_f32(self.plan.handle, net.handle, audio.data_ptr(), B, n, audio.stride(0),
                                                      key.data_ptr(), tonic.data_ptr(), genre.data_ptr() if genre is not None else None,
                                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                           "ake_pipeline_forward_f32")
            else:
                lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
                assert lengths.shape == (B,)
                _lib.check(L.ake_pipeline_forward_ragged_f32(self.plan.handle, net.handle, audio.data_ptr(), B, n, audio.stride(0), lengths.data_ptr(),
                                                             key.data_ptr(), tonic.data_ptr(), genre.data_ptr() if genre is not None else None,
                                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                           "ake_pipeline_forward_ragged_f32")
        return (key, tonic, genre) if net.genre else (key, tonic)

    def _run_whole_song(self, slot, audio, lengths):
        """frames=0: per-clip-hop CQT, then the net at (B, 1, n_bins, F) with no seq_length; one stream, no host synchronisation
        (W <= 592, or host lengths)."""
        net, L = self.net, _lib.lib()
        if audio.dtype == torch.int16:                               # 16-bit PCM: logmag_hops reads it in place
            audio = audio.to(device=self.device)
        else:
            audio = audio.to(device=self.device, dtype=torch.float32)
            if audio.stride(-1) != 1:
                audio = audio.contiguous()
        B, n = audio.shape
        W = self.window_size
        if W <= WHOLE_SONG_FRAMES:
            F = WHOLE_SONG_FRAMES                                    # T_i <= W <= 592
        else:                                                        # (the width depends on the longest clip's frame count)
            lens_host = torch.full((B,), n, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths).cpu().to(torch.int64)
            F = max(min(W, int((1 + lens_host // hop_for_window(lens_host, W)).max())), WHOLE_SONG_FRAMES)
        if lengths is None:
            hops = torch.full((B,), hop_for_window(n, W), dtype=torch.int32, device=self.device)
        else:
            lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int64).contiguous()
            hops = hop_for_window(lengths, W).to(torch.int32)
        nbytes = max(self.plan.workspace_bytes_hops(B, n, F), int(L.ake_pcnet_workspace_bytes(net.handle, B, F)))
        if slot["ws"] is None or slot["ws"].numel() < nbytes:
            slot["ws"] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        ws = slot["ws"]                                              # the CQT's, then (same stream, after it) the net's
        mel = self.plan.logmag_hops(audio, hops, lengths, out_frames=F, workspace=ws)
        key = torch.empty((B, 12), dtype=torch.float32, device=self.device)
        tonic = torch.empty((B, 12), dtype=torch.float32, device=self.device)
        genre = torch.empty((B, 11), dtype=torch.float32, device=self.device) if net.genre else None
        with torch.cuda.device(self.device):
            _lib.check(L.ake_pcnet_forward_f32(net.handle, mel.data_ptr(), B, F, None, key.data_ptr(), tonic.data_ptr(),
                                               genre.data_ptr() if genre is not None else None, ws.data_ptr(), ws.numel(),
                                               torch.cuda.current_stream().cuda_stream), "ake_pcnet_forward_f32")
        return (key, tonic, genre) if net.genre else (key, tonic)


def _device_e_step(emissions, log_trans, log_prior, counts):
    """The E-step of ``fit_key_transition`` on float32 (R, W, 24) ``emissions`` that live on the GPU: ``ake_key_posteriors_f32`` ->
    ``(loglik, xi_sum)``.  Runs on the current stream, in a workspace of its own."""
    L, dev = _lib.lib(), emissions.device
    R, W, _ = emissions.shape
    e = emissions.to(torch.float32).contiguous()
    A = torch.as_tensor(log_trans).to(device=dev, dtype=torch.float32).contiguous()
    prior = None if log_prior is None else torch.as_tensor(log_prior).to(device=dev, dtype=torch.float32).reshape(24).contiguous()
    cnt = None if counts is None else torch.as_tensor(counts).to(device=dev, dtype=torch.int32).reshape(R).contiguous()
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    post, loglik, xi = f32(R, W, 24), f32(R), f32(R, 24, 24)
    nbytes = L.ake_key_posteriors_workspace_bytes(R, W)
    if nbytes == 0:
        _lib.check(-1, "ake_key_posteriors_workspace_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(L.ake_key_posteriors_f32(e.data_ptr(), R, W, ptr(cnt), A.data_ptr(), ptr(prior), None, post.data_ptr(), loglik.data_ptr(),
                                            xi.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                   "ake_key_posteriors_f32")
    return loglik, xi


def fit_key_transition(tracks, init=None, iterations=10, tied=True, pseudo_count=1.0):
    """Fit a transition matrix to smooth tracks' own emissions by EM -> ``(log_trans, log_likelihoods)`` as ``metrics.fit_key_transition``,
    whose loop this is: the E-step (``ake_key_posteriors_f32``) runs on every track's device emissions and counts, the M-step on its 576
    numbers is ordinary torch (``metrics.transition_m_step``).  ``tracks``: one ``KeyTrack`` of ``track(smooth=True)`` or a list of
    them.  ``log_trans`` (float64, on the host) goes straight into ``track(transition=...)``.  It is the matrix under which these
    emissions score highest; ``profiles/track_accuracy.md`` scores tracks under it against ground truth on synthesised recordings."""
    tracks = list(tracks) if isinstance(tracks, (list, tuple)) else [tracks]
    if not tracks or any(not isinstance(t, KeyTrack) or t.emissions is None for t in tracks):
        raise ValueError("fit_key_transition: needs smooth tracks (KeyTrack.emissions); make them with track(..., smooth=True)")
    tracks = [t for t in tracks if t.emissions.shape[1] > 0]
    if not tracks:
        raise ValueError("fit_key_transition: every recording is shorter than one window")
    return metrics.fit_key_transition([t.emissions for t in tracks], counts=[t.counts for t in tracks], init=init, iterations=iterations,
                                      tied=tied, pseudo_count=pseudo_count, e_step=_device_e_step)
