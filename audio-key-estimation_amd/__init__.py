"""MI355X-native key-estimation hot path: CQT front end + PitchClassNet forward on HIP kernels.

Import as ``import ake_amd`` (the directory name carries a hyphen; ``ake_amd.py`` at the repo
root aliases it).  Reference-shaped modules: ``models`` (PitchClassNet), ``KeyDataset``
(KeyDataset + loaders), ``cqt`` (librosa.cqt stand-in), ``metrics`` (MIREX score).
"""
from . import _lib  # noqa: F401
from .audio import Resampler, StreamResampler, get_resampler, pcm16_to_float, prepare as prepare_audio  # noqa: F401
from .cqt import CQTPlan, cqt_logmag, get_any_hop_plan, get_plan, hop_for, hop_for_window  # noqa: F401
from .KeyDataset import DatasetLoader, KeyDataset, SyntheticSineMixLoader, WaveformLoader  # noqa: F401
from .metrics import (KEY_NAMES, KEY_PROFILES, KEY_SIGNATURE_MAP, decode_keys, key_emissions, key_posteriors, key_stream, key_stream_posteriors, key_transition_log, mirex_score,  # noqa: F401
                      retune_reference, track_score, transition_from_labels, transition_m_step, viterbi_keys, weighted_general_step, window_labels,
                      window_truth)
from .models import PitchClassNet  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .lightning_shim import Trainer  # noqa: F401
from .pipeline import KeyAnnotations, KeyEstimator, KeyTrack, TrackScore, fit_key_transition  # noqa: F401
from .keyprofile import fit_key_profiles, profile_emissions  # noqa: F401
from .keychanges import key_changes  # noqa: F401
from .synth import synth_partials  # noqa: F401
from .tuning import (StreamRetuner, estimate_tuning, retune, retune_curve, retune_curve_positions, retune_out_len,  # noqa: F401
                     tuning_track)
from .windows import TrackWindows, draw_windows, window_batch  # noqa: F401
from .sequence import key_sequence_loss  # noqa: F401
from .feeder import HostFeeder  # noqa: F401
from .stream import KeyStream, StreamUpdate  # noqa: F401

__all__ = ["PitchClassNet", "KeyDataset", "DatasetLoader", "SyntheticSineMixLoader", "WaveformLoader", "CQTPlan",
           "cqt_logmag", "get_plan", "hop_for", "KEY_SIGNATURE_MAP", "mirex_score", "decode_keys", "key_emissions", "viterbi_keys", "key_transition_log", "key_posteriors",
           "transition_m_step", "fit_key_transition", "KEY_NAMES", "KeyEstimator", "KeyTrack", "Resampler", "get_resampler",
           "prepare_audio", "pcm16_to_float", "HostFeeder", "KeyAnnotations", "TrackScore", "track_score", "window_truth",
           "transition_from_labels", "synth_partials", "TrackWindows", "draw_windows", "window_batch", "window_labels", "weighted_general_step",
           "estimate_tuning", "retune", "retune_out_len", "retune_reference", "tuning_track", "retune_curve", "retune_curve_positions",
           "profile_emissions", "fit_key_profiles", "KEY_PROFILES", "key_sequence_loss",
           "key_stream", "KeyStream", "StreamUpdate", "key_stream_posteriors", "StreamResampler", "StreamRetuner", "key_changes"]
