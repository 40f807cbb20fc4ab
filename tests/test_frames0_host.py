"""Host side of the whole-song data mode (--frames 0): the per-clip hop rule, the frame counts and the new C ABI entries (no GPU)."""
import os
import re

import pytest

from ake_amd import _lib
from ake_amd.cqt import WHOLE_SONG_FRAMES, hop_for_window, whole_song_frames
from conftest import REPO

LENGTHS = [1, 591, 592, 593, 22050 * 3, 44100 * 200]


@pytest.mark.parametrize("n", LENGTHS)
def test_hop_follows_the_reference_formula(n):
    w_length = n                                                      # KeyDataset.py:485,490: hop_length = w_length // opt.window_size + 1
    assert hop_for_window(n, 592) == w_length // 592 + 1
    assert hop_for_window(n) == hop_for_window(n, WHOLE_SONG_FRAMES) and WHOLE_SONG_FRAMES == 592


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("window", [592, 300, 1000])
def test_frame_count_never_exceeds_the_window(n, window):
    T = 1 + n // hop_for_window(n, window)                            # librosa center=True framing
    assert 1 <= T <= window


def test_padded_length_rule():
    # zero-padded to 592 (KeyDataset.py:212-215), cropped to the window (:501-503)
    for n in LENGTHS:
        T = 1 + n // hop_for_window(n, 592)
        assert whole_song_frames(n, 592) == 592 >= T
    assert whole_song_frames(22050 * 180, 1000) == 1000               # hop 3970: T = 1 + 999, more than 592 and not padded
    assert whole_song_frames(5000, 1000) == 834                       # hop 6: T = 834
    assert whole_song_frames(500, 1000) == 592                        # hop 1: T = 501, padded


def test_hop_rule_on_tensors():
    import torch
    n = torch.tensor(LENGTHS, dtype=torch.int64)
    assert hop_for_window(n, 592).tolist() == [v // 592 + 1 for v in LENGTHS]


def test_new_symbols_are_declared_and_bound():
    src = open(os.path.join(REPO, "include", "ake_hip.h")).read()
    for name in ("ake_cqt_workspace_bytes_hops", "ake_cqt_logmag_hops_f32"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().ake_version() >= 102
    # null plan: no workspace, and the call is refused before anything touches a device
    assert _lib.lib().ake_cqt_workspace_bytes_hops(None, 4, 1000, 592) == 0
    assert _lib.lib().ake_cqt_logmag_hops_f32(None, None, 1, 1000, 1000, None, None, None, 592, None, 0, None) == -1
