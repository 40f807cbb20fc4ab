"""The float64 model of the change-point refinement of key tracks (metrics.key_changes): no GPU."""
import numpy as np
import pytest
import torch

from ake_amd import metrics

MAJOR = (0, 2, 4, 5, 7, 9, 11)
C_MAJOR, FS_MAJOR = 12, 18


def scale_logmag(tonics, P=36):
    """A log-CQT (1, P, T) whose frame t holds the major scale on ``tonics[t]`` (1.0 on the centre bins of its seven semitones);
    a tonic of None leaves the frame silent."""
    L = torch.zeros((1, P, len(tonics)), dtype=torch.float64)
    for t, tonic in enumerate(tonics):
        if tonic is not None:
            for j in MAJOR:
                L[0, 3 * ((j + tonic) % 12), t] = 1.0
    return L


def random_case(seed, R=2, P=36, T=90, W=18):
    g = torch.Generator().manual_seed(seed)
    L = torch.rand((R, P, T), generator=g, dtype=torch.float64) * 3.0
    labels = torch.randint(0, 24, (R, W), generator=g)
    return L, labels


def by_hand(s, a, b, lo, hi, g):
    """change_frame, gain, contrast of one span, restated with numpy on the frame scores s (T, 24)."""
    C = [0.0]
    for t in range(lo, hi):
        C.append(C[-1] + (float(s[t, a]) - float(s[t, b])))
    j = int(np.argmax(C))                                            # (numpy's argmax is the first maximum)
    return lo + j, C[j] - C[g - lo], (2 * C[j] - C[-1]) / (hi - lo)


def test_a_change_from_c_major_to_f_sharp_major_is_found_at_its_frame():
    L = scale_logmag([0] * 17 + [6] * 23)
    frame, gain, contrast, margin = metrics.key_changes(L, torch.tensor([[C_MAJOR, FS_MAJOR]]), 16, 8)
    assert frame.dtype == torch.int32 and tuple(frame.shape) == (1, 1) and int(frame[0, 0]) == 17
    assert float(gain[0, 0]) >= 0.0 and float(contrast[0, 0]) > 0.0 and float(margin[0, 0]) > 0.0


def test_gain_and_contrast_follow_their_formulas_on_a_case_added_by_hand():
    """Frames of the C-major scale score p for C major and q for F sharp major; frames a tritone up score the other way round.  With
    delta = p - q, m_0 = 8, m_1 = 16 and slack 8 the span is 0..24: C rises by delta for 17 frames and falls for 7, so C_17 = 17 delta
    is the maximum, C_24 = 10 delta, the grid's frame is g = 8 + 4 = 12 and C_12 = 12 delta."""
    L = scale_logmag([0] * 17 + [6] * 23)
    prof = np.array(metrics.KEY_PROFILES["krumhansl"][1])
    x = np.array([1.0 if j in MAJOR else 0.0 for j in range(12)])
    delta = np.corrcoef(x, prof)[0, 1] - np.corrcoef(x, np.roll(prof, 6))[0, 1]
    assert delta > 0.5
    frame, gain, contrast, margin = metrics.key_changes(L, torch.tensor([[C_MAJOR, FS_MAJOR]]), 16, 8)
    assert int(frame[0, 0]) == 17
    assert float(gain[0, 0]) == pytest.approx(5 * delta, rel=1e-12)
    assert float(contrast[0, 0]) == pytest.approx((2 * 17 - 10) * delta / 24, rel=1e-12)
    assert float(margin[0, 0]) == pytest.approx(delta, rel=1e-12)   # (C_16 and C_18 are the runners-up)
    # the labels the wrong way round: C never rises above C_0 and ends at -10 delta, so the change stays at lo: the whole span goes
    # to the second key, C major, which 17 of its 24 frames fit
    frame, gain, contrast, _ = metrics.key_changes(L, torch.tensor([[FS_MAJOR, C_MAJOR]]), 16, 8)
    assert int(frame[0, 0]) == 0 and float(gain[0, 0]) == pytest.approx(12 * delta, rel=1e-12)
    assert float(contrast[0, 0]) == pytest.approx(10 * delta / 24, rel=1e-12)
    # a random recording against the restatement, slack 0 and 3
    L, labels = random_case(3)
    s = metrics.key_frame_scores(L).numpy()
    for slack in (0, 3):
        frame, gain, contrast, _ = metrics.key_changes(L, labels[:, :2], 16, 4, slack_frames=slack)
        for r in range(2):
            a, b = int(labels[r, 0]), int(labels[r, 1])
            assert a != b
            lo, hi = max(8 - slack, 0), 12 + slack
            want = by_hand(s[r], a, b, lo, hi, 10)
            assert int(frame[r, 0]) == want[0]
            assert float(gain[r, 0]) == pytest.approx(want[1], abs=1e-12) and float(contrast[r, 0]) == pytest.approx(want[2], abs=1e-12)
            assert float(gain[r, 0]) >= 0.0 and -2.0 <= float(contrast[r, 0]) <= 2.0


@pytest.mark.parametrize("compression", metrics.PROFILE_COMPRESSIONS)
def test_frame_scores_are_the_emissions_of_one_frame_windows(compression):
    L, _ = random_case(7, R=3, T=40)
    L[1, :, 5] = 0.0                                                 # a silent frame
    L[2, :, 9] = 1.5                                                 # a frame of constant chroma: silent by the rule
    counts = [40, 33, 12]
    prof = torch.rand((2, 12), generator=torch.Generator().manual_seed(2), dtype=torch.float64) + 0.2
    for profiles in ("krumhansl", prof):
        s = metrics.key_frame_scores(L, counts, profiles, compression)
        want = metrics.profile_emissions(L, 1, 1, counts, profiles, compression, sharpness=1.0)[1]
        assert torch.equal(s, want)
        assert not bool(s[1, 5].any()) and not bool(s[2, 9].any()) and not bool(s[1, 33:].any()) and not bool(s[2, 12:].any())
        assert bool(s[0].abs().amax(dim=1).gt(0).all())


@pytest.mark.parametrize("slack,long_runs", [(11, False), (4, False), (2, True), (0, True)])
def test_runs_of_one_window_clip_the_span_and_the_frames_never_decrease(slack, long_runs):
    """Runs of one window: the span stops at the centres of the windows on either side, so neighbouring spans share one frame at the
    most and the change frames never decrease, whatever the slack.  (A run of k >= 2 windows keeps its two spans apart only when
    (k - 1) * stride_frames >= 2 * slack_frames: the cases with longer runs keep the slack at half a stride or less.)"""
    wf, sf = 16, 4
    for seed in range(6):
        L, labels = random_case(100 + seed)
        R, W = labels.shape
        steps = torch.randint(1, 24, (R, W), generator=torch.Generator().manual_seed(seed))
        labels = steps.cumsum(dim=1) % 24                            # every window differs from the one before it
        if long_runs:
            labels[0, 5:9] = labels[0, 5]
            labels[1, 10:12] = labels[1, 10]
        frame, gain, _, _ = metrics.key_changes(L, labels, wf, sf, slack_frames=slack)
        s = metrics.key_frame_scores(L).numpy()
        for r in range(R):
            seen = -1
            for w in range(W - 1):
                a, b = int(labels[r, w]), int(labels[r, w + 1])
                if a == b:
                    assert int(frame[r, w]) == -1
                    continue
                m0, m1 = w * sf + wf // 2, (w + 1) * sf + wf // 2
                lo = m0 if w >= 1 and int(labels[r, w - 1]) != a else max(m0 - slack, 0)
                hi = m1 if w + 2 < W and int(labels[r, w + 2]) != b else min(m1 + slack, L.shape[2])
                f = int(frame[r, w])
                assert lo <= f <= hi, (seed, r, w)
                assert f == by_hand(s[r], a, b, lo, hi, min(max(m0 + 2, lo), hi))[0]
                assert f >= seen, (seed, r, w)                       # non-decreasing along the recording
                seen = f
                assert float(gain[r, w]) >= 0.0


def test_windows_without_a_key_and_behind_the_count_have_no_boundary():
    L, labels = random_case(11)
    labels[:, :] = torch.arange(18)[None, :] % 24                    # every neighbouring pair differs
    labels[0, 4] = -1
    labels[0, 9] = 24                                                # no key either
    frame, gain, contrast, margin = metrics.key_changes(L, labels, 16, 4, counts=[90, 50], window_counts=[18, 12])
    none = torch.zeros((2, 17), dtype=torch.bool)
    none[0, [3, 4, 8, 9]] = True
    none[1, 8:] = True                                               # 50 frames hold (50 - 16) // 4 + 1 = 9 windows: fewer than the 12 given
    assert torch.equal(frame < 0, none)
    assert bool((frame[none] == -1).all()) and not bool(gain[none].any()) and not bool(contrast[none].any()) and not bool(margin[none].any())
    assert bool((frame[~none] >= 0).all())
    short = metrics.key_changes(L, labels, 16, 4, window_counts=[1, 0])
    assert bool((short[0] == -1).all()) and not bool(short[1].any()) and not bool(short[2].any())
    assert bool((metrics.key_changes(L, labels, 16, 4, counts=[19, 0])[0] == -1).all())      # one window each, or none
    assert [tuple(t.shape) for t in metrics.key_changes(L, labels[:, :1], 16, 4)] == [(2, 0)] * 4
    # the last boundary's span ends with the recording's frames
    frame, *_ = metrics.key_changes(L, labels, 16, 4, counts=[90, 49], slack_frames=40)
    assert int(frame[1, 7]) <= 49 and bool((frame[1, 8:] == -1).all())


def test_an_all_silent_span_stays_at_its_first_frame():
    L = scale_logmag([0] * 4 + [None] * 30 + [6] * 6)
    frame, gain, contrast, margin = metrics.key_changes(L, torch.tensor([[C_MAJOR, FS_MAJOR]]), 16, 8, slack_frames=2)
    assert int(frame[0, 0]) == 6 and float(gain[0, 0]) == 0.0 and float(contrast[0, 0]) == 0.0 and float(margin[0, 0]) == 0.0


def test_arguments_are_checked():
    L, labels = random_case(1)
    for bad in (dict(window_frames=0), dict(stride_frames=0), dict(slack_frames=-1), dict(compression="sqrt"), dict(profiles="nobody")):
        kw = dict(window_frames=16, stride_frames=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            metrics.key_changes(L, labels, **kw)
    with pytest.raises(ValueError):
        metrics.key_changes(L[:, :35], labels, 16, 4)
    with pytest.raises(ValueError):
        metrics.key_changes(L, labels[:1], 16, 4)


def hand_track(labels, change_frame, counts, smooth=True, cents=None):
    """A KeyTrack on the host with the geometry of 15 s windows 5 s apart at 5 frames a second, and refined boundaries given by hand."""
    from ake_amd import KeyTrack
    labels = torch.tensor(labels, dtype=torch.int32)
    R, W = labels.shape
    z = torch.zeros((R, W, 12))
    times = (torch.arange(W, dtype=torch.float64) * 25 + 75 / 2) * 4410 / 22050
    track = KeyTrack(z, z, None, labels if not smooth else torch.full_like(labels, -1), labels, labels, torch.zeros((R, W)),
                     torch.tensor(counts, dtype=torch.int32), times, 76 * 0.2, 5.0)
    track.hop, track.window_frames, track.stride_frames, track.sample_rate = 4410, 76, 25, 22050
    if smooth:
        track.emissions, track.smooth_key_id = torch.zeros((R, W, 24)), labels
    if change_frame is not None:
        track.change_frame = torch.tensor(change_frame, dtype=torch.int32)
        track.change_gain, track.change_contrast = torch.ones((R, W - 1)), torch.full((R, W - 1), 0.5)
        track.refined_source = "smooth_key_id" if smooth else "key_id"
    if cents is not None:
        track.tuning_cents = torch.tensor(cents, dtype=torch.float32)
    return track


def test_a_track_reads_its_refined_boundaries():
    sec = lambda frame: frame * 4410 / 22050                      # the track's own arithmetic, to the bit
    import ake_amd
    labels = [[3, 3, 3, 15, 15, 7, 7], [9, 9, 4, 4, 4, 4, 4]]
    frames = [[-1, -1, 101, -1, 158, -1], [-1, 77, -1, -1, -1, -1]]
    track, plain = hand_track(labels, frames, [7, 5]), hand_track(labels, None, [7, 5])
    assert len(track._tensors()) == len(plain._tensors()) + 3
    segs = track.segments(0)
    assert [(s[2], s[3]) for s in segs] == [(3, "Eb minor"), (15, "Eb major"), (7, "G minor")]
    assert [s[1] for s in segs[:-1]] == [sec(101), sec(158)] == [s[0] for s in segs[1:]]
    assert segs[0][0] == 0.0 and segs[-1][1] == plain.segments(0)[-1][1]
    assert track.segments(0, refined=False) == plain.segments(0) and track.segments(0, refined=True) == segs
    assert plain.segments(0)[0][1] == pytest.approx((2 * 25 + 37.5 + 12.5) * 0.2)           # the grid: halfway between two centres
    assert track.change_points(0) == [(sec(101), 3, 15, 1.0, 0.5), (sec(158), 15, 7, 1.0, 0.5)]
    assert track.change_points(1) == [(sec(77), 9, 4, 1.0, 0.5)]
    for refused in (lambda: plain.segments(0, refined=True), lambda: plain.change_points(0), lambda: track.segments(0, smoothed=False, refined=True),
                    lambda: plain.boundary_score(None, refined=True)):
        with pytest.raises(ValueError):
            refused()
    # two changes placed in the wrong order: the run between them is read as empty
    crossed = hand_track(labels, [[-1, -1, 120, -1, 110, -1], frames[1]], [7, 5])
    assert [(s[0], s[1]) for s in crossed.segments(0)[1:2]] == [(sec(120), sec(120))]
    # boundary_score: annotated changes at 20.0 s and 33.0 s (recording 0) and 14.0 s (recording 1); recording 1's second annotated
    # segment repeats its key and its third is unlabelled: neither is a key change
    ann = ake_amd.KeyAnnotations.from_segments([[(0.0, 3), (20.0, 15), (33.0, 7)], [(0.0, 9), (14.0, 4), (30.0, 4), (40.0, -1)]], 22050)
    got = track.boundary_score(ann, tolerance_seconds=0.5)
    assert got["count"] == 3
    want = sorted([abs(20.0 - 20.2), abs(33.0 - 31.6), abs(14.0 - 15.4)])
    assert got["median_abs_seconds"] == pytest.approx(want[1], abs=1e-9) and got["within_tolerance"] == pytest.approx(1 / 3)
    grid = track.boundary_score(ann, refined=False)
    want = sorted([abs(20.0 - 20.0), abs(33.0 - 30.0), abs(14.0 - 15.0)])                   # boundaries at (w * 25 + 50) frames of 0.2 s
    assert grid["median_abs_seconds"] == pytest.approx(want[1], abs=1e-9) and grid == plain.boundary_score(ann)
    still = hand_track([[5] * 7, [5] * 7], None, [7, 7]).boundary_score(ann)                # a track that never moves: infinitely far
    assert still["count"] == 3 and still["median_abs_seconds"] == float("inf") and still["within_tolerance"] == 0.0
    none = track.boundary_score(ake_amd.KeyAnnotations.from_segments([[(0.0, 3)], []], 22050))
    assert none["count"] == 0 and none["median_abs_seconds"] != none["median_abs_seconds"]
    # a retuned track: the refined times and the distances are seconds of the recording as it was handed in
    rho = 2.0 ** (30.0 / 1200.0)
    retuned = hand_track(labels, frames, [7, 5], cents=[30.0, 0.0])
    assert retuned.change_points(0)[0][0] == pytest.approx(sec(101) / rho, rel=1e-7)
    assert retuned.segments(0)[0][1] == pytest.approx(sec(101) / rho, rel=1e-7)
    got = retuned.boundary_score(ann)
    want = sorted([abs(int(20.0 * 22050 * rho) / 22050 - 20.2) / rho, abs(int(33.0 * 22050 * rho) / 22050 - 31.6) / rho, abs(14.0 - 15.4)])
    assert got["median_abs_seconds"] == pytest.approx(want[1], abs=1e-4)
