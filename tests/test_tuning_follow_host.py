"""Host: the float64 models of the tuning track and the curve retuner (metrics.tuning_track, metrics.retune_curve_forward,
metrics.retune_curve_positions, metrics.retune_curve_reference), what they promise on a recording whose tuning drifts, through the
float64 oracle CQT, and the time translation of a followed track.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics
from test_tuning_host import HOP, SR, harmonic_clip, oracle_logmag

WF, SF = 25, 5                        # windows of 5 s every second at 5 frames per second: KeyEstimator's defaults for tuning="follow"
SECONDS = 40
KNOT_FIRST, KNOT_STEP = (WF - 1) // 2 * HOP, SF * HOP


def ramp_cents(t, seconds=SECONDS):
    """-35 cents at the start, +35 at the end (t in seconds)."""
    return -35.0 + 70.0 * np.asarray(t, dtype=np.float64) / seconds


def sine_cents(t, seconds=SECONDS):
    return 25.0 * np.sin(2 * np.pi * np.asarray(t, dtype=np.float64) / 30.0) + 5.0


def drifting_clip(seed, cents_fn, seconds=SECONDS, sr=SR):
    """harmonic_clip's notes with every frequency multiplied by 2 ** (c(t) / 1200): the phase is the running sum of the scale, float64."""
    n = seconds * sr
    rng = np.random.default_rng(9000 + seed)
    notes = int(rng.integers(8, 11))
    midi = rng.integers(40, 85, size=notes)
    phase = rng.uniform(0.0, 2 * np.pi, size=(notes, 5))
    scale = 2.0 ** (cents_fn(np.arange(n, dtype=np.float64) / sr, seconds) / 1200.0)
    warped = (np.cumsum(scale) - scale[0]) / sr                      # the time an in-tune copy has reached
    y, total = np.zeros(n), 0.0
    for i in range(notes):
        f0 = 440.0 * 2.0 ** ((midi[i] - 69) / 12.0)
        for h in range(1, 6):
            y += np.sin(2 * np.pi * f0 * h * warped + phase[i, h - 1]) / h
            total += 1.0 / h
    return y / (0.5 * total)


def window_centre_seconds(W, wf=WF, sf=SF):
    return (np.arange(W) * sf + (wf - 1) / 2) * HOP / SR


def phase_logmag(cents_rows, strength_rows=None, bins=36):
    """A log-CQT (B, bins, T) whose frame t of row b estimates to cents_rows[b][t]: power 1 + cos(angle - 2 pi j / 3) on bin position j,
    or the same power on all three where strength_rows[b][t] is False."""
    cents = np.asarray(cents_rows, dtype=np.float64)
    B, T = cents.shape
    L = np.zeros((B, bins, T))
    for j in range(3):
        p = 1.0 + np.cos(2 * np.pi * (cents / 100.0 - j / 3.0))
        if strength_rows is not None:
            p = np.where(np.asarray(strength_rows, dtype=bool), p, 1.0)
        L[:, j::3, :] = np.log1p(np.sqrt(p))[:, None, :]
    return L


# ---- the track: hand-built cases ----

def test_window_sums_equal_the_estimate_on_the_windows_frames():
    rng = np.random.default_rng(1)
    L = rng.uniform(0.0, 3.0, size=(3, 36, 13))
    c, s, _, n = metrics.tuning_track(L, 13, 4)                      # wf = T: the whole-recording estimate, the same bits
    want_c, want_s = metrics.estimate_tuning(L)
    assert c.shape == (3, 1) and n.tolist() == [1, 1, 1] and n.dtype == torch.int32
    assert torch.equal(c[:, 0], want_c) and torch.equal(s[:, 0], want_s)
    c, s, _, n = metrics.tuning_track(L, 5, 3)
    assert c.shape == (3, 3) and n.tolist() == [3, 3, 3]
    for w in range(3):
        want_c, want_s = metrics.estimate_tuning(L[:, :, 3 * w:3 * w + 5])
        assert float((c[:, w] - want_c).abs().max()) < 1e-9 and float((s[:, w] - want_s).abs().max()) < 1e-9
    c, s, _, n = metrics.tuning_track(L, 5, 3, counts=[13, 9, 7])    # ragged: a window ends with its recording
    assert n.tolist() == [3, 2, 1] and not bool(c[1, 2:].any()) and not bool(s[2, 1:].any())
    want_c, _ = metrics.estimate_tuning(L[1:2, :, 3:8])
    assert abs(float(c[1, 1] - want_c[0])) < 1e-9


def test_the_curve_unwraps_across_the_seam_and_saturates():
    """Raw cents 45, -48, -40: the second is 52 once unwrapped and is clamped to 50, the third 60 and stays there: no jump."""
    raw, strength, curve, _ = metrics.tuning_track(phase_logmag([[45.0, -48.0, -40.0]]), 1, 1)
    assert np.allclose(raw[0].numpy(), [45.0, -48.0, -40.0], atol=1e-9)
    assert np.allclose(curve[0].numpy(), [45.0, 50.0, 50.0], atol=1e-9)
    back = metrics.tuning_track(phase_logmag([[-45.0, 48.0, 40.0, 10.0]]), 1, 1)[2]
    assert np.allclose(back[0].numpy(), [-45.0, -50.0, -50.0, -50.0], atol=1e-9)       # -52, -60, -90


def test_weak_windows_hold_the_nearest_earlier_strong_value():
    cents = [[10.0, 20.0, 30.0, -10.0, 5.0], [10.0, 20.0, 30.0, -10.0, 5.0], [1.0, 2.0, 3.0, 4.0, 5.0]]
    strong = [[False, True, False, False, True], [True, True, True, True, True], [False, False, False, False, False]]
    raw, strength, curve, n = metrics.tuning_track(phase_logmag(cents, strong), 1, 1, min_strength=0.2)
    assert np.allclose(curve[0].numpy(), [20.0, 20.0, 20.0, 20.0, 5.0], atol=1e-9)     # the leading one takes the first strong window's
    assert np.allclose(curve[1].numpy(), cents[1], atol=1e-9)
    assert not bool(curve[2].any()) and float(strength[2].max()) < 1e-12                 # an all-weak row: 0
    assert np.allclose(raw[1].numpy(), cents[1], atol=1e-9)                              # min_strength is not applied to the windows
    at = metrics.tuning_track(phase_logmag(cents, strong), 1, 1, min_strength=float(strength[1, 0]))[2]
    assert np.allclose(at[1].numpy(), cents[1], atol=1e-9)                               # at equality a window is strong


def test_window_counts_of_short_and_empty_recordings():
    L = phase_logmag(np.tile(np.linspace(-30.0, 30.0, 12), (4, 1)))
    raw, strength, curve, n = metrics.tuning_track(L, 5, 2, counts=[12, 5, 3, 0])
    assert raw.shape == (4, 4) and n.tolist() == [4, 1, 1, 0]
    want, _ = metrics.estimate_tuning(L[2:3, :, :3])                                     # T_i < wf: one window over all its frames
    assert abs(float(raw[2, 0] - want[0])) < 1e-9
    assert not bool(raw[3].any()) and not bool(strength[3].any()) and not bool(curve[3].any())
    assert bool((curve[2, 1:] == curve[2, 0]).all()) and bool((curve[1, 1:] == curve[1, 0]).all())   # behind the count: the last value
    assert [metrics.tuning_track_windows(t, 5, 2) for t in (0, 1, 4, 5, 6, 7, 12)] == [0, 1, 1, 1, 1, 2, 4]
    assert metrics.tuning_track(np.zeros((2, 36, 3)), 25, 5)[0].shape == (2, 1)          # wf > T
    with pytest.raises(ValueError):
        metrics.tuning_track(L, 0, 1)
    with pytest.raises(ValueError):
        metrics.tuning_track(np.zeros((1, 37, 4)), 5, 1)


# ---- the curve's maps ----

def test_forward_and_inverse_maps_undo_each_other():
    rng = np.random.default_rng(2)
    curves = [rng.uniform(-50.0, 50.0, size=(3, 30)), np.tile(np.where(np.arange(30) % 2 == 0, 50.0, -50.0), (2, 1)), np.full((1, 1), 33.3),
              np.array([[np.nan, 80.0, -80.0, 12.5]])]
    for cents in curves:
        for first, step in ((0, 64), (1000, 1000), (55125, 22050)):
            B, K = cents.shape
            p = torch.tensor(rng.uniform(0.0, first + (K + 2.0) * step, size=(B, 300)))
            k = metrics.retune_curve_forward(p, cents, first, step)
            back = metrics.retune_curve_positions(k, cents, first, step)
            assert float((back - p).abs().max()) < 1e-9, (cents.shape, first, step)
            assert bool((k[:, 1:][p[:, 1:] > p[:, :-1]] > k[:, :-1][p[:, 1:] > p[:, :-1]]).all())   # increasing
    rho = 2.0 ** (20.0 / 1200.0)
    k = metrics.retune_curve_forward(torch.tensor([0.0, 100.0, 5000.0], dtype=torch.float64), np.full(4, np.float32(20.0)), 500, 700)
    assert np.allclose(k.numpy(), np.array([0.0, 100.0, 5000.0]) * 2.0 ** (float(np.float32(20.0)) / 1200.0), rtol=1e-14) and rho > 1
    # a ramp of the ratio between two knots: the mean ratio times the distance
    k = metrics.retune_curve_forward(torch.tensor([1000.0, 2000.0], dtype=torch.float64), np.array([0.0, 50.0], dtype=np.float32), 1000, 1000)
    assert abs(float(k[1] - k[0]) - 1000.0 * (1.0 + metrics.RETUNE_MAX_RATIO) / 2.0) < 1e-9


def test_a_constant_curve_is_the_one_ratio_retuner():
    x = harmonic_clip(3, 20.0, n=SECONDS * SR)
    y, n_out = metrics.retune_curve_reference(x, np.full(36, 20.0), KNOT_FIRST, KNOT_STEP)
    want, want_n = metrics.retune_reference(x, 20.0)
    err = float(np.abs(y - want).max())
    print(f"constant curve of +20 cents against retune_reference on {SECONDS} s: n_out {n_out} / {want_n}, worst difference {err:.2e}")
    assert n_out == want_n and err < 1e-6
    z, n_z = metrics.retune_curve_reference(x[:5000], np.zeros(4), 0, 64)                # an all-zero curve: a copy
    assert n_z == 5000 and np.array_equal(z[:5000], x[:5000]) and not z[5000:].any()
    rows, n_rows = metrics.retune_curve_reference(np.stack([x[:3000], x[:3000]]), np.array([[np.nan, 0.0], [10.0, -10.0]]), 100, 64, [3000, 1000])
    assert n_rows[0] == 3000 and np.array_equal(rows[0, :3000], x[:3000]) and 0 < n_rows[1] <= 1001 and not rows[1, n_rows[1]:].any()


# ---- the drift table: a 40 s ramp from -35 to +35 cents through the oracle transform ----

@functools.lru_cache(maxsize=None)
def ramp_case():
    x = drifting_clip(0, ramp_cents)
    return x, oracle_logmag(x)


def windowed_detuning(y):
    """The worst |cents| over the windows of y's oracle transform."""
    raw, strength, _, _ = metrics.tuning_track(oracle_logmag(y), WF, SF)
    return float(raw.abs().max()), float(strength.min())


def test_drift_table_on_a_ramp():
    x, L = ramp_case()
    whole_c, whole_s = metrics.estimate_tuning(L)
    raw, strength, curve, n = metrics.tuning_track(L, WF, SF)
    W = int(n[0])
    truth = ramp_cents(window_centre_seconds(W))
    est_err = float(np.abs(raw[0].numpy() - truth).max())
    followed, n_f = metrics.retune_curve_reference(x, curve[0].numpy(), KNOT_FIRST, KNOT_STEP)
    left_follow, s_follow = windowed_detuning(followed[:n_f])
    one, n_one = metrics.retune_reference(x, float(whole_c))
    left_one, _ = windowed_detuning(one[:n_one])
    print(f"ramp -35 .. +35 over {SECONDS} s: whole-recording estimate {float(whole_c):+.2f} cents / strength {float(whole_s):.2f}; {W} windows, "
          f"worst error at the window centres {est_err:.2f} cents; worst windowed detuning left after following {left_follow:.2f} cents "
          f"(weakest window {s_follow:.2f}), after one-number retune {left_one:.2f} cents")
    assert est_err <= 3.0
    assert left_follow <= 3.0
    assert left_one >= 20.0


# ---- track times ----

def _followed_track():
    ids = torch.tensor([[3, 3, 15, 15, 15], [7, 7, 7, -1, -1]], dtype=torch.int32)
    z = torch.zeros((2, 5, 12))
    times = (torch.arange(5, dtype=torch.float64) * 25 + 37.5) * HOP / SR
    tr = ake_amd.KeyTrack(z, z, None, ids, ids, ids, torch.zeros((2, 5)), torch.tensor([5, 3], dtype=torch.int32), times, 76 * HOP / SR, 25 * HOP / SR)
    tr.hop, tr.window_frames, tr.stride_frames, tr.sample_rate = HOP, 76, 25, SR
    tr.tuning_curve = torch.stack([torch.linspace(-35.0, 35.0, 40), torch.linspace(20.0, -45.0, 40)]).to(torch.float32)
    tr.tuning_curve_strength = torch.ones((2, 40))
    tr.tuning_knot_first, tr.tuning_knot_step = KNOT_FIRST, KNOT_STEP
    return tr


def test_segments_of_a_followed_track_go_through_the_curve():
    tr = _followed_track()
    assert tr.tuning_cents is None and len(tr._tensors()) == 10 and tr._tensors()[-2] is tr.tuning_curve
    plain = _followed_track()
    plain.tuning_curve = plain.tuning_curve_strength = None
    for r in range(2):
        want = plain.segments(r)
        got = tr.segments(r)
        assert [g[2:] for g in got] == [w[2:] for w in want] and len(got) == (2 if r == 0 else 1)
        for g, w in zip(got, want):
            for mine, retuned_s in zip(g[:2], w[:2]):                                    # by hand through the model
                k = retuned_s * SR
                assert abs(k - round(k)) < 1e-6
                own = float(metrics.retune_curve_positions(torch.tensor([float(round(k))], dtype=torch.float64), tr.tuning_curve[r], KNOT_FIRST, KNOT_STEP)[0]) / SR
                assert abs(mine - own) < 1e-9
                back = float(metrics.retune_curve_forward(torch.tensor([mine * SR], dtype=torch.float64), tr.tuning_curve[r], KNOT_FIRST, KNOT_STEP)[0])
                assert abs(back - k) < 1e-6
        assert got[0][0] == 0.0
    # row 0 is flat at its start (its retuned copy is shorter there): the first boundary lies later in the recording's own time
    assert tr.segments(0)[0][1] > plain.segments(0)[0][1]


def test_score_of_a_followed_track_moves_the_boundaries_with_the_forward_map():
    tr = _followed_track()
    seg_start = torch.tensor([[0, 380000, 900000, metrics._I64_MAX], [0, 777777, metrics._I64_MAX, metrics._I64_MAX]], dtype=torch.int64)
    moved = metrics.curve_boundaries(seg_start, tr.tuning_curve, KNOT_FIRST, KNOT_STEP)
    assert int(moved[0, 3]) == metrics._I64_MAX and int(moved[0, 0]) == 0
    for r, s in ((0, 1), (0, 2), (1, 1)):
        want = float(metrics.retune_curve_forward(torch.tensor([float(seg_start[r, s])], dtype=torch.float64), tr.tuning_curve[r], KNOT_FIRST, KNOT_STEP)[0])
        assert int(moved[r, s]) == int(np.floor(want))
    assert int(moved[0, 1]) < 380000                                                     # row 0 is flat at its start: its copy is shorter
    with pytest.raises(ValueError):
        metrics.curve_boundaries(seg_start, tr.tuning_curve[:1], KNOT_FIRST, KNOT_STEP)
