"""Host: the float64 models of the tuning estimate and the retuner (metrics.estimate_tuning, metrics.retune_reference), what they promise
on synthesised detuned clips through the float64 oracle CQT, and the time translation of a retuned track.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics
from oracle import cqt_oracle

SR, HOP = 22050, 4410
N15 = 15 * SR
DETUNINGS = (-45.0, -15.0, 20.0, 45.0)
THIRD = 100.0 / 3.0


def harmonic_clip(seed, cents, n=N15, sr=SR):
    """8 to 10 sustained notes (MIDI 40..84) of 5 partials each (amplitude 1 / h), every frequency scaled by 2 ** (cents / 1200); the
    same seed gives the same notes and phases at every detuning, so the in-tune clip is the detuned one played back at 1 / rho."""
    rng = np.random.default_rng(9000 + seed)
    notes = int(rng.integers(8, 11))
    midi = rng.integers(40, 85, size=notes)
    phase = rng.uniform(0.0, 2 * np.pi, size=(notes, 5))
    t = np.arange(n, dtype=np.float64) / sr
    y, total = np.zeros(n), 0.0
    for i in range(notes):
        f0 = 440.0 * 2.0 ** ((midi[i] - 69) / 12.0) * 2.0 ** (cents / 1200.0)
        for h in range(1, 6):
            y += np.sin(2 * np.pi * f0 * h * t + phase[i, h - 1]) / h
            total += 1.0 / h
    return y / (0.5 * total)


@functools.lru_cache(maxsize=None)
def _oracle():
    return cqt_oracle.FastDirectCQT(SR, HOP, dtype=torch.float64)


def oracle_logmag(y):
    """(n,) or (B, n) float64 -> (B, 288, T) float64 log-CQT of the oracle."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    return _oracle()(y).numpy()


@functools.lru_cache(maxsize=None)
def clip_case(seed, cents):
    """-> (clip, its oracle log-CQT (288, T))."""
    y = harmonic_clip(seed, cents)
    return y, oracle_logmag(y)[0]


def _positions(P0, P1, P2, B=1, bins=36, T=5):
    """A log-CQT whose power on the bin positions 0, 1, 2 is P0, P1, P2 per bin and frame."""
    L = np.zeros((B, bins, T))
    for j, p in enumerate((P0, P1, P2)):
        L[:, j::3] = np.log1p(np.sqrt(p))
    return L


# ---- estimate: hand-built cases ----

@pytest.mark.parametrize("powers, cents, strength", [((2.0, 0.0, 0.0), 0.0, 1.0), ((0.0, 3.0, 0.0), THIRD, 1.0), ((0.0, 0.0, 0.5), -THIRD, 1.0),
                                                     ((1.5, 1.5, 1.5), 0.0, 0.0), ((0.0, 0.0, 0.0), 0.0, 0.0)])
def test_estimate_hand_built(powers, cents, strength):
    c, s = metrics.estimate_tuning(_positions(*powers))
    assert c.dtype == torch.float64 and c.shape == (1,) and s.shape == (1,)
    assert not bool(torch.isnan(c).any() | torch.isnan(s).any())
    assert abs(float(c) - cents) < 1e-9 and abs(float(s) - strength) < 1e-9, (float(c), float(s))


def test_estimate_refuses_other_bin_counts():
    with pytest.raises(ValueError):
        metrics.estimate_tuning(np.zeros((1, 37, 4)))
    with pytest.raises(ValueError):
        metrics.estimate_tuning(np.zeros((36, 4)))


def test_estimate_ignores_frames_behind_the_count():
    L = _positions(1.0, 0.2, 0.0, B=3, T=6)
    L[:, :, 4:] = _positions(0.0, 0.0, 50.0, B=3, T=2)               # loud, flat junk behind frame 4
    want_c, want_s = metrics.estimate_tuning(L[:, :, :4])
    c, s = metrics.estimate_tuning(L, counts=[4, 4, 0])
    assert torch.equal(c[:2], want_c[:2]) and torch.equal(s[:2], want_s[:2])
    assert float(c[2]) == 0.0 and float(s[2]) == 0.0                # a count of 0: no power, (0, 0)
    junk_c, _ = metrics.estimate_tuning(L)
    assert float(junk_c[0]) < -20.0 < float(c[0])


def test_min_strength_at_equality_keeps_the_estimate():
    L = _positions(0.0, 1.0, 0.25)
    c, s = metrics.estimate_tuning(L)
    assert 0.0 < float(s) < 1.0 and float(c) > 20.0
    kept, s_kept = metrics.estimate_tuning(L, min_strength=float(s))
    assert float(kept) == float(c) and float(s_kept) == float(s)
    dropped, s_dropped = metrics.estimate_tuning(L, min_strength=float(np.nextafter(float(s), 1.0)))
    assert float(dropped) == 0.0 and float(s_dropped) == float(s)


# ---- estimate: accuracy through the oracle transform ----

@pytest.mark.parametrize("cents", DETUNINGS)
def test_estimate_accuracy_on_detuned_clips(cents):
    """Within 3 cents (a tenth of a bin) of the truth on 15 s harmonic clips."""
    seed = DETUNINGS.index(cents)
    _, L = clip_case(seed, cents)
    got, strength = metrics.estimate_tuning(L[None])
    print(f"detuned {cents:+.1f} cents (seed {seed}): estimate {float(got):+.3f}, strength {float(strength):.3f}")
    assert abs(float(got) - cents) <= 3.0


# ---- retune: design error and structure ----

@pytest.mark.parametrize("cents", [-49.0, 37.0])
@pytest.mark.parametrize("freq", [100.0, 3000.0, 8200.0])
def test_retune_design_error(freq, cents):
    """A sine at f * rho comes out as the sine at f to 1e-4 of its amplitude, 200 samples away from the ends: the fixed cutoff
    c = 0.94, Z = 32, beta = 9 and the 256-per-sample table together."""
    rho = 2.0 ** (cents / 1200.0)
    n = 20000
    x = np.sin(2 * np.pi * freq * rho * np.arange(n) / SR + 0.3)
    y, n_out = metrics.retune_reference(x, cents)
    assert n_out == int(np.floor(n * rho))
    ideal = np.sin(2 * np.pi * freq * np.arange(n_out) / SR + 0.3)
    err = float(np.abs(y[:n_out] - ideal)[200:n_out - 200].max())
    print(f"retune {freq:.0f} Hz at {cents:+.0f} cents: {err:.2e}")
    assert err <= 1e-4


def test_retune_structure():
    rng = np.random.default_rng(5)
    n = 700
    x = rng.standard_normal((4, n))
    lengths = np.array([700, 1, 0, 333])
    cents = np.array([33.3, -50.0, 20.0, 0.0], dtype=np.float32)
    y, n_out = metrics.retune_reference(x, cents, lengths)
    assert y.shape == (4, metrics.retune_out_len(n)) and metrics.retune_out_len(n) == int(np.floor(n * 2 ** (50 / 1200))) + 1
    rho = 2.0 ** (cents.astype(np.float64) / 1200.0)
    assert n_out.tolist() == [int(np.floor(l * r)) for l, r in zip(lengths, rho)]
    assert n_out[1] == 0 and n_out[2] == 0                          # floor(1 * 0.9715) = 0, and an empty row
    for b in range(4):
        assert not y[b, n_out[b]:].any()                             # zero behind every row's end
    assert np.array_equal(y[3, :333], x[3, :333])                    # 0 cents: the input itself
    one, n_one = metrics.retune_reference(np.array([0.7]), 50.0)     # n = 1, stretched: floor(1.0293) = 1 sample
    assert n_one == 1 and one.shape == (2,) and abs(one[0] - 0.7 * metrics.RETUNE_CUTOFF) < 1e-6 and one[1] == 0.0
    none, n_none = metrics.retune_reference(np.zeros((2, 0)), [10.0, -10.0])
    assert none.shape == (2, 1) and n_none.tolist() == [0, 0]
    # cents are what the kernel receives: float32, NaN read as 0, clamped to +-50
    a, na = metrics.retune_reference(x[:1], np.float32(33.3))
    b, nb = metrics.retune_reference(x[:1], float(np.float32(33.3)))
    assert np.array_equal(a, b) and na == nb
    c, nc = metrics.retune_reference(x[:2], [np.nan, 80.0])
    assert np.array_equal(c[0, :n], x[0]) and nc.tolist() == [n, int(np.floor(n * 2 ** (50 / 1200)))]


# ---- round trip: estimate, retune, transform again ----

@pytest.mark.parametrize("cents", [-45.0, 20.0])
def test_round_trip_restores_the_in_tune_transform(cents):
    """The oracle log-CQT of the retuned clip against the in-tune clip's, interior frames: at most a quarter of what the detuned
    clip's own transform differs by."""
    seed = DETUNINGS.index(cents)
    detuned, L_det = clip_case(seed, cents)
    _, L_ref = clip_case(seed, 0.0)
    est, _ = metrics.estimate_tuning(L_det[None])
    y, n_out = metrics.retune_reference(detuned, float(est))
    L_ret = oracle_logmag(y[:n_out])[0]
    T = min(L_ret.shape[1], L_ref.shape[1]) - 8
    comp = float(np.abs(L_ret[:, 8:T] - L_ref[:, 8:T]).max())
    uncomp = float(np.abs(L_det[:, 8:T] - L_ref[:, 8:T]).max())
    print(f"round trip at {cents:+.1f} cents (estimate {float(est):+.3f}): compensated {comp:.3f}, uncompensated {uncomp:.3f}, "
          f"peak {float(L_ref.max()):.2f}")
    assert comp <= 0.25 * uncomp


# ---- track times ----

def _hand_track(tuning_cents=None):
    ids = torch.tensor([[3, 3, 15, 15, 15], [7, 7, 7, -1, -1]], dtype=torch.int32)
    z = torch.zeros((2, 5, 12))
    times = (torch.arange(5, dtype=torch.float64) * 25 + 37.5) * HOP / SR
    tr = ake_amd.KeyTrack(z, z, None, ids, ids, ids, torch.zeros((2, 5)), torch.tensor([5, 3], dtype=torch.int32), times, 15.2, 5.0)
    tr.tuning_cents = tuning_cents
    return tr


def test_segments_of_a_retuned_track_are_in_the_recordings_own_time():
    plain = _hand_track()
    assert plain.tuning_cents is None and plain.tuning_strength is None and len(plain._tensors()) == 8
    cents = torch.tensor([40.0, -25.0])
    tuned = _hand_track(cents)
    assert len(tuned._tensors()) == 9 and tuned._tensors()[-1] is cents
    for r in range(2):
        rho = 2.0 ** (float(cents[r]) / 1200.0)
        want = [(a / rho, b / rho, k, name) for a, b, k, name in plain.segments(r)]
        got = tuned.segments(r)
        assert [g[2:] for g in got] == [w[2:] for w in want]
        assert np.allclose([g[:2] for g in got], [w[:2] for w in want], rtol=1e-15, atol=0.0)
    assert tuned.segments(0)[1][0] < plain.segments(0)[1][0]         # sharp: the retuned copy is longer, so its times shrink back


def test_track_score_scaling_equals_prescaled_boundaries():
    g = torch.Generator().manual_seed(3)
    R, W, S = 3, 40, 4
    pred = torch.randint(-1, 24, (R, W), generator=g).to(torch.int32)
    counts = torch.tensor([40, 31, 0], dtype=torch.int32)
    seg_start = torch.tensor([[0, 380000, 900000, 1500000], [0, 777777, metrics._I64_MAX, metrics._I64_MAX], [0, 5, 6, 7]], dtype=torch.int64)
    seg_key = torch.randint(0, 24, (R, S), generator=g).to(torch.int32)
    seg_count = torch.tensor([4, 2, 4], dtype=torch.int32)
    cents = torch.tensor([45.0, -33.3, 0.0], dtype=torch.float32)
    rho = 2.0 ** (cents.double() / 1200.0)
    scaled = torch.where(seg_start == metrics._I64_MAX, seg_start, torch.floor(seg_start.double() * rho[:, None]).long())
    assert torch.equal(metrics.scale_boundaries(seg_start, cents), scaled)
    assert int(scaled[0, 1]) == int(np.floor(380000 * 2.0 ** (45.0 / 1200.0))) and int(scaled[1, 2]) == metrics._I64_MAX
    got = metrics.track_score(pred, counts, seg_start, seg_key, seg_count, HOP, 76, 25, tuning_cents=cents)
    want = metrics.track_score(pred, counts, scaled, seg_key, seg_count, HOP, 76, 25)
    plain = metrics.track_score(pred, counts, seg_start, seg_key, seg_count, HOP, 76, 25)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], plain[0])                         # the boundaries did move under some window centre
