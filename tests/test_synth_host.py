"""Host side of the additive synthesiser and the modulating recordings: the Philox generator, the envelopes, the recipe and
KeyAnnotations.  No GPU."""
import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics, synthetic


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = synthetic.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert got.dtype == np.uint32 and " ".join(f"{int(x):08x}" for x in got) == want


def test_philox_is_vectorised_over_leading_axes():
    c = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], dtype=np.uint64)
    k = np.array([[0, 0], [0xFFFFFFFF] * 2], dtype=np.uint64)
    got = synthetic.philox4x32_10(c, k)
    assert got.shape == (2, 4) and int(got[0, 0]) == 0x6627E8D5 and int(got[1, 3]) == 0x6D5451FD


def test_uniform_is_exact_in_float32_and_strictly_inside_the_unit_interval():
    x = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.uint32)
    x = np.concatenate([x, np.random.default_rng(5).integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)])
    u = synthetic.philox_uniform(x)
    assert u.dtype == np.float64 and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert float(u.min()) == 2.0 ** -24 and float(u.max()) == 1.0 - 2.0 ** -24
    assert np.all(u > 0.0) and np.all(u < 1.0) and np.all(np.log(u) < 0.0)


def test_normals_follow_their_block_and_seed():
    a = synthetic.philox_normal(1027, 77, 2)
    assert a.shape == (1027,) and np.array_equal(a[:64], synthetic.philox_normal(64, 77, 2))          # sample t depends on t alone
    assert not np.array_equal(a[:64], synthetic.philox_normal(64, 78, 2))
    assert not np.array_equal(a[:64], synthetic.philox_normal(64, 77, 3))
    hi = synthetic.philox_normal(8, (5 << 32) | 77, 2)                                               # the seed's high word is key word 1
    assert not np.array_equal(hi, a[:8])


@pytest.mark.parametrize("fade", [1, 2, 7, 11025])
def test_a_cross_fading_pair_sums_to_one(fade):
    E = 3 * fade + 5                                                   # (long enough that the first partial's fade-in is over)
    t = np.arange(E - fade, E, dtype=np.int64)
    out = synthetic.fade_envelope(t, 0, E, fade)                       # ends at E
    inn = synthetic.fade_envelope(t, E - fade, E + 5 * fade, fade)     # starts at E - fade
    assert np.max(np.abs(out + inn - 1.0)) < 4e-16
    assert np.all(np.diff(inn) > 0) and 0.0 < inn[0] and inn[-1] < 1.0
    # outside the ramps the gain is 1, and fade 0 is no envelope at all
    assert np.all(synthetic.fade_envelope(np.arange(fade, E - fade), 0, E, fade) == 1.0)
    assert np.all(synthetic.fade_envelope(np.arange(0, 50), 0, 50, 0) == 1.0)


def test_reference_adds_cross_fading_partials_to_a_steady_tone():
    """Two partials of one frequency and phase that cross-fade are one steady tone; rows end in zeros."""
    fade, E, n = 64, 500, 1000
    one = dict(offsets=[0, 1, 1], cps=[0.01], phase=[0.25], amp=[0.5], start=[0], end=[n + fade], fade=0, n=[n, 3])
    two = dict(offsets=[0, 2, 2], cps=[0.01, 0.01], phase=[0.25, 0.25], amp=[0.5, 0.5], start=[-fade, E - fade], end=[E, n + fade], fade=fade, n=[n, 3])
    a, b = synthetic.synth_partials_reference(**one), synthetic.synth_partials_reference(**two)
    assert a.shape == (2, n) and np.max(np.abs(a - b)) < 1e-15
    assert np.all(a[1] == 0.0) and abs(a[0, 0] - 0.5) < 1e-15
    p = synthetic.synth_partials_reference(**dict(one, peak=0.9))
    assert abs(np.max(np.abs(p[0])) - 0.9) < 1e-15 and np.all(p[1] == 0.0) and np.all(np.isfinite(p))


@pytest.mark.parametrize("i, seconds", [(0, 300.0), (7, 300.0), (29, 95.5), (3, 12.0)])
def test_modulating_recipe_is_deterministic_and_covers_the_recording(i, seconds):
    sr = synthetic.SR
    p, segs = synthetic.modulating_recipe(i, seconds)
    p2, segs2 = synthetic.modulating_recipe(i, seconds)
    assert segs == segs2 and all(np.array_equal(p[k], p2[k]) for k in p)
    n = int(round(seconds * sr))
    assert p["n"] == n and p["fade"] == 11025 and p["noise_sigma"] == 0.003 and p["peak"] == 0.9
    starts, keys = [s for s, _ in segs], [k for _, k in segs]
    assert starts[0] == 0 and keys[0] == i % 24 and all(b > a for a, b in zip(starts, starts[1:])) and starts[-1] < n
    ends = starts[1:] + [n]
    lengths = [e - s for s, e in zip(starts, ends)]
    assert all(l >= 20 * sr - 1 for l in lengths[:-1])                  # (a boundary is rounded to a sample)
    if len(segs) > 1:
        assert lengths[-1] >= 20 * sr - 1                               # a short last piece has joined the one before it
    assert all(0 <= k < 24 for k in keys) and all(a != b for a, b in zip(keys, keys[1:]))
    # 12 partials per segment, sounding from fade/2 before the boundary to fade/2 behind the next: neighbours cross-fade exactly
    assert len(p["cps"]) == 12 * len(segs) and p["cps"].dtype == np.float64 and p["amp"].dtype == np.float32 and p["start"].dtype == np.int64
    half = p["fade"] // 2
    for s in range(len(segs)):
        sl = slice(12 * s, 12 * s + 12)
        assert np.all(p["start"][sl] == starts[s] - half) and np.all(p["end"][sl] == ends[s] - half + p["fade"])
        scale = np.flatnonzero(synthetic.key_pitch_classes(keys[s]))
        midi = np.round(69 + 12 * np.log2(p["cps"][sl] * sr / 440.0)).astype(int)
        assert np.all(np.isin(midi % 12, scale)) and np.all((midi // 12 - 1 >= 2) & (midi // 12 - 1 <= 6))
    assert np.all((p["cps"] > 0) & (p["cps"] < 0.5)) and np.all((p["phase"] >= 0) & (p["phase"] < 1))
    assert np.all((p["amp"] >= 0.05) & (p["amp"] <= 0.25))


def test_modulating_recipe_moves_mostly_to_related_keys():
    related = total = 0
    for i in range(40):
        keys = [k for _, k in synthetic.modulating_recipe(i, 600.0)[1]]
        for a, b in zip(keys, keys[1:]):
            total += 1
            related += b in synthetic._related_keys(a)
    assert total > 300 and abs(related / total - 0.9) < 4 * (0.9 * 0.1 / total) ** 0.5


def test_modulating_recipe_takes_its_own_lengths():
    _, segs = synthetic.modulating_recipe(1, 60.0, min_seconds=5.0, mean_seconds=8.0, fade_seconds=0.1)
    assert len(segs) >= 4
    arrays, all_segs = synthetic.modulating_batch_arrays([1, 2], [60.0, 30.0], min_seconds=5.0, mean_seconds=8.0, fade_seconds=0.1)
    assert all_segs[0] == segs and arrays["offsets"].tolist() == [0, 12 * len(segs), 12 * (len(segs) + len(all_segs[1]))]
    assert arrays["n"].tolist() == [60 * synthetic.SR, 30 * synthetic.SR] and arrays["fade"] == 2205


def test_key_annotations_from_segments():
    ann = ake_amd.KeyAnnotations.from_segments([[(0.0, "A minor"), (10.00002, 12), (20.5, -1)], [(0, 23)], []], 22050)
    assert ann.seg_start.dtype == torch.int64 and ann.seg_key.dtype == torch.int32 and ann.seg_count.dtype == torch.int32
    assert ann.seg_count.tolist() == [3, 1, 0] and ann.sample_rate == 22050
    big = 2 ** 63 - 1
    assert ann.seg_start.tolist() == [[0, round(10.00002 * 22050), 452025], [0, big, big], [big, big, big]]
    assert ann.seg_key.tolist() == [[9, 12, -1], [23, -1, -1], [-1, -1, -1]]
    assert metrics.KEY_NAMES[9] == "A minor"
    assert ake_amd.KeyAnnotations.from_segments([[(0.0, 1), (0.49999 / 22050 + 1.0, 2)]], 22050).seg_start.tolist() == [[0, 22050]]
    assert ake_amd.KeyAnnotations.from_segments([[(0.0, 1), (0.50001 / 22050 + 1.0, 2)]], 22050).seg_start.tolist() == [[0, 22051]]


@pytest.mark.parametrize("segments", [
    [[(0.5, 3)]],                                  # segment 0 does not start at 0
    [[(0.0, 3), (4.0, 5), (4.0, 6)]],              # not strictly ascending
    [[(0.0, 3), (4.0, 5), (3.0, 6)]],
    [[(0.0, 3), (1.00001, 5), (1.00002, 6)]],      # ascending in seconds, the same sample
    [[(0.0, "H major")]],
    [[(0.0, 24)]],
    [[(0.0, -2)]],
])
def test_key_annotations_refusals(segments):
    with pytest.raises(ValueError):
        ake_amd.KeyAnnotations.from_segments(segments, 22050)
