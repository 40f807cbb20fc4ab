"""Host restatement of the track score (metrics.window_truth / key_category / track_score) and the transition counted from labels.
No GPU."""
import math

import pytest
import torch

import ake_amd
from ake_amd import metrics

HOP, WF, SF = 4410, 76, 25               # 15 s windows, 5 s stride at 22.05 kHz and 5 frames per second
CENTRE0 = (WF - 1) * HOP // 2            # centre sample of window 0: 165375


def annotations(*recordings):
    """((start_sample, key), ...) per recording -> (seg_start, seg_key, seg_count) tensors, padded as KeyAnnotations pads."""
    S = max(1, max(len(r) for r in recordings))
    start = torch.full((len(recordings), S), 2 ** 63 - 1, dtype=torch.int64)
    key = torch.full((len(recordings), S), -1, dtype=torch.int32)
    for r, segs in enumerate(recordings):
        for s, (a, k) in enumerate(segs):
            start[r, s], key[r, s] = a, k
    return start, key, torch.tensor([len(r) for r in recordings], dtype=torch.int32)


def test_category_of_every_pair_against_the_transition_matrix():
    """exp(key_transition_log(0.9, 0.5, 0.3, 0.2, 0.02))[truth][pred] takes five distinct values, one per relation: an independent
    statement of which pairs are fifths, relatives and parallels."""
    P = torch.exp(metrics.key_transition_log(0.9, 0.5, 0.3, 0.2, 0.02))
    scale = 0.1 / (2 * 0.5 + 0.3 + 0.2 + 19 * 0.02)
    by_value = {0.9: 0, 0.5 * scale: 1, 0.3 * scale: 2, 0.2 * scale: 3, 0.02 * scale: 4}
    pred = torch.arange(-1, 24)[:, None].expand(25, 24)
    truth = torch.arange(24)[None, :].expand(25, 24)
    got = metrics.key_category(pred, truth)
    assert got.dtype == torch.int32 and got.shape == (25, 24)
    seen = set()
    for p in range(-1, 24):
        for t in range(24):
            if p < 0:
                want = 5
            else:
                hits = [c for v, c in by_value.items() if math.isclose(float(P[t, p]), v, rel_tol=1e-12)]
                assert len(hits) == 1
                want = hits[0]
            assert int(got[p + 1, t]) == want, (p, t)
            seen.add(want)
    assert seen == {0, 1, 2, 3, 4, 5}
    # each true key has 1 correct, 2 fifths, 1 relative, 1 parallel, 19 others
    assert [int((got[1:, 0] == c).sum()) for c in range(5)] == [1, 2, 1, 1, 19]
    # no truth, no category, whatever was decoded
    assert bool((metrics.key_category(torch.arange(-1, 24), torch.full((25,), -1)) == -1).all())
    assert metrics.SCORE_CATEGORIES == ("correct", "fifth", "relative", "parallel", "other", "undecoded")
    assert metrics.SCORE_WEIGHTS == (1.0, 0.5, 0.3, 0.2, 0.0, 0.0)


def test_window_centres_are_the_tracks_times():
    lo, hi, centre = metrics._window_spans(9, HOP, WF, SF, "cpu")
    times = (torch.arange(9, dtype=torch.float64) * SF + (WF - 1) / 2) * HOP / 22050              # KeyTrack.times
    assert torch.equal(centre, (times * 22050).round().to(torch.int64))
    assert lo.tolist()[:2] == [0, SF * HOP] and hi.tolist()[0] == (WF - 1) * HOP
    # an odd hop and an even window: the centre is rounded down
    assert metrics._window_spans(2, 5, 4, 1, "cpu")[2].tolist() == [7, 12]


@pytest.mark.parametrize("offset, want", [(0, 7), (-1, 7), (1, 3)])
def test_a_boundary_on_and_beside_the_centre_sample(offset, want):
    """The segment that starts exactly on the centre sample holds it; one sample later it does not."""
    start, key, count = annotations([(0, 3), (CENTRE0 + offset, 7)])
    truth, pure = metrics.window_truth(start, key, count, 1, HOP, WF, SF)
    assert truth.dtype == torch.int32 and truth.tolist() == [[want]] and pure.tolist() == [[False]]


def test_purity_and_window_edges():
    last0 = (WF - 1) * HOP                                   # last sample of window 0
    first1 = SF * HOP                                        # first sample of window 1
    # a boundary on the window's last sample overlaps it; one sample behind it does not
    for b, want in ((last0, False), (last0 + 1, True)):
        start, key, count = annotations([(0, 3), (b, 7)])
        truth, pure = metrics.window_truth(start, key, count, 1, HOP, WF, SF)
        assert truth.tolist() == [[3]] and pure.tolist() == [[want]]
    # a segment that ends on window 1's first sample (the next starts there) does not overlap window 1; one sample later it does
    for b, want in ((first1, True), (first1 + 1, False)):
        start, key, count = annotations([(0, 3), (b, 7)])
        truth, pure = metrics.window_truth(start, key, count, 2, HOP, WF, SF)
        assert truth.tolist() == [[7, 7]] and pure.tolist() == [[False, want]]        # (the boundary lies before window 0's centre)


def test_two_boundaries_back_to_the_same_key_are_not_pure():
    start, key, count = annotations([(0, 3), (CENTRE0 + 1000, 7), (CENTRE0 + 2000, 3)],      # centre in the first 3
                                    [(0, 3), (1000, 7), (2000, 3)],                          # centre in the second 3
                                    [(0, 3), (CENTRE0 - 10, 7), (CENTRE0 + 10, 3)],          # centre in the 7 between
                                    [(0, 3), (10 ** 9, 3)])                                  # one key all along: pure
    truth, pure = metrics.window_truth(start, key, count, 1, HOP, WF, SF)
    assert truth.tolist() == [[3], [3], [7], [3]] and pure.tolist() == [[False], [False], [False], [True]]


def test_unlabelled_segments_counts_and_empty_annotations():
    start, key, count = annotations([(0, 3), (SF * HOP * 2, -1), (SF * HOP * 4, 5)], [], [(0, 9)])
    truth, pure = metrics.window_truth(start, key, count, 8, HOP, WF, SF, counts=[8, 8, 3])
    assert truth[1].tolist() == [-1] * 8 and truth[2].tolist() == [9, 9, 9, -1, -1, -1, -1, -1]
    assert truth[0].tolist() == [3, -1, -1, 5, 5, 5, 5, 5]
    assert pure[0].tolist() == [False, False, False, False, True, True, True, True] and not bool(pure[1].any())
    # an unlabelled neighbour under the window makes it impure; entries behind seg_count are not read
    start[2, 1], key[2, 1] = 5, 4
    assert metrics.window_truth(start, key, count, 8, HOP, WF, SF, counts=[8, 8, 3])[0][2].tolist() == truth[2].tolist()


def test_truth_scores_one_and_a_fifth_scores_half():
    start, key, count = annotations([(0, 3), (SF * HOP * 3, 17), (SF * HOP * 7, 20)], [(0, 12)])
    W, counts = 12, torch.tensor([12, 9], dtype=torch.int32)
    truth, _ = metrics.window_truth(start, key, count, W, HOP, WF, SF, counts=counts)
    t2, cat, tally, changes = metrics.track_score(truth, counts, start, key, count, HOP, WF, SF)
    assert torch.equal(t2, truth) and tally.dtype == torch.int32 and tally.shape == (2, 2, 6) and changes.shape == (2, 2)
    assert tally[:, 0].tolist() == [[12, 0, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0]]
    assert cat[0].tolist() == [0] * 12 and cat[1].tolist() == [0] * 9 + [-1] * 3
    assert changes.tolist() == [[2, 2], [0, 0]]
    fifth = torch.where(truth >= 0, (truth + 7) % 12 + 12 * (truth // 12), truth).to(torch.int32)
    score = ake_amd.TrackScore(*metrics.track_score(fifth, counts, start, key, count, HOP, WF, SF))
    per, pooled = score.weighted()
    assert per.tolist() == [0.5, 0.5] and pooled == 0.5
    assert score.fractions()[1].tolist() == [0, 1, 0, 0, 0, 0]
    assert ake_amd.TrackScore(t2, cat, tally, changes).weighted() [1] == 1.0
    pure_total = int(tally[:, 1].sum())
    assert 0 < pure_total < 21 and ake_amd.TrackScore(t2, cat, tally, changes).weighted(pure=True)[1] == 1.0
    # a flickering track: changes at every window against the truth's two
    flick = truth.clone()
    flick[0, ::2] = -1
    s = ake_amd.TrackScore(*metrics.track_score(flick, counts, start, key, count, HOP, WF, SF))
    assert s.changes.tolist() == [[11, 2], [0, 0]] and s.flicker()[1] == 5.5
    assert s.tally[0, 0].tolist() == [6, 0, 0, 0, 0, 6] and s.weighted()[0].tolist() == [0.5, 1.0]


def test_relative_parallel_and_other_weights():
    start, key, count = annotations([(0, 12)])                                                 # C major throughout
    pred = torch.tensor([[12, 19, 17, 9, 0, 14, -1, 12, 12, 12]], dtype=torch.int32)            # C, G, F, a, c, D, none, C C C
    _, cat, tally, _ = metrics.track_score(pred, None, start, key, count, HOP, WF, SF)
    assert cat.tolist() == [[0, 1, 1, 2, 3, 4, 5, 0, 0, 0]]
    s = ake_amd.TrackScore(None, cat, tally, torch.zeros((1, 2), dtype=torch.int32))
    assert abs(s.weighted()[1] - (4 + 2 * 0.5 + 0.3 + 0.2) / 10) < 1e-15


def test_track_score_without_segments_or_windows_is_all_zeros():
    start, key, count = annotations([], [(0, 3)])
    pred = torch.tensor([[1, 2, 3], [1, 2, 3]], dtype=torch.int32)
    truth, cat, tally, changes = metrics.track_score(pred, [3, 0], start, key, count, HOP, WF, SF)
    assert int(tally.abs().sum()) == 0 and int(changes.abs().sum()) == 0
    assert bool((truth == -1).all()) and bool((cat == -1).all())


def test_transition_from_labels_recovers_a_planted_stay_share():
    """Labels drawn from a chain with P(stay) = 0.8 and every move a fifth up."""
    g = torch.Generator().manual_seed(11)
    R, W = 6, 2000
    labels = torch.zeros((R, W), dtype=torch.int64)
    labels[:, 0] = torch.arange(R) * 5 % 24
    move = torch.rand((R, W), generator=g) >= 0.8
    for w in range(1, W):
        k = labels[:, w - 1]
        labels[:, w] = torch.where(move[:, w], 12 * (k // 12) + (k % 12 + 7) % 12, k)
    A = metrics.transition_from_labels(labels)
    P = torch.exp(A)
    assert A.dtype == torch.float64 and A.shape == (24, 24) and torch.allclose(P.sum(dim=1), torch.ones(24, dtype=torch.float64))
    stay_se = (0.8 * 0.2 / (R * (W - 1) / 2)) ** 0.5                       # (the tie pools a mode's 12 keys)
    assert abs(float(P[0, 0]) - 0.8) < 4 * stay_se + 1e-3 and abs(float(P[12, 12]) - 0.8) < 4 * stay_se + 1e-3
    assert abs(float(P[0, 7]) - 0.2) < 4 * stay_se + 1e-3 and float(P[0, 5]) < 1e-3
    # tied: a cell depends on the modes and the interval moved, not on the key left
    cls = metrics._transposition_classes()
    for c in range(48):
        v = A[cls == c]
        assert v.numel() == 12 and float(v.max() - v.min()) < 1e-12
    # untied: keys that were never left keep the pseudo-counts' matrix
    U = metrics.transition_from_labels(labels, tied=False)
    never = [k for k in range(24) if not bool((labels[:, :-1] == k).any())]
    assert torch.allclose(U[never], metrics.key_transition_log(0.9)[never])
    assert torch.isfinite(A).all() and torch.isfinite(U).all()


def test_transition_from_labels_skips_unlabelled_pairs_and_windows_behind_the_count():
    labels = torch.tensor([[3, 3, -1, 3, 10, 10, 5, 5]])
    plain = metrics.transition_from_labels(labels, counts=[6], tied=False, pseudo_count=0.5)
    C = torch.zeros((24, 24), dtype=torch.float64)
    C[3, 3] += 1; C[3, 10] += 1; C[10, 10] += 1                            # (3,-1), (-1,3) skipped; (10,5), (5,5) lie behind the count
    want = metrics.transition_m_step(C, metrics.key_transition_log(0.9), tied=False, pseudo_count=0.5)
    assert torch.equal(plain, want)
    assert torch.equal(metrics.transition_from_labels(labels[0], tied=False), metrics.transition_from_labels(labels, tied=False))
