"""Host models of the training-window route (no GPU): metrics.draw_windows (Python-int arithmetic on the synthesiser's Philox),
metrics.window_labels (integer torch ops on window_truth's geometry) and metrics.weighted_general_step (float64)."""
import collections
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ake_amd
from ake_amd import metrics, synthetic
from ake_amd.KeyDataset import labels_for_signature

HOP, WF = 4410, 76
FRAMES = (78, 40, 92, 76)                    # recording 1 is shorter than one window
I64_MAX = 2 ** 63 - 1


# ---- the draw ----

def test_population_and_valid_starts():
    prefix = metrics.window_prefix(FRAMES, WF)
    assert prefix == [0, 3, 3, 20, 21]
    rec, start, index = metrics.draw_windows(prefix, 0, 0, 0, 2000)
    assert 1 not in rec and set(rec) == {0, 2, 3}
    for r, s, i in zip(rec, start, index):
        assert 0 <= s <= FRAMES[r] - WF and i == prefix[r] + s
    with pytest.raises(ValueError):
        metrics.draw_windows(metrics.window_prefix((40, 75), WF), 0, 0, 0, 4)


def test_same_arguments_same_list_and_every_argument_matters():
    prefix = metrics.window_prefix(FRAMES, WF)
    base = metrics.draw_windows(prefix, 5, 2, 0, 64)
    assert metrics.draw_windows(prefix, 5, 2, 0, 64) == base
    assert metrics.draw_windows(prefix, 5, 3, 0, 64) != base             # epoch
    assert metrics.draw_windows(prefix, 6, 2, 0, 64) != base             # seed
    assert metrics.draw_windows(prefix, 5 + 2 ** 32, 2, 0, 64) != base   # the seed's high word
    assert metrics.draw_windows(prefix, 5, 2, 1, 64) != base             # first_slot
    assert metrics.draw_windows(prefix, 5, 2, 2 ** 32, 64) != base       # the slot's high word


def test_slots_do_not_depend_on_how_they_are_split():
    prefix = metrics.window_prefix(FRAMES, WF)
    whole, a, b = (metrics.draw_windows(prefix, 9, 1, f, n) for f, n in ((0, 16), (0, 8), (8, 8)))
    assert all(w == x + y for w, x, y in zip(whole, a, b))


def test_the_draw_is_uniform_over_the_population():
    """21 000 draws over 21 cells: every cell is hit and lies within 4 binomial standard deviations of 1000."""
    prefix = metrics.window_prefix(FRAMES, WF)
    _, _, index = metrics.draw_windows(prefix, 1234, 0, 0, 21000)
    cells = collections.Counter(index)
    sd = math.sqrt(21000 * (1 / 21) * (20 / 21))
    worst = max(abs(cells.get(i, 0) - 1000) for i in range(21)) / sd
    print("largest deviation:", worst, "standard deviations")
    assert len(cells) == 21 and set(cells) == set(range(21))
    assert worst < 4.0


# N = 2^33 + 7 start frames: five recordings, so that every start still fits the int32 the kernel writes
BIG_PREFIX = [0] + [k * (2 ** 31 - 1) for k in range(1, 5)] + [2 ** 33 + 7]


def test_a_population_beyond_32_bits():
    N = BIG_PREFIX[-1]
    rec, start, index = metrics.draw_windows(BIG_PREFIX, 3, 0, 0, 64)
    assert N == 2 ** 33 + 7 and max(index) > 2 ** 32 and all(0 <= i < N for i in index)
    assert all(BIG_PREFIX[r] <= i < BIG_PREFIX[r + 1] and s == i - BIG_PREFIX[r] < 2 ** 31 for r, s, i in zip(rec, start, index))
    assert len(set(rec)) > 2


# ---- labels and weights ----

def annotations(rows, S=None):
    """rows: per recording a list of (start_sample, key) -> (seg_start, seg_key, seg_count), padded as KeyAnnotations pads."""
    S = S or max([len(r) for r in rows] + [1])
    start = torch.full((len(rows), S), I64_MAX, dtype=torch.int64)
    key = torch.full((len(rows), S), -1, dtype=torch.int32)
    for r, segs in enumerate(rows):
        for s, (a, k) in enumerate(segs):
            start[r, s], key[r, s] = a, k
    return start, key, torch.tensor([len(r) for r in rows], dtype=torch.int32)


def test_grid_list_agrees_with_window_truth():
    g = torch.Generator().manual_seed(11)
    W, SF = 40, 7
    span = (W * SF + WF) * HOP
    rows = []
    for r in range(3):
        cuts = sorted(set(torch.randint(1, span, (6,), generator=g).tolist()))
        rows.append([(a, int(torch.randint(-1, 24, (1,), generator=g))) for a in [0] + cuts])
    start, key, count = annotations(rows)
    truth, pure = metrics.window_truth(start, key, count, W, HOP, WF, SF)
    rec = torch.arange(3).repeat_interleave(W)
    st = (torch.arange(W) * SF).repeat(3)
    lab = metrics.window_labels(start, key, count, rec, st, HOP, WF)
    assert lab["truth"].dtype == torch.int32 and torch.equal(lab["truth"].reshape(3, W), truth)
    assert torch.equal((lab["sample_weight"] > 0).reshape(3, W), truth >= 0)
    assert torch.equal((lab["purity"] == 1).reshape(3, W), pure)
    assert bool(pure.any()) and bool((~pure & (truth >= 0)).any()) and bool((truth < 0).any())
    assert torch.equal(lab["seq_length"], torch.full((3 * W,), WF, dtype=torch.int64))


def test_labels_of_all_24_keys():
    start, key, count = annotations([[(0, k)] for k in range(24)])
    lab = metrics.window_labels(start, key, count, torch.arange(24), torch.zeros(24, dtype=torch.int64), HOP, WF)
    for k in range(24):
        key_labels, key_signature_id, _, tonic = labels_for_signature(k, None, True)
        assert torch.equal(lab["key_labels"][k], key_labels) and lab["key_labels"].dtype == torch.float32
        assert torch.equal(lab["tonic_labels"][k], tonic) and torch.equal(lab["key_signature_id"][k], key_signature_id)
        assert torch.equal(lab["key_labels"][k], torch.from_numpy(synthetic.key_pitch_classes(k)))
    assert bool((lab["sample_weight"] == 1).all()) and bool((lab["purity"] == 1).all())


SPAN = (WF - 1) * HOP + 1                    # samples of a window, lo..hi inclusive
CENTRE = (WF - 1) * HOP // 2


def purity_cases():
    rows = [[(0, 3), (CENTRE, 7)],           # 0: a boundary on the centre sample: the window takes the later key
            [(0, 3), (CENTRE + 1, 7)],       # 1: one sample behind it: the earlier key
            [(0, 3), (CENTRE - 1, 7)],       # 2: one sample before it
            [(0, 5), (1000, -1), (2000, 5)],         # 3: an unlabelled stretch inside a window of key 5
            [(0, -1), (CENTRE + 5, 9)],      # 4: the centre lies in an unlabelled stretch
            [],                              # 5: no segments
            [(0, 20)],                       # 6: one segment covers everything
            [(0, 4), (SPAN // 4, 6), (SPAN // 2 - 10, 4)]]   # 7: back to the first key before the centre: both of its stretches count
    return annotations(rows), torch.arange(len(rows)), torch.zeros(len(rows), dtype=torch.int64)


def test_purity_cases():
    (start, key, count), rec, st = purity_cases()
    lab = metrics.window_labels(start, key, count, rec, st, HOP, WF)
    f32 = lambda c: float(np.float32(np.float64(c) / np.float64(SPAN)))
    assert lab["truth"].tolist() == [7, 3, 7, 5, -1, -1, 20, 4]
    want = [f32(SPAN - CENTRE), f32(CENTRE + 1), f32(SPAN - CENTRE + 1), f32(SPAN - 1000), 0.0, 0.0, 1.0, f32(SPAN // 4 + SPAN - (SPAN // 2 - 10))]
    assert lab["purity"].tolist() == want
    assert lab["sample_weight"].tolist() == [w if t >= 0 else 0.0 for w, t in zip(want, lab["truth"].tolist())]
    for name in ("key_labels", "tonic_labels", "key_signature_id"):
        assert float(lab[name][4].abs().sum()) == 0 and float(lab[name][5].abs().sum()) == 0
    # min_purity cuts below it, not at it
    at = float(lab["purity"][0])
    keep = metrics.window_labels(start, key, count, rec, st, HOP, WF, min_purity=at)
    cut = metrics.window_labels(start, key, count, rec, st, HOP, WF, min_purity=float(np.nextafter(np.float32(at), np.float32(1))))
    assert float(keep["sample_weight"][0]) == at and float(cut["sample_weight"][0]) == 0.0 and float(cut["sample_weight"][6]) == 1.0
    assert torch.equal(cut["key_labels"], lab["key_labels"])                     # the labels stay: only the weight goes
    uni = metrics.window_labels(start, key, count, rec, st, HOP, WF, min_purity=0.5, uniform=True)
    assert uni["sample_weight"].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0]
    # a window further into the recording: the geometry moves with its start frame
    far = metrics.window_labels(start, key, count, torch.tensor([0]), torch.tensor([WF]), HOP, WF)
    assert far["truth"].tolist() == [7] and far["purity"].tolist() == [1.0]


# ---- the weighted loss ----

def loss_case(B, seed, genre=True):
    g = torch.Generator().manual_seed(seed)
    key = (torch.rand((B, 12), generator=g) * 0.98 + 0.01).double()
    tonic = (torch.randn((B, 12), generator=g) * 2).double()
    gen = (torch.randn((B, 11), generator=g) * 2).double() if genre else None
    kid = torch.randint(0, 24, (B,), generator=g)
    key_labels = ake_amd.KEY_SIGNATURE_MAP[torch.randint(0, 21, (B,), generator=g)].clone()
    key[::3] = (key_labels[::3] * 0.9 + 0.05).double()
    tonic_labels = F.one_hot(torch.randint(0, 12, (B,), generator=g), 12).float()
    tonic[::2] += 6 * tonic_labels[::2]
    genre_labels = F.one_hot(torch.randint(0, 11, (B,), generator=g), 11).float() if genre else None
    if genre:
        genre_labels[1::4] = 0
    return key, tonic, gen, key_labels, tonic_labels, genre_labels, F.one_hot(kid, 24).float()


def unweighted(key, tonic, gen, key_labels, tonic_labels, genre_labels, sig, weights, use_cos):
    """general_step's torch formulas (PitchClassNet.general_step off the fused path), float64."""
    t_idx = tonic_labels.long().argmax(1)
    loss = weights[0] * F.binary_cross_entropy(key, key_labels.double()) + weights[1] * F.cross_entropy(tonic, t_idx)
    acc_g = torch.tensor(0.0)
    if gen is not None:
        gl = genre_labels.long()
        m = (gl.sum(1) == 1).double()
        per = F.cross_entropy(gen, gl.argmax(1), reduction="none")
        loss = loss + weights[2] * ((per * m).sum() / m.sum().clamp(min=1.0))
        acc_g = ((gen.argmax(1) == gl.argmax(1)).double() * m).sum() / m.sum().clamp(min=1.0)
    if use_cos:
        loss = loss + (1 - F.cosine_similarity(key, key_labels.double(), dim=1).sum() / key.shape[0])
    mirex, correct, fifths, relative, parallel, other, accuracy = metrics.mirex_score(key_labels.double(), key, tonic_labels.long(), tonic, sig)
    acc_t = (tonic.argmax(1) == t_idx).double().mean()
    return loss, accuracy, mirex, correct, fifths, relative, parallel, other, acc_t, acc_g


@pytest.mark.parametrize("genre,use_cos", [(True, False), (False, True), (True, True)])
def test_all_ones_weights_are_the_unweighted_step(genre, use_cos):
    case = loss_case(37, 1, genre)
    weights = (1.0, 0.7, 0.1)
    got = metrics.weighted_general_step(*case, torch.ones(37), weights, use_cos)
    want = unweighted(*case, weights, use_cos)
    assert abs(float(got[0]) - float(want[0])) < 1e-12
    for g, w in zip(got[1:], want[1:]):
        assert abs(float(g) - float(w)) < 1e-6          # (mirex_score returns float32 shares)
    assert got[0].dtype == torch.float64


def test_zero_weight_rows_count_for_nothing_and_all_zero_gives_zeros():
    case = list(loss_case(16, 2))
    w = torch.rand(16, generator=torch.Generator().manual_seed(3))
    w[[1, 4, 9]] = 0
    base, base_g = metrics.weighted_general_step(*case, w, (1.0, 0.7, 0.1), True, grads=True)
    other = [t.clone() for t in case]
    other[0][[1, 4]] = torch.tensor([0.0, 1.0] * 6, dtype=torch.float64)        # key outputs exactly 0 and 1
    other[0][9] = float("nan")
    other[1][[1, 4, 9]] = 1e30
    other[2][9] = float("inf")
    other[3][[1, 4, 9]] = 1 - other[3][[1, 4, 9]]
    other[4][[1, 4, 9]] = 0
    other[5][[1, 4, 9]] = 1
    other[6][[1, 4, 9]] = 0
    got, got_g = metrics.weighted_general_step(*other, w, (1.0, 0.7, 0.1), True, grads=True)
    assert all(torch.equal(a, b) for a, b in zip(base, got))
    assert all(torch.equal(a, b) for a, b in zip(base_g, got_g))
    assert all(float(g[[1, 4, 9]].abs().sum()) == 0 for g in got_g)
    zero, zero_g = metrics.weighted_general_step(*other, torch.zeros(16), (1.0, 0.7, 0.1), True, grads=True)
    assert all(float(v) == 0.0 for v in zero) and all(float(g.abs().sum()) == 0 for g in zero_g)
    # no labelled genre row among the rows that count: the genre term is an exact zero
    none = [t.clone() for t in case]
    none[5][w > 0] = 0
    a = metrics.weighted_general_step(*none, w, (0.0, 0.0, 1.0), False)
    assert float(a[0]) == 0.0 and float(a[9]) == 0.0


@pytest.mark.parametrize("genre,use_cos", [(True, False), (True, True), (False, True)])
def test_gradients_match_float64_autograd(genre, use_cos):
    case = list(loss_case(9, 4, genre))
    w = torch.tensor([0.3, 1.0, 0.0, 0.7, 0.0, 1.0, 0.25, 0.9, 0.5], dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in case[:3]]
    scal, grads = metrics.weighted_general_step(*leaves, *case[3:], w, (1.0, 0.7, 0.1), use_cos, grads=True)
    scal[0].backward()
    for leaf, g in zip(leaves, grads):
        if leaf is None:
            assert g is None
            continue
        assert float((leaf.grad - g).abs().max()) < 1e-13 * max(1.0, float(leaf.grad.abs().max()))
        assert float(leaf.grad[[2, 4]].abs().sum()) == 0
    # the loss is the formula: written out once more with plain sums
    key, tonic, gen, yl, tl, gl, _ = case
    W = float(w.sum())
    bce = F.binary_cross_entropy(key, yl.double(), reduction="none").sum(1)
    ce = F.cross_entropy(tonic, tl.argmax(1), reduction="none")
    want = float((w * bce).sum()) / (12 * W) + 0.7 * float((w * ce).sum()) / W
    if genre:
        m = (gl.sum(1) == 1).double()
        want += 0.1 * float((w * m * F.cross_entropy(gen, gl.argmax(1), reduction="none")).sum()) / float((w * m).sum())
    if use_cos:
        want += 1 - float((w * F.cosine_similarity(key, yl.double(), dim=1)).sum()) / W
    assert abs(float(scal[0].detach()) - want) < 1e-12


# ---- KeyEstimator.training_windows refuses what track refuses, before anything touches a device ----

def test_training_windows_refuses_what_track_refuses():
    from argparse import Namespace
    from ake_amd import pipeline as P

    def bare(frames=5, wrap_mode="dataset_max", local=False):
        est = P.KeyEstimator.__new__(P.KeyEstimator)                 # (the constructor uploads the CQT tables: it needs a GPU)
        est.frames, est.wrap_mode, est.sample_rate = frames, wrap_mode, 22050
        est.net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True, local=local, frames=5, loc_window_size=10))
        return est

    audio = torch.zeros((2, 330750))
    ann = P.KeyAnnotations.from_segments([[(0.0, 3)], [(0.0, "A minor")]], 22050)
    for match, est in (("frames=0", bare(frames=0)), ("true_end", bare(wrap_mode="true_end")), ("--local", bare(local=True))):
        with pytest.raises(ValueError, match=match) as caught:
            est.training_windows(audio, ann)
        with pytest.raises(ValueError) as tracked:
            est.track(audio)
        assert str(caught.value) == str(tracked.value)               # the same messages
    with pytest.raises(ValueError, match="44100"):
        bare().training_windows(audio, P.KeyAnnotations(ann.seg_start, ann.seg_key, ann.seg_count, 44100))
    with pytest.raises(ValueError, match="recordings"):
        bare().training_windows(audio[:1], ann)
