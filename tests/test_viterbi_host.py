"""Smooth key tracks, the parts that need no GPU: ``metrics.key_emissions``, ``metrics.viterbi_keys``, ``metrics.key_transition_log`` and
``KeyTrack.segments(smoothed=...)``."""
import itertools
import math

import numpy as np
import pytest
import torch

from ake_amd import metrics
from ake_amd import pipeline as P

SCALE = (0, 2, 4, 5, 7, 9, 11)


def test_viterbi_equals_an_exhaustive_search_over_all_paths():
    """W = 4: all 24^4 paths scored in float64 under the default transition (5 s stride, 60 s mean key length); the best one is the
    Viterbi path.  Seeded Gaussian emissions (no ties), three draws: one whose best path stays in one key, two whose best path changes
    key and is not the per-window maximum either."""
    A = metrics.key_transition_log(stay=math.exp(-5.0 / 60.0))
    paths = torch.tensor(list(itertools.product(range(24), repeat=4)))                          # (331776, 4)
    kinds = set()
    for seed in (11, 13, 16):
        g = torch.Generator().manual_seed(seed)
        e = torch.randn((4, 24), generator=g, dtype=torch.float64) * 4
        score = e[0, paths[:, 0]].clone()
        for w in range(1, 4):
            score += A[paths[:, w - 1], paths[:, w]] + e[w, paths[:, w]]
        best = paths[int(torch.argmax(score))]
        top = torch.sort(score).values
        assert float(top[-1] - top[-2]) > 1e-9
        got = metrics.viterbi_keys(e, A)
        assert got.dtype == torch.int32 and got.shape == (4,) and got.tolist() == best.tolist()
        kinds.add((len(set(got.tolist())) > 1, got.tolist() == e.argmax(dim=1).tolist()))
        # a prior shifts the first window: scored the same way
        prior = torch.randn(24, generator=g, dtype=torch.float64) * 3
        best_p = paths[int(torch.argmax(score + prior[paths[:, 0]]))]
        assert metrics.viterbi_keys(e[None], A, log_prior=prior)[0].tolist() == best_p.tolist()
    assert kinds == {(False, False), (True, False)}


def first_max(e):
    return np.argmax(e.numpy(), axis=-1)                                                       # numpy: the first maximum


def test_a_uniform_matrix_gives_the_per_window_first_maximum():
    g = torch.Generator().manual_seed(12)
    e = torch.randint(-3, 4, (3, 30, 24), generator=g).double()                                # small integers: many exact ties
    assert int((e == e.max(dim=2, keepdim=True).values).sum(dim=2).max()) > 1
    A = torch.full((24, 24), math.log(1 / 24), dtype=torch.float64)
    got = metrics.viterbi_keys(e, A, counts=[30, 7, 0])
    want = first_max(e)
    assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1, :7].numpy(), want[1, :7])
    assert bool((got[1, 7:] == -1).all()) and bool((got[2] == -1).all())
    assert torch.equal(metrics.viterbi_keys(e.float(), A)[1], torch.from_numpy(want[1]).int())


def test_one_deviant_window_is_absorbed():
    e = torch.zeros((21, 24), dtype=torch.float64)
    e[:, 14] = 3.0                                                                             # 20 windows favour key 14 by 3 nats
    e[10, 14], e[10, 5] = 0.0, 3.0                                                             # the one in the middle favours key 5
    sticky = metrics.viterbi_keys(e, metrics.key_transition_log(stay=0.99))
    assert sticky.tolist() == [14] * 21                                                        # two changes cost 2 * log(0.99 / ~0.0004) >> 6
    loose = metrics.viterbi_keys(e, torch.full((24, 24), math.log(1 / 24), dtype=torch.float64))
    assert loose.tolist() == [14] * 10 + [5] + [14] * 10


def test_viterbi_refuses_infinite_transitions():
    A = metrics.key_transition_log(stay=0.9)
    A[3, 4] = -math.inf
    with pytest.raises(ValueError, match="large negative"):
        metrics.viterbi_keys(torch.zeros((2, 24)), A)
    with pytest.raises(ValueError):
        metrics.key_transition_log(stay=1.0)


def test_key_transition_log_rows_neighbours_and_symmetry():
    for stay in (0.5, math.exp(-5 / 60), 0.999):
        A = metrics.key_transition_log(stay=stay)
        assert A.shape == (24, 24) and A.dtype == torch.float64 and bool(torch.isfinite(A).all())
        Pm = A.exp()
        assert float((Pm.sum(dim=1) - 1).abs().max()) < 1e-12
        assert torch.equal(A, A.T)
        assert float((Pm.diagonal() - stay).abs().max()) < 1e-12
    Pm = metrics.key_transition_log(stay=0.9).exp()
    names = metrics.KEY_NAMES
    off = 0.1 / (2 * 0.5 + 0.3 + 0.2 + 19 * 0.02)
    for key, fifths, relative, parallel in (("C major", ("G major", "F major"), "A minor", "C minor"),
                                            ("A minor", ("E minor", "D minor"), "C major", "A major")):
        i = names.index(key)
        want = {names.index(n): 0.5 * off for n in fifths}
        want[names.index(relative)] = 0.3 * off
        want[names.index(parallel)] = 0.2 * off
        assert (names.index("C major"), names.index("A minor")) == (12, 9)
        for j in range(24):
            if j != i:
                assert float(Pm[i, j]) == pytest.approx(want.get(j, 0.02 * off), rel=1e-12), (key, names[j])
    # other weights are honoured
    Q = metrics.key_transition_log(stay=0.8, fifth=1.0, relative=1.0, parallel=1.0, other=1.0).exp()
    assert float((Q[0, 1:] - 0.2 / 23).abs().max()) < 1e-15


def emissions_loop(key, tonic, weight):
    """The formula of the issue as a plain loop, in Python floats (float64)."""
    out = np.zeros(key.shape[:-1] + (24,))
    for idx in np.ndindex(*key.shape[:-1]):
        p, t = [float(v) for v in key[idx]], [float(v) for v in tonic[idx]]
        mx = max(t)
        lse = mx + math.log(sum(math.exp(v - mx) for v in t))
        for k in range(24):
            maj = k - 12 if k >= 12 else (k + 3) % 12
            s = 0.0
            for j in range(12):
                inside = (j - maj) % 12 in SCALE
                q = p[j] if inside else -p[j]
                term = (math.log(q) if q > 0 else -math.inf) if inside else (math.log1p(q) if q > -1 else -math.inf)
                s += max(term, -100.0)
            out[idx + (k,)] = t[k % 12] - lse + weight / 12 * s
    return out


def test_key_emissions_equal_the_formula_and_clamp():
    g = torch.Generator().manual_seed(13)
    key = torch.rand((2, 9, 12), generator=g, dtype=torch.float64)
    tonic = torch.randn((2, 9, 12), generator=g, dtype=torch.float64) * 4
    key[0, 0, :4] = torch.tensor([0.0, 1.0, 1e-30, 1.0 - 1e-16])                                # saturated memberships
    key[1, 3] = torch.tensor([1.0, 0.0] * 6)
    for weight in (1.0, 2.5):
        got = metrics.key_emissions(key, tonic, signature_weight=weight)
        assert got.shape == (2, 9, 24) and bool(torch.isfinite(got).all())
        assert np.abs(got.numpy() - emissions_loop(key.numpy(), tonic.numpy(), weight)).max() < 1e-9
    # the clamp: a membership of exactly 0 inside the scale, or exactly 1 outside it, costs 100 / 12 and no more
    one = torch.full((1, 12), 0.5, dtype=torch.float64)
    flat = torch.zeros((1, 12), dtype=torch.float64)
    base = metrics.key_emissions(one, flat)
    zero_in = one.clone(); zero_in[0, 0] = 0.0                                                  # C: in C major (12), not in D major (14)
    d = metrics.key_emissions(zero_in, flat) - base
    assert float(d[0, 12]) == pytest.approx((-100 - math.log(0.5)) / 12) and float(d[0, 14]) == pytest.approx((0 - math.log(0.5)) / 12)
    one_out = one.clone(); one_out[0, 0] = 1.0
    d = metrics.key_emissions(one_out, flat) - base
    assert float(d[0, 14]) == pytest.approx((-100 - math.log(0.5)) / 12) and float(d[0, 12]) == pytest.approx((0 - math.log(0.5)) / 12)
    # counts: zeros behind a recording's count
    got = metrics.key_emissions(key, tonic, counts=torch.tensor([9, 4]))
    assert bool((got[1, 4:] == 0).all()) and bool((got[1, :4] != 0).all()) and bool((got[0] != 0).all())
    assert metrics.key_emissions(key.float(), tonic.float()).dtype == torch.float32


def test_the_emissions_argmax_is_a_key_whose_tonic_fits_its_signature():
    """Clean inputs -- the scale of a key as memberships, its tonic as the largest logit -- score that key highest; and whatever the
    inputs, the argmax is one of the 24 keys, each of which is a (signature, fitting tonic) pair by construction: decode_keys agrees
    with it wherever it finds a key at all on clean inputs."""
    keys, tonics = [], []
    for k in range(24):
        keys.append(metrics.KEY_SCALES[k] * 0.9 + 0.05)
        tonics.append(torch.nn.functional.one_hot(torch.tensor(k % 12), 12).double() * 5)
    key, tonic = torch.stack(keys), torch.stack(tonics)
    e = metrics.key_emissions(key, tonic)
    assert first_max(e).tolist() == list(range(24))
    key_id = metrics.decode_keys(key, tonic)[0]
    assert key_id.tolist() == list(range(24))
    # a tonic that does not fit the signature: decode_keys says -1, the emissions still name a key, with the signature's scale or the tonic
    e = metrics.key_emissions(key[12:13], tonic[2:3])                                           # C major scale, tonic D
    assert int(metrics.decode_keys(key[12:13], tonic[2:3])[0]) == -1
    k = int(first_max(e)[0])
    assert 0 <= k < 24 and (metrics.KEY_MAJOR_TONIC[k] == 0 or k % 12 == 2)
    g = torch.Generator().manual_seed(14)
    noisy = first_max(metrics.key_emissions(torch.rand((50, 12), generator=g), torch.randn((50, 12), generator=g)))
    assert ((noisy >= 0) & (noisy < 24)).all()


def _track(key_id, smooth, counts):
    key_id = torch.tensor(key_id, dtype=torch.int32)
    R, W = key_id.shape
    z = torch.zeros((R, W, 12))
    times = (torch.arange(W, dtype=torch.float64) * 25 + 37.5) * 4410 / 22050
    smooth_id = None if smooth is None else torch.tensor(smooth, dtype=torch.int32)
    return P.KeyTrack(z, z, None, key_id, key_id, key_id, torch.zeros((R, W)), torch.tensor(counts, dtype=torch.int32), times, 15.2, 5.0,
                      emissions=None if smooth is None else torch.zeros((R, W, 24)), smooth_key_id=smooth_id)


def test_segments_read_the_smoothed_path_when_there_is_one():
    raw = [[9, -1, 9, 12, -1, 9, 9], [0, 0, -1, -1, -1, -1, -1]]
    tr = _track(raw, [[9, 9, 9, 9, 9, 9, 9], [0, 12, -1, -1, -1, -1, -1]], [7, 2])
    assert len(tr._tensors()) == 10 and tr._tensors()[-1] is tr.smooth_key_id and tr._tensors()[-2] is tr.emissions
    assert tr.segments(0) == [(0.0, pytest.approx(37.5 + 7.6), 9, "A minor")]
    assert tr.segments(0) == tr.segments(0, smoothed=True)
    assert [s[2] for s in tr.segments(0, smoothed=False)] == [9, -1, 9, 12, -1, 9]
    assert [(s[2], s[3]) for s in tr.segments(1)] == [(0, "C minor"), (12, "C major")]
    assert [s[1] for s in tr.segments(1)] == pytest.approx([10.0, 12.5 + 7.6])
    plain = _track(raw, None, [7, 2])
    assert plain.emissions is None and plain.smooth_key_id is None and len(plain._tensors()) == 8      # a plain track lists what it did
    assert plain.segments(0) == tr.segments(0, smoothed=False) == plain.segments(0, smoothed=False)
    with pytest.raises(ValueError, match="smooth=True"):
        plain.segments(0, smoothed=True)
