"""Host: metrics.key_posteriors (the float64 model of ake_key_posteriors_f32), transition_m_step and fit_key_transition.  No GPU."""
import itertools

import pytest
import torch

import ake_amd
from ake_amd import metrics


def brute_force(e, A, prior):
    """Sum over all 24^W paths of one recording (W <= 3), float64 -> (post, loglik, xi_sum)."""
    W = e.shape[0]
    paths = torch.tensor(list(itertools.product(range(24), repeat=W)), dtype=torch.int64)          # (24^W, W)
    score = prior[paths[:, 0]] + e[0, paths[:, 0]]
    for w in range(1, W):
        score = score + A[paths[:, w - 1], paths[:, w]] + e[w, paths[:, w]]
    loglik = torch.logsumexp(score, dim=0)
    weight = torch.exp(score - loglik)
    post = torch.zeros((W, 24), dtype=torch.float64)
    xi = torch.zeros((24, 24), dtype=torch.float64)
    for w in range(W):
        post[w].index_add_(0, paths[:, w], weight)
        if w > 0:
            xi.view(-1).index_add_(0, paths[:, w - 1] * 24 + paths[:, w], weight)
    return post, loglik, xi


@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("with_prior", [False, True])
def test_posteriors_equal_a_sum_over_all_paths(W, with_prior):
    g = torch.Generator().manual_seed(100 + W)
    e = 3 * torch.randn((W, 24), generator=g, dtype=torch.float64)
    prior = torch.randn(24, generator=g, dtype=torch.float64) if with_prior else None
    A = metrics.key_transition_log(0.7)
    post, loglik, xi = metrics.key_posteriors(e, A, log_prior=prior, transitions=True)
    assert post.shape == (W, 24) and loglik.shape == () and xi.shape == (24, 24) and post.dtype == torch.float64
    want_post, want_ll, want_xi = brute_force(e, A, torch.zeros(24, dtype=torch.float64) if prior is None else prior)
    assert float((post - want_post).abs().max()) <= 1e-12 * float(want_post.abs().max())
    assert abs(float(loglik - want_ll)) <= 1e-12 * abs(float(want_ll))
    assert float((xi - want_xi).abs().max()) <= 1e-12 * max(float(want_xi.abs().max()), 1e-300)
    if W == 1:
        assert bool((xi == 0).all())
    # the two-value form is the same call without the transition sums
    post2, ll2 = metrics.key_posteriors(e, A, log_prior=prior)
    assert torch.equal(post2, post) and torch.equal(ll2, loglik)


@pytest.fixture(scope="module")
def ragged():
    g = torch.Generator().manual_seed(7)
    W, counts = 30, [30, 7, 1, 0]
    e = 3 * torch.randn((4, W, 24), generator=g, dtype=torch.float64)
    A = metrics.key_transition_log(0.7)
    return e, A, counts, metrics.key_posteriors(e, A, counts=counts, transitions=True)


def test_counts(ragged):
    e, A, counts, (post, loglik, xi) = ragged
    assert post.shape == (4, 30, 24) and loglik.shape == (4,) and xi.shape == (4, 24, 24)
    for r, n in enumerate(counts):
        assert bool((post[r, n:] == 0).all())
        if n <= 1:
            assert bool((xi[r] == 0).all())
        if n == 0:
            assert float(loglik[r]) == 0.0
            continue
        p1, l1, x1 = metrics.key_posteriors(e[r, :n], A, transitions=True)                      # the recording alone, at its own length
        assert float((post[r, :n] - p1).abs().max()) <= 1e-12
        assert abs(float(loglik[r] - l1)) <= 1e-12 * abs(float(l1))
        assert float((xi[r] - x1).abs().max()) <= 1e-12 * max(float(x1.abs().max()), 1.0)
    # counts beyond the tensor are clamped to it
    pc, lc = metrics.key_posteriors(e, A, counts=[99, 7, 1, -3])
    assert torch.equal(pc, post) and torch.equal(lc, loglik)


def test_sums(ragged):
    e, A, counts, (post, loglik, xi) = ragged
    for r, n in enumerate(counts):
        if n == 0:
            continue
        assert float((post[r, :n].sum(dim=1) - 1).abs().max()) <= 1e-10
        assert abs(float(xi[r].sum()) - (n - 1)) <= 1e-10
        # a move into j at window w is being in j at w; a move out of i at w - 1 is being in i at w - 1
        assert float((xi[r].sum(dim=0) - post[r, 1:n].sum(dim=0)).abs().max()) <= 1e-10
        assert float((xi[r].sum(dim=1) - post[r, :n - 1].sum(dim=0)).abs().max()) <= 1e-10


def transpositions():
    """The 12 transpositions of the 24 keys as index tensors: key (mode, t) -> (mode, t + s)."""
    k = torch.arange(24)
    return [(k // 12) * 12 + (k % 12 + s) % 12 for s in range(12)]


def test_m_step(ragged):
    _, _, _, (_, _, xi) = ragged
    init = metrics.key_transition_log(0.8)
    for tied in (True, False):
        A = metrics.transition_m_step(xi, init, tied=tied)
        assert A.shape == (24, 24) and A.dtype == torch.float64 and bool(torch.isfinite(A).all())
        assert float((torch.exp(A).sum(dim=1) - 1).abs().max()) <= 1e-12
    A = metrics.transition_m_step(xi, init, tied=True)
    for T in transpositions():
        assert float((A[T][:, T] - A).abs().max()) <= 1e-12
    assert len(set(torch.round(A.reshape(-1) * 1e9).tolist())) <= 48                                 # 48 classes of 12 cells
    untied = metrics.transition_m_step(xi, init, tied=False)
    assert float((untied[transpositions()[1]][:, transpositions()[1]] - untied).abs().max()) > 1e-3       # (tying does something)
    for tied in (True, False):
        back = metrics.transition_m_step(torch.zeros((3, 24, 24)), init, tied=tied, pseudo_count=2.5)
        assert float((back - init).abs().max()) <= 1e-12
    with pytest.raises(ValueError):
        metrics.transition_m_step(torch.zeros((24, 12)), init)


@pytest.mark.parametrize("tied", [True, False])
def test_em_does_not_lower_the_score(tied):
    g = torch.Generator().manual_seed(11)
    e = [3 * torch.randn((3, 40, 24), generator=g, dtype=torch.float64), 3 * torch.randn((25, 24), generator=g, dtype=torch.float64)]
    A, scores = metrics.fit_key_transition(e, counts=[[40, 22, 1], None], iterations=8, tied=tied)
    assert A.dtype == torch.float64 and A.shape == (24, 24) and len(scores) == 8 and all(isinstance(s, float) for s in scores)
    for before, after in zip(scores, scores[1:]):
        assert after >= before - 1e-9 * abs(before)
    assert scores[-1] > scores[0]
    # the first score is the recordings' score under the initial matrix
    init = metrics.key_transition_log(stay=0.9)
    want = float(metrics.key_posteriors(e[0], init, counts=[40, 22, 1])[1].sum() + metrics.key_posteriors(e[1], init)[1])
    assert scores[0] == pytest.approx(want, rel=1e-12)


def test_em_recovers_a_planted_transition():
    """64 chains x 200 windows sampled from exp(key_transition_log(0.9)), emissions randn + 10 on the sampled key; fitted from
    key_transition_log(0.5).  The mean fitted stay probability lies within 0.02 of 0.9: 7 standard errors of the empirical stay
    frequency over 12 736 transitions (sqrt(0.9 * 0.1 / 12736) = 0.0027); the pseudo-counts move it by under 0.002."""
    torch.manual_seed(0)
    P = torch.exp(metrics.key_transition_log(0.9))
    R, W = 64, 200
    keys = torch.zeros((R, W), dtype=torch.int64)
    keys[:, 0] = torch.randint(0, 24, (R,))
    for w in range(1, W):
        keys[:, w] = torch.multinomial(P[keys[:, w - 1]], 1)[:, 0]
    e = torch.randn((R, W, 24), dtype=torch.float64)
    e.scatter_add_(2, keys[..., None], torch.full((R, W, 1), 10.0, dtype=torch.float64))
    A, scores = metrics.fit_key_transition(e, init=metrics.key_transition_log(0.5), iterations=8, tied=True)
    stay = float(torch.exp(torch.diagonal(A)).mean())
    empirical = float((keys[:, 1:] == keys[:, :-1]).double().mean())
    print(f"fitted stay {stay:.4f}, empirical {empirical:.4f}")
    assert abs(stay - 0.9) <= 0.02
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(scores, scores[1:]))


def test_validation():
    e = torch.zeros((2, 5, 24), dtype=torch.float64)
    A = metrics.key_transition_log(0.9)
    bad = A.clone()
    bad[0, 1] = -float("inf")
    with pytest.raises(ValueError, match="large negative"):
        metrics.key_posteriors(e, bad)
    with pytest.raises(ValueError, match="large negative"):
        metrics.key_posteriors(e, A, log_prior=torch.full((24,), float("nan"), dtype=torch.float64))
    with pytest.raises(ValueError, match="24, 24"):
        metrics.key_posteriors(e, A[:12])
    with pytest.raises(ValueError, match=r"\(R, W, 24\)"):
        metrics.key_posteriors(torch.zeros((5, 12)), A)
    with pytest.raises(ValueError, match="large negative"):
        metrics.fit_key_transition(e, init=bad)
    with pytest.raises(ValueError, match="24, 24"):
        metrics.fit_key_transition(e, init=A[:12])
    # posteriors=True without smooth=True is refused before anything else is looked at
    with pytest.raises(ValueError, match="smooth=True"):
        ake_amd.KeyEstimator.track(object.__new__(ake_amd.KeyEstimator), torch.zeros((1, 8)), posteriors=True)
    ids = torch.zeros((1, 3), dtype=torch.int32)
    plain = ake_amd.KeyTrack(None, None, None, ids, ids, ids, torch.zeros((1, 3)), torch.tensor([3], dtype=torch.int32),
                             torch.arange(3, dtype=torch.float64), 15.0, 5.0)
    assert len(plain.segments(0)) == 1 and len(plain.segments(0)[0]) == 4
    with pytest.raises(ValueError, match="posteriors"):
        plain.segments(0, confidence=True)
    plain.smooth_key_id, plain.smooth_confidence = ids, torch.tensor([[0.5, 0.75, 1.0]])
    assert plain.segments(0, confidence=True) == [plain.segments(0)[0] + (0.75,)]
    assert "key_posteriors" in ake_amd.__all__ and "transition_m_step" in ake_amd.__all__ and "fit_key_transition" in ake_amd.__all__
