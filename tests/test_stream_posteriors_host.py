"""Host: fixed-lag posteriors and the running log-likelihood of a stream (metrics.key_stream_posteriors) against their definitions --
key_posteriors on the prefix every window was decided on -- computed with the existing functions.  No GPU."""
import random

import pytest
import torch

import ake_amd
from ake_amd import metrics

LAGS = (0, 1, 3, 6, 39, 255)
WS = (1, 2, 7, 40)


def emissions(kind, R, W, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn((R, W, 24), generator=g, dtype=torch.float64) * 3
    if kind == "deep":                                                            # emissions down to -256: a saturated row per recording
        e = e - 200.0
        e[:, W // 2] = -256.0
        e[:, W // 2, 5] = -250.0
    return e.to(dtype)


def transition(kind):
    A = metrics.key_transition_log(0.9)
    if kind == "forbidden":
        A = A.clone()
        A[torch.arange(24), (torch.arange(24) + 6) % 24] = -1e4                  # a forbidden transition, written as -1e4
        A[3, 3] = -1e4
    return A


CASES = (("gauss", "plain", False), ("gauss", "forbidden", True), ("deep", "forbidden", True), ("deep", "plain", False))


def case(kind, trans, with_prior, R, W, dtype=torch.float64):
    e = emissions(kind, R, W, dtype, seed=10 * W + len(kind))
    prior = torch.randn(24, generator=torch.Generator().manual_seed(5), dtype=torch.float64) if with_prior else None
    return e, transition(trans), prior


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("kind,trans,with_prior", CASES)
def test_every_window_is_key_posteriors_on_its_prefix(kind, trans, with_prior, W):
    e, A, prior = case(kind, trans, with_prior, 2, W)
    for lag in LAGS:
        post, loglik = metrics.key_stream_posteriors(e, A, prior, lag=lag, flush=False)
        first, k_out = metrics.key_stream_count(0, W, lag, False)
        assert first == 0 and post.shape == (2, k_out, 24) and post.dtype == e.dtype and loglik.shape == (2, W)
        for v in range(k_out):
            want = metrics.key_posteriors(e[:, :v + lag + 1], A, prior)[0][:, v]
            assert float((post[:, v] - want).abs().max()) <= 1e-12, (lag, v)
        for w in range(W):
            want = metrics.key_posteriors(e[:, :w + 1], A, prior)[1]
            assert float((loglik[:, w] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (lag, w)
        # with a flush: the same windows, then the last `lag` from the whole recording's posteriors
        flushed, loglik2 = metrics.key_stream_posteriors(e, A, prior, lag=lag)
        whole = metrics.key_posteriors(e, A, prior)[0]
        assert flushed.shape == (2, W, 24) and torch.equal(flushed[:, :k_out], post) and torch.equal(loglik2, loglik)
        assert float((flushed[:, k_out:] - whole[:, k_out:]).abs().max() if k_out < W else 0.0) <= 1e-12, lag
        if lag >= W:
            assert float((flushed - whole).abs().max()) <= 1e-12
        assert float((flushed.sum(dim=2) - 1).abs().max()) <= 1e-12 and bool((flushed >= 0).all()) and bool(torch.isfinite(loglik).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lag_zero_is_the_softmax_of_filtered(dtype):
    e, A, prior = case("gauss", "forbidden", True, 3, 40, dtype)
    filtered, _ = metrics.key_stream(e, A, prior, lag=0)
    post, _ = metrics.key_stream_posteriors(e, A, prior, lag=0)
    assert torch.equal(post, torch.softmax(filtered, dim=2))


def test_single_recording_and_dtype():
    e, A, prior = case("gauss", "plain", False, 2, 7, torch.float32)
    _, path = metrics.key_stream(e, A, lag=3)
    both = metrics.key_stream_posteriors(e, A, lag=3, path=path)
    single = metrics.key_stream_posteriors(e[0], A, lag=3, path=path[0])
    assert [t.shape for t in single] == [(7, 24), (7,), (7,)] and all(t.dtype == torch.float32 for t in both)
    for a, b in zip(single, both):
        assert torch.equal(a, b[0])


def run_in_pieces(e, A, prior, lag, pieces, with_path=True):
    state, sstate, ps, ls, pps, at = None, None, [], [], [], 0
    for i, k in enumerate(pieces):
        flush = i == len(pieces) - 1
        _, path, sstate = metrics.key_stream(e[:, at:at + k], A, prior, lag=lag, state=sstate, flush=flush, return_state=True)
        p, ll, pp, state = metrics.key_stream_posteriors(e[:, at:at + k], A, prior, lag=lag, state=state, flush=flush, return_state=True,
                                                         path=path)
        first, k_out = metrics.key_stream_count(at, k, lag, flush)
        assert p.shape == (e.shape[0], k_out, 24) and ll.shape == (e.shape[0], k) and pp.shape == path.shape and state["windows"] == at + k
        ps.append(p); ls.append(ll); pps.append(pp); at += k
    assert at == e.shape[1]
    return torch.cat(ps, dim=1), torch.cat(ls, dim=1), torch.cat(pps, dim=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pieces_with_carried_state_are_identical(dtype):
    """200 random cuts (k = 0 pieces among them) of one sequence, at every lag: torch.equal on all three outputs."""
    W = 40
    e, A, prior = case("gauss", "forbidden", True, 2, W, dtype)
    rng = random.Random(7)
    whole = {}
    for lag in LAGS:
        _, path = metrics.key_stream(e, A, prior, lag=lag)
        whole[lag] = metrics.key_stream_posteriors(e, A, prior, lag=lag, path=path)
        assert torch.equal(whole[lag][2], whole[lag][0].gather(2, path.long()[..., None])[..., 0])     # (no -1 in a stream's path)
    fixed = [[1] * W, [7, 33], [W, 0], [0, 7, 0, 33]]
    for n in range(200):
        lag = LAGS[n % len(LAGS)]
        if n < len(fixed) * len(LAGS):
            pieces = fixed[n // len(LAGS)]
        else:
            cuts = sorted(rng.randrange(0, W + 1) for _ in range(rng.randrange(0, 8)))
            pieces = [b - a for a, b in zip([0] + cuts, cuts + [W])]
        got = run_in_pieces(e, A, prior, lag, pieces)
        for a, b in zip(got, whole[lag]):
            assert torch.equal(a, b), (lag, pieces)


def test_path_post_is_zero_where_the_path_holds_none():
    e, A, _ = case("gauss", "plain", False, 2, 7)
    path = torch.tensor([[0, -1, 5, 23, -1, 2, 2]] * 2, dtype=torch.int32)
    post, _, pp = metrics.key_stream_posteriors(e, A, lag=2, path=path)
    want = torch.where(path >= 0, post.gather(2, path.long().clamp(min=0)[..., None])[..., 0], torch.zeros(()).double())
    assert torch.equal(pp, want) and float(pp[0, 1]) == 0.0 and float(pp[0, 0]) > 0.0


def test_model_refuses_bad_arguments():
    e, A = emissions("gauss", 1, 4, torch.float32), transition("plain")
    for lag in (-1, 256):
        with pytest.raises(ValueError):
            metrics.key_stream_posteriors(e, A, lag=lag)
    with pytest.raises(ValueError):
        metrics.key_stream_posteriors(e[..., :23], A)
    with pytest.raises(ValueError):
        metrics.key_stream_posteriors(e, A[:23])
    with pytest.raises(ValueError):
        metrics.key_stream_posteriors(e, A, path=torch.zeros((1, 3), dtype=torch.int32))          # not the windows this call decides
    for where in ("trans", "prior", "emissions"):
        bad_A, bad_p, bad_e = A.clone(), torch.zeros(24), e.clone()
        {"trans": bad_A, "prior": bad_p, "emissions": bad_e[0]}[where][0, ...].fill_(float("-inf"))
        with pytest.raises(ValueError):
            metrics.key_stream_posteriors(bad_e, bad_A, bad_p)
    assert "key_stream_posteriors" in ake_amd.__all__ and ake_amd.key_stream_posteriors is metrics.key_stream_posteriors


def test_stream_refuses_posteriors_without_a_smoother():
    from types import SimpleNamespace
    from ake_amd.pipeline import KeyEstimator
    est = object.__new__(KeyEstimator)
    est.net, est.frames, est.wrap_mode, est.sample_rate = SimpleNamespace(local=False), 5, "dataset_max", 22050
    with pytest.raises(ValueError, match="smooth=True"):
        est.stream(1, smooth=False, posteriors=True)


def test_update_concat_joins_the_new_fields():
    from ake_amd.stream import StreamUpdate
    z = lambda *s: torch.zeros(s)
    mk = lambda k, k2, first, post: StreamUpdate(first, k, z(1, k, 12), z(1, k, 12), None, z(1, k), z(1, k), z(1, k), z(1, k), torch.zeros(k), z(1, k, 24),
                                                 z(1, k, 24), 0, z(1, k2), *((torch.full((1, k2, 24), float(k)), torch.full((1, k2), float(k)),
                                                                              torch.full((1, k), float(k))) if post else ()))
    u = StreamUpdate.concat([mk(2, 0, 0, True), mk(3, 4, 2, True)])
    assert u.posteriors.shape == (1, 4, 24) and u.smooth_confidence.shape == (1, 4) and u.log_likelihood.tolist() == [[2, 2, 3, 3, 3]]
    u = StreamUpdate.concat([mk(2, 0, 0, False), mk(3, 4, 2, False)])
    assert u.posteriors is None and u.smooth_confidence is None and u.log_likelihood is None and u.smooth_key_id.shape == (1, 4)
