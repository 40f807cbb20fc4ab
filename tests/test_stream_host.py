"""Host: the smoother with carried state (metrics.key_stream) against its two definitions -- prefix Viterbi decodes and key_posteriors'
forward rows -- computed with the existing functions, and the stream's geometry (ake_amd.stream: which frames are final, where the
re-transform starts, which windows are ready, how many windows leave the lag).  No GPU."""
import random
from types import SimpleNamespace

import pytest
import torch

import ake_amd
from ake_amd import metrics, stream
from ake_amd.pipeline import KeyEstimator, track_counts

LAGS = (0, 1, 3, 12, 255)
HOP, WF = 4410, 76


def emissions(kind, R, W, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "gauss":
        return (torch.randn((R, W, 24), generator=g, dtype=torch.float64) * 3).to(dtype)
    return torch.randint(-2, 3, (R, W, 24), generator=g).to(dtype)               # tie-heavy: small integers


def transition(kind):
    A = metrics.key_transition_log(0.9)
    if kind == "forbidden":
        A = A.clone()
        A[torch.arange(24), (torch.arange(24) + 6) % 24] = -1e4                  # a forbidden transition, written as -1e4
        A[3, 3] = -1e4
    return A


def prefix_paths(e, A, prior, lag):
    """path[v] by its definition: W decodes with the existing function."""
    W = e.shape[1]
    return torch.stack([metrics.viterbi_keys(e[:, :min(W, v + lag + 1)], A, prior)[:, v] for v in range(W)], dim=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["gauss", "ties"])
@pytest.mark.parametrize("W", [1, 2, 40])
def test_path_is_the_prefix_decodes(dtype, kind, W):
    e = emissions(kind, 2, W, dtype, seed=W)
    g = torch.Generator().manual_seed(5)
    prior = torch.randn(24, generator=g, dtype=torch.float64)
    for trans, pr in (("plain", None), ("forbidden", prior)):
        A = transition(trans)
        for lag in LAGS:
            filtered, path = metrics.key_stream(e, A, pr, lag=lag)
            assert path.dtype == torch.int32 and path.shape == (2, W) and filtered.shape == (2, W, 24) and filtered.dtype == dtype
            assert torch.equal(path, prefix_paths(e, A, pr, lag)), (trans, lag)
            if lag >= W:
                assert torch.equal(path, metrics.viterbi_keys(e, A, pr))
    single_f, single_p = metrics.key_stream(e[0], A, lag=3)
    both_f, both_p = metrics.key_stream(e, A, lag=3)
    assert torch.equal(single_f, both_f[0]) and torch.equal(single_p, both_p[0])


@pytest.mark.parametrize("kind", ["gauss", "ties"])
def test_lag_zero_is_the_first_maximum_of_every_step(kind):
    """d_w by viterbi_keys' recurrence, restated: the lag-0 label is the smallest j attaining its maximum."""
    e, A = emissions(kind, 3, 40, torch.float64, seed=9), transition("plain").double()
    _, path = metrics.key_stream(e, A, lag=0)
    d = e[:, 0] - e[:, 0].max(dim=1, keepdim=True).values
    for w in range(40):
        if w:
            raw = (d[:, :, None] + A[None]).max(dim=1).values + e[:, w]
            d = raw - raw.max(dim=1, keepdim=True).values
        first = torch.stack([torch.nonzero(row == row.max()).flatten()[0] for row in d])
        assert torch.equal(path[:, w].long(), first), w


@pytest.mark.parametrize("W", [1, 2, 40])
def test_filtered_is_the_forward_row_of_key_posteriors(W):
    """exp(filtered[w]) = the posterior of window w given windows 0..w = key_posteriors(e[:w + 1]).post[w] (its b is 0 there)."""
    e = emissions("gauss", 2, W, torch.float64, seed=20 + W)
    g = torch.Generator().manual_seed(6)
    prior = torch.randn(24, generator=g, dtype=torch.float64)
    for trans, pr in (("plain", None), ("forbidden", prior)):
        A = transition(trans)
        filtered, _ = metrics.key_stream(e, A, pr, lag=3)
        for w in range(W):
            post, _ = metrics.key_posteriors(e[:, :w + 1], A, pr)
            assert float((filtered[:, w].exp() - post[:, w]).abs().max()) <= 1e-12, (trans, w)


def run_in_pieces(e, A, prior, lag, pieces):
    state, fs, ps, at = None, [], [], 0
    for i, k in enumerate(pieces):
        f, p, state = metrics.key_stream(e[:, at:at + k], A, prior, lag=lag, state=state, flush=i == len(pieces) - 1, return_state=True)
        first, k_out = metrics.key_stream_count(at, k, lag, i == len(pieces) - 1)
        assert p.shape[1] == k_out and first == max(0, at - lag)
        fs.append(f); ps.append(p); at += k
    assert at == e.shape[1]
    return torch.cat(fs, dim=1), torch.cat(ps, dim=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["gauss", "ties"])
def test_pieces_with_carried_state_are_identical(dtype, kind):
    e, A = emissions(kind, 2, 40, dtype, seed=31), transition("forbidden")
    prior = torch.linspace(-1, 1, 24, dtype=torch.float64)
    for lag in LAGS:
        whole_f, whole_p = metrics.key_stream(e, A, prior, lag=lag)
        for pieces in ([1] * 40, [7, 33], [40], [40, 0], [0, 7, 0, 33]):
            f, p = run_in_pieces(e, A, prior, lag, pieces)
            assert torch.equal(f, whole_f) and torch.equal(p, whole_p), (lag, pieces)


def test_model_refuses_bad_arguments():
    e, A = emissions("gauss", 1, 4, torch.float32), transition("plain")
    for lag in (-1, 256):
        with pytest.raises(ValueError):
            metrics.key_stream(e, A, lag=lag)
    with pytest.raises(ValueError):
        metrics.key_stream(e[..., :23], A)
    with pytest.raises(ValueError):
        metrics.key_stream(e, A[:23])
    bad = A.clone()
    bad[0, 1] = float("-inf")
    with pytest.raises(ValueError):
        metrics.key_stream(e, bad)
    assert "key_stream" in ake_amd.__all__ and "KeyStream" in ake_amd.__all__ and "StreamUpdate" in ake_amd.__all__


# ---- the geometry -----------------------------------------------------------------------------------------------------------------------

def test_final_frames_is_its_definition():
    for hop, H in ((4410, 20968), (5, 7), (3, 0)):
        for N in list(range(0, 6 * hop + 2 * H, max(1, hop // 7))) + [H, H + 1, H + hop, H + hop + 1]:
            want = sum(1 for t in range(N // hop + 2) if t * hop + H <= N - 1)
            assert stream.final_frames(N, hop, H) == want, (hop, H, N)
            assert stream.final_frames(N, hop, H, finished=True) == 1 + N // hop
            assert stream.final_frames(N, hop, H) <= 1 + N // hop


def test_smooth_count():
    for before in (0, 1, 5, 300):
        for k in (0, 1, 7):
            for lag in (0, 1, 3, 255):
                first, n = stream.smooth_count(before, k, lag, False)
                assert first == max(0, before - lag) and n == max(0, before + k - lag) - first
                first, n = stream.smooth_count(before, k, lag, True)
                assert n == before + k - first


@pytest.mark.parametrize("sf", [25, 5, 100])
def test_random_chunk_schedules(sf):
    """200 chunk sequences: every window once and in order, none before its last frame is final, track's count after finish, s0 a
    multiple of hop and never ahead of the first needed frame's support -- and the history a stream keeps stays within its bound."""
    rng = random.Random(sf)
    H = 20968
    special = [0, 1, HOP - 1, HOP, HOP + 1]
    for case in range(200):
        lag = rng.choice(LAGS)
        chunks = [rng.choice(special) if rng.random() < 0.4 else rng.randrange(0, 60000) for _ in range(rng.randrange(1, 40))]
        N = F = W = s0 = 0
        emitted, smoothed = [], []
        for i, m in enumerate(chunks + [None]):
            finishing = m is None
            N_old, N = N, N + (0 if finishing else m)
            s0_new = stream.transform_start(F, HOP, H)
            assert s0_new % HOP == 0 and s0_new >= s0 and s0_new <= max(0, F * HOP - H) and (s0_new == 0 or s0_new > F * HOP - H - HOP)
            assert N_old - s0_new <= 2 * H + HOP                                  # what survives a push
            s0 = s0_new
            F_new = stream.final_frames(N, HOP, H, finishing)
            assert F_new >= F
            if F_new > F and not finishing:
                assert (F_new - 1) * HOP + H <= N - 1 and F_new * HOP + H > N - 1      # the last final frame, and the first that is not
            first_local = F - s0 // HOP
            assert first_local >= 0 and (N == s0 or first_local + (F_new - F) <= 1 + (N - s0) // HOP)
            F = F_new
            ready = stream.windows_ready(F, WF, sf)
            for w in range(W, ready):
                assert w * sf + WF <= F                                           # its last frame is final
                emitted.append(w)
            first, n = stream.smooth_count(W, ready - W, lag, finishing)
            smoothed += list(range(first, first + n))
            W = ready
        assert emitted == list(range(track_counts(1 + N // HOP, WF, sf)))
        assert smoothed == emitted


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------

def stub_estimator(**kw):
    est = object.__new__(KeyEstimator)
    est.net, est.frames, est.wrap_mode, est.sample_rate = SimpleNamespace(local=False), 5, "dataset_max", 22050
    for k, v in kw.items():
        setattr(est, k, v)
    return est


def test_stream_refusals():
    with pytest.raises(ValueError, match="rate"):
        stub_estimator().stream(1, rate=44100)
    with pytest.raises(ValueError, match="tuning"):
        stub_estimator().stream(1, tuning="auto")
    for lag in (-1, 256):
        with pytest.raises(ValueError, match="lag_windows"):
            stub_estimator().stream(1, lag_windows=lag)
    with pytest.raises(ValueError, match="recordings"):
        stub_estimator().stream(0)
    with pytest.raises(ValueError, match="without one"):
        stub_estimator(net=None).stream(1)
    with pytest.raises(ValueError, match="frames=0"):
        stub_estimator(frames=0).stream(1)
    with pytest.raises(ValueError, match="true_end"):
        stub_estimator(wrap_mode="true_end").stream(1)
    with pytest.raises(ValueError, match="--local"):
        stub_estimator(net=SimpleNamespace(local=True)).stream(1)


def test_push_refusals():
    s = object.__new__(stream.KeyStream)
    s.R, s.finished, s.dtype = 2, False, torch.float32
    with pytest.raises(ValueError, match="R = 2"):
        s.push(torch.zeros(3, 10))
    with pytest.raises(ValueError, match="R = 2"):
        s.push(torch.zeros(2, 2, 10))                                             # channels: a stream does not pick one
    with pytest.raises(ValueError, match="float32 or int16"):
        s.push(torch.zeros(2, 10, dtype=torch.float64))
    with pytest.raises(ValueError, match="takes torch.float32"):
        s.push(torch.zeros(2, 10, dtype=torch.int16))
    s.finished = True
    with pytest.raises(ValueError, match="finished"):
        s.push(torch.zeros(2, 10))
    with pytest.raises(ValueError, match="finished"):
        s.finish()
