"""GPU: posterior key probabilities -- ake_key_posteriors_f32 (key_forward_backward_kernel, key_posteriors_kernel and the ordered sum of
the transition counts), KeyEstimator.track(smooth=True, posteriors=True) and ake_amd.fit_key_transition.

The model is metrics.key_posteriors in float64 on the device's own float32 inputs.  The bounds on the kernel's error are measured ones:
the device's worst error over the cases of test_kernel_against_the_float64_model and over five more seeds of its W = 9, 65 and 300, times
4 (another ROCm version's exp / log, the spread over seeds), rounded up to one digit.  Beside each stands what the SAME model costs in
float32 on the host on the same inputs, the yardstick for rounding alone (a device error above 10 x that would be a finding, not a bound):

    output                                         device worst    float32 host model    bound
    post     (absolute)                            7.9e-7          8.3e-7                4e-6
    loglik   (relative to the batch's largest)     3.2e-7          3.1e-7                2e-6
    xi_sum   (absolute, W <= 300)                  5.7e-6          5.8e-6                3e-5
    fitted P (absolute, 3 EM iterations, R = 8)    2.0e-8          --                    8e-8

(profiles/track_posteriors.md has the figures per window count, W = 2000 included.)"""
import json
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N45 = 992250                         # 45 s at 22.05 kHz: 226 frames; 7 windows at a 5 s stride, 31 at 1 s

TOL_POST = 4e-6                      # the module docstring's bounds
TOL_LOGLIK = 2e-6
TOL_XI = 3e-5
TOL_EM_P = 8e-8


def device_posteriors(e, A, counts=None, prior=None, path=None, xi=True, poison=True):
    """ake_key_posteriors_f32 on float32 tensors given on the CPU -> (post, loglik, xi_sum, path_post) on the CPU.  Outputs and workspace
    are poisoned before the call: whatever the kernels do not write shows."""
    L = _lib.lib()
    R, W, _ = e.shape
    e_d, A_d = e.to(DEV).contiguous(), A.to(DEV).contiguous()
    assert e_d.dtype == torch.float32 and A_d.dtype == torch.float32
    c_d = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    p_d = None if prior is None else prior.to(DEV).contiguous()
    path_d = None if path is None else path.to(DEV).contiguous()
    nbytes = L.ake_key_posteriors_workspace_bytes(R, W)
    assert nbytes >= 2 * R * W * 24 * 4
    ws = torch.full((nbytes,), 0xAB if poison else 0, dtype=torch.uint8, device=DEV)
    nan = float("nan")
    post = torch.full((R, W, 24), nan, dtype=torch.float32, device=DEV)
    loglik = torch.full((R,), nan, dtype=torch.float32, device=DEV)
    xi_sum = torch.full((R, 24, 24), nan, dtype=torch.float32, device=DEV) if xi else None
    pp = torch.full((R, W), nan, dtype=torch.float32, device=DEV) if path is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()                                          # noqa: E731
    _lib.check(L.ake_key_posteriors_f32(e_d.data_ptr(), R, W, ptr(c_d), A_d.data_ptr(), ptr(p_d), ptr(path_d), post.data_ptr(), loglik.data_ptr(),
                                        ptr(xi_sum), ptr(pp), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
               "ake_key_posteriors_f32")
    torch.cuda.synchronize()
    return post.cpu(), loglik.cpu(), None if xi_sum is None else xi_sum.cpu(), None if pp is None else pp.cpu()


def device_viterbi(e, A, counts=None):
    L = _lib.lib()
    R, W, _ = e.shape
    e_d, A_d = e.to(DEV).contiguous(), A.to(DEV).contiguous()
    c_d = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    ws = torch.empty((L.ake_viterbi_keys_workspace_bytes(R, W),), dtype=torch.uint8, device=DEV)
    path = torch.full((R, W), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.ake_viterbi_keys_f32(e_d.data_ptr(), R, W, None if c_d is None else c_d.data_ptr(), A_d.data_ptr(), None, path.data_ptr(),
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "ake_viterbi_keys_f32")
    torch.cuda.synchronize()
    return path.cpu()


def default_trans(stride=5.0):
    return metrics.key_transition_log(stay=math.exp(-stride / 60.0)).float()


def net_like_emissions(R, W, seed, tonic_scale=4.0, saturated=False):
    """float32 emissions as the emission kernel's: metrics.key_emissions on seeded key rows and tonic logits."""
    g = torch.Generator().manual_seed(seed)
    key = torch.rand((R, W, 12), generator=g)
    if saturated:
        key = (key > 0.5).float()                                                               # exact 0s and 1s: the -100 clamps
    tonic = torch.randn((R, W, 12), generator=g) * tonic_scale
    return metrics.key_emissions(key, tonic), g


def errors(got, want):
    """(post abs, loglik rel, xi abs) of a (post, loglik, xi_sum, ...) triple against the float64 model's.  The log-likelihoods are
    compared relative to the batch's largest: a sum of c_w of either sign can lie near 0, where its own magnitude is no scale."""
    post = float((got[0].double() - want[0]).abs().max())
    ll = float((got[1].double() - want[1]).abs().max() / want[1].abs().max())
    xi = float((got[2].double() - want[2]).abs().max())
    return post, ll, xi


def check_invariants(post, loglik, xi, counts, W):
    assert bool(torch.isfinite(post).all()) and bool(torch.isfinite(loglik).all()) and (xi is None or bool(torch.isfinite(xi).all()))
    for r, n in enumerate(counts):
        n = min(max(n, 0), W)
        assert bool((post[r, n:] == 0).all())
        if n:
            assert float((post[r, :n].sum(dim=1) - 1).abs().max()) <= 1e-5 and bool((post[r, :n] >= 0).all())
        else:
            assert float(loglik[r]) == 0.0
        if xi is None:
            continue
        if n <= 1:
            assert bool((xi[r] == 0).all())
        else:
            assert abs(float(xi[r].double().sum()) - (n - 1)) <= 1e-5 * (n - 1)


CHUNK_PLUS_1 = 65                    # ake_key_posteriors_chunk_windows() + 1 (asserted below)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("W", [1, 2, 7, 8, 9, 40, CHUNK_PLUS_1, 300])
def test_kernel_against_the_float64_model(W, with_prior):
    """R = 4, counts (W, W - 3, 1, 0): one and two windows, both sides of the 8-row prefetch batch, one window past the posterior
    kernel's chunk, and many chunks.  Bounds: the module docstring."""
    assert _lib.lib().ake_key_posteriors_chunk_windows() + 1 == CHUNK_PLUS_1
    counts = [W, max(W - 3, 0), 1, 0]
    e, g = net_like_emissions(4, W, 300 + W)
    A = default_trans()
    prior = torch.randn(24, generator=g) if with_prior else None
    got = device_posteriors(e, A, counts, prior)
    want = metrics.key_posteriors(e.double(), A.double(), log_prior=None if prior is None else prior.double(), counts=counts, transitions=True)
    host32 = metrics.key_posteriors(e, A, log_prior=prior, counts=counts, transitions=True)
    d, h = errors(got, want), errors(host32, want)
    print(f"posteriors W={W} prior={with_prior}: device post {d[0]:.2e} loglik {d[1]:.2e} xi {d[2]:.2e} | "
          f"float32 host post {h[0]:.2e} loglik {h[1]:.2e} xi {h[2]:.2e}")
    check_invariants(got[0], got[1], got[2], counts, W)
    assert got[0].dtype == torch.float32 and got[3] is None
    assert d[0] <= TOL_POST and d[1] <= TOL_LOGLIK and d[2] <= TOL_XI


def test_path_posterior_null_counts_and_determinism():
    W, counts = 70, [70, 41, 1, 0]
    e, _ = net_like_emissions(4, W, 77)
    A = default_trans(1.0)
    path = device_viterbi(e, A, counts)
    assert bool((path[1, 41:] == -1).all())
    post, loglik, xi, pp = device_posteriors(e, A, counts, path=path)
    gathered = torch.where(path >= 0, post.gather(2, path.clamp_min(0).long()[..., None])[..., 0], torch.zeros_like(pp))
    assert torch.equal(pp, gathered) and bool((pp[path < 0] == 0).all()) and bool((pp[path >= 0] > 0).all())
    again = device_posteriors(e, A, counts, path=path, poison=False)                            # a second run, another workspace content
    for x, y in zip((post, loglik, xi, pp), again):
        assert torch.equal(x, y)
    # without the transition sums and the path, post and loglik are the same bits
    p2, l2, x2, pp2 = device_posteriors(e, A, counts, xi=False)
    assert x2 is None and pp2 is None and torch.equal(p2, post) and torch.equal(l2, loglik)
    full, null = device_posteriors(e, A, [W] * 4, path=path.clamp_min(0)), device_posteriors(e, A, None, path=path.clamp_min(0))
    for x, y in zip(full, null):
        assert torch.equal(x, y)
    clamped = device_posteriors(e, A, [99, W, W, W + 1], path=path.clamp_min(0))                  # counts beyond the tensor are clamped to it
    for x, y in zip(full, clamped):
        assert torch.equal(x, y)


def test_errors_of_the_entry_point():
    L = _lib.lib()
    e = torch.zeros((2, 5, 24), device=DEV)
    A = default_trans().to(DEV)
    post, ll, pp = torch.empty((2, 5, 24), device=DEV), torch.empty(2, device=DEV), torch.empty((2, 5), device=DEV)
    nbytes = L.ake_key_posteriors_workspace_bytes(2, 5)
    assert nbytes > 0 and L.ake_key_posteriors_workspace_bytes(0, 5) == 0 and L.ake_key_posteriors_workspace_bytes(2, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    call = lambda path, pp_, ws_bytes: L.ake_key_posteriors_f32(e.data_ptr(), 2, 5, None, A.data_ptr(), None, path, post.data_ptr(),      # noqa: E731
                                                                ll.data_ptr(), None, pp_, ws.data_ptr(), ws_bytes, None)
    assert call(None, pp.data_ptr(), nbytes) == -1                                                # AKE_ERR_INVALID: path_post without path
    assert call(None, None, nbytes - 1) == -4                                                     # AKE_ERR_WORKSPACE
    assert call(None, None, nbytes) == 0
    torch.cuda.synchronize()


def argmax_where_clear(post, want_post, counts):
    """The device argmax equals the model's wherever the model's top two posteriors differ by more than 1e-3."""
    top = want_post.topk(2, dim=2).values
    live = torch.arange(post.shape[1])[None, :] < torch.tensor(counts)[:, None]
    clear = live & (top[..., 0] - top[..., 1] > 1e-3)
    assert int(clear.sum()) > 0
    assert torch.equal(post.argmax(dim=2)[clear], want_post.argmax(dim=2)[clear])
    return int(clear.sum()), int(live.sum())


def test_extreme_emissions():
    """Key rows of exact 0s and 1s and 30 * randn tonic logits: emissions down to about -236.  Held to the measured bounds as well."""
    W, counts = 40, [40, 37, 1, 0]
    e, _ = net_like_emissions(4, W, 91, tonic_scale=30.0, saturated=True)
    assert float(e.min()) < -200
    A = default_trans()
    got = device_posteriors(e, A, counts)
    want = metrics.key_posteriors(e.double(), A.double(), counts=counts, transitions=True)
    d = errors(got, want)
    print(f"extreme emissions (min {float(e.min()):.1f}): device post {d[0]:.2e} loglik {d[1]:.2e} xi {d[2]:.2e}; "
          f"clear windows {argmax_where_clear(got[0], want[0], counts)}")
    check_invariants(got[0], got[1], got[2], counts, W)
    assert d[0] <= TOL_POST and d[1] <= TOL_LOGLIK and d[2] <= TOL_XI


def test_forbidden_transitions():
    """A matrix of two bands, minor to minor and major to major, with -1e4 off them, and emissions that force a change of mode: the
    planted path changes mode once, and every key of the other mode scores 1000 lower in each window, so staying costs more than the
    forbidden move.  At magnitude 1e4 one float32 ulp is 1e-3, so no measured bound applies: finite, normalised, and the model's argmax
    wherever it is clear."""
    W, counts = 40, [40, 23]
    k = torch.arange(24)
    same_mode = (k[:, None] // 12) == (k[None, :] // 12)
    A = torch.where(same_mode, default_trans(), torch.full((24, 24), -1e4))
    g = torch.Generator().manual_seed(92)
    planted = torch.zeros((2, W), dtype=torch.int64)
    planted[0, :15], planted[0, 15:] = 3, 17                                                    # minor -> major: forbidden
    planted[1, :10], planted[1, 10:] = 20, 8
    e = torch.randn((2, W, 24), generator=g)
    e.scatter_add_(2, planted[..., None], torch.full((2, W, 1), 30.0))
    e = e - 1000.0 * ((k[None, None, :] // 12) != (planted[..., None] // 12)).float()
    got = device_posteriors(e, A, counts)
    want = metrics.key_posteriors(e.double(), A.double(), counts=counts, transitions=True)
    check_invariants(got[0], got[1], got[2], counts, W)
    print(f"forbidden transitions: loglik device {got[1].tolist()} model {want[1].tolist()}; clear windows "
          f"{argmax_where_clear(got[0], want[0], counts)}")
    assert torch.equal(want[0].argmax(dim=2)[0], planted[0]) and torch.equal(want[0].argmax(dim=2)[1, :23], planted[1, :23])
    assert bool((want[2].sum(dim=0) * ~same_mode).sum() > 1.99)                                 # (both recordings made the forbidden move)


def test_posteriors_agree_with_viterbi_on_a_clear_path():
    W = 120
    g = torch.Generator().manual_seed(93)
    A = default_trans()
    planted = torch.zeros((3, W), dtype=torch.int64)
    for r in range(3):
        cur = int(torch.randint(0, 24, (1,), generator=g))
        for w in range(W):
            if w and float(torch.rand(1, generator=g)) < 0.1:
                cur = int(torch.randint(0, 24, (1,), generator=g))
            planted[r, w] = cur
    e = torch.randn((3, W, 24), generator=g)
    e.scatter_add_(2, planted[..., None], torch.full((3, W, 1), 30.0))
    path = device_viterbi(e, A)
    post, _, _, pp = device_posteriors(e, A, path=path)
    assert torch.equal(path.long(), planted) and torch.equal(post.argmax(dim=2), planted)
    assert float(pp.min()) > 0.999


# ---- end to end: KeyEstimator.track(smooth=True, posteriors=True) ----

@pytest.fixture(scope="module")
def net(gold_default):
    opt = Namespace(**json.loads(str(gold_default["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold_default), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def est(net):
    return ake_amd.KeyEstimator(net, 22050, 5)


@pytest.fixture(scope="module")
def audio():
    """3 recordings of 45 s whose key changes: three 15 s clips of different keys each, concatenated."""
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7), (3, 8, 4))]
    a = np.stack(rows).astype(np.float32)
    assert a.shape == (3, N45)
    return torch.from_numpy(a).to(DEV)


LENS = [N45, 500000, 22050 * 10]     # the ragged batch: 31, 8 and 0 windows at a 1 s stride


def tracks(est, audio, posteriors, **kw):
    out = [est.track(audio, stride_seconds=5.0, smooth=True, posteriors=posteriors, **kw),
           est.track(audio, stride_seconds=1.0, smooth=True, posteriors=posteriors, **kw),
           est.track(audio, lengths=torch.tensor(LENS), stride_seconds=1.0, smooth=True, posteriors=posteriors, **kw)]
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def with_posteriors(est, audio):
    return tracks(est, audio, True)


def test_track_posteriors_equal_the_stand_alone_call(est, audio, with_posteriors):
    plain = tracks(est, audio, False)
    for tr, off, stride in zip(with_posteriors, plain, (5.0, 1.0, 1.0)):
        R, W = tr.key_id.shape
        assert off.posteriors is None and off.smooth_confidence is None and off.log_likelihood is None and len(off._tensors()) == 10
        assert len(tr._tensors()) == 13
        for x, y in zip(tr._tensors()[:10], off._tensors()):                                     # nothing else of the track changes
            assert (x is None and y is None) or torch.equal(x, y)
        assert tr.posteriors.shape == (R, W, 24) and tr.smooth_confidence.shape == (R, W) and tr.log_likelihood.shape == (R,)
        A = metrics.key_transition_log(stay=math.exp(-tr.stride_seconds / 60.0)).float()
        assert tr.stride_seconds == pytest.approx(stride)
        counts = tr.counts.cpu().tolist()
        post, loglik, _, pp = device_posteriors(tr.emissions.cpu(), A, counts, path=tr.smooth_key_id.cpu(), xi=False)
        assert torch.equal(tr.posteriors.cpu(), post) and torch.equal(tr.log_likelihood.cpu(), loglik) and torch.equal(tr.smooth_confidence.cpu(), pp)
        check_invariants(post, loglik, None, counts, W)
        for r in range(R):
            four, five = tr.segments(r), tr.segments(r, confidence=True)
            assert four == off.segments(r) and [s[:4] for s in five] == four and all(len(s) == 5 and 0.0 < s[4] <= 1.0 + 1e-6 for s in five)
        with pytest.raises(ValueError, match="posteriors"):
            off.segments(0, confidence=True)
    assert with_posteriors[2].counts.tolist() == [31, 8, 0] and with_posteriors[2].segments(2, confidence=True) == []
    # every recording shorter than one window: empty posteriors, a log-likelihood of 0
    empty = est.track(audio[:, :22050 * 10], smooth=True, posteriors=True)
    assert empty.posteriors.shape == (3, 0, 24) and empty.smooth_confidence.shape == (3, 0) and empty.log_likelihood.tolist() == [0.0] * 3
    with pytest.raises(ValueError, match="smooth=True"):
        est.track(audio, posteriors=True)


def test_segment_confidence_is_the_mean_of_the_path_posterior(with_posteriors):
    tr = with_posteriors[1]
    conf, ids = tr.smooth_confidence[0].cpu().double(), tr.smooth_key_id[0].tolist()
    a = 0
    for seg in tr.segments(0, confidence=True):
        b = a
        while b + 1 < len(ids) and ids[b + 1] == ids[a]:
            b += 1
        assert seg[2] == ids[a] and seg[4] == pytest.approx(float(conf[a:b + 1].mean()), abs=1e-6)
        a = b + 1
    assert a == len(ids)


def test_two_streams_give_the_same_track(net, est, audio, with_posteriors):
    est2 = ake_amd.KeyEstimator(net, 22050, 5, streams=2)
    got = tracks(est2, audio, True)
    est2.join()
    torch.cuda.synchronize()
    for a, b in zip(got, with_posteriors):
        assert a.posteriors is not None and len(a._tensors()) == 13
        for x, y in zip(a._tensors(), b._tensors()):
            assert torch.equal(x, y)
    assert est2._slots[0]["stream"] is not None and est2._slots[1]["stream"] is not None


def test_posteriors_false_launches_nothing_new(est, audio):
    new = ("key_forward_backward_kernel", "key_posteriors_kernel", "key_xi_reduce_kernel")
    _lib.prof_results()
    _lib.prof_enable("", True)
    try:
        est.track(audio, stride_seconds=1.0, smooth=True)
        off = _lib.prof_results()
        est.track(audio, stride_seconds=1.0, smooth=True, posteriors=True)
        on = _lib.prof_results()
    finally:
        _lib.prof_enable("", False)
    assert "viterbi_keys_kernel" in off and not any(k in off for k in new)
    assert on["key_forward_backward_kernel"][1] == 1 and on["key_posteriors_kernel"][1] == 1 and "key_xi_reduce_kernel" not in on
    assert {k: v[1] for k, v in on.items() if k not in new} == {k: v[1] for k, v in off.items()}


def test_device_em_equals_the_host_fit():
    """R = 8, W = 64 (ragged), 3 iterations, tied.  The fitted transition PROBABILITIES are compared: a fitted row is C / rowsum(C) with
    C the summed xi_sum plus the pseudo-counts, so an error d in a cell of the summed xi_sum moves a probability by about d / rowsum(C)
    (a row holds about 8 * 63 / 24 = 21 transitions here) -- the bound is the measured one (module docstring).  The float64 score of
    each iteration's device matrix does not fall."""
    counts = [64, 64, 50, 64, 33, 64, 2, 64]
    e, _ = net_like_emissions(8, 64, 95)
    e = e * (torch.arange(64)[None, :] < torch.tensor(counts)[:, None])[..., None]
    ids = torch.zeros((8, 64), dtype=torch.int32)
    tr = ake_amd.KeyTrack(None, None, None, ids, ids, ids, None, torch.tensor(counts, dtype=torch.int32, device=DEV), torch.zeros(64),
                          emissions=e.to(DEV), smooth_key_id=ids)
    init = metrics.key_transition_log(stay=0.9)
    dev = [ake_amd.fit_key_transition(tr, iterations=k) for k in (1, 2, 3)]
    A_host, s_host = metrics.fit_key_transition(e.double(), counts=counts, iterations=3)
    A_dev, s_dev = dev[2]
    assert A_dev.dtype == torch.float64 and A_dev.shape == (24, 24) and len(s_dev) == 3
    assert torch.equal(dev[0][0], ake_amd.fit_key_transition([tr], iterations=1)[0])             # deterministic, and a list of one
    assert s_dev[:2] == dev[1][1] and s_dev[:1] == dev[0][1]
    dP = float((torch.exp(A_dev) - torch.exp(A_host)).abs().max())
    dS = max(abs(a - b) / abs(b) for a, b in zip(s_dev, s_host))
    print(f"device EM: largest |P_dev - P_host| {dP:.2e}, largest relative score difference {dS:.2e}")
    assert dP <= TOL_EM_P and dS <= TOL_LOGLIK
    score = lambda A: float(metrics.key_posteriors(e.double(), A, counts=counts)[1].sum())      # noqa: E731
    scores = [score(init)] + [score(A) for A, _ in dev]
    print(f"float64 scores of the device's matrices: {scores}")
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(scores, scores[1:])) and scores[-1] > scores[0]
    with pytest.raises(ValueError, match="smooth"):
        ake_amd.fit_key_transition(ake_amd.KeyTrack(None, None, None, ids, ids, ids, None, tr.counts, torch.zeros(64)))
