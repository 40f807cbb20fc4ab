"""GPU: fixed-lag key posteriors and the running log-likelihood of a stream -- ake_key_stream_posteriors_f32 against
metrics.key_stream_posteriors, and KeyEstimator.stream(posteriors=True) end to end.

The bound, in the form test_gpu_stream.py uses for `filtered`, from the models alone: with X_32 / X_64 the host model in float32 /
float64 on the CPU on the same float32 inputs,

    |X_kernel - X_64| <= max(4 * max|X_32 - X_64|, 2^-20 * max|X_64 row|)

the float32 model's error taken over the tensor, the floor per row: a window's 24 probabilities for `post` (two float32 ulps of the
row's largest), a single running sum for `loglik` (against its own magnitude).  `path_post` is a gather of `post`, to the bit.

The audio of the end-to-end tests is test_gpu_stream.py's: two 45 s recordings, 31 windows at a 1 s stride, the trained fixture net."""
import ctypes as C
import functools
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict, load_golden
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
N45 = 992250
LAGS = (0, 1, 6, 30, 255)
IRREGULAR = (1, 4409, 4410, 4411, 0, 22050, 100000)
KERNELS = {"key_stream_sweep_kernel", "key_stream_loglik_kernel"}


# ---- the entry alone -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_inputs(kind, R, W):
    """`gauss`: Gaussian emissions; `deep`: the same with one window of every recording saturated at -256, a forbidden transition in
    every row of A and a prior."""
    g = torch.Generator().manual_seed(1000 * R + W + len(kind))
    e = torch.randn((R, W, 24), generator=g) * 3
    A = metrics.key_transition_log(0.9).float()
    prior = None
    if kind == "deep":
        for r in range(R):
            e[r, (W // 2 + 5 * r) % W] = -256.0
        A = A.clone()
        A[torch.arange(24), (torch.arange(24) + 6) % 24] = -1e4
        prior = torch.randn(24, generator=g)
    return e, A, prior


@functools.lru_cache(maxsize=None)
def host_models(kind, R, W, lag):
    """(post, loglik) of the float32 and of the float64 host model, computed once and left unchanged."""
    e, A, prior = case_inputs(kind, R, W)
    m32 = metrics.key_stream_posteriors(e, A, prior, lag=lag)
    m64 = metrics.key_stream_posteriors(e.double(), A.double(), None if prior is None else prior.double(), lag=lag)
    return m32, m64


def row_ratio(got, f32, f64):
    """worst |got - f64| / bound over the rows of (..., 24), with the module docstring's bound."""
    host = float((f32.double() - f64).abs().max())
    bound = torch.clamp(f64.abs().amax(dim=-1) * 2.0 ** -20, min=4 * host)
    return float(((got.double() - f64).abs().amax(dim=-1) / bound).max()) if got.numel() else 0.0


def scalar_ratio(got, f32, f64):
    """the same for a tensor of scalars: every element is its own row."""
    return row_ratio(got[..., None], f32[..., None], f64[..., None])


def device_run(e, A, prior, lag, pieces, fill, outputs=(True, True)):
    """The step entry and, right behind it, ake_key_stream_posteriors_f32 over (R, W, 24) float32 emissions cut into `pieces` (the last
    one flushes) -> (post, path_post, loglik, path, state bytes) on the CPU.  The new state and the new outputs sit in guarded buffers;
    `outputs`: whether path_post / loglik are asked for."""
    L = _lib.lib()
    R, W, _ = e.shape
    stream = torch.cuda.current_stream().cuda_stream
    A_d = A.to(DEV).contiguous()
    prior_d = None if prior is None else prior.to(DEV).contiguous()
    p_d = None if prior is None else prior_d.data_ptr()
    step_state = torch.empty(max(L.ake_key_stream_state_bytes(R, lag), 16), dtype=torch.uint8, device=DEV)
    nbytes = L.ake_key_stream_posteriors_state_bytes(R, lag)
    assert nbytes == R * (16 + 2 * max(lag, 1) * 96)
    state, state_check = guarded(nbytes, fill)
    posts, pps, lls, paths, at = [], [], [], [], 0
    for i, k in enumerate(pieces):
        flush = i == len(pieces) - 1
        _, k2 = metrics.key_stream_count(at, k, lag, flush)
        e_d = e[:, at:at + k].to(DEV).contiguous()
        f_d, path = torch.empty((R, k, 24), device=DEV), torch.empty((R, k2), dtype=torch.int32, device=DEV)
        k_out = C.c_int(-7)
        _lib.check(L.ake_key_stream_step_f32(e_d.data_ptr() if k else None, R, k, at, lag, int(flush), A_d.data_ptr(), p_d, step_state.data_ptr(),
                                             step_state.numel(), f_d.data_ptr() if k else None, path.data_ptr() if k2 else None, C.byref(k_out),
                                             stream), "ake_key_stream_step_f32")
        assert k_out.value == k2
        post, pp, ll = GuardedTensor((R, k2, 24)), GuardedTensor((R, k2)), GuardedTensor((R, k))
        k_out = C.c_int(-7)
        _lib.check(L.ake_key_stream_posteriors_f32(e_d.data_ptr() if k else None, f_d.data_ptr() if k else None, R, k, at, lag, int(flush),
                                                   A_d.data_ptr(), p_d, path.data_ptr() if k2 and outputs[0] else None, state.data_ptr(),
                                                   state.numel(), post.t.data_ptr() if k2 else None,
                                                   pp.t.data_ptr() if k2 and outputs[0] else None,
                                                   ll.t.data_ptr() if k and outputs[1] else None, C.byref(k_out), stream),
                   "ake_key_stream_posteriors_f32")
        assert k_out.value == k2
        post.check("post"); pp.check("path_post"); ll.check("loglik"); state_check("state")
        posts.append(post.t.cpu()); pps.append(pp.t.cpu()); lls.append(ll.t.cpu()); paths.append(path.cpu())
        at += k
    assert at == W
    return torch.cat(posts, dim=1), torch.cat(pps, dim=1), torch.cat(lls, dim=1), torch.cat(paths, dim=1), state.cpu().clone()


def chunkings(W):
    """one window at a time; 7 + 33 + the rest, ending on k = 0 with the flush; all at once"""
    second = [7, 33] + ([W - 40] if W > 40 else []) if W >= 40 else [W]
    return [[1] * W, second + [0], [W]]


@pytest.mark.parametrize("kind", ["gauss", "deep"])
@pytest.mark.parametrize("W", [1, 2, 17, 300])
@pytest.mark.parametrize("R", [1, 3])
def test_entry_against_the_float64_model_and_every_cut_to_the_bit(R, W, kind):
    """(a) and (b), with (d)'s guards: three schedules under three fill bytes of the fresh state and of the outputs."""
    e, A, prior = case_inputs(kind, R, W)
    worst_post = worst_ll = 0.0
    for n, lag in enumerate(LAGS):
        (p32, l32), (p64, l64) = host_models(kind, R, W, lag)
        runs = [device_run(e, A, prior, lag, pieces, fill) for pieces, fill in zip(chunkings(W), (0x00, 0xFF, 0x77))]
        if n == 0:
            runs.append(device_run(e, A, prior, lag, [W], 0x77))                    # a rerun
        post, pp, ll, path, state = runs[0]
        assert post.shape == (R, W, 24) and ll.shape == (R, W) and pp.shape == (R, W)
        assert bool(torch.isfinite(post).all()) and bool(torch.isfinite(ll).all())
        for other in runs[1:]:                                                      # every schedule, a fresh state of any bytes: bit for bit
            for name, x, y in zip(("post", "path_post", "loglik", "path", "state"), other, runs[0]):
                assert torch.equal(x, y), (lag, name)
        assert torch.equal(pp, post.gather(2, path.long()[..., None])[..., 0]), lag
        assert float((post.double().sum(dim=2) - 1).abs().max()) <= 1e-5
        a, b = row_ratio(post, p32, p64), scalar_ratio(ll, l32, l64)
        print(f"\n  STREAM posteriors R {R} W {W} {kind} lag {lag} | error / bound: post {a:.3f} loglik {b:.3f}")
        worst_post, worst_ll = max(worst_post, a), max(worst_ll, b)
    assert worst_post <= 1.0 and worst_ll <= 1.0, (worst_post, worst_ll)


def test_null_optional_outputs_are_accepted():
    e, A, prior = case_inputs("deep", 3, 17)
    full = device_run(e, A, prior, 6, [5, 12], 0x77)
    for outputs in ((False, True), (True, False), (False, False)):
        got = device_run(e, A, prior, 6, [5, 12], 0x77, outputs)                     # (an output not asked for keeps its 0xFF fill)
        assert torch.equal(got[0], full[0]) and torch.equal(got[4], full[4])
        assert torch.equal(got[1], full[1]) if outputs[0] else bool(torch.isnan(got[1]).all())
        assert torch.equal(got[2], full[2]) if outputs[1] else bool(torch.isnan(got[2]).all())


@pytest.mark.parametrize("lag", [30, 255])
def test_a_lag_of_the_whole_recording_is_the_offline_posteriors(lag):
    """(c): 17 windows, a planted key path with two changes and a clear margin."""
    R, W = 2, 17
    g = torch.Generator().manual_seed(lag)
    e = torch.randn((R, W, 24), generator=g)
    planted = torch.tensor([[3] * 6 + [10] * 5 + [15] * 6, [20] * 4 + [8] * 9 + [1] * 4])
    e.scatter_add_(2, planted[..., None], torch.full((R, W, 1), 12.0))
    A = metrics.key_transition_log(0.9).float()
    post, _, _, path, _ = device_run(e, A, None, lag, [4, 0, 13], 0x77)
    f64 = metrics.key_posteriors(e.double(), A.double())[0]
    f32 = metrics.key_stream_posteriors(e, A, lag=lag)[0]
    ratio = row_ratio(post, f32, f64)
    print(f"\n  STREAM posteriors lag {lag} >= W | against key_posteriors in float64: error / bound {ratio:.3f}")
    assert ratio <= 1.0
    vit = metrics.viterbi_keys(e, A)
    assert torch.equal(vit.long(), planted) and torch.equal(path, vit) and torch.equal(post.argmax(dim=2), vit.long())


def test_entry_errors_launch_nothing():
    L = _lib.lib()
    R, k, lag = 2, 5, 3
    e, f = torch.zeros((R, k, 24), device=DEV), torch.zeros((R, k, 24), device=DEV)
    A = metrics.key_transition_log(0.9).float().to(DEV)
    nbytes = L.ake_key_stream_posteriors_state_bytes(R, lag)
    state = torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)
    post, pp, ll = torch.empty((R, k, 24), device=DEV), torch.empty((R, k), device=DEV), torch.empty((R, k), device=DEV)
    path = torch.zeros((R, k), dtype=torch.int32, device=DEV)
    k_out = C.c_int(0)
    stream = torch.cuda.current_stream().cuda_stream

    def call(emis=e.data_ptr(), filt=f.data_ptr(), R=R, k=k, before=0, lag=lag, trans=A.data_ptr(), path=path.data_ptr(), st=state.data_ptr(),
             st_bytes=nbytes, post=post.data_ptr(), pp=pp.data_ptr(), out=C.byref(k_out), flush=1):
        return L.ake_key_stream_posteriors_f32(emis, filt, R, k, before, lag, flush, trans, None, path, st, st_bytes, post, pp, ll.data_ptr(), out,
                                               stream)

    _lib.prof_enable("", True)
    try:
        assert call(st_bytes=nbytes - 1) == -4                                       # AKE_ERR_WORKSPACE
        assert b"state" in L.ake_last_error()
        for bad in (dict(lag=-1), dict(lag=256), dict(k=-1), dict(R=0), dict(before=-1), dict(trans=None), dict(st=None), dict(out=None),
                    dict(emis=None), dict(filt=None), dict(post=None), dict(path=None), dict(st=state.data_ptr() + 4)):
            assert call(**bad) == -1, bad                                            # AKE_ERR_INVALID (path=None: path_post without its path)
        assert call(k=0, emis=None, filt=None, post=None, path=None, pp=None, flush=0) == 0 and k_out.value == 0    # nothing to do: no launch
        assert call(k=0, emis=None, filt=None, post=None, path=None, pp=None, flush=1) == 0 and k_out.value == 0    # a flush of nothing
        torch.cuda.synchronize()
        assert not set(_lib.prof_results()) & KERNELS
        assert call() == 0 and k_out.value == k
        assert call(path=None, pp=None) == 0
        torch.cuda.synchronize()
        names = _lib.prof_results()
        assert names["key_stream_sweep_kernel"][1] == 2 and names["key_stream_loglik_kernel"][1] == 2
        assert call(k=2, before=5, flush=0) == 0 and k_out.value == 2               # lag 3, windows 5 and 6 stepped: 2 and 3 leave the lag
        assert call(k=0, before=7, emis=None, filt=None, flush=1) == 0 and k_out.value == 3     # a flush alone: sweeps, no state update
        torch.cuda.synchronize()
        names = _lib.prof_results()
        assert names["key_stream_sweep_kernel"][1] == 2 and names["key_stream_loglik_kernel"][1] == 1
    finally:
        _lib.prof_enable("", False)
    assert L.ake_key_stream_posteriors_state_bytes(0, 3) == 0 and L.ake_key_stream_posteriors_state_bytes(1, 256) == 0
    assert L.ake_key_stream_posteriors_state_bytes(1, -1) == 0 and L.ake_key_stream_posteriors_state_bytes(2, 0) == 2 * (16 + 192)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------

def schedule_irregular(n=N45):
    out, left = list(IRREGULAR), n - sum(IRREGULAR)
    while left > 0:
        out.append(min(SR, left))
        left -= out[-1]
    assert sum(out) == n
    return out


@pytest.fixture(scope="module")
def est():
    gold = load_golden("pcnet_trained.npz")
    opt = Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return ake_amd.KeyEstimator(net.to(DEV).eval(), SR, 5)


@pytest.fixture(scope="module")
def recordings():
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7))]
    audio = torch.from_numpy(np.stack(rows).astype(np.float32))
    assert audio.shape == (2, N45)
    return audio


def run_streams(est, audio, schedule, streams):
    """Push `audio` (R, n) in the chunks of `schedule` into every stream of `streams` in turn, then finish -> a list of updates each."""
    src, at, ups = audio.to(DEV), 0, [[] for _ in streams]
    for m in schedule:
        for s, u in zip(streams, ups):
            u.append(s.push(src[:, at:at + m]))
        at += m
    assert at == audio.shape[1]
    for s, u in zip(streams, ups):
        u.append(s.finish())
    torch.cuda.synchronize()
    return ups


def joined(ups, name):
    return torch.cat([getattr(u, name) for u in ups], dim=1)


def check_stream(s, ups, W, lag, prior=None):
    """(e): the stream's joined posteriors / smooth_confidence / log_likelihood against the entry alone on the stream's own joined
    emissions and filtered (to the bit), against the float64 model and key_posteriors on every prefix (the bound), and the gather."""
    L = _lib.lib()
    emis, filt, path = joined(ups, "emissions").contiguous(), joined(ups, "filtered").contiguous(), joined(ups, "smooth_key_id").contiguous()
    post, conf, ll = joined(ups, "posteriors"), joined(ups, "smooth_confidence"), joined(ups, "log_likelihood")
    R = emis.shape[0]
    assert emis.shape == (R, W, 24) and post.shape == (R, W, 24) and conf.shape == (R, W) and ll.shape == (R, W)
    for u in ups:
        assert u.posteriors.shape[1] == u.smooth_confidence.shape[1] == u.smooth_key_id.shape[1] and u.log_likelihood.shape[1] == u.windows
    alone = [torch.empty_like(post), torch.empty_like(conf), torch.empty_like(ll)]
    state = torch.empty(L.ake_key_stream_posteriors_state_bytes(R, lag), dtype=torch.uint8, device=DEV)
    prior_d = None if prior is None else prior.to(DEV).float().contiguous()
    k_out = C.c_int(-1)
    _lib.check(L.ake_key_stream_posteriors_f32(emis.data_ptr(), filt.data_ptr(), R, W, 0, lag, 1, s.trans.data_ptr(),
                                               None if prior is None else prior_d.data_ptr(), path.data_ptr(),
                                               state.data_ptr(), state.numel(), *(t.data_ptr() for t in alone), C.byref(k_out),
                                               torch.cuda.current_stream().cuda_stream), "ake_key_stream_posteriors_f32")
    torch.cuda.synchronize()
    assert k_out.value == W
    for name, a, b in zip(("posteriors", "smooth_confidence", "log_likelihood"), (post, conf, ll), alone):
        assert torch.equal(a, b), name
    assert torch.equal(conf, post.gather(2, path.long()[..., None])[..., 0])
    e_c, A_c = emis.cpu(), s.trans.cpu()
    p_c = None if prior is None else prior.float().cpu()
    p32, l32 = metrics.key_stream_posteriors(e_c, A_c, p_c, lag=lag)
    p64, l64 = metrics.key_stream_posteriors(e_c.double(), A_c.double(), None if p_c is None else p_c.double(), lag=lag)
    ratios = row_ratio(post.cpu(), p32, p64), scalar_ratio(ll.cpu(), l32, l64)
    assert max(ratios) <= 1.0, ratios
    host = float((p32.double() - p64).abs().max())
    for v in range(W):                                                               # the definition itself, on every prefix
        want, want_ll = metrics.key_posteriors(e_c[:, :min(W, v + lag + 1)].double(), A_c.double(), None if p_c is None else p_c.double())
        bound = torch.clamp(want[:, v].amax(dim=-1) * 2.0 ** -20, min=4 * host)
        assert bool(((post[:, v].cpu().double() - want[:, v]).abs().amax(dim=-1) <= bound).all()), v
    return ratios


@pytest.fixture(scope="module")
def base(est, recordings):
    s = est.stream(2, stride_seconds=1.0, lag_windows=3, posteriors=True)
    return s, run_streams(est, recordings, schedule_irregular(), [s])[0]


def test_end_to_end_posteriors(base):
    s, ups = base
    ratios = check_stream(s, ups, 31, 3)
    print(f"\n  STREAM posteriors end to end | error / bound: post {ratios[0]:.3f} loglik {ratios[1]:.3f}")
    assert any(u.windows and not u.smooth_key_id.shape[1] for u in ups) and ups[-1].smooth_key_id.shape[1] >= 3     # the lag shows


def test_end_to_end_with_a_transition_a_prior_and_int16_chunks(est, recordings, base):
    T = metrics.key_transition_log(0.5).float()
    prior = torch.linspace(-2.0, 1.0, 24)
    pcm = (recordings * 32767).round().to(torch.int16)
    sT = est.stream(2, stride_seconds=1.0, lag_windows=6, transition=T, posteriors=True)
    sP = est.stream(2, stride_seconds=1.0, lag_windows=3, log_prior=prior, posteriors=True)
    sI = est.stream(2, stride_seconds=1.0, lag_windows=3, posteriors=True)
    upsT, upsP = run_streams(est, recordings, schedule_irregular(), [sT, sP])        # two streams side by side
    upsI = run_streams(est, pcm, schedule_irregular(), [sI])[0]
    check_stream(sT, upsT, 31, 6)
    check_stream(sP, upsP, 31, 3, prior)
    check_stream(sI, upsI, 31, 3)
    assert not torch.equal(joined(upsP, "posteriors"), joined(base[1], "posteriors"))     # the prior and the transition reach the kernel
    assert not torch.equal(joined(upsT, "log_likelihood"), joined(base[1], "log_likelihood"))


def test_two_streams_side_by_side_equal_each_alone(est, recordings, base):
    a = est.stream(2, stride_seconds=1.0, lag_windows=3, posteriors=True)
    b = est.stream(2, stride_seconds=1.0, lag_windows=12, posteriors=True)
    ups_a, ups_b = run_streams(est, recordings, schedule_irregular(), [a, b])
    for name in ("posteriors", "smooth_confidence", "log_likelihood", "smooth_key_id", "filtered"):
        assert torch.equal(joined(ups_a, name), joined(base[1], name)), name
    check_stream(b, ups_b, 31, 12)


def test_launch_sets(est, recordings):
    """(f): without `posteriors` a stream launches what it launched before and leaves the three fields None."""
    short = recordings[:, :30 * SR]
    names = {}
    for posteriors in (False, True):
        _lib.prof_enable("", True)
        try:
            s = est.stream(2, posteriors=posteriors)
            ups = run_streams(est, short, [10 * SR] * 3, [s])[0]
            names[posteriors] = set(_lib.prof_results())
        finally:
            _lib.prof_enable("", False)
        for u in ups:
            for n in ("posteriors", "smooth_confidence", "log_likelihood"):
                assert (getattr(u, n) is not None) == posteriors
    assert not names[False] & KERNELS and {"key_stream_step_kernel", "key_emissions_kernel"} <= names[False]
    assert names[True] - names[False] == KERNELS and names[False] <= names[True]
    with pytest.raises(ValueError):
        est.stream(2, smooth=False, posteriors=True)
