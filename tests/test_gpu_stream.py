"""GPU: key tracking on audio as it arrives -- KeyEstimator.stream / KeyStream, the support query ake_cqt_plan_half_support and the
smoother with carried state ake_key_stream_step_f32 against metrics.key_stream.

The audio is test_gpu_track.py's two 45 s recordings (226 frames; 7 windows at 5 s stride, (226 - 76) // 5 + 1 = 31 at 1 s), the net the trained fixture
(tests/golden/pcnet_trained.npz), whose outputs respond to the input.

The bound on `filtered`, in the form test_gpu_sequence_loss.py uses, from the models alone: with X_32 / X_64 metrics.key_stream in float32
/ float64 on the CPU on the same float32 inputs,

    |X_kernel - X_64| <= max(4 * max|X_32 - X_64|, 2^-20 * max|X_64 row|)

the float32 model's error taken over the tensor, the floor per window row (two float32 ulps of the row's largest magnitude).  `path` is
bit-identical to the float32 host model: the Viterbi step is additions, subtractions and comparisons only."""
import ctypes as C
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict, load_golden, rel_err
from oracle import cqt_oracle, pcnet_oracle
from sensitive import MIN_RESPONSE
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, HOP, WF = 22050, 4410, 76
N45 = 992250
LAGS = (0, 1, 3, 12, 255)
BUDGET = 1e-3                        # the project's end-to-end budget
IRREGULAR = (1, 4409, 4410, 4411, 0, 22050, 100000)


def schedule_irregular(n=N45):
    out, left = list(IRREGULAR), n - sum(IRREGULAR)
    while left > 0:
        out.append(min(SR, left))
        left -= out[-1]
    assert sum(out) == n
    return out


@pytest.fixture(scope="module")
def weights():
    gold = load_golden("pcnet_trained.npz")
    sd32 = golden_state_dict(gold)
    return sd32, pcnet_oracle.to_dtype(sd32, torch.float64), Namespace(**json.loads(str(gold["opt"])))


@pytest.fixture(scope="module")
def est(weights):
    sd32, _, opt = weights
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(sd32, strict=True)
    return ake_amd.KeyEstimator(net.to(DEV).eval(), SR, 5)


@pytest.fixture(scope="module")
def recordings():
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7))]
    audio = torch.from_numpy(np.stack(rows).astype(np.float32))
    assert audio.shape == (2, N45)
    return audio


@pytest.fixture(scope="module")
def oracle_frames(recordings):
    return cqt_oracle.FastDirectCQT(SR, HOP, dtype=torch.float64)(recordings.numpy())


def run_stream(est, audio, schedule, **kw):
    """Push `audio` (R, n) in the chunks of `schedule`, then finish -> (stream, updates)."""
    s = est.stream(audio.shape[0], **kw)
    src, at, ups = audio.to(DEV), 0, []
    for m in schedule:
        ups.append(s.push(src[:, at:at + m]))
        at += m
    assert at == audio.shape[1]
    ups.append(s.finish())
    torch.cuda.synchronize()
    return s, ups


def joined(ups, name):
    return torch.cat([getattr(u, name) for u in ups], dim=1)


def check_window_order(ups, W):
    at = 0
    for u in ups:
        assert u.first_window == at and u.key.shape[1] == u.windows == u.key_id.shape[1] == len(u.times)
        at += u.windows
    assert at == W


@pytest.fixture(scope="module")
def streamed(est, recordings):
    """The irregular schedule at both strides, frames kept, lag 3: shared by the tests below and left unchanged."""
    return {stride: run_stream(est, recordings, schedule_irregular(), stride_seconds=stride, lag_windows=3, keep_frames=True)
            for stride in (5.0, 1.0)}


# ---- 1. the support ------------------------------------------------------------------------------------------------------------------------

def test_half_support_bounds_what_a_frame_depends_on(est):
    L = _lib.lib()
    plan = est.plan
    H = int(L.ake_cqt_plan_half_support(plan.handle))
    print(f"\n  STREAM half support H = {H} samples = {H / HOP:.3f} hops = {H / SR:.3f} s")
    assert 0 < H <= 6 * HOP
    assert L.ake_cqt_plan_half_support(None) == -1
    n = 30 * HOP
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((1, n), generator=g) - 0.5).to(DEV)
    other = (torch.rand((1, n), generator=g) - 0.5).to(DEV)
    fx = plan.logmag(x)
    t = torch.arange(fx.shape[2], device=DEV) * HOP
    for s in (15 * HOP, 15 * HOP + 1234, 12 * HOP - 777):                            # the first on a frame centre
        behind = x.clone()
        behind[:, s:] = other[:, s:]
        fb = plan.logmag(behind)
        same = t + H < s                                                             # frames whose support ends in front of s
        assert int(same.sum()) >= 5 and torch.equal(fb[:, :, same], fx[:, :, same]), s
        near = (t - s).abs() <= H
        assert bool((fb[:, :, near] != fx[:, :, near]).any())                        # not vacuous: a frame within H of s does change
        front = x.clone()
        front[:, :s] = other[:, :s]
        ff = plan.logmag(front)
        same = t - H >= s                                                            # frames whose support begins at or behind s
        assert int(same.sum()) >= 5 and torch.equal(ff[:, :, same], fx[:, :, same]), s
        assert bool((ff[:, :, near] != fx[:, :, near]).any())


# ---- 2. the frames -------------------------------------------------------------------------------------------------------------------------

def test_streamed_frames_against_the_direct_form_oracle(streamed, oracle_frames, est, recordings):
    s, _ = streamed[5.0]
    frames = s.frames
    assert frames.shape == (2, 288, 1 + N45 // HOP) == tuple(oracle_frames.shape)
    e = rel_err(frames, oracle_frames)
    offline = est.plan.logmag(recordings.to(DEV))
    print(f"\n  STREAM frames | against the float64 oracle {e:.2e}; streamed against offline frames (s0 not on the decimation grid) "
          f"{rel_err(frames, offline):.2e}")
    assert e < 5e-4
    assert torch.equal(streamed[1.0][0].frames, frames)                              # the frames do not depend on the windows' stride


def test_int16_stream_equals_the_float_stream_on_the_converted_audio(est, recordings):
    pcm = (recordings * 32767).round().to(torch.int16)
    a, _ = run_stream(est, pcm, schedule_irregular(), smooth=False, keep_frames=True)
    b, _ = run_stream(est, ake_amd.pcm16_to_float(pcm), schedule_irregular(), smooth=False, keep_frames=True)
    assert a.frames.shape == (2, 288, 226) and torch.equal(a.frames, b.frames)


# ---- 3. the windows ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [5.0, 1.0])
def test_windows_against_the_oracle_net_on_the_streams_own_frames(streamed, weights, est, recordings, stride):
    _, sd64, _ = weights
    s, ups = streamed[stride]
    sf = int(round(stride * 5))
    W = (226 - WF) // sf + 1
    check_window_order(ups, W)
    tr = est.track(recordings.to(DEV), stride_seconds=stride)
    assert tr.key.shape[1] == W == (7 if stride == 5.0 else 31)
    got = [joined(ups, n) for n in ("key", "tonic", "genre")]
    win = s.frames.cpu().double().unfold(2, WF, sf).permute(0, 2, 1, 3).reshape(2 * W, 1, 288, WF)
    seq = torch.full((2 * W,), WF)
    with torch.no_grad():
        ref = pcnet_oracle.pcnet_forward(sd64, win, seq)
    with torch.no_grad():                                                            # (a silent window gives the same outputs wherever it lies)
        silent = pcnet_oracle.pcnet_forward(sd64, torch.zeros_like(win[:1]), seq[:1])
    r = [float((a - b).abs().max()) / float(a.abs().max()) for a, b in zip(ref, silent)]      # sensitive.response
    assert min(r) >= MIN_RESPONSE, r
    e = [rel_err(a.reshape(2 * W, -1), b) for a, b in zip(got, ref)]
    print(f"\n  STREAM windows stride {stride} | against the float64 oracle on the stream's frames: " + " ".join(f"{v:.1e}" for v in e)
          + " | against track: " + " ".join(f"{rel_err(a, getattr(tr, n)):.1e}" for a, n in zip(got, ("key", "tonic", "genre"))))
    assert max(e) < BUDGET, e
    key_id, sig, tonic_id, conf = metrics.decode_keys(got[0], got[1])
    for name, want in (("key_id", key_id), ("signature_id", sig), ("tonic_id", tonic_id)):
        assert torch.equal(joined(ups, name).long(), want.long()), name
    assert float((joined(ups, "confidence") - conf).abs().max()) < 1e-5              # (test_gpu_track.py's bound; to the bit: the test below)
    times = torch.cat([u.times for u in ups])
    assert torch.equal(times, tr.times)
    # a second schedule: everything at once
    _, ups2 = run_stream(est, recordings, [N45], stride_seconds=stride, lag_windows=3)
    check_window_order(ups2, W)
    for n, a in zip(("key", "tonic", "genre"), got):
        assert rel_err(joined(ups2, n), a) < BUDGET, n


@pytest.mark.parametrize("stride", [5.0, 1.0])
def test_confidence_equals_the_host_decode_to_the_bit(streamed, stride):
    """The stream's `confidence` torch.equal to metrics.decode_keys on the stream's own key / tonic, on the device and on the CPU.  The
    stream's confidence is ake_decode_keys_f32's; metrics.decode_keys restates that kernel's arithmetic in its own order (the first two
    squares in one fused multiply-add, every other sum in turn, roots and quotients rounded once).  A first build compared against torch
    reductions, which add in another order, and missed by 1.8e-07 (one to three float32 ulps of a cosine near 1)."""
    _, ups = streamed[stride]
    conf = metrics.decode_keys(joined(ups, "key"), joined(ups, "tonic"))[3]
    got = joined(ups, "confidence")
    print(f"\n  STREAM windows stride {stride} | confidence against metrics.decode_keys: max difference {float((got - conf).abs().max()):.1e}")
    assert torch.equal(got, conf)
    assert torch.equal(got.cpu(), metrics.decode_keys(joined(ups, "key").cpu(), joined(ups, "tonic").cpu())[3])
    g = torch.Generator().manual_seed(int(stride))                                   # and on rows that are no net's outputs
    key, tonic = torch.rand((1, 5000, 12), generator=g).to(DEV), torch.randn((1, 5000, 12), generator=g).to(DEV)
    out = [torch.empty((1, 5000), dtype=torch.int32, device=DEV) for _ in range(3)] + [torch.empty((1, 5000), device=DEV)]
    _lib.check(_lib.lib().ake_decode_keys_f32(key.data_ptr(), tonic.data_ptr(), 5000, None, 1, *(t.data_ptr() for t in out),
                                              torch.cuda.current_stream().cuda_stream), "ake_decode_keys_f32")
    for a, b in zip(out, metrics.decode_keys(key, tonic)):
        assert torch.equal(a, b)


def test_a_stride_longer_than_a_window_and_a_long_chunk_in_pieces(est, recordings):
    """20 s stride, 15 s windows: frames between two windows are skipped.  max_chunk_samples = 3 s: the one 45 s chunk goes in 15 pieces."""
    tr = est.track(recordings.to(DEV), stride_seconds=20.0)
    _, ups = run_stream(est, recordings, [N45], stride_seconds=20.0, max_chunk_samples=3 * SR, lag_windows=1)
    assert tr.key.shape[1] == 2
    check_window_order(ups, 2)
    for n in ("key", "tonic", "genre"):
        assert rel_err(joined(ups, n), getattr(tr, n)) < BUDGET, n
    assert joined(ups, "smooth_key_id").shape == (2, 2)


# ---- 4. the smoother entry -----------------------------------------------------------------------------------------------------------------

def case_inputs(kind, R, W, seed):
    g = torch.Generator().manual_seed(seed)
    A = metrics.key_transition_log(0.9).float()
    prior = None
    if kind == "gauss":
        e = torch.randn((R, W, 24), generator=g) * 3
    elif kind == "ties":
        e = torch.randint(-2, 3, (R, W, 24), generator=g).float()
        prior = torch.randint(-1, 2, (24,), generator=g).float()
    else:                                                                            # emissions near -240, forbidden transitions, a prior
        e = torch.randn((R, W, 24), generator=g) * 3 - 240.0
        A = A.clone()
        A[torch.arange(24), (torch.arange(24) + 6) % 24] = -1e4
        prior = torch.randn(24, generator=g)
    return e, A, prior


def device_steps(e, A, prior, lag, pieces, fill):
    """ake_key_stream_step_f32 over (R, W, 24) float32 emissions cut into `pieces` (the last one flushes) -> (filtered, path) on the
    CPU.  The state and every output sit in guarded buffers."""
    L = _lib.lib()
    R, W, _ = e.shape
    A_d = A.to(DEV).contiguous()
    p_d = None if prior is None else prior.to(DEV).contiguous()
    nbytes = L.ake_key_stream_state_bytes(R, lag)
    assert nbytes == R * (192 + (24 * lag + 15) // 16 * 16)
    state, state_check = guarded(nbytes, fill)
    fs, ps, at = [], [], 0
    for i, k in enumerate(pieces):
        flush = i == len(pieces) - 1
        first, k2 = metrics.key_stream_count(at, k, lag, flush)
        e_d = e[:, at:at + k].to(DEV).contiguous()
        f_out, p_out = GuardedTensor((R, k, 24)), GuardedTensor((R, k2), torch.int32)
        k_out = C.c_int(-7)
        _lib.check(L.ake_key_stream_step_f32(e_d.data_ptr() if k else None, R, k, at, lag, int(flush), A_d.data_ptr(),
                                             None if p_d is None else p_d.data_ptr(), state.data_ptr(), state.numel(),
                                             f_out.t.data_ptr() if k else None, p_out.t.data_ptr() if k2 else None, C.byref(k_out),
                                             torch.cuda.current_stream().cuda_stream), "ake_key_stream_step_f32")
        assert k_out.value == k2
        f_out.check("filtered"); p_out.check("path"); state_check("state")
        fs.append(f_out.t.cpu()); ps.append(p_out.t.cpu())
        at += k
    assert at == W
    return torch.cat(fs, dim=1), torch.cat(ps, dim=1)


def filtered_ratio(got, f32, f64):
    """worst |got - f64| / bound over the rows, with the module docstring's bound."""
    host = float((f32.double() - f64).abs().max())
    bound = torch.clamp(f64.abs().amax(dim=-1) * 2.0 ** -20, min=4 * host)
    return float(((got.double() - f64).abs().amax(dim=-1) / bound).max())


@pytest.mark.parametrize("kind", ["gauss", "ties", "deep"])
@pytest.mark.parametrize("W", [1, 2, 40, 300])
@pytest.mark.parametrize("R", [1, 3])
def test_stream_step_against_the_host_model(R, W, kind):
    e, A, prior = case_inputs(kind, R, W, seed=100 * R + W)
    worst = 0.0
    for n, lag in enumerate(LAGS):
        f32, p32 = metrics.key_stream(e, A, prior, lag=lag)
        f64, _ = metrics.key_stream(e.double(), A.double(), None if prior is None else prior.double(), lag=lag)
        chunkings = [[1] * W, ([7, 33] + [W - 40] if W > 40 else [W]) + [0], [W]]      # the second ends on k = 0 with flush
        if W == 40:
            chunkings[1] = [7, 33, 0]
        runs = [device_steps(e, A, prior, lag, pieces, fill) for pieces, fill in zip(chunkings, (0x00, 0xFF, 0x77))]
        if n == 0:
            runs.append(device_steps(e, A, prior, lag, chunkings[2], 0x77))             # a rerun
        f, p = runs[0]
        assert p.shape == (R, W) and torch.equal(p, p32), lag
        assert bool(torch.isfinite(f).all())
        for f2, p2 in runs[1:]:
            assert torch.equal(f2, f) and torch.equal(p2, p), lag                      # every chunking, bit for bit
        worst = max(worst, filtered_ratio(f, f32, f64))
    print(f"\n  STREAM step R {R} W {W} {kind} | filtered: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_stream_step_errors():
    L = _lib.lib()
    R, k, lag = 2, 5, 3
    e = torch.zeros((R, k, 24), device=DEV)
    A = metrics.key_transition_log(0.9).float().to(DEV)
    nbytes = L.ake_key_stream_state_bytes(R, lag)
    state = torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)
    f, p = torch.empty((R, k, 24), device=DEV), torch.empty((R, k), dtype=torch.int32, device=DEV)
    k_out = C.c_int(0)
    stream = torch.cuda.current_stream().cuda_stream

    def call(emis=e.data_ptr(), R=R, k=k, before=0, lag=lag, trans=A.data_ptr(), st=state.data_ptr(), st_bytes=nbytes, path=p.data_ptr(),
             out=C.byref(k_out), flush=1):
        return L.ake_key_stream_step_f32(emis, R, k, before, lag, flush, trans, None, st, st_bytes, f.data_ptr(), path, out, stream)

    assert call() == 0 and k_out.value == k
    assert call(st_bytes=nbytes - 1) == -4                                           # AKE_ERR_WORKSPACE
    assert b"state" in L.ake_last_error()
    for bad in (dict(lag=-1), dict(lag=256), dict(k=-1), dict(R=0), dict(before=-1), dict(trans=None), dict(st=None), dict(out=None),
                dict(emis=None), dict(path=None), dict(st=state.data_ptr() + 4)):
        assert call(**bad) == -1, bad                                                # AKE_ERR_INVALID
    assert L.ake_key_stream_state_bytes(0, 3) == 0 and L.ake_key_stream_state_bytes(1, 256) == 0 and L.ake_key_stream_state_bytes(1, -1) == 0
    assert call(k=0, emis=None, path=None, flush=0) == 0 and k_out.value == 0        # nothing to do: no launch, no error
    torch.cuda.synchronize()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------

def lib_emissions(key, tonic, weight):
    out = torch.empty(key.shape[:2] + (24,), device=DEV)
    _lib.check(_lib.lib().ake_key_emissions_f32(key.contiguous().data_ptr(), tonic.contiguous().data_ptr(), key.shape[0] * key.shape[1], None, 1,
                                                weight, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "ake_key_emissions_f32")
    return out


def check_smoothed(s, ups, W, lag, weight=1.0):
    check_window_order(ups, W)
    emis = joined(ups, "emissions")
    assert torch.equal(emis, lib_emissions(joined(ups, "key"), joined(ups, "tonic"), weight))
    at = 0
    for u in ups:                                                                    # every window smoothed once, in order
        assert u.smooth_first_window == at and u.filtered.shape == u.emissions.shape
        at += u.smooth_key_id.shape[1]
    assert at == W
    A = s.trans.cpu()
    f32, p32 = metrics.key_stream(emis.cpu(), A, lag=lag)
    f64, _ = metrics.key_stream(emis.cpu().double(), A.double(), lag=lag)
    assert torch.equal(joined(ups, "smooth_key_id").cpu(), p32)
    ratio = filtered_ratio(joined(ups, "filtered").cpu(), f32, f64)
    assert ratio <= 1.0, ratio
    return emis, A, ratio


def test_end_to_end_smoothed_stream(streamed, est, recordings):
    s, ups = streamed[1.0]
    emis, A, ratio = check_smoothed(s, ups, 31, 3)
    print(f"\n  STREAM end to end | filtered: worst error / bound {ratio:.3f}")
    # a lag of the whole recording is the offline Viterbi path
    s255, ups255 = run_stream(est, recordings, schedule_irregular(), stride_seconds=1.0, lag_windows=255)
    emis255 = joined(ups255, "emissions")
    assert all(u.smooth_key_id.shape[1] == 0 for u in ups255[:-1]) and ups255[-1].smooth_key_id.shape == (2, 31)
    assert torch.equal(ups255[-1].smooth_key_id.cpu(), metrics.viterbi_keys(emis255.cpu(), s255.trans.cpu()))
    # a user transition and a signature weight pass through
    T = metrics.key_transition_log(0.5).float()
    sT, upsT = run_stream(est, recordings, schedule_irregular(), stride_seconds=1.0, lag_windows=3, transition=T, signature_weight=0.5)
    assert torch.equal(sT.trans.cpu(), T)
    check_smoothed(sT, upsT, 31, 3, weight=0.5)
    assert not torch.equal(joined(upsT, "emissions"), emis)


def test_a_stream_without_a_smoother_launches_none(est, recordings):
    short = recordings[:, :30 * SR]
    for smooth in (False, True):
        _lib.prof_enable("", True)
        try:
            _, ups = run_stream(est, short, [10 * SR] * 3, smooth=smooth)
            names = set(_lib.prof_results())
        finally:
            _lib.prof_enable("", False)
        assert ("key_stream_step_kernel" in names) == smooth and ("key_emissions_kernel" in names) == smooth, names
        assert {"stream_history_kernel", "decode_keys_kernel"} <= names
        for u in ups:
            for n in ("emissions", "filtered", "smooth_key_id", "smooth_first_window"):
                assert (getattr(u, n) is not None) == smooth


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device(est, weights):
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(None, SR, 5, device=DEV).stream(1)
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(est.net, SR, 0).stream(1)
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(est.net, SR, 5, wrap_mode="true_end").stream(1)
    for kw in (dict(rate=44100), dict(tuning="auto"), dict(lag_windows=256), dict(lag_windows=-1)):
        with pytest.raises(ValueError):
            est.stream(1, **kw)
    s = est.stream(2)
    with pytest.raises(ValueError):
        s.push(torch.zeros((3, 100), device=DEV))
    with pytest.raises(ValueError):
        s.push(torch.zeros((2, 2, 100), device=DEV))
    u = s.push(torch.zeros((2, 100), device=DEV))
    assert u.windows == 0 and u.key.shape == (2, 0, 12) and u.smooth_key_id.shape == (2, 0)
    with pytest.raises(ValueError):
        s.push(torch.zeros((2, 100), dtype=torch.int16, device=DEV))
    assert s.finish().windows == 0
    with pytest.raises(ValueError):
        s.push(torch.zeros((2, 100), device=DEV))
    with pytest.raises(ValueError):
        s.finish()
    torch.cuda.synchronize()
