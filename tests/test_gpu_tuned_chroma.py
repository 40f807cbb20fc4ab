"""GPU: the tuned chroma against its float64 model (ake_profile_emissions_tuned_f32 / metrics.profile_emissions(cents=...)), the entry
point's workspace contract, and tuned_chroma=True through KeyEstimator.

The bounds are those of tests/test_gpu_profiles.py on the same four outputs: both sides are double chains rounded once to float32,
    |emissions - model| <= 2^-22 * sharpness,   |confidence - model| <= 2^-22,   |chroma - model| <= 2^-22
and the model reads what the kernel reads: the float32 log-CQT, the profile table rounded to float32 and the cents rounded to float32.
key_id is compared wherever the model's two best correlations differ by at least 1e-9; the seeds are such that the model alone leaves
out no cell (asserted), and at most 2 % could be.  The largest errors measured over these cases are in profiles/tuned_chroma.md.
"""
import math

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics, synthetic
from test_gpu_profiles import BOUND, COMPRESSIONS, MIN_MARGIN, MIN_SPREAD, as_kernel_reads, run_profile, user_profile
from test_gpu_tuning import E2E_CENTS, E2E_LENGTHS
from test_tuning_host import harmonic_clip
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, HOP = 22050, 4410
AKE_ERR_INVALID, AKE_ERR_WORKSPACE, AKE_ERR_UNSUPPORTED = -1, -4, -5
OLD_KERNELS = ("profile_chroma_kernel", "profile_score_kernel")
NEW_KERNELS = ("profile_fold_kernel", "profile_tuned_score_kernel")
CHUNK = 64                       # frames per block of profile_fold_kernel
CENTS = (0.0, 50.0, -50.0, 16.6, -33.4, float("nan"), 80.0)
ROW_PAD = 3                      # a cents grid is handed over as the first W columns of rows W + ROW_PAD wide


def run_tuned(mel, frames_major, counts, wf, sf, profiles, compression, sharpness, cents, fill=0x5A, ws_bytes=None, windows=None):
    """ake_profile_emissions_tuned_f32 with guarded outputs and a guarded workspace of exactly ake_profile_tuned_workspace_bytes `fill`
    bytes -> (rc, chroma, emissions, key_id, confidence).  cents: a host tensor (R,), handed over with a window stride of 0, or (R, W),
    handed over inside rows of W + ROW_PAD (NaN in the padding)."""
    L = ake_amd._lib.lib()
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    need = L.ake_profile_tuned_workspace_bytes(R, T)
    assert need >= R * T * 36 * 8
    W = L.ake_profile_windows(T, wf, sf) if windows is None else windows
    ws, ws_check = guarded(need if ws_bytes is None else ws_bytes, fill)
    outs = [GuardedTensor((R, W, 12)), GuardedTensor((R, W, 24)), GuardedTensor((R, W), dtype=torch.int32, fill=0x7F), GuardedTensor((R, W))]
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    prof = as_kernel_reads(profiles).to(device=DEV, dtype=torch.float32).contiguous()
    if cents.dim() == 1:
        c, rec_stride, win_stride = cents.to(device=DEV, dtype=torch.float32).contiguous(), 1, 0
    else:
        c = torch.full((R, cents.shape[1] + ROW_PAD), float("nan"), device=DEV)
        c[:, :cents.shape[1]] = cents.to(DEV)
        rec_stride, win_stride = c.stride(0), 1
    rc = L.ake_profile_emissions_tuned_f32(mel.data_ptr(), 1 if frames_major else 0, R, P, T, cnt.data_ptr() if cnt is not None else None, wf, sf,
                                           W, prof.data_ptr(), COMPRESSIONS.index(compression), float(sharpness), c.data_ptr(), rec_stride,
                                           win_stride, *[o.t.data_ptr() for o in outs], ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream().cuda_stream)
    ws_check("tuned profile workspace")
    for o, name in zip(outs, ("chroma", "emissions", "key_id", "confidence")):
        o.check(name)
    return (rc,) + tuple(o.t.clone() for o in outs)


def model_case(mel_pt, counts, wf, sf, profiles, compression, sharpness, cents, what):
    """The float64 model on these inputs, and what it alone says about them: no decided window sits near a tie or near the silence
    rule -> (the model's four outputs, decided (R, W), number of silent windows)."""
    want = metrics.profile_emissions(mel_pt, wf, sf, counts, as_kernel_reads(profiles), compression, sharpness, cents=cents)
    want_c, want_e, want_k, _ = want
    R, W = want_k.shape
    T = mel_pt.shape[2]
    n = torch.full((R,), T) if counts is None else torch.tensor(counts).clamp(0, T)
    live = torch.arange(W)[None, :] < metrics.profile_window_counts(n, wf, sf)[:, None]
    decided = want_k >= 0
    assert bool((decided <= live).all())
    top2 = (want_e / sharpness).topk(2, dim=2).values
    clear = decided & ((top2[..., 0] - top2[..., 1]) >= MIN_MARGIN)
    assert torch.equal(clear, decided), what                         # the model leaves out no cell (2 % would be allowed)
    x = want_c[decided]
    mean = x.mean(dim=1, keepdim=True)
    assert x.numel() == 0 or float((((x - mean) ** 2).sum(dim=1) / (12 * mean[:, 0] ** 2)).min()) >= MIN_SPREAD, what
    return want, decided, int((live & ~decided).sum())


worst = {"emissions": 0.0, "confidence": 0.0, "chroma": 0.0}


def check_case(mel_pt, counts, wf, sf, profiles, compression, sharpness, cents, what):
    """mel_pt (R, P, T) float32 on the host: both layouts against the float64 model on the same float32 numbers, and against each
    other to the bit."""
    (want_c, want_e, want_k, want_f), decided, n_silent = model_case(mel_pt, counts, wf, sf, profiles, compression, sharpness, cents, what)
    got = []
    for fm in (False, True):
        mel = (mel_pt.transpose(1, 2) if fm else mel_pt).contiguous().to(DEV)
        rc, c, e, k, f = run_tuned(mel, fm, counts, wf, sf, profiles, compression, sharpness, cents)
        assert rc == 0, ake_amd._lib.lib().ake_last_error()
        errs = {"emissions": float((e.cpu().double() - want_e).abs().max()) / sharpness, "confidence": float((f.cpu().double() - want_f).abs().max()),
                "chroma": float((c.cpu().double() - want_c).abs().max())}
        print(f"tuned {what} {'frames-major' if fm else 'pitch-major'}: " + ", ".join(f"{name} {v:.2e}" for name, v in errs.items()))
        for name, v in errs.items():
            worst[name] = max(worst[name], v)
            assert v <= BOUND, (what, fm, name, v)
        assert torch.equal(k.cpu(), want_k), (what, fm)
        dead = ~decided.to(DEV)                                      # silent and behind-count cells: exact zeros and -1
        assert bool((k[dead] == -1).all()) and not bool(c[dead].any()) and not bool(e[dead].any()) and not bool(f[dead].any())
        got.append((c, e, k, f))
    assert all(torch.equal(a, b) for a, b in zip(*got)), what       # the two layouts: the same bits
    return n_silent


def shape_cases(P, T):
    """-> the (mel, counts, wf, sf, profiles, compression, sharpness, cents, what) of one (P, T): 8 recordings, the last of exact
    zeros; the windows (1, 1), (5, 2), (76, 1) and the whole clip over the three compressions and a user profile; the cents once per
    recording and once as a grid over ragged counts that hold a 0 and one below a window."""
    g = torch.Generator().manual_seed(5000 + 7 * T + P)
    mel = torch.rand((8, P, T), generator=g) * 3.0
    mel[7] = 0.0
    per_rec = torch.tensor(CENTS + (16.6,))
    for wf, sf, profiles, compression, sharpness in ((1, 1, "krumhansl", "log", 10.0), (5, 2, user_profile(), "power", 30.0),
                                                     (76, 1, "temperley", "magnitude", 3.0), (0, 1, "krumhansl", "magnitude", 10.0)):
        if wf > T:
            continue
        name = profiles if isinstance(profiles, str) else "user"
        what = f"{P}x{T} wf {wf} sf {sf} {name} {compression}"
        W = 1 if wf == 0 else (T - wf) // sf + 1
        yield mel, None, wf, sf, profiles, compression, sharpness, per_rec, what + " cents per recording"
        grid = torch.tensor([[CENTS[(r + 3 * w) % len(CENTS)] for w in range(W)] for r in range(8)])
        mid = max((T + wf) // 2, 1)
        counts = [T, max(wf - 1, 0), 0, mid, T, T, mid, T] if wf else [T, T // 2, 0, mid, T, 1, mid, T]
        yield mel, counts, wf, sf, profiles, compression, sharpness, grid, what + " ragged, a cents grid"


@pytest.mark.parametrize("P", [36, 288])
@pytest.mark.parametrize("T", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_kernel_equals_the_model(P, T):
    L = ake_amd._lib.lib()
    for mel, counts, wf, sf, profiles, compression, sharpness, cents, what in shape_cases(P, T):
        n_silent = check_case(mel, counts, wf, sf, profiles, compression, sharpness, cents, what)
        if counts is None:                                           # the recording of exact zeros: every window of it is silent
            assert n_silent == L.ake_profile_windows(T, wf, sf), what
    print("largest errors so far (emissions / sharpness, confidence, chroma):", {k: f"{v:.2e}" for k, v in worst.items()})


def _launched(fn):
    ake_amd._lib.prof_enable("", True)
    try:
        fn()
        return {k: v[1] for k, v in ake_amd._lib.prof_results().items()}
    finally:
        ake_amd._lib.prof_enable("", False)


def test_outputs_do_not_depend_on_what_the_workspace_held():
    """Bit-identical outputs across workspace fills 0x00 / 0xFF / 0x77, after a call of another shape, and across reruns (the guards are
    checked inside run_tuned)."""
    g = torch.Generator().manual_seed(56)
    mel = (torch.rand((3, 36, 2 * CHUNK + 1), generator=g) * 3.0).to(DEV)
    other = (torch.rand((2, 288, CHUNK + 1), generator=g) * 3.0).to(DEV)
    cents = torch.tensor([16.6, -50.0, 33.0])
    args = ([2 * CHUNK + 1, 70, 0], 5, 5, "krumhansl", "magnitude", 10.0, cents)
    for fm in (False, True):
        m = mel.transpose(1, 2).contiguous() if fm else mel
        first = run_tuned(m, fm, *args, fill=0x00)
        assert first[0] == 0
        for fill in (0xFF, 0x77, 0x00):
            o = other.transpose(1, 2).contiguous() if fm else other
            assert run_tuned(o, fm, None, 0, 1, "temperley", "power", 3.0, torch.tensor([-20.0, 45.0]), fill=fill)[0] == 0
            again = run_tuned(m, fm, *args, fill=fill)
            assert again[0] == 0 and all(torch.equal(a, b) for a, b in zip(again[1:], first[1:])), (fm, fill)
    # the package call, in a workspace the allocator hands it after other work: the same bits
    got = ake_amd.profile_emissions(mel, 5, 5, torch.tensor(args[0]), compression="magnitude", cents=cents)
    assert all(torch.equal(a, b) for a, b in zip(got, run_tuned(mel, False, *args)[1:]))
    got = ake_amd.profile_emissions(mel.transpose(1, 2).contiguous(), 5, 5, torch.tensor(args[0]), frames_major=True, compression="magnitude",
                                    cents=cents.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(got, first[1:]))


def test_refusals_launch_nothing():
    L = ake_amd._lib.lib()
    R, P, T, wf, sf = 3, 36, 20, 5, 5
    mel = torch.rand((R, P, T), device=DEV)
    need = L.ake_profile_tuned_workspace_bytes(R, T)
    W = L.ake_profile_windows(T, wf, sf)
    assert W == 4 and need >= R * T * 36 * 8
    assert L.ake_profile_tuned_workspace_bytes(0, T) == 0 and L.ake_profile_tuned_workspace_bytes(R, 0) == 0
    assert L.ake_profile_tuned_workspace_bytes(65536, T) == 0
    cents = torch.tensor([10.0, -10.0, 0.0])
    rc, c, e, k, f = run_tuned(mel, False, None, wf, sf, "krumhansl", "log", 10.0, cents, ws_bytes=need - 1)      # one byte short
    assert rc == AKE_ERR_WORKSPACE and b"workspace" in L.ake_last_error()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(e).all()) and bool(torch.isnan(f).all())            # nothing ran
    prof = as_kernel_reads("krumhansl").to(device=DEV, dtype=torch.float32)
    f32 = lambda *shape: torch.zeros(shape, device=DEV)
    c, e, k, f = f32(R, W, 12), f32(R, W, 24), torch.zeros((R, W), dtype=torch.int32, device=DEV), f32(R, W)
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    cd = cents.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(mel_p=mel.data_ptr(), pitches=P, wf=wf, sf=sf, windows=W, prof_p=prof.data_ptr(), compression=0, sharpness=10.0, outs=None,
             ws_p=ws.data_ptr(), ws_n=need, cents_p=cd.data_ptr(), rec_stride=1, win_stride=0):
        outs = [c.data_ptr(), e.data_ptr(), k.data_ptr(), f.data_ptr()] if outs is None else outs
        return L.ake_profile_emissions_tuned_f32(mel_p, 0, R, pitches, T, None, wf, sf, windows, prof_p, compression, sharpness, cents_p,
                                                 rec_stride, win_stride, *outs, ws_p, ws_n, stream)

    assert _launched(lambda: call()) == dict.fromkeys(NEW_KERNELS, 1) and call() == 0
    refused = [(dict(mel_p=None), AKE_ERR_INVALID), (dict(prof_p=None), AKE_ERR_INVALID), (dict(cents_p=None), AKE_ERR_UNSUPPORTED),
               (dict(pitches=35), AKE_ERR_UNSUPPORTED), (dict(pitches=39), AKE_ERR_UNSUPPORTED),
               (dict(pitches=24), AKE_ERR_UNSUPPORTED), (dict(compression=3), AKE_ERR_INVALID), (dict(compression=-1), AKE_ERR_INVALID),
               (dict(sharpness=float("nan")), AKE_ERR_INVALID), (dict(sharpness=0.0), AKE_ERR_INVALID), (dict(sharpness=-1.0), AKE_ERR_INVALID),
               (dict(sf=0), AKE_ERR_INVALID), (dict(wf=-1), AKE_ERR_INVALID), (dict(windows=W + 1), AKE_ERR_INVALID),
               (dict(windows=W - 1), AKE_ERR_INVALID), (dict(wf=0, windows=2), AKE_ERR_INVALID), (dict(ws_p=None), AKE_ERR_WORKSPACE),
               (dict(ws_n=need - 1), AKE_ERR_WORKSPACE), (dict(ws_p=ws.data_ptr() + 4), AKE_ERR_INVALID), (dict(rec_stride=-1), AKE_ERR_INVALID),
               (dict(win_stride=-1), AKE_ERR_INVALID)]
    for i in range(4):
        outs = [c.data_ptr(), e.data_ptr(), k.data_ptr(), f.data_ptr()]
        outs[i] = None
        refused.append((dict(outs=outs), AKE_ERR_INVALID))
    for kw, want in refused:
        rcs = []
        assert _launched(lambda: rcs.append(call(**kw))) == {}, kw   # a refused call launches nothing
        assert rcs == [want], (kw, rcs)
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(torch.rand((1, 39, 8), device=DEV), 2, 1, cents=0.0)
    ake_amd.profile_emissions(torch.rand((1, 39, 8), device=DEV), 2, 1)                    # (the entry without cents takes it)
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(mel, 2, 1, cents=torch.zeros(4))
    with pytest.raises(ake_amd._lib.AkeError):
        ake_amd.profile_emissions(mel.cpu(), 2, 1, cents=0.0)


def test_the_package_call_with_and_without_cents():
    """cents=0.0 is the uniform chroma within the bound (its classes are added in another order); cents=None launches what it launched
    and returns the old entry's bits."""
    g = torch.Generator().manual_seed(77)
    mel = (torch.rand((3, 288, CHUNK + 1), generator=g) * 3.0).to(DEV)
    counts = [CHUNK + 1, 40, 0]
    got = []
    plain_launches = _launched(lambda: got.append(ake_amd.profile_emissions(mel, 5, 2, torch.tensor(counts), sharpness=10.0)))
    assert plain_launches == dict.fromkeys(OLD_KERNELS, 1)
    plain = got[0]
    assert all(torch.equal(a, b) for a, b in zip(plain, run_profile(mel, False, counts, 5, 2, "krumhansl", "log", 10.0)[1:]))
    tuned_launches = _launched(lambda: got.append(ake_amd.profile_emissions(mel, 5, 2, torch.tensor(counts), sharpness=10.0, cents=0.0)))
    assert tuned_launches == dict.fromkeys(NEW_KERNELS, 1)
    zero = got[1]
    assert torch.equal(zero[2], plain[2])
    for a, b, scale in zip(zero, plain, (1.0, 10.0, None, 1.0)):
        if scale is not None:
            assert float((a.double() - b.double()).abs().max()) <= BOUND * scale
    grid = torch.full((3, 40), float("nan"), device=DEV)             # a (R, W) view of wider rows goes in as it is
    W = plain[2].shape[1]
    grid[:, :W] = 22.0
    a = ake_amd.profile_emissions(mel, 5, 2, torch.tensor(counts), cents=grid[:, :W])
    b = ake_amd.profile_emissions(mel, 5, 2, torch.tensor(counts), cents=22.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], zero[0])


# ---- the estimator ----

WF, SF = 76, 25                  # 15 s windows, 5 s apart
DETUNE = (-31.0, 43.0)


@pytest.fixture(scope="module")
def est():
    return ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)


@pytest.fixture(scope="module")
def recordings():
    """Two modulating recordings of 75 s and 52 s, played 31 cents flat and 43 cents sharp (ake_amd.retune the other way round), with
    their lengths."""
    arrays, _ = synthetic.modulating_batch_arrays((3, 8), (75.0, 52.0))
    audio = ake_amd.synth_partials(device=DEV, **arrays)
    lengths = torch.as_tensor(arrays["n"], device=DEV)
    audio, lengths = ake_amd.retune(audio, -torch.tensor(DETUNE, device=DEV), lengths)
    return audio.contiguous(), lengths


def track_by_hand(est, audio, lengths, cents_of, profiles, compression, sharpness):
    """plan.logmag, the cents from that transform (cents_of(mel, frames) -> (cents, strength)), profile_emissions(cents=...), then the
    Viterbi and posterior entries: what track(method="profile", tuned_chroma=True, smooth=True, posteriors=True) must equal, tensor for
    tensor."""
    L = ake_amd._lib.lib()
    mel = est.plan.logmag(audio, lengths=lengths)
    R, _, T = mel.shape
    frames = None if lengths is None else (1 + lengths.to(torch.int64) // HOP).clamp(max=T).to(torch.int32)
    cents, strength = cents_of(mel, frames)
    chroma, em, key_id, conf = ake_amd.profile_emissions(mel, WF, SF, frames, profiles=profiles, compression=compression, sharpness=sharpness,
                                                         cents=cents)
    W = key_id.shape[1]
    assert W == (T - WF) // SF + 1
    counts = torch.full((R,), W, dtype=torch.int32, device=DEV) if frames is None else \
        torch.where(frames < WF, torch.zeros_like(frames), (frames - WF) // SF + 1).to(torch.int32)
    trans = metrics.key_transition_log(stay=math.exp(-(SF * HOP / SR) / 60.0)).to(device=DEV, dtype=torch.float32)
    path = torch.empty((R, W), dtype=torch.int32, device=DEV)
    post, path_conf, loglik = torch.empty((R, W, 24), device=DEV), torch.empty((R, W), device=DEV), torch.empty((R,), device=DEV)
    ws = torch.empty(max(L.ake_viterbi_keys_workspace_bytes(R, W), L.ake_key_posteriors_workspace_bytes(R, W)), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    ake_amd._lib.check(L.ake_viterbi_keys_f32(em.data_ptr(), R, W, counts.data_ptr(), trans.data_ptr(), None, path.data_ptr(), ws.data_ptr(),
                                              ws.numel(), stream), "viterbi")
    ake_amd._lib.check(L.ake_key_posteriors_f32(em.data_ptr(), R, W, counts.data_ptr(), trans.data_ptr(), None, path.data_ptr(), post.data_ptr(),
                                                loglik.data_ptr(), None, path_conf.data_ptr(), ws.data_ptr(), ws.numel(), stream), "posteriors")
    return dict(key=chroma, emissions=em, key_id=key_id, confidence=conf, counts=counts, smooth_key_id=path, posteriors=post,
                smooth_confidence=path_conf, log_likelihood=loglik, tuning_cents=cents, tuning_strength=strength)


def same_as_by_hand(track, want):
    assert track.tuned_chroma and track.tuning_curve is None
    for name, t in want.items():
        got = getattr(track, name)
        assert (got is None and t is None) or torch.equal(got, t), name


AUTO = lambda mel, frames: ake_amd.estimate_tuning(mel)
FOLLOW = lambda mel, frames: ake_amd.tuning_track(mel, WF, SF, frames)[2:0:-1]           # (curve, strength)


@pytest.mark.parametrize("mode", ["equal", "ragged", "int16", "streams", "given", "follow"])
def test_tuned_track_equals_the_manual_chain(est, recordings, mode):
    audio, lengths = recordings
    profiles, compression, sharpness = ("temperley", "magnitude", 3.0) if mode == "ragged" else ("krumhansl", "log", 10.0)
    kw = dict(method="profile", smooth=True, posteriors=True, profiles=profiles, compression=compression, profile_sharpness=sharpness,
              tuning="auto", tuned_chroma=True)
    hand = lambda a, l, cents_of=AUTO: track_by_hand(est, a, l, cents_of, profiles, compression, sharpness)
    if mode == "equal":
        short = audio[:, :int(lengths.min())].contiguous()
        track = est.track(short, **kw)
        same_as_by_hand(track, hand(short, None))
        assert int(track.counts.min()) == track.key_id.shape[1] > 0
        assert torch.equal(track.times, est.track(short, method="profile").times)
        return
    if mode == "int16":
        pcm = (audio * 32767.0).round().to(torch.int16)
        same_as_by_hand(est.track(pcm, lengths, **kw), hand(pcm, lengths))
        return
    if mode == "given":
        cents = torch.tensor([12.5, -20.0], device=DEV)
        track = est.track(audio, lengths, **dict(kw, tuning=cents))
        same_as_by_hand(track, hand(audio, lengths, lambda mel, frames: (cents, None)))
        one = est.track(audio, lengths, **dict(kw, tuning=12.5))
        assert torch.equal(one.key[0], track.key[0]) and one.tuning_cents.tolist() == [12.5, 12.5] and one.tuning_strength is None
        return
    if mode == "follow":
        # (tuning_window_seconds and tuning_stride_seconds are not read: the tuning track runs on the key track's own windows)
        track = est.track(audio, lengths, **dict(kw, tuning="follow", tuning_window_seconds=1.0, tuning_stride_seconds=3.0))
        want = hand(audio, lengths, FOLLOW)
        same_as_by_hand(track, want)
        assert track.tuning_cents.shape == track.key_id.shape == track.tuning_strength.shape
        return
    e = ake_amd.KeyEstimator(None, SR, 5, streams=2, device=DEV, pitches=288) if mode == "streams" else est
    track = e.track(audio, lengths, **kw)
    again = e.track(audio, lengths, **kw)                                              # (streams: the second call runs on the other stream)
    e.join()
    want = hand(audio, lengths)
    same_as_by_hand(track, want)
    same_as_by_hand(again, want)
    assert float((track.tuning_cents.cpu() - torch.tensor(DETUNE)).abs().max()) <= 3.0   # the estimate finds the detuning
    plain = est.track(audio, lengths, method="profile")                                # tuning=None: the same windows at the same times
    assert torch.equal(track.times, plain.times) and torch.equal(track.counts, plain.counts)
    assert (track.hop, track.window_frames, track.stride_frames, track.sample_rate) == (HOP, WF, SF, SR)
    assert track.segments(0) and track.segments(1, smoothed=False)
    fitted, _ = ake_amd.fit_key_transition(track, iterations=2)
    assert fitted.shape == (24, 24)


def test_times_of_a_tuned_track_are_the_recordings_own(est):
    """Nothing was resampled, so score and segments translate nothing: on a track with tuned_chroma they equal those of the same
    labels on a track without tuning fields."""
    arrays, segments = synthetic.modulating_batch_arrays((3, 8), (75.0, 52.0))
    audio = ake_amd.synth_partials(device=DEV, **arrays)
    lengths = torch.as_tensor(arrays["n"], device=DEV)
    ann = ake_amd.KeyAnnotations.from_segments([[(s / SR, k) for s, k in segs] for segs in segments], SR, DEV)
    track = est.track(audio, lengths, method="profile", smooth=True, tuning=torch.tensor([30.0, -30.0]), tuned_chroma=True)
    score = track.score(ann)
    ref = metrics.track_score(track.smooth_key_id, track.counts, ann.seg_start, ann.seg_key, ann.seg_count, HOP, WF, SF)
    for a, b in zip((score.truth, score.category, score.tally, score.changes), ref):
        assert torch.equal(a, b)
    bare_copy = ake_amd.KeyTrack(**{**track.__dict__, "tuning_cents": None, "tuning_strength": None, "tuned_chroma": False})
    assert track.segments(0) == bare_copy.segments(0) and track.segments(1, smoothed=False) == bare_copy.segments(1, smoothed=False)


def test_what_a_tuned_track_launches(est, recordings):
    """One transform, the estimate's kernels and the two new kernels; no retuner, no second transform, neither kernel of the uniform
    chroma.  tuned_chroma=False launches what it launched."""
    audio, lengths = recordings
    kw = dict(method="profile", tuning="auto")
    est.track(audio, lengths, **kw); est.track(audio, lengths, tuned_chroma=True, **kw); torch.cuda.synchronize()     # (workspaces exist)
    mel = est.plan.logmag(audio, lengths=lengths)
    transform = _launched(lambda: est.plan.logmag(audio, lengths=lengths))
    estimate = _launched(lambda: ake_amd.estimate_tuning(mel))
    tuned = _launched(lambda: est.track(audio, lengths, tuned_chroma=True, **kw))
    want = dict(transform)
    for name, n in estimate.items():
        want[name] = want.get(name, 0) + n
    assert transform and estimate and tuned == dict(want, profile_fold_kernel=1, profile_tuned_score_kernel=1), sorted(tuned.items())
    retuned = _launched(lambda: est.track(audio, lengths, **kw))
    assert any("retune" in name for name in retuned) and not any("retune" in name for name in tuned)
    assert all(retuned[name] == 2 * n for name, n in transform.items()) and not set(retuned) & set(NEW_KERNELS)
    assert retuned == _launched(lambda: est.track(audio, lengths, tuned_chroma=False, **kw))
    follow = _launched(lambda: est.track(audio, lengths, method="profile", tuning="follow", tuned_chroma=True))
    assert all(follow[name] == n for name, n in transform.items()) and not any("retune" in name for name in follow)
    key = _launched(lambda: est.profile_key(audio, lengths, tuning="auto", tuned_chroma=True))
    assert key == tuned


def test_estimator_refusals(est, recordings):
    """(A plan's bins are always whole octaves on the device: the refusal of other bin counts is held in the host tests.)"""
    audio, lengths = recordings

    def refused(fn):
        with pytest.raises(ValueError):
            fn()

    for fn in (lambda: est.track(audio, lengths, tuning="auto", tuned_chroma=True),
               lambda: est.track(audio, lengths, method="profile", tuned_chroma=True),
               lambda: est.track(audio, lengths, method="profile", tuning="auto", refine=True, tuned_chroma=True),
               lambda: est.track(audio, lengths, method="profile", tuning="sharp", tuned_chroma=True),
               lambda: est.profile_key(audio, lengths, tuned_chroma=True)):
        assert _launched(lambda: refused(fn)) == {}


def test_profile_key_on_detuned_harmonic_clips(est):
    """The three ragged 15 s harmonic clips of tests/test_gpu_tuning.py's end-to-end test, 38 cents flat, 22 and 47 cents sharp (the
    trio that file builds with in-tune twins): profile_key(tuning="auto", tuned_chroma=True) on the detuned clips names the key
    profile_key names on the in-tune ones.  "follow" is the same call; given cents go in as they are."""
    rows, twins = np.zeros((3, E2E_LENGTHS[0])), np.zeros((3, E2E_LENGTHS[0]))
    for i, (c, n) in enumerate(zip(E2E_CENTS, E2E_LENGTHS)):
        rows[i, :n] = harmonic_clip(20 + i, c, n)
        twins[i, :n] = harmonic_clip(20 + i, 0.0, n)
    lengths = torch.tensor(E2E_LENGTHS, device=DEV)
    on_dev = lambda x: torch.from_numpy(x.astype(np.float32)).to(DEV)
    want = est.profile_key(on_dev(twins), lengths)[0]
    got = est.profile_key(on_dev(rows), lengths, tuning="auto", tuned_chroma=True)
    uniform = est.profile_key(on_dev(rows), lengths)[0]
    print("keys: in tune", want.tolist(), "tuned chroma on the detuned clips", got[0].tolist(), "uniform chroma on them", uniform.tolist())
    assert bool((want >= 0).all()) and torch.equal(got[0], want)
    follow = est.profile_key(on_dev(rows), lengths, tuning="follow", tuned_chroma=True)
    assert all(torch.equal(a, b) for a, b in zip(got, follow))
    mel = est.plan.logmag(on_dev(rows), lengths=lengths)
    frames = (1 + lengths // HOP).clamp(max=mel.shape[2]).to(torch.int32)
    cents, _ = ake_amd.estimate_tuning(mel)
    by_hand = ake_amd.profile_emissions(mel, 0, 1, frames, cents=cents)
    assert all(torch.equal(a, b[:, 0]) for a, b in zip(got, (by_hand[2], by_hand[3], by_hand[0], by_hand[1])))
    given = est.profile_key(on_dev(rows), lengths, tuning=torch.tensor(E2E_CENTS), tuned_chroma=True)
    assert torch.equal(given[0], want)
