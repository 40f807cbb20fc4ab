"""GPU: the key-profile emissions against their float64 model (ake_profile_emissions_f32 / metrics.profile_emissions), the entry point's
workspace contract, and method="profile" through KeyEstimator.

Both sides are double chains rounded once to float32, so the bounds are four float32 roundings of a value bounded by the sharpness or by 1:
    |emissions - model| <= 2^-22 * sharpness,   |confidence - model| <= 2^-22,   |chroma - model| <= 2^-22
The model reads the numbers the kernel reads: the float32 log-CQT and the profile table rounded to float32 (the C entry takes it as
float32 [2][12]).  The largest errors measured over these cases are in profiles/key_profiles.md.
"""
import math

import pytest
import torch

import ake_amd
from ake_amd import metrics, synthetic
from conftest import golden_state_dict
from test_gpu_pipeline import default_opt
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, HOP = 22050, 4410
AKE_ERR_INVALID, AKE_ERR_WORKSPACE, AKE_ERR_UNSUPPORTED = -1, -4, -5
BOUND = 2.0 ** -22
MIN_SPREAD, MIN_MARGIN = 1e-6, 1e-9
NEW_KERNELS = ("profile_chroma_kernel", "profile_score_kernel")
CHUNK = 64                       # frames per block of profile_chroma_kernel
COMPRESSIONS = metrics.PROFILE_COMPRESSIONS


def user_profile():
    return torch.rand((2, 12), generator=torch.Generator().manual_seed(41), dtype=torch.float64) + 0.2


def as_kernel_reads(profiles):
    """The (2, 12) table rounded to float32, in float64: what the model must read to be compared with the kernel."""
    return metrics.key_profile_table(profiles).to(torch.float32).to(torch.float64)


def run_profile(mel, frames_major, counts, wf, sf, profiles, compression, sharpness, fill=0x5A, ws_bytes=None, windows=None):
    """ake_profile_emissions_f32 with guarded outputs and a guarded workspace of exactly ake_profile_workspace_bytes `fill` bytes
    -> (rc, chroma, emissions, key_id, confidence)."""
    L = ake_amd._lib.lib()
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    need = L.ake_profile_workspace_bytes(R, T)
    assert need >= R * T * 12 * 8
    W = L.ake_profile_windows(T, wf, sf) if windows is None else windows
    ws, ws_check = guarded(need if ws_bytes is None else ws_bytes, fill)
    outs = [GuardedTensor((R, W, 12)), GuardedTensor((R, W, 24)), GuardedTensor((R, W), dtype=torch.int32, fill=0x7F), GuardedTensor((R, W))]
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    prof = as_kernel_reads(profiles).to(device=DEV, dtype=torch.float32).contiguous()
    rc = L.ake_profile_emissions_f32(mel.data_ptr(), 1 if frames_major else 0, R, P, T, cnt.data_ptr() if cnt is not None else None, wf, sf, W,
                                     prof.data_ptr(), COMPRESSIONS.index(compression), float(sharpness), *[o.t.data_ptr() for o in outs],
                                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    ws_check("profile workspace")
    for o, name in zip(outs, ("chroma", "emissions", "key_id", "confidence")):
        o.check(name)
    return (rc,) + tuple(o.t.clone() for o in outs)


worst = {"emissions": 0.0, "confidence": 0.0, "chroma": 0.0}


def check_case(mel_pt, counts, wf, sf, profiles, compression, sharpness, what):
    """mel_pt (R, P, T) float32 on the host: both layouts against the float64 model on the same float32 numbers."""
    want_c, want_e, want_k, want_f = metrics.profile_emissions(mel_pt, wf, sf, counts, as_kernel_reads(profiles), compression, sharpness)
    # what the model alone says about these inputs: no window sits near the silence rule or near a tie
    R, W = want_k.shape
    T = mel_pt.shape[2]
    n = torch.full((R,), T) if counts is None else torch.tensor(counts).clamp(0, T)
    live = torch.arange(W)[None, :] < metrics.profile_window_counts(n, wf, sf)[:, None]
    silent = live & (want_k < 0)
    decided = want_k >= 0
    assert bool((decided <= live).all())
    top2 = (want_e / sharpness).topk(2, dim=2).values
    assert not bool(decided.any()) or float((top2[..., 0] - top2[..., 1])[decided].min()) > MIN_MARGIN, what
    x = want_c[decided]                                              # sum-normalised: the relative spread is that of x itself
    mean = x.mean(dim=1, keepdim=True)
    assert x.numel() == 0 or float((((x - mean) ** 2).sum(dim=1) / (12 * mean[:, 0] ** 2)).min()) >= MIN_SPREAD, what
    for fm in (False, True):
        mel = (mel_pt.transpose(1, 2) if fm else mel_pt).contiguous().to(DEV)
        rc, c, e, k, f = run_profile(mel, fm, counts, wf, sf, profiles, compression, sharpness)
        assert rc == 0, ake_amd._lib.lib().ake_last_error()
        errs = {"emissions": float((e.cpu().double() - want_e).abs().max()) / sharpness, "confidence": float((f.cpu().double() - want_f).abs().max()),
                "chroma": float((c.cpu().double() - want_c).abs().max())}
        print(f"profile {what} {'frames-major' if fm else 'pitch-major'}: " + ", ".join(f"{name} {v:.2e}" for name, v in errs.items()))
        for name, v in errs.items():
            worst[name] = max(worst[name], v)
            assert v <= BOUND, (what, fm, name, v)
        assert torch.equal(k.cpu(), want_k), (what, fm)             # (the model's margin exceeds 1e-9 everywhere: no window is left out)
        dead = ~decided.to(DEV)                                      # silent and behind-count cells: exact zeros and -1
        assert bool((k[dead] == -1).all()) and not bool(c[dead].any()) and not bool(e[dead].any()) and not bool(f[dead].any())
        rc2, *again = run_profile(mel, fm, counts, wf, sf, profiles, compression, sharpness, fill=0xFF)     # a poisoned workspace, a rerun
        assert rc2 == 0 and all(torch.equal(a, b) for a, b in zip(again, (c, e, k, f)))
    return int(silent.sum())


@pytest.mark.parametrize("P", [36, 288])
@pytest.mark.parametrize("T", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_kernel_equals_the_model(P, T):
    g = torch.Generator().manual_seed(1000 + 7 * T + P)
    mel = torch.rand((3, P, T), generator=g) * 3.0
    zeros = mel.clone()
    zeros[1] = 0.0                                                   # a recording of exact zeros: silent windows
    configs = [(1, 1, "krumhansl", "log", 10.0), (5, 5, "temperley", "magnitude", 3.0), (5, 1, user_profile(), "power", 30.0),
               (76, 5, "krumhansl", "log", 10.0), (76, 1, "temperley", "power", 10.0), (0, 1, "krumhansl", "magnitude", 10.0)]
    for wf, sf, profiles, compression, sharpness in configs:
        if wf > T:
            continue                                                 # (no window at all: test_no_window_at_all)
        name = profiles if isinstance(profiles, str) else "user"
        what = f"{P}x{T} wf {wf} sf {sf} {name} {compression}"
        n_silent = check_case(zeros, None, wf, sf, profiles, compression, sharpness, what)
        assert n_silent == ake_amd._lib.lib().ake_profile_windows(T, wf, sf)
        mid = max((T + wf) // 2, 1)
        check_case(mel, [T, max(wf - 1, 0), 0] if wf else [T, T // 2, 0], wf, sf, profiles, compression, sharpness, what + " ragged")
        check_case(mel[:1], [mid], wf, sf, profiles, compression, sharpness, what + " one recording")
        check_case(mel[:1], None, wf, sf, profiles, compression, sharpness, what + " one recording, all frames")
    print("largest errors so far (emissions / sharpness, confidence, chroma):", {k: f"{v:.2e}" for k, v in worst.items()})


def test_no_window_at_all():
    """Recordings shorter than one window: W = 0, the entry accepts it and writes nothing; the package call returns empty tensors."""
    L = ake_amd._lib.lib()
    mel = torch.rand((2, 36, 9), device=DEV)
    assert L.ake_profile_windows(9, 10, 1) == 0
    prof = as_kernel_reads("krumhansl").to(device=DEV, dtype=torch.float32)
    need = L.ake_profile_workspace_bytes(2, 9)
    ws, ws_check = guarded(need, 0x5A)
    out = GuardedTensor((4,))                                        # (an empty tensor has no address to hand over)
    rc = L.ake_profile_emissions_f32(mel.data_ptr(), 0, 2, 36, 9, None, 10, 1, 0, prof.data_ptr(), 0, 10.0, out.t.data_ptr(), out.t.data_ptr(),
                                     out.t.data_ptr(), out.t.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    ws_check("workspace"); out.check("outputs")
    assert rc == 0 and bool(torch.isnan(out.t).all())
    got = ake_amd.profile_emissions(mel, 10, 1)
    assert [tuple(o.shape) for o in got] == [(2, 0, 12), (2, 0, 24), (2, 0), (2, 0)]


def test_outputs_do_not_depend_on_what_the_workspace_held():
    """Bit-identical outputs across workspace fills 0x00 / 0xFF / 0x77, after a call of another shape, and across reruns (the guards are
    checked inside run_profile)."""
    g = torch.Generator().manual_seed(55)
    mel = (torch.rand((3, 36, 2 * CHUNK + 1), generator=g) * 3.0).to(DEV)
    other = (torch.rand((2, 288, CHUNK + 1), generator=g) * 3.0).to(DEV)
    args = ([2 * CHUNK + 1, 70, 0], 5, 5, "krumhansl", "magnitude", 10.0)
    for fm in (False, True):
        m = mel.transpose(1, 2).contiguous() if fm else mel
        first = run_profile(m, fm, *args, fill=0x00)
        assert first[0] == 0
        for fill in (0xFF, 0x77, 0x00):
            assert run_profile(other.transpose(1, 2).contiguous() if fm else other, fm, None, 0, 1, "temperley", "power", 3.0, fill=fill)[0] == 0
            again = run_profile(m, fm, *args, fill=fill)
            assert again[0] == 0 and all(torch.equal(a, b) for a, b in zip(again[1:], first[1:])), (fm, fill)
    # the package call, in a workspace the allocator hands it after other work: the same bits
    got = ake_amd.profile_emissions(mel, 5, 5, torch.tensor(args[0]), compression="magnitude")
    assert all(torch.equal(a, b) for a, b in zip(got, run_profile(mel, False, *args)[1:]))
    got = ake_amd.profile_emissions(mel.transpose(1, 2).contiguous(), 5, 5, torch.tensor(args[0]), frames_major=True, compression="magnitude")
    assert all(torch.equal(a, b) for a, b in zip(got, first[1:]))


def test_refusals():
    L = ake_amd._lib.lib()
    R, P, T, wf, sf = 3, 36, 20, 5, 5
    mel = torch.rand((R, P, T), device=DEV)
    need = L.ake_profile_workspace_bytes(R, T)
    W = L.ake_profile_windows(T, wf, sf)
    assert W == 4 and L.ake_profile_windows(T, 0, 1) == 1 and L.ake_profile_windows(T, T + 1, 1) == 0
    assert L.ake_profile_windows(0, 5, 1) == -1 and L.ake_profile_windows(T, -1, 1) == -1 and L.ake_profile_windows(T, 5, 0) == -1
    assert L.ake_profile_workspace_bytes(0, T) == 0 and L.ake_profile_workspace_bytes(R, 0) == 0
    rc, c, e, k, f = run_profile(mel, False, None, wf, sf, "krumhansl", "log", 10.0, ws_bytes=need - 1)     # one byte short
    assert rc == AKE_ERR_WORKSPACE and b"workspace" in L.ake_last_error()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(e).all()) and bool(torch.isnan(f).all())         # nothing ran
    prof = as_kernel_reads("krumhansl").to(device=DEV, dtype=torch.float32)
    f32 = lambda *shape: torch.zeros(shape, device=DEV)
    c, e, k, f = f32(R, W, 12), f32(R, W, 24), torch.zeros((R, W), dtype=torch.int32, device=DEV), f32(R, W)
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(mel_p=mel.data_ptr(), pitches=P, wf=wf, sf=sf, windows=W, prof_p=prof.data_ptr(), compression=0, sharpness=10.0, outs=None,
             ws_p=ws.data_ptr(), ws_n=need):
        outs = [c.data_ptr(), e.data_ptr(), k.data_ptr(), f.data_ptr()] if outs is None else outs
        return L.ake_profile_emissions_f32(mel_p, 0, R, pitches, T, None, wf, sf, windows, prof_p, compression, sharpness, *outs, ws_p, ws_n, stream)

    assert call() == 0
    assert call(mel_p=None) == AKE_ERR_INVALID and call(prof_p=None) == AKE_ERR_INVALID
    for i in range(4):
        outs = [c.data_ptr(), e.data_ptr(), k.data_ptr(), f.data_ptr()]
        outs[i] = None
        assert call(outs=outs) == AKE_ERR_INVALID
    assert call(pitches=35) == AKE_ERR_UNSUPPORTED
    assert call(compression=3) == AKE_ERR_INVALID and call(compression=-1) == AKE_ERR_INVALID
    assert call(sharpness=float("nan")) == AKE_ERR_INVALID and call(sharpness=0.0) == AKE_ERR_INVALID and call(sharpness=-1.0) == AKE_ERR_INVALID
    assert call(sf=0) == AKE_ERR_INVALID and call(wf=-1) == AKE_ERR_INVALID
    assert call(windows=W + 1) == AKE_ERR_INVALID and call(windows=W - 1) == AKE_ERR_INVALID and call(wf=0, windows=2) == AKE_ERR_INVALID
    assert call(ws_p=None) == AKE_ERR_WORKSPACE and call(ws_n=need - 1) == AKE_ERR_WORKSPACE
    assert call(ws_p=ws.data_ptr() + 4) == AKE_ERR_INVALID          # 8-byte alignment
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(torch.rand((1, 37, 8), device=DEV), 2, 1)
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(mel, 2, 1, profiles="aarden")
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(mel, 2, 1, profiles=torch.ones((2, 12)))
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(mel, 2, 1, compression="sqrt")
    with pytest.raises(ValueError):
        ake_amd.profile_emissions(mel, 2, 1, sharpness=0.0)
    with pytest.raises(ake_amd._lib.AkeError):
        ake_amd.profile_emissions(mel.cpu(), 2, 1)


# ---- the estimator ----

@pytest.fixture(scope="module")
def net(gold_default):
    n = ake_amd.PitchClassNet(288, 12, 2, 7, default_opt())
    n.load_state_dict(golden_state_dict(gold_default), strict=True)
    return n.to(DEV).eval()


@pytest.fixture(scope="module")
def est(net):
    return ake_amd.KeyEstimator(net, SR, 5)


@pytest.fixture(scope="module")
def bare():
    return ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)


@pytest.fixture(scope="module")
def recordings():
    """Two modulating recordings of 75 s and 52 s with their annotations."""
    arrays, segments = synthetic.modulating_batch_arrays((3, 8), (75.0, 52.0))
    audio = ake_amd.synth_partials(device=DEV, **arrays)
    ann = ake_amd.KeyAnnotations.from_segments([[(s / SR, k) for s, k in segs] for segs in segments], SR, DEV)
    return audio, torch.as_tensor(arrays["n"], device=DEV), ann


@pytest.fixture(scope="module")
def mixed_recordings():
    """Three modulating recordings of 60 s, 45 s and 75 s that visit minor and major keys, with their annotations."""
    arrays, segments = synthetic.modulating_batch_arrays((1, 2, 3), (60.0, 45.0, 75.0))
    assert {k // 12 for segs in segments for _, k in segs} == {0, 1}
    audio = ake_amd.synth_partials(device=DEV, **arrays)
    ann = ake_amd.KeyAnnotations.from_segments([[(s / SR, k) for s, k in segs] for segs in segments], SR, DEV)
    return audio, torch.as_tensor(arrays["n"], device=DEV), ann


WF, SF = 76, 25                  # 15 s windows, 5 s apart


def track_by_hand(est, audio, lengths, profiles, compression, sharpness):
    """plan.logmag, profile_emissions, then the Viterbi and posterior entries: what track(method="profile", smooth=True,
    posteriors=True) must equal, tensor for tensor."""
    L = ake_amd._lib.lib()
    mel = est.plan.logmag(audio, lengths=lengths)
    R, _, T = mel.shape
    frames = None if lengths is None else (1 + lengths.to(torch.int64) // HOP).clamp(max=T).to(torch.int32)
    chroma, em, key_id, conf = ake_amd.profile_emissions(mel, WF, SF, frames, profiles=profiles, compression=compression, sharpness=sharpness)
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
                smooth_confidence=path_conf, log_likelihood=loglik)


def same_as_by_hand(track, want):
    for name, t in want.items():
        assert torch.equal(getattr(track, name), t), name
    e = track.emissions
    assert track.genre is None and torch.equal(track.tonic, torch.maximum(e[..., :12], e[..., 12:]))
    k = track.key_id.cpu()
    rows = metrics.MAJOR_TONIC.tolist()
    assert track.tonic_id.cpu().tolist() == [[-1 if v < 0 else v % 12 for v in row] for row in k.tolist()]
    assert track.sig.cpu().tolist() == [[-1 if v < 0 else rows.index(metrics.KEY_MAJOR_TONIC[v]) for v in row] for row in k.tolist()]
    n = track.counts.cpu().tolist()
    for r, c in enumerate(n):
        assert bool((k[r, c:] == -1).all()) and bool((track.smooth_key_id[r, :c] >= 0).all())


@pytest.mark.parametrize("mode", ["equal", "ragged", "int16", "streams", "tuning"])
def test_profile_track_equals_the_manual_chain(est, recordings, mode):
    audio, lengths, ann = recordings
    profiles, compression, sharpness = ("temperley", "magnitude", 3.0) if mode == "ragged" else ("krumhansl", "log", 10.0)
    kw = dict(method="profile", smooth=True, posteriors=True, profiles=profiles, compression=compression, profile_sharpness=sharpness)
    if mode == "equal":
        short = audio[:, :int(lengths.min())].contiguous()
        track = est.track(short, **kw)
        same_as_by_hand(track, track_by_hand(est, short, None, profiles, compression, sharpness))
        assert int(track.counts.min()) == track.key_id.shape[1] > 0
        return
    if mode == "int16":
        pcm = (audio * 32767.0).round().to(torch.int16)
        track = est.track(pcm, lengths, **kw)
        same_as_by_hand(track, track_by_hand(est, pcm, lengths, profiles, compression, sharpness))
        as_float = est.track(ake_amd.pcm16_to_float(pcm), lengths, **kw)              # int16 PCM = the float32 route
        assert len(track._tensors()) == len(as_float._tensors())
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(track._tensors(), as_float._tensors()))
        return
    if mode == "tuning":
        cents = torch.tensor([12.5, -20.0], device=DEV)
        track = est.track(audio, lengths, tuning=cents, **kw)
        retuned, len2 = ake_amd.retune(audio, cents, lengths)
        same_as_by_hand(track, track_by_hand(est, retuned, len2, profiles, compression, sharpness))
        assert torch.equal(track.tuning_cents, cents) and track.tuning_strength is None
        return
    e = ake_amd.KeyEstimator(est.net, SR, 5, streams=2) if mode == "streams" else est
    track = e.track(audio, lengths, **kw)
    again = e.track(audio, lengths, **kw)                                              # (streams: the second call runs on the other stream)
    e.join()
    want = track_by_hand(est, audio, lengths, profiles, compression, sharpness)
    same_as_by_hand(track, want)
    same_as_by_hand(again, want)
    assert track.counts.cpu().tolist() == [(1 + int(n) // HOP - WF) // SF + 1 for n in lengths.cpu()]
    assert (track.hop, track.window_frames, track.stride_frames, track.sample_rate) == (HOP, WF, SF, SR)
    plain = est.track(audio, lengths, **dict(kw, smooth=False, posteriors=False))      # without smooth: the emissions are there, no path
    assert torch.equal(plain.emissions, track.emissions) and plain.smooth_key_id is None and plain.posteriors is None
    for smoothed in (False, True):                                                     # score runs on such a track
        score = track.score(ann, smoothed=smoothed)
        ref = metrics.track_score(track.smooth_key_id if smoothed else track.key_id, track.counts, ann.seg_start, ann.seg_key, ann.seg_count,
                                  HOP, WF, SF)
        for a, b in zip((score.truth, score.category, score.tally, score.changes), ref):
            assert torch.equal(a, b)
    assert track.segments(0) and track.segments(1, smoothed=False)
    fitted, logliks = ake_amd.fit_key_transition(track, iterations=2)
    assert fitted.shape == (24, 24)


def test_profile_key_equals_the_whole_clip_call(est, recordings):
    audio, lengths, _ = recordings
    mel = est.plan.logmag(audio, lengths=lengths)
    frames = (1 + lengths // HOP).clamp(max=mel.shape[2]).to(torch.int32)
    chroma, em, key_id, conf = ake_amd.profile_emissions(mel, 0, 1, frames, profiles="temperley", compression="power", sharpness=3.0)
    got = est.profile_key(audio, lengths, profiles="temperley", compression="power", sharpness=3.0)
    assert all(torch.equal(a, b[:, 0]) for a, b in zip(got, (key_id, conf, chroma, em)))
    assert got[0].shape == (2,) and got[3].shape == (2, 24) and bool((got[0] >= 0).all())
    want_c, want_e, want_k, want_f = metrics.profile_emissions(mel.cpu(), 0, 1, frames.cpu(), as_kernel_reads("temperley"), "power", 3.0)
    assert torch.equal(key_id.cpu(), want_k) and float((em.cpu().double() - want_e).abs().max()) <= BOUND * 3.0
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(est.net, SR, 0).profile_key(audio, lengths)


def test_fit_key_profiles_on_the_estimator(est, recordings, mixed_recordings):
    with pytest.raises(ValueError):                                  # (these two recordings stay in minor keys throughout)
        est.fit_key_profiles(*[recordings[i] for i in (0, 2, 1)])
    audio, lengths, ann = mixed_recordings
    fitted = est.fit_key_profiles(audio, ann, lengths, compression="magnitude", min_purity=0.5)
    assert fitted.shape == (2, 12) and fitted.dtype == torch.float64
    mel = est.plan.logmag(audio, lengths=lengths)
    frames = (1 + lengths // HOP).clamp(max=mel.shape[2]).to(torch.int32)
    chroma, _, key_id, _ = ake_amd.profile_emissions(mel, WF, SF, frames, compression="magnitude")
    R, W = key_id.shape
    lab = metrics.window_labels(ann.seg_start, ann.seg_key, ann.seg_count, torch.arange(R, device=DEV).repeat_interleave(W),
                                torch.arange(W, device=DEV).repeat(R) * SF, HOP, WF, min_purity=0.5)
    weight = lab["sample_weight"] * (key_id.reshape(-1) >= 0)
    assert int((weight > 0).sum()) > 0 and int((weight == 0).sum()) > 0
    assert torch.equal(fitted, ake_amd.fit_key_profiles(chroma.reshape(-1, 12), lab["truth"], weight))
    track = est.track(audio, lengths, method="profile", profiles=fitted)               # goes straight into profiles=
    assert bool((track.key_id[0, :int(track.counts[0])] >= 0).all())


def test_an_estimator_without_a_net(est, bare, recordings, mixed_recordings):
    audio, lengths, ann = recordings
    kw = dict(method="profile", smooth=True, posteriors=True)
    a, b = bare.track(audio, lengths, **kw), est.track(audio, lengths, **kw)
    assert len(a._tensors()) == len(b._tensors())
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a._tensors(), b._tensors()))
    assert all(torch.equal(x, y) for x, y in zip(bare.profile_key(audio, lengths), est.profile_key(audio, lengths)))
    m_audio, m_lengths, m_ann = mixed_recordings
    assert torch.equal(bare.fit_key_profiles(m_audio, m_ann, m_lengths), est.fit_key_profiles(m_audio, m_ann, m_lengths))
    for refused in (lambda: bare(audio), lambda: bare.track(audio, lengths), lambda: bare.track(audio, lengths, method="net"),
                    lambda: bare.training_windows(audio, ann, lengths)):
        with pytest.raises(ValueError):
            refused()
    with pytest.raises(ValueError):
        est.track(audio, lengths, method="profile", signature_weight=0.5)
    with pytest.raises(ValueError):
        est.track(audio, lengths, method="chroma")
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(est.net, SR, 5, device=DEV)
    with pytest.raises(ValueError):
        ake_amd.KeyEstimator(None, SR, 0, device=DEV).track(audio, lengths, method="profile")


def _launched(fn):
    ake_amd._lib.prof_enable("", True)
    try:
        fn()
        return {k: v[1] for k, v in ake_amd._lib.prof_results().items()}
    finally:
        ake_amd._lib.prof_enable("", False)


def test_what_the_two_methods_launch(net, est, recordings):
    """method="profile" launches the transform and the two new kernels, no net kernel; the default track() launches what
    ake_pipeline_track_ragged_f32 launches, neither new kernel, and returns that entry's bits."""
    L = ake_amd._lib.lib()
    audio, lengths, _ = recordings
    est.track(audio, lengths); est.track(audio, lengths, method="profile"); torch.cuda.synchronize()      # (workspaces and weights exist)
    R, n = audio.shape
    W = (1 + n // HOP - WF) // SF + 1
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)
    outs = [f32(R, W, 12), f32(R, W, 12), f32(R, W, 11), i32(R, W), i32(R, W), i32(R, W), f32(R, W), i32(R)]
    len64 = lengths.to(torch.int64).contiguous()

    def by_hand():
        ws = torch.empty(L.ake_pipeline_track_workspace_bytes(est.plan.handle, net.handle, R, n, WF, SF), dtype=torch.uint8, device=DEV)
        ake_amd._lib.check(L.ake_pipeline_track_ragged_f32(est.plan.handle, net.handle, audio.data_ptr(), R, n, audio.stride(0), len64.data_ptr(),
                                                           WF, SF, *[o.data_ptr() for o in outs], ws.data_ptr(), ws.numel(),
                                                           torch.cuda.current_stream().cuda_stream), "track")

    tracks = []
    default = _launched(lambda: tracks.append(est.track(audio, lengths)))
    assert default and default == _launched(by_hand) and not set(default) & set(NEW_KERNELS), sorted(default)
    t = tracks[0]
    for got, want in zip((t.key, t.tonic, t.genre, t.key_id, t.sig, t.tonic_id, t.confidence, t.counts), outs):
        assert torch.equal(got, want)
    assert t.emissions is None and t.smooth_key_id is None
    transform = _launched(lambda: est.plan.logmag(audio, lengths=lengths))
    profile = _launched(lambda: est.track(audio, lengths, method="profile"))
    assert transform and profile == dict(transform, profile_chroma_kernel=1, profile_score_kernel=1), sorted(profile)
    assert set(default) - set(transform) and not (set(default) - set(transform)) & set(profile)           # the net's kernels: none of them
