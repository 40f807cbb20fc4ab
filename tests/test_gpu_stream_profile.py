"""GPU: net-free key streams -- ake_stream_frame_stats_f32 and ake_stream_profile_emissions_f32 against the offline entry
ake_profile_emissions_f32 on the joined frames (to the bit) and against metrics.stream_tuning (the bound below), their state and
refusals, and KeyEstimator.stream(method="profile", tuning_meter=True) end to end.

Bounds.  The chroma and the scores are the offline kernels' own arithmetic (csrc/profile.h) on the same frames: torch.equal.  The tuning
meter's two numbers are a double chain rounded once to float32, compared with the float64 model on the same float32 frames: cents within
2^-22 * 50 = 1.2e-5 (the float32 output's half ulp at 50 is 1.9e-6; double-library differences scale with 1 / strength <= 20 and stay
orders below that), strength within 2^-22, on inputs with strength >= 0.05.

A piece of n frames always completes a window that begins in front of frames_before - window_frames + stride_frames, so a ring must hold
more than window_frames + n - stride_frames rows: the pattern 1, 0, 3, 2, 7, 1 with wf = 5, sf = 2 runs on a ring of 5 + 7 = 12 rows
(metrics.stream_profile_ring_frames), a ring of 7 rows takes that pattern with its pieces held to 2 frames, and a piece of 7 into the ring of 7 is one of
the refusals."""
import ctypes as C
import itertools
import json
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from ake_amd.pipeline import KeyEstimator, track_counts
from conftest import golden_state_dict, load_golden
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, HOP, WF = 22050, 4410, 76
N45 = 992250
IRREGULAR = (1, 4409, 4410, 4411, 0, 22050, 100000)           # test_gpu_stream.py's schedule
AKE_ERR_INVALID, AKE_ERR_WORKSPACE, AKE_ERR_UNSUPPORTED = -1, -4, -5
CENTS_BOUND, STRENGTH_BOUND = 2.0 ** -22 * 50.0, 2.0 ** -22
TRANSFORM_BOUND = 5e-4                                       # streamed against offline frames (test_gpu_stream.py)
PATTERN = (1, 0, 3, 2, 7, 1)
NEW_KERNELS = {"stream_frame_stats_kernel", "stream_profile_score_kernel"}
NET_ONLY = {"stream_frames_fm_kernel", "stream_frames_pm_kernel", "key_emissions_kernel", "decode_keys_kernel", "layer0_fused_kernel",
            "pc2pc_fused_kernel", "heads_fused_kernel"}
PROFILE_STREAM = {"stream_history_kernel", "key_stream_step_kernel"} | NEW_KERNELS       # besides the transform's cqt_* kernels
OUT_NAMES = ("chroma", "emissions", "key_id", "confidence", "tonic", "tonic_id", "signature_id")


def launched(fn):
    _lib.prof_enable("", True)
    try:
        _lib.prof_results()                                          # (start from an empty log)
        fn()
        return {k: v[1] for k, v in _lib.prof_results().items() if v[1]}
    finally:
        _lib.prof_enable("", False)


def cut_by(pattern, T, longest=None):
    out, left = [], T
    for m in itertools.cycle(pattern):
        if left == 0:
            return out
        m = min(m, left, longest or m)
        out.append(m)
        left -= m


def state_bytes(R, ring):
    n = _lib.lib().ake_stream_profile_state_bytes(R, ring)
    assert n == (R * (ring * 12 + 3) * 8 + 15) // 16 * 16
    return n


def sig_table():
    return KeyEstimator._key_sig_table(torch.device(DEV))


def device_profile(profiles="krumhansl"):
    return metrics.key_profile_table(profiles).to(device=DEV, dtype=torch.float32).contiguous()


def new_outputs(R, k, guards):
    shapes = (((R, k, 12), torch.float32), ((R, k, 24), torch.float32), ((R, k), torch.int32), ((R, k), torch.float32),
              ((R, k, 12), torch.float32), ((R, k), torch.int32), ((R, k), torch.int32))
    if guards:
        return [GuardedTensor(s, dtype=d, fill=0x7F if d == torch.int32 else 0xFF) for s, d in shapes]
    return [Namespace(t=torch.empty(s, dtype=d, device=DEV), check=lambda what="": None) for s, d in shapes]


def run_entries(mel, fm, cuts, wf, sf, ring, compression=0, parts=3, min_strength=0.0, profiles="krumhansl", sharpness=10.0, fill=None):
    """The two entries over `mel` ((R, P, T) float32 on the device, or (R, T, P) with `fm`) cut into pieces of `cuts` frames: each piece
    is frames `first` .. of the one transform output, as in a stream.  `fill`: the state and all outputs sit in guarded buffers, the
    state filled with that byte.  -> (the seven joined outputs, the state's defined bytes, [(cents, strength) after every piece that
    had frames])."""
    L = _lib.lib()
    R, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if fm else mel.shape
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = state_bytes(R, ring)
    state, state_check = guarded(nbytes, fill) if fill is not None else (torch.empty(nbytes, dtype=torch.uint8, device=DEV), lambda what: None)
    prof, sig = device_profile(profiles), sig_table()
    F = W = 0
    joined, meter = [[] for _ in OUT_NAMES], []
    for m in cuts:
        cents, strength = (GuardedTensor((R,)), GuardedTensor((R,))) if fill is not None else (new_outputs(R, 1, False)[3], new_outputs(R, 1, False)[3])
        rc = L.ake_stream_frame_stats_f32(mel.data_ptr(), int(fm), R, P, T, F, m, F, ring, parts, compression, min_strength, state.data_ptr(),
                                          state.numel(), cents.t.data_ptr(), strength.t.data_ptr(), stream)
        assert rc == 0, L.ake_last_error()
        F += m
        if m and parts & 2:
            meter.append((cents.t.reshape(R).clone(), strength.t.reshape(R).clone()))
        k = track_counts(F, wf, sf) - W
        outs = new_outputs(R, k, fill is not None)
        if parts & 1:
            rc = L.ake_stream_profile_emissions_f32(state.data_ptr(), state.numel(), R, ring, F, wf, sf, W, k, prof.data_ptr(), sharpness,
                                                    sig.data_ptr(), *[o.t.data_ptr() if k else None for o in outs], stream)
            assert rc == 0, L.ake_last_error()
        for o, name in zip(outs + [cents, strength], OUT_NAMES + ("cents", "strength")):
            o.check(name)
        state_check("state")
        for j, o in zip(joined, outs):
            j.append(o.t.clone())
        W += k
    assert F == T
    torch.cuda.synchronize()
    return [torch.cat(j, dim=1) for j in joined], state[:R * (ring * 12 + 3) * 8].clone(), meter


def offline(mel, fm, wf, sf, compression, profiles="krumhansl", sharpness=10.0):
    """ake_profile_emissions_f32 on the joined frames, and _run_profile_track's torch expressions for the other three."""
    c, e, k, f = ake_amd.profile_emissions(mel, wf, sf, frames_major=fm, profiles=profiles, compression=metrics.PROFILE_COMPRESSIONS[compression],
                                           sharpness=sharpness)
    tonic = torch.maximum(e[..., :12], e[..., 12:])
    minus = torch.full_like(k, -1)
    tonic_id = torch.where(k < 0, minus, k % 12)
    sig = torch.where(k < 0, minus, sig_table()[k.clamp_min(0).to(torch.int64)])
    return [c, e, k, f, tonic, tonic_id, sig]


def random_frames(R, P, T, seed):
    """Random log-magnitudes in [0, 3] and, in the last recording, a stretch of exact zeros long enough for silent windows."""
    mel = torch.rand((R, P, T), generator=torch.Generator().manual_seed(seed)) * 3.0
    mel[R - 1, :, T // 3:T // 3 + 14] = 0.0
    return mel


def placed_frames(R, P, T, seed):
    """Hand-placed bin positions (test_stream_profile_host.py): position 0 carries most of the power, so strength >= 0.05 by far."""
    power = torch.rand((R, P, T), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    power[:, 0::3] = 1.0 + power[:, 0::3]
    power[:, 1::3] = 0.5 * power[:, 1::3]
    power[:, 2::3] = 0.3 * power[:, 2::3]
    return torch.log1p(torch.sqrt(power)).to(torch.float32)


# ---- 1. the entries against the offline entry ----------------------------------------------------------------------------------------------

# (wf, sf, T, the ring of the cut runs, their patterns)
GEOMETRIES = [(5, 2, 41, 12, (PATTERN, (1,), (7, 0))), (5, 2, 41, 7, ((1, 0, 2, 2, 2, 1), (1,))), (1, 1, 41, 8, (PATTERN,)), (5, 9, 41, 12, (PATTERN,)),
              (76, 5, 100, 79, ((1, 0, 3, 2, 3, 1),))]


@pytest.mark.parametrize("P", [36, 288])
@pytest.mark.parametrize("R", [1, 3])
def test_entries_equal_the_offline_entry_under_every_chunking(R, P):
    n_silent = 0
    for g, (wf, sf, T, ring, patterns) in enumerate(GEOMETRIES):
        host = random_frames(R, P, T, 100 * P + 10 * R + g)
        for fm in (False, True):
            mel = (host.transpose(1, 2) if fm else host).contiguous().to(DEV)
            for compression in ((0, 1, 2) if g == 0 else ((g + int(fm)) % 3,)):
                want = offline(mel, fm, wf, sf, compression)
                n_silent += int((want[2] < 0).sum())
                states = []
                for pattern in patterns:
                    got, state, _ = run_entries(mel, fm, cut_by(pattern, T), wf, sf, ring, compression)
                    states.append(state)
                    for name, a, b in zip(OUT_NAMES, got, want):
                        assert a.shape == b.shape and torch.equal(a, b), (name, wf, sf, fm, compression, pattern)
                for s in states[1:]:
                    assert torch.equal(s, states[0]), (wf, sf, fm, compression)
                whole, state, _ = run_entries(mel, fm, [T], wf, sf, wf + T, compression)        # all at once, with a ring that fits
                for name, a, b in zip(OUT_NAMES, whole, want):
                    assert torch.equal(a, b), (name, wf, sf, fm, compression, "at once")
                # the ring rows are the frames' chroma whatever the ring's length: the last `ring` frames, by frame index
                rows = state[:R * (wf + T) * 96].view(torch.float64).view(R, wf + T, 12)[:, :T]
                small = states[0][:R * ring * 96].view(torch.float64).view(R, ring, 12)
                for t in range(max(0, T - ring), T):
                    assert torch.equal(small[:, t % ring], rows[:, t]), t
    assert n_silent > 0                                              # the zero stretch did give silent windows


def test_a_user_profile_and_another_sharpness_reach_the_kernel():
    host = random_frames(2, 36, 41, 5)
    mel = host.contiguous().to(DEV)
    user = torch.rand((2, 12), generator=torch.Generator().manual_seed(41), dtype=torch.float64) + 0.2
    want = offline(mel, False, 5, 2, 1, user, 3.0)
    got, _, _ = run_entries(mel, False, cut_by(PATTERN, 41), 5, 2, 12, 1, profiles=user, sharpness=3.0)
    for name, a, b in zip(OUT_NAMES, got, want):
        assert torch.equal(a, b), name
    assert not torch.equal(got[1], offline(mel, False, 5, 2, 1)[1])


# ---- 2. the tuning part --------------------------------------------------------------------------------------------------------------------

# T: more than two tiles of 64 in the run that takes all at once.  P: up to 4623 bins a round of the kernel's LDS stage holds a frame
# (288: 16 frames a round, so a tile of 64 takes four; 4623: one frame a round); from 4624 on the adding thread computes the squares itself
@pytest.mark.parametrize("R, P, T", [(1, 36, 150), (3, 36, 150), (1, 288, 150), (3, 288, 150), (1, 4623, 70), (2, 4626, 70)])
def test_tuning_meter_against_the_float64_model(R, P, T):
    host = placed_frames(R, P, T, 7 * P + R)
    worst = [0.0, 0.0]
    finals = []
    for fm in (False, True):
        mel = (host.transpose(1, 2) if fm else host).contiguous().to(DEV)
        for cuts, parts in ((cut_by(PATTERN, T), 3), ([T], 2), ([64, T - 64], 2), (cut_by(PATTERN, T), 2)):
            _, _, meter = run_entries(mel, fm, cuts, 5, 2, 12, 2, parts=parts)
            model = metrics.stream_tuning([host[:, :, a:a + m] for a, m in zip(np.cumsum([0] + cuts[:-1]), cuts) if m])
            assert len(meter) == len(model)
            for (c, s), (mc, ms) in zip(meter, model):
                assert float(ms.min()) >= 0.05
                worst[0] = max(worst[0], float((c.cpu().double() - mc).abs().max()))
                worst[1] = max(worst[1], float((s.cpu().double() - ms).abs().max()))
            finals.append(meter[-1])
            again = run_entries(mel, fm, cuts, 5, 2, 12, 2, parts=parts)[2]
            assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(meter, again))      # a rerun: the same bits
    print(f"\n  STREAM tuning meter R {R} P {P} | cents {worst[0]:.2e} (bound {CENTS_BOUND:.2e}), strength {worst[1]:.2e} (bound {STRENGTH_BOUND:.2e})")
    assert worst[0] <= CENTS_BOUND and worst[1] <= STRENGTH_BOUND
    for c, s in finals[1:]:                                          # every chunking, both layouts, with and without the chroma part
        assert torch.equal(c, finals[0][0]) and torch.equal(s, finals[0][1])


def test_min_strength_is_decided_on_the_double_and_at_equality():
    # equal power p on the positions 1 and 2 (the same numbers added in the same order), none on 0: z = -p and the total 2 p exactly, so
    # strength == 0.5 and cents == 50
    host = torch.zeros((1, 36, 9))
    host[:, 1::3] = math.log1p(math.sqrt(0.75))
    host[:, 2::3] = math.log1p(math.sqrt(0.75))
    mel = host.to(DEV)
    for min_strength, cents in ((0.5, 50.0), (float(np.nextafter(np.float32(0.5), np.float32(1.0))), 0.0)):
        (c, s), = run_entries(mel, False, [9], 5, 2, 14, parts=2, min_strength=min_strength)[2]
        assert float(s) == 0.5 and float(c) == cents, (min_strength, float(c), float(s))
    # a strength that is no float32: with min_strength the float32 next to it, the double decides, not the rounded output
    host = placed_frames(1, 36, 9, 3)
    host[:, 1::3] += 0.4
    mel = host.to(DEV)
    (mc, ms), = metrics.stream_tuning([host])
    (c, s), = run_entries(mel, False, [9], 5, 2, 14, parts=2)[2]
    s32 = float(s)
    assert abs(float(c)) > 1.0 and abs(float(ms) - s32) > 1e-11 and abs(float(ms) - s32) <= STRENGTH_BOUND
    (c_eq, s_eq), = run_entries(mel, False, [9], 5, 2, 14, parts=2, min_strength=s32)[2]
    assert float(s_eq) == s32 and (float(c_eq) == 0.0) == (float(ms) < s32) and float(c_eq) in (0.0, float(c))


def test_no_power_gives_zeros():
    (c, s), = run_entries(torch.zeros((2, 36, 70), device=DEV), False, [70], 5, 2, 75, parts=2)[2]
    assert not bool(c.any()) and not bool(s.any())


# ---- 3. state and refusals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x77])
def test_guarded_state_and_outputs_over_a_poisoned_fresh_state(fill):
    """frames_before == 0 reads nothing of the state and writes it whole: three fill bytes give the same outputs and the same state."""
    for P, fm in ((36, True), (288, False)):
        host = torch.cat([random_frames(3, P, 41, 9), placed_frames(3, P, 20, 4)], dim=2)
        mel = (host.transpose(1, 2) if fm else host).contiguous().to(DEV)
        want = offline(mel, fm, 5, 2, 2)
        for cuts in (cut_by(PATTERN, 61), [0, 61], [3, 58]):         # (the first piece leaves most rows of the ring untouched by frames)
            got, state, meter = run_entries(mel, fm, cuts, 5, 2, 5 + 61, 2, fill=fill)
            for name, a, b in zip(OUT_NAMES, got, want):
                assert torch.equal(a, b), (name, cuts)
            clean = run_entries(mel, fm, cuts, 5, 2, 5 + 61, 2)
            assert torch.equal(state, clean[1]) and torch.equal(meter[-1][0], clean[2][-1][0])
            rows = state[:3 * 66 * 96].view(torch.float64).view(3, 66, 12)
            assert not bool(rows[:, 61:].any())                      # the rows no frame has reached: zeros, whatever the fill


def _stats(mel, state, R=1, P=36, T=10, first=0, n_new=3, before=0, ring=8, parts=3, compression=0, min_strength=0.0, nbytes=None, null=()):
    L = _lib.lib()
    out = torch.zeros((2, R), device=DEV)
    return L.ake_stream_frame_stats_f32(None if "mel" in null else mel.data_ptr(), 0, R, P, T, first, n_new, before, ring, parts, compression, min_strength,
                                        None if "state" in null else state.data_ptr(), state.numel() if nbytes is None else nbytes,
                                        None if "cents" in null else out[0].data_ptr(), None if "strength" in null else out[1].data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)


def _score(state, outs, R=1, ring=8, frames=8, wf=5, sf=2, first=0, k=1, sharpness=10.0, nbytes=None, null=()):
    L = _lib.lib()
    prof, sig = device_profile(), sig_table()
    ptrs = [None if name in null else o.data_ptr() for name, o in zip(OUT_NAMES, outs)]
    return L.ake_stream_profile_emissions_f32(None if "state" in null else state.data_ptr(), state.numel() if nbytes is None else nbytes, R, ring, frames,
                                              wf, sf, first, k, None if "profiles" in null else prof.data_ptr(), sharpness,
                                              None if "sig" in null else sig.data_ptr(), *ptrs, torch.cuda.current_stream().cuda_stream)


def test_refusals_launch_nothing():
    L = _lib.lib()
    assert L.ake_stream_profile_state_bytes(0, 8) == 0 and L.ake_stream_profile_state_bytes(65536, 8) == 0 and L.ake_stream_profile_state_bytes(1, 0) == 0
    mel = torch.rand((1, 36, 10), device=DEV)
    mel38 = torch.rand((1, 38, 10), device=DEV)
    need = state_bytes(1, 8)
    state = torch.zeros(need, dtype=torch.uint8, device=DEV)
    outs = [o.t for o in new_outputs(1, 4, False)]
    nan = float("nan")
    codes = []

    def all_refusals():
        s = lambda **kw: codes.append((("stats", tuple(kw)), _stats(mel, state, **kw)))
        for null in ("mel", "state", "cents", "strength"):
            s(null=(null,))
        for kw in (dict(R=0), dict(R=65536), dict(ring=0), dict(first=-1), dict(n_new=-1), dict(first=8, n_new=3), dict(first=11, n_new=0), dict(before=-1),
                   dict(parts=0), dict(parts=4), dict(compression=-1), dict(compression=3), dict(min_strength=nan), dict(T=0)):
            s(**kw)
        codes.append((("stats", "pitches"), _stats(mel38, state, P=38)))
        codes.append((("stats", "pitches of the tuning part alone"), _stats(mel38, state, P=38, parts=2)))
        s(nbytes=need - 1)
        e = lambda **kw: codes.append((("score", tuple(kw)), _score(state, outs, **kw)))
        for null in ("state", "profiles", "sig") + OUT_NAMES:
            e(null=(null,))
        for kw in (dict(R=0), dict(R=65536), dict(ring=4), dict(wf=0), dict(sf=0), dict(k=-1), dict(first=-1), dict(sharpness=0.0), dict(sharpness=-1.0),
                   dict(sharpness=nan), dict(frames=-1),
                   dict(frames=6, first=1),                          # window 1 ends at frame 7: not yet in the ring
                   dict(frames=9, k=2),                              # window 1 needs frames up to 7; window 0 begins at 0 < 9 - 8: no longer there
                   dict(ring=7, frames=13, first=1, k=4)):           # a piece of 7 into a ring of 7 behind 6 frames (wf 5, sf 2): window 1 is gone
            e(**kw)
        e(nbytes=need - 1)

    assert launched(all_refusals) == {}
    for (what, rc) in codes:
        want = AKE_ERR_WORKSPACE if "nbytes" in what[1] else AKE_ERR_UNSUPPORTED if "pitches" in str(what[1]) else AKE_ERR_INVALID
        assert rc == want, (what, rc, L.ake_last_error())
    torch.cuda.synchronize()
    assert not bool(state.any())                                     # and nothing was written


def test_no_new_frames_and_no_new_windows_launch_nothing():
    mel = torch.rand((1, 36, 10), device=DEV)
    state = torch.full((state_bytes(1, 8),), 0x5A, dtype=torch.uint8, device=DEV)
    outs = [o.t for o in new_outputs(1, 0, False)]
    codes = []
    assert launched(lambda: codes.extend([_stats(mel, state, n_new=0), _stats(mel, state, n_new=0, before=5, parts=2), _score(state, outs, k=0),
                                          _score(state, outs, k=0, frames=0)])) == {}
    assert codes == [0, 0, 0, 0]
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all())
    ok = []
    assert launched(lambda: ok.extend([_stats(mel, state, n_new=8), _score(state, [o.t for o in new_outputs(1, 2, False)], k=2)])) == \
        {"stream_frame_stats_kernel": 1, "stream_profile_score_kernel": 1}
    assert ok == [0, 0]


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------

def schedule_irregular(n=N45):
    out, left = list(IRREGULAR), n - sum(IRREGULAR)
    while left > 0:
        out.append(min(SR, left))
        left -= out[-1]
    return out


@pytest.fixture(scope="module")
def recordings():
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7))]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


@pytest.fixture(scope="module")
def est_net():
    gold = load_golden("pcnet_trained.npz")
    opt = Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return ake_amd.KeyEstimator(net.to(DEV).eval(), SR, 5)


@pytest.fixture(scope="module")
def est_none():
    return ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)


def run_streams(audio, schedule, streams, time_axis=1):
    """Push `audio` in the chunks of `schedule` into every stream in turn, then finish -> per stream its updates and the frames it had
    after each of them."""
    src, at = audio.to(DEV), 0
    ups, counts = [[] for _ in streams], [[] for _ in streams]
    for m in schedule:
        for s, u, c in zip(streams, ups, counts):
            u.append(s.push(src.narrow(time_axis, at, m)))
            c.append(s.F)
        at += m
    assert at == audio.shape[time_axis]
    for s, u, c in zip(streams, ups, counts):
        u.append(s.finish())
        c.append(s.F)
    torch.cuda.synchronize()
    return ups, counts


def joined(ups, name):
    return torch.cat([getattr(u, name) for u in ups], dim=1)


def check_profile_stream(s, ups, counts, lag, sf, compression="log", meter=True):
    """Every field of every update against the two entries called by hand on the stream's own frames (pitch-major here, whatever the
    stream's transform wrote), the joined windows against ake_amd.profile_emissions on them, and the smoother's outputs against its
    entries on the stream's own emissions."""
    L = _lib.lib()
    frames = s.frames.contiguous()
    R, P, T = frames.shape
    assert T == counts[-1]
    stream = torch.cuda.current_stream().cuda_stream
    ring = WF + T                                                    # fits a push of any length (a long chunk is several pieces of the stream)
    state = torch.empty(state_bytes(R, ring), dtype=torch.uint8, device=DEV)
    prof, sig = device_profile(), sig_table()
    mode = metrics.PROFILE_COMPRESSIONS.index(compression)
    F = W = 0
    tuning = (torch.zeros(R, device=DEV), torch.zeros(R, device=DEV))
    for u, F_new in zip(ups, counts):
        m = F_new - F
        if meter and m:
            tuning = (torch.empty(R, device=DEV), torch.empty(R, device=DEV))
        _lib.check(L.ake_stream_frame_stats_f32(frames.data_ptr(), 0, R, P, T, F, m, F, ring, 3 if meter else 1, mode, 0.0, state.data_ptr(),
                                                state.numel(), tuning[0].data_ptr(), tuning[1].data_ptr(), stream), "ake_stream_frame_stats_f32")
        F = F_new
        k = track_counts(F, WF, sf) - W
        outs = [o.t for o in new_outputs(R, k, False)]
        _lib.check(L.ake_stream_profile_emissions_f32(state.data_ptr(), state.numel(), R, ring, F, WF, sf, W, k, prof.data_ptr(), 10.0,
                                                      sig.data_ptr(), *[o.data_ptr() if k else None for o in outs], stream),
                   "ake_stream_profile_emissions_f32")
        assert u.first_window == W and u.windows == k and u.genre is None
        W += k
        for name, field, o in zip(OUT_NAMES, ("key", "emissions", "key_id", "confidence", "tonic", "tonic_id", "signature_id"), outs):
            assert torch.equal(getattr(u, field), o), (name, F)
        if meter:
            assert torch.equal(u.tuning_cents, tuning[0]) and torch.equal(u.tuning_strength, tuning[1]), F
        else:
            assert u.tuning_cents is None and u.tuning_strength is None
    Wt = track_counts(T, WF, sf)
    assert W == Wt and sum(u.windows for u in ups) == Wt
    c, e, kid, conf = ake_amd.profile_emissions(frames, WF, sf, compression=compression)
    assert torch.equal(joined(ups, "emissions"), e) and torch.equal(joined(ups, "key_id"), kid)
    assert torch.equal(joined(ups, "key"), c) and torch.equal(joined(ups, "confidence"), conf)
    if meter:
        mc, ms = metrics.estimate_tuning(frames.cpu())
        assert float(ms.min()) >= 0.05
        assert float((ups[-1].tuning_cents.cpu().double() - mc).abs().max()) <= CENTS_BOUND
        assert float((ups[-1].tuning_strength.cpu().double() - ms).abs().max()) <= STRENGTH_BOUND
    if s.smooth:
        check_smoother(s, ups, Wt, lag)


def check_smoother(s, ups, W, lag):
    """filtered / smooth_key_id / posteriors / smooth_confidence / log_likelihood: the two smoother entries alone, on the stream's own
    joined emissions, to the bit."""
    L = _lib.lib()
    emis = joined(ups, "emissions").contiguous()
    R = emis.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    filt, path = torch.empty_like(emis), torch.empty((R, W), dtype=torch.int32, device=DEV)
    st = torch.empty(max(L.ake_key_stream_state_bytes(R, lag), 16), dtype=torch.uint8, device=DEV)
    k_out = C.c_int(-1)
    _lib.check(L.ake_key_stream_step_f32(emis.data_ptr(), R, W, 0, lag, 1, s.trans.data_ptr(), None, st.data_ptr(), st.numel(), filt.data_ptr(),
                                         path.data_ptr(), C.byref(k_out), stream), "ake_key_stream_step_f32")
    assert k_out.value == W
    assert torch.equal(joined(ups, "filtered"), filt) and torch.equal(joined(ups, "smooth_key_id"), path)
    if not s.posteriors:
        return
    post, pp, ll = torch.empty_like(emis), torch.empty((R, W), device=DEV), torch.empty((R, W), device=DEV)
    pst = torch.empty(L.ake_key_stream_posteriors_state_bytes(R, lag), dtype=torch.uint8, device=DEV)
    _lib.check(L.ake_key_stream_posteriors_f32(emis.data_ptr(), filt.data_ptr(), R, W, 0, lag, 1, s.trans.data_ptr(), None, path.data_ptr(),
                                               pst.data_ptr(), pst.numel(), post.data_ptr(), pp.data_ptr(), ll.data_ptr(), C.byref(k_out), stream),
               "ake_key_stream_posteriors_f32")
    torch.cuda.synchronize()
    for name, want in (("posteriors", post), ("smooth_confidence", pp), ("log_likelihood", ll)):
        assert torch.equal(joined(ups, name), want), name


@pytest.fixture(scope="module")
def profile_streams(est_none, est_net, recordings):
    """method="profile" with the smoother, the posteriors and the meter, on the estimator without a net (5 s and 1 s strides) and on one
    with a net (1 s), side by side on the irregular schedule: shared below and left unchanged."""
    streams = [est_none.stream(2, stride_seconds=5.0, lag_windows=3, keep_frames=True, method="profile", posteriors=True, tuning_meter=True),
               est_none.stream(2, stride_seconds=1.0, lag_windows=3, keep_frames=True, method="profile", posteriors=True, tuning_meter=True),
               est_net.stream(2, stride_seconds=1.0, lag_windows=6, keep_frames=True, method="profile", tuning_meter=True)]
    ups, counts = run_streams(recordings, schedule_irregular(), streams)
    return list(zip(streams, ups, counts))


@pytest.mark.parametrize("which, lag, sf", [(0, 3, 25), (1, 3, 5), (2, 6, 5)])
def test_profile_stream_equals_the_entries_by_hand(profile_streams, which, lag, sf):
    s, ups, counts = profile_streams[which]
    assert s.cache is None and s.net_ws is None and s.stats_state.numel() == state_bytes(2, WF + s.max_mel)
    check_profile_stream(s, ups, counts, lag, sf)
    assert any(u.windows and not u.smooth_key_id.shape[1] for u in ups)                  # the lag shows
    assert torch.equal(profile_streams[1][0].frames, profile_streams[2][0].frames)       # side by side, with and without a net: the same frames


@pytest.mark.parametrize("stride", [5.0, 1.0])
def test_profile_stream_against_the_offline_track(profile_streams, est_none, recordings, stride):
    s, ups, _ = profile_streams[0 if stride == 5.0 else 1]
    tr = est_none.track(recordings.to(DEV), stride_seconds=stride, method="profile")
    times = torch.cat([u.times for u in ups])
    assert joined(ups, "key").shape[1] == tr.key.shape[1] == (7 if stride == 5.0 else 31) and torch.equal(times, tr.times)
    # compression "log": a window's chroma x_j is a sum of P * wf / 12 log-magnitudes, each within d = 5e-4 of the offline frame's (the
    # transform's bound); with S = sum_j x_j, |x_j / S - x'_j / S'| <= |x_j - x'_j| / S + x'_j |S - S'| / (S S') <= 2 P wf d / S
    sf = int(round(stride * 5))
    S = s.frames.double().unfold(2, WF, sf).sum(dim=(1, 3))                                # (R, W): the windows' chroma totals
    bound = 2 * 288 * WF * TRANSFORM_BOUND / S
    diff = (joined(ups, "key").double() - tr.key.double()).abs().amax(dim=2)
    agree = float((joined(ups, "key_id") == tr.key_id).float().mean())
    print(f"\n  STREAM profile stride {stride} | chroma against the offline track: largest {float(diff.max()):.2e}, largest diff / bound "
          f"{float((diff / bound).max()):.2e}; key labels agree on {agree:.3f} of {tr.key_id.numel()} windows")
    assert bool((diff <= bound).all())


def test_int16_chunks_and_a_48k_stereo_source(est_none, recordings):
    pcm = (recordings * 32767).round().to(torch.int16)
    a = est_none.stream(2, stride_seconds=5.0, keep_frames=True, method="profile", tuning_meter=True, lag_windows=3)
    b = est_none.stream(2, stride_seconds=5.0, keep_frames=True, method="profile", tuning_meter=True, lag_windows=3)
    (ua,), (ca,) = run_streams(pcm, schedule_irregular(), [a])
    (ub,), _ = run_streams(ake_amd.pcm16_to_float(pcm), schedule_irregular(), [b])
    check_profile_stream(a, ua, ca, 3, 25)
    for name in ("key", "emissions", "key_id", "filtered", "smooth_key_id"):
        assert torch.equal(joined(ua, name), joined(ub, name)), name
    assert torch.equal(ua[-1].tuning_cents, ub[-1].tuning_cents)
    # 48 kHz stereo, 20 s, the mean of the channels: the carried resampler stands in front of the history
    n = 20 * 48000
    t = torch.arange(n, dtype=torch.float64, device=DEV) / 48000
    left = sum(torch.sin(2 * math.pi * f * t) for f in (220.0, 277.18, 329.63)) / 3
    right = sum(torch.sin(2 * math.pi * f * t) for f in (196.0, 246.94, 392.0)) / 3
    src = torch.stack([torch.stack([left, right]), torch.stack([right, 0.5 * left])]).float()     # (2, 2, n)
    s48 = est_none.stream(2, stride_seconds=1.0, keep_frames=True, method="profile", tuning_meter=True, lag_windows=2, source_rate=48000,
                          source_channels=2, channel=-1)
    (u48,), (c48,) = run_streams(src, [1, 4799, 48000, 0, 100000, n - 152800], [s48], time_axis=2)
    assert s48.frames.shape[2] == 1 + (20 * SR) // HOP == 101
    check_profile_stream(s48, u48, c48, 2, 5)
    assert joined(u48, "key").shape[1] == 6 and bool((joined(u48, "key_id") >= 0).all())


def test_smooth_false_still_has_emissions_and_options_are_checked(est_none, est_net, recordings):
    s = est_none.stream(2, smooth=False, method="profile", compression="power", profiles="temperley", profile_sharpness=4.0, keep_frames=True)
    (ups,), (counts,) = run_streams(recordings[:, :20 * SR], [20 * SR], [s])
    assert all(u.emissions is not None and u.filtered is None and u.smooth_key_id is None and u.tuning_cents is None for u in ups)
    c, e, k, f = ake_amd.profile_emissions(s.frames, WF, 25, profiles="temperley", compression="power", sharpness=4.0)
    assert torch.equal(joined(ups, "emissions"), e) and torch.equal(joined(ups, "key_id"), k) and e.shape[1] == 2
    one = ake_amd.stream.StreamUpdate.concat(ups)
    assert one.windows == 2 and one.tuning_cents is None
    for kw in (dict(method="profile", signature_weight=0.5), dict(method="profile", profile_sharpness=0.0), dict(method="profile", compression="sqrt"),
               dict(method="profile", profiles="nobody"), dict(method="chroma"), dict(tuning="auto"), dict(tuning_meter=True, tuning_min_strength=float("nan"))):
        with pytest.raises(ValueError):
            est_net.stream(2, **kw)
    with pytest.raises(ValueError, match="tuning_meter"):
        est_none.stream(2, method="profile", tuning=3.0)
    with pytest.raises(ValueError):
        est_none.stream(2)                                           # method="net" needs the net


# ---- 5. launch sets ------------------------------------------------------------------------------------------------------------------------

def test_launch_sets(est_net, est_none, recordings):
    short = recordings[:, :30 * SR]
    schedule = [10 * SR, 0, 10 * SR, 100, 10 * SR - 100]
    runs = {}
    for name, est, kw in (("net", est_net, {}), ("net+meter", est_net, dict(tuning_meter=True, keep_frames=True)),
                          ("profile", est_none, dict(method="profile")), ("profile+meter", est_none, dict(method="profile", tuning_meter=True))):
        s = est.stream(2, **kw)
        out = {}
        runs[name] = (launched(lambda: out.update(r=run_streams(short, schedule, [s]))), s, out["r"][0][0], out["r"][1][0])
    plain, meter = runs["net"][0], runs["net+meter"][0]
    assert not set(plain) & NEW_KERNELS and {"key_emissions_kernel", "key_stream_step_kernel"} <= set(plain)
    assert all(u.tuning_cents is None and u.tuning_strength is None for u in runs["net"][2])
    counts = runs["net+meter"][3]
    with_frames = sum(1 for a, b in zip([0] + counts[:-1], counts) if b > a)
    assert 0 < with_frames < len(counts)                             # the schedule has pieces without a new frame
    assert meter == {**plain, "stream_frame_stats_kernel": with_frames}          # one more launch per piece that has new frames, nothing else
    for name in ("profile", "profile+meter"):
        got = runs[name][0]
        assert not set(got) & NET_ONLY and all(k in PROFILE_STREAM or k.startswith("cqt_") for k in got), got
        assert got["stream_frame_stats_kernel"] == with_frames and got["stream_profile_score_kernel"] == sum(1 for u in runs[name][2] if u.windows)
        assert set(got) - NEW_KERNELS <= set(plain)
    assert runs["profile"][0] == runs["profile+meter"][0]            # the meter rides in the profile method's frame launch
    # the meter's values on the net stream: the entry by hand on the stream's frames, and the offline estimate at the end
    s, ups, counts = runs["net+meter"][1:]
    L = _lib.lib()
    frames = s.frames.contiguous()
    state = torch.empty(state_bytes(2, 1), dtype=torch.uint8, device=DEV)
    F, last = 0, (torch.zeros(2, device=DEV), torch.zeros(2, device=DEV))
    for u, F_new in zip(ups, counts):
        if F_new > F:
            last = (torch.empty(2, device=DEV), torch.empty(2, device=DEV))
        _lib.check(L.ake_stream_frame_stats_f32(frames.data_ptr(), 0, 2, 288, frames.shape[2], F, F_new - F, F, 1, 2, 0, 0.0, state.data_ptr(), state.numel(),
                                                last[0].data_ptr(), last[1].data_ptr(), torch.cuda.current_stream().cuda_stream), "ake_stream_frame_stats_f32")
        F = F_new
        assert torch.equal(u.tuning_cents, last[0]) and torch.equal(u.tuning_strength, last[1])
    mc, ms = metrics.estimate_tuning(frames.cpu())
    assert float((ups[-1].tuning_cents.cpu().double() - mc).abs().max()) <= CENTS_BOUND
    assert float((ups[-1].tuning_strength.cpu().double() - ms).abs().max()) <= STRENGTH_BOUND
