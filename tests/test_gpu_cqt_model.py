"""ROUNDING (GPU): the CQT kernels against the float64 model of their own algorithm (oracle/cqt_multirate_oracle.py).

tests/test_gpu_cqt.py holds the kernels to the direct-form specification, where the multirate *design* costs up to 1.6e-4 of the peak
and the tolerance is 5e-4 of the tensor's peak.  Against the model of the algorithm the plan builds there is no design error left, only
rounding, so the kernels are held here to a bound thousands of times tighter, per element:

    e[k, t] = | expm1(out[k, t]) - |C_model[k, t]| | / F_k,      F_k = max|y| sqrt(N_k) / 2      (M.err_full_scale)

Every tolerance is computed at test time FROM THE MODEL, never from what the kernels give:

    tol = 4 * max over the clips of the case of  e(model in the engine's reduced precision, model in float64)

with ``dtype=float32`` for engines 1 and 2 (exact-f32 bank), ``dtype=float32, split_bf16=True`` for engine 3, the per-clip-hop path and
the frames-major path, and ``stages=4`` on top for engine 5.  Factor 4: a kernel sums in another order than numpy (MFMA blocks of 4 or 32
taps, packed FMA pairs), which moves a rounding error by a small factor, not by an order of magnitude.  The reduced-precision model
includes the float32 ``log(1 + x)`` of the output, which is the floor for small amplitudes.  Each test prints the measured e and its tol
(run with -s); DESIGN.md section 2 records them.
"""
import functools

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, synthetic
from ake_amd.cqt import CQTPlan
from oracle import cqt_multirate_oracle as M

pytestmark = pytest.mark.gpu
SR, HOP, DEV = 22050, 4410, "cuda:0"
F32 = dict(dtype=np.float32)
MODE = {1: F32, 2: F32, 3: dict(dtype=np.float32, split_bf16=True), 5: dict(dtype=np.float32, split_bf16=True, stages=4)}
FACTOR = 4.0
AMPS = (2.0 ** -12, 1.0, 2.0 ** 10)


# ---- the model side ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def model(sr=SR, n_bins=288, bpo=36, q_mode=0, half_len=23, beta=8.0):
    return M.MultirateCQT(sr, n_bins, bpo, None, q_mode, half_len, beta)


@functools.lru_cache(maxsize=None)
def plan(sr=SR, hop=HOP, n_bins=288, bpo=36, engine=0, q_mode=0, half_len=0, beta=0.0):
    return CQTPlan(sr, hop, n_bins, bpo, q_mode=q_mode, device=DEV, engine=engine, decim_half_len=half_len, decim_beta=beta)


def mode_key(mode):
    return tuple(sorted((k, str(v)) for k, v in mode.items()))


class Clip:
    """One clip at amplitude 1 with its model results cached; ``amp`` evaluates it at a power-of-two amplitude (the float64 model,
    float32 decimators and the bf16 split are exactly invariant under powers of two, so only the log is redone)."""

    def __init__(self, y, mdl, hop, frames=None):
        self.y, self.mdl, self.hop, self.frames = np.asarray(y, np.float64), mdl, int(hop), frames
        self._c = {}

    def complex(self, mode=None):
        key = mode_key(mode or {})
        if key not in self._c:
            self._c[key] = self.mdl.cqt_complex(self.y, self.hop, frames=self.frames, **(mode or {}))
        return self._c[key]

    def model_err(self, mode, amp=1.0):
        """e(reduced-precision model, float64 model) at amplitude ``amp``, (n_bins, T)."""
        lm = M.logmag(amp * self.complex(mode), np.float32)
        return M.err_full_scale(np.expm1(lm.astype(np.float64)), amp * self.complex(), amp * self.y, self.mdl.lengths)

    def gpu_err(self, out, amp=1.0):
        """e(kernel output (n_bins, T) log-magnitudes, float64 model)."""
        out = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
        ref = amp * self.complex()
        assert out.shape == ref.shape, (out.shape, ref.shape)
        assert np.isfinite(out).all()
        return M.err_full_scale(np.expm1(out.astype(np.float64)), ref, amp * self.y, self.mdl.lengths)


def assert_within(label, clips, outs, mode, amp=1.0):
    """outs[i]: the kernels' (n_bins, T_i) for clips[i].  tol from the model over the clips of the case; prints both figures."""
    tol = FACTOR * max(float(c.model_err(mode, amp).max()) for c in clips)
    errs = [float(c.gpu_err(o, amp).max()) for c, o in zip(clips, outs)]
    worst = int(np.argmax(errs))
    print(f"\n{label}: max e = {errs[worst]:.3e} (clip {worst}), tol = {tol:.3e}")
    assert errs[worst] <= tol, (label, worst, errs[worst], tol)
    return errs[worst], tol


def batch_of(ys, amp=1.0, n_max=None, fill=0.0):
    n_max = n_max or max(len(y) for y in ys)
    rows = np.full((len(ys), n_max), fill, np.float32)
    for i, y in enumerate(ys):
        rows[i, :len(y)] = (amp * np.asarray(y)).astype(np.float32)
    return torch.from_numpy(rows).to(DEV), torch.tensor([len(y) for y in ys], dtype=torch.int64, device=DEV)


def f32(y):
    """The clip as the kernels receive it (float32 samples), back in float64 for the model."""
    return np.asarray(y, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def probe_clips(seconds=3):
    P = M.probe_set(SR * seconds, SR, HOP)
    return {name: Clip(f32(y), model(), HOP) for name, y in P.items()}


def frames_of(n, hop):
    return 1 + n // hop


# ---- probe set x engines x amplitude classes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("amp", AMPS)
@pytest.mark.parametrize("engine", [1, 2, 3, 5])
def test_probe_set(engine, amp):
    """Bin-centre tones, tones in the decimators' transition bands and above the top bin, a treble tone 80 dB under a bass tone, impulses
    at the clip's ends, around a frame centre and on a cascade tick boundary, DC, a chirp, white noise: 3 s each, all in one call."""
    clips = list(probe_clips().values())
    audio, _ = batch_of([c.y for c in clips], amp)
    out = plan(engine=engine).logmag(audio)
    assert out.shape == (len(clips), 288, frames_of(SR * 3, HOP))
    assert_within(f"probe set, engine {engine}, amplitude {amp:g}", clips, out, MODE[engine], amp)


@pytest.mark.parametrize("engine", [1, 2, 3, 5])
def test_batch_17_and_a_full_length_clip(engine):
    """17 clips leave a 16-clip wave with one live row; one clip of 15 s is the BASELINE shape (76 frames)."""
    names = list(probe_clips())
    clips = [probe_clips()[names[(5 * i) % len(names)]] for i in range(17)]
    audio, _ = batch_of([c.y for c in clips])
    out = plan(engine=engine).logmag(audio)
    assert_within(f"batch 17, engine {engine}", clips, out, MODE[engine])
    rng = np.random.default_rng(3)
    y = f32(synthetic.make_clip(7)[0] + rng.normal(0.0, 0.05, synthetic.N_SAMPLES))
    clip = Clip(y, model(), HOP)
    out = plan(engine=engine).logmag(batch_of([y])[0])
    assert out.shape == (1, 288, 76)
    assert_within(f"15 s clip, engine {engine}", [clip], out, MODE[engine])


# ---- decimator lengths 15 and 31, beta 6 ------------------------------------------------------------------------------------------------

DECIM_PROBES = ("white", "chirp", "transition1_edge", "transition2_above", "tone_low", "bass_treble", "impulse_tick", "impulse_last", "tone_bursts")


def decim_clips(half_len, beta, hop=HOP):
    P = M.probe_set(SR * 3, SR, HOP)
    return [Clip(f32(P[k]), model(half_len=half_len, beta=beta), hop) for k in DECIM_PROBES]


def kernels_of(fn):
    _lib.prof_enable("", True)
    try:
        _lib.prof_results()
        fn()
        torch.cuda.synchronize()
        return set(_lib.prof_results())
    finally:
        _lib.prof_enable("", False)


@pytest.mark.parametrize("half_len,beta,engines", [(15, 8.0, (1, 2, 3)), (23, 6.0, (1, 2, 3, 5)), (31, 8.0, (0, 1))])
def test_decimator_lengths(half_len, beta, engines):
    """ake_cqt_config::decim_half_len 15 and 31 and decim_beta: cqt_cascade_kernel<8, ...>, cqt_decimate_kernel<8> and <16>.  A 63-tap
    decimator does not fit the fused cascade: engine 0 resolves to 1 (one cqt_decimate_kernel per stage, no cascade), 2 and 3 are refused."""
    clips = decim_clips(half_len, beta)
    audio, _ = batch_of([c.y for c in clips])
    for engine in engines:
        p = plan(engine=engine, half_len=half_len, beta=beta)
        out = p.logmag(audio)
        assert_within(f"half_len {half_len} beta {beta}, engine {engine}", clips, out, MODE[engine or 1])
        names = kernels_of(lambda: p.logmag(audio))
        if half_len == 31 or engine == 1:
            assert "cqt_decimate_kernel" in names and "cqt_bank_kernel" in names and "cqt_cascade_kernel" not in names, names
        else:
            assert "cqt_cascade_kernel" in names and "cqt_decimate_kernel" not in names, names
    if half_len == 31:
        for engine in (2, 3, 5):
            with pytest.raises(_lib.AkeError):
                CQTPlan(SR, HOP, 288, 36, device=DEV, engine=engine, decim_half_len=31)


def test_per_clip_hops_with_the_31_tap_decimator():
    """cqt_cascade_kernel<8, ..., true, true>: the per-clip-hop cascade at decim_half_len 15."""
    P = M.probe_set(SR * 3, SR, HOP)
    hops = [559, 75, 4410, 1001]
    ys = [f32(P[k][:n]) for k, n in zip(("white", "chirp", "transition1_edge", "bass_treble"), (SR * 3, 40000, SR * 3, 50001))]
    clips = [Clip(y, model(half_len=15), h) for y, h in zip(ys, hops)]
    audio, lens = batch_of(ys)
    p = plan(hop=1, engine=3, half_len=15)
    out = p.logmag_hops(audio, torch.tensor(hops, dtype=torch.int32), lens, out_frames=592)
    outs = [out[i, :, :frames_of(len(y), h)] for i, (y, h) in enumerate(zip(ys, hops))]
    assert_within("per-clip hops, half_len 15", clips, outs, MODE[3])
    for i, o in enumerate(outs):
        assert torch.all(out[i, :, o.shape[1]:] == 0)


# ---- every phase table ---------------------------------------------------------------------------------------------------------------

def noise_and_tone(n, seed, sr=SR):
    rng = np.random.default_rng(seed)
    return f32(rng.normal(0.0, 0.2, n) + 0.4 * np.sin(2 * np.pi * (sr / 4.0) * np.arange(n) / sr + seed))


def test_every_phase_table_of_the_any_hop_plan():
    """Odd hops: t * hop mod 128 visits all 128 phases of the deepest octave (and every phase of the others) within 128 frames.  Ragged
    lengths, 592 output frames, every clip close to 592 frames of its own."""
    cases = [(75, 44100), (177, 100000), (559, 330000), (13, 7000), (337, 150001)]
    for hop, n in cases:
        assert hop % 2 == 1 and 128 <= frames_of(n, hop) <= 592
    # noise + tone, and on top the probe set's tone bursts: low-octave tones switching on and off inside every window, which follow the
    # window position to 2 / N_k ~ 1e-4 of full scale per sample -- a table one phase off is a window one sample off
    ys = [f32(noise_and_tone(n, 10 + i) + M.probe_set(n, SR, HOP)["tone_bursts"]) for i, (_, n) in enumerate(cases)]
    clips = [Clip(y, model(), hop) for y, (hop, _) in zip(ys, cases)]
    audio, lens = batch_of(ys, fill=np.nan)                                # what follows a clip in its row is never read
    out = ake_amd.cqt.get_any_hop_plan(SR, 288, device=DEV).logmag_hops(audio, torch.tensor([h for h, _ in cases], dtype=torch.int32), lens,
                                                                        out_frames=592)
    outs = [out[i, :, :frames_of(n, hop)] for i, (hop, n) in enumerate(cases)]
    assert_within("any-hop plan, all phases", clips, outs, MODE[3])
    for i, o in enumerate(outs):
        assert torch.all(out[i, :, o.shape[1]:] == 0)


@pytest.mark.parametrize("hop", [4410, 4411, 2205, 512, 64])
def test_fixed_hop_phase_tables(hop):
    """hop_twos 1, 0, 0, 9, 6: a fixed-hop plan holds nph = 2^o >> min(hop_twos, o) tables per octave and indexes them by phase >> shift."""
    ys = [noise_and_tone(SR * 3 // 2, 20), f32(noise_and_tone(SR * 3 // 2, 21) + M.probe_set(SR * 3 // 2, SR, HOP)["tone_bursts"])]
    clips = [Clip(y, model(), hop) for y in ys]
    audio, _ = batch_of(ys)
    for engine in (2, 3):
        out = plan(hop=hop, engine=engine).logmag(audio)
        assert_within(f"hop {hop}, engine {engine}", clips, out, MODE[engine])


# ---- lengths and segment boundaries ------------------------------------------------------------------------------------------------------

LENGTHS = (1, 2, 47, 48, 511, 512, 513, 3583, 3584, 3585, 4095, 4096, 4097, HOP - 1, HOP, HOP + 1)


def length_clip(n):
    y = np.random.default_rng(n).normal(0.0, 0.3, n)
    y[-1] = 1.0                                                            # the last sample is heard
    return f32(y)


@pytest.mark.parametrize("engine", [3, 5])
def test_lengths_as_one_ragged_batch(engine):
    ys = [length_clip(n) for n in LENGTHS]
    clips = [Clip(y, model(), HOP) for y in ys]
    audio, lens = batch_of(ys, fill=np.nan)
    out = plan(engine=engine).logmag(audio, lengths=lens, out_frames=3)
    outs = [out[i, :, :frames_of(len(y), HOP)] for i, y in enumerate(ys)]
    assert_within(f"ragged lengths, engine {engine}", clips, outs, MODE[engine])
    for i, o in enumerate(outs):
        assert torch.all(out[i, :, o.shape[1]:] == 0)


@pytest.mark.parametrize("engine", [1, 2, 3])
def test_lengths_each_alone(engine):
    """The fixed-hop engines 1 and 2 take equal lengths only; every length as a call of its own."""
    clips, outs = [], []
    for n in LENGTHS:
        y = length_clip(n)
        clips.append(Clip(y, model(), HOP))
        outs.append(plan(engine=engine).logmag(batch_of([y])[0])[0])
    assert_within(f"single lengths, engine {engine}", clips, outs, MODE[engine])


def cascade_segments(n, n_stage, ticks=4096):
    """Full-rate sample at which each cascade segment after the first begins (fill_cascade_on in csrc/cqt.hip): the frontier starts at
    -512, a tick is 4096 samples, the ticks are dealt to min(4, ticks) segments."""
    lag = 16 if n_stage == 1 else 24
    total = -(-(n + (25 + lag) * 2 ** n_stage + 512 + 512) // ticks)
    per_seg = -(-total // max(1, min(total, 4)))
    return [k * ticks - 512 for k in range(per_seg, total, per_seg)]


@pytest.mark.parametrize("engine", [1, 2, 3, 5])
def test_impulses_on_cascade_segment_boundaries(engine):
    """A segment's workgroup warms its LDS history up over 3 ticks before the first tick it owns: an impulse on the boundary, one sample
    before and one after it, must come through every level exactly as in a single pass."""
    n = SR * 3
    bounds = cascade_segments(n, 7)
    assert len(bounds) == 3 and all((b + 512) % 4096 == 0 and 0 < b < n for b in bounds)
    ys = []
    for d in (-1, 0, 1):
        y = np.zeros(n)
        y[[b + d for b in bounds]] = (1.0, -0.5, 0.75)
        ys.append(y)
    clips = [Clip(y, model(), HOP) for y in ys]
    # an impulse alone has rounding error in one product per sum: the class tolerance comes from the same clips plus a noise floor
    noisy = [f32(y + np.random.default_rng(7 + i).normal(0.0, 0.05, n)) for i, y in enumerate(ys)]
    clips += [Clip(y, model(), HOP) for y in noisy]
    audio, _ = batch_of([c.y for c in clips])
    out = plan(engine=engine).logmag(audio)
    assert_within(f"segment boundaries, engine {engine}", clips, out, MODE[engine])


# ---- other geometries -----------------------------------------------------------------------------------------------------------------

GEOMETRIES = {
    "44k1_8oct": (dict(sr=44100, hop=8820, n_bins=288), (1, 2, 3, 5)),
    "22k05_7oct": (dict(sr=22050, hop=4410, n_bins=252), (1, 2, 3, 5)),
    "11k025_6oct": (dict(sr=11025, hop=2205, n_bins=216), (1, 2, 3, 5)),          # engine 5's lower limit
    "44k1_9oct": (dict(sr=44100, hop=8820, n_bins=324), (1, 2)),                   # engine 3 stops at 8 octaves
    "bpo12_hop512": (dict(sr=22050, hop=512, n_bins=84, bpo=12), (1, 2, 3, 5)),
    "q_mode1": (dict(sr=22050, hop=4410, n_bins=288, q_mode=1), (1, 2, 3, 5)),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_other_geometries(name):
    geo, engines = GEOMETRIES[name]
    sr, hop = geo["sr"], geo["hop"]
    mdl = model(sr, geo["n_bins"], geo.get("bpo", 36), geo.get("q_mode", 0))
    n = 2 * sr
    P = M.probe_set(n, sr, hop, geo["n_bins"], geo.get("bpo", 36))
    ys = [f32(P[k]) for k in ("white", "chirp", "transition1_edge", "tone_low", "impulse_centre_p1")]
    clips = [Clip(y, mdl, hop) for y in ys]
    audio, _ = batch_of(ys)
    for engine in engines:
        out = plan(engine=engine, **geo).logmag(audio)
        assert_within(f"{name}, engine {engine}", clips, out, MODE[engine])


# ---- positions beyond 2^24 --------------------------------------------------------------------------------------------------------------

def test_sample_positions_beyond_2_to_24():
    """cascade_level decides whether to store a decimated sample with float arithmetic on its full-rate position, which is not exact past
    2^24 samples (12.7 min at 22.05 kHz; whole songs are what --frames 0 is for).  One clip of 2^24 + 3 * 4410 + 7 samples, a tone and then
    noise in the last second; the last frames (their windows straddle and pass 2^24) against the model, at the fixed hop and at the
    whole-song hop n // 592 + 1."""
    n = 2 ** 24 + 3 * HOP + 7
    rng = np.random.default_rng(24)
    y = 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / SR)
    y[-SR:] += rng.normal(0.0, 0.3, SR)
    y = f32(y)
    audio = torch.from_numpy(y.astype(np.float32)).to(DEV)[None]
    T = frames_of(n, HOP)
    assert (T - 1) * HOP > 2 ** 24 + 2 * HOP
    frames = np.arange(T - 12, T)                                          # the last 8 and those around sample 2^24 (frame 3804.4): one range
    assert frames[0] * HOP < 2 ** 24 - 7 * HOP
    out = plan(engine=3).logmag(audio)[0]
    assert out.shape == (288, T)
    clip = Clip(y, model(), HOP, frames=frames)
    assert_within("beyond 2^24, hop 4410", [clip], [out[:, frames]], MODE[3])
    del out
    hop = n // 592 + 1
    Th = frames_of(n, hop)
    assert hop % 2 == 1 and Th == 592
    fr = np.arange(Th - 8, Th)
    out = ake_amd.cqt.get_any_hop_plan(SR, 288, device=DEV).logmag_hops(audio, torch.tensor([hop], dtype=torch.int32), out_frames=592)[0]
    assert_within(f"beyond 2^24, hop {hop}", [Clip(y, model(), hop, frames=fr)], [out[:, fr]], MODE[3])


# ---- stale workspace ---------------------------------------------------------------------------------------------------------------------

def frames_major(p, audio, ws=None):
    """ake_cqt_logmag_frames_major_f32 -> (B, T, n_bins); ``ws``: a workspace tensor, or the plan's own."""
    B, n = audio.shape
    if ws is None:
        ws = p._workspace(_lib.lib().ake_cqt_workspace_bytes(p.handle, B, n))
    out = torch.empty((B, p.num_frames(n), p.n_bins), dtype=torch.float32, device=DEV)
    L = _lib.lib()
    assert L.ake_cqt_frames_major_supported(p.handle) == 1
    assert ws.numel() >= L.ake_cqt_workspace_bytes(p.handle, B, n)
    _lib.check(L.ake_cqt_logmag_frames_major_f32(p.handle, audio.data_ptr(), B, n, audio.stride(0), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 torch.cuda.current_stream().cuda_stream), "ake_cqt_logmag_frames_major_f32")
    return out


def stale_cases():
    """(label, plan factory, {"test" | "dirty" | "other": call}): the call under test; the same entry point on the same batch and n_max with
    other audio (noise at amplitude 2^10), other lengths and other hops; and on another batch and n_max, which carves the workspace up
    differently, as a plan that serves changing batch shapes from one buffer does."""
    rng = np.random.default_rng(99)
    B, n = 5, 30011

    def noise(b, m, amp):
        return batch_of([f32(amp * rng.normal(0.0, 0.3, m)) for _ in range(b)])[0]

    audio, dirty, other = noise(B, n, 1.0), noise(B, n, 1024.0), noise(B + 1, n - 1003, 1024.0)

    def ints(v, dtype=torch.int64):
        return torch.tensor(v, dtype=dtype, device=DEV)

    lens, lens_dirty, lens_other = ints([n, 4409, 20000, 513, 29999]), ints([n, n - 1, 9000, n, 25000]), ints([n - 1003, 777, 20000, 1, 15000, 28000])
    hops, hops_dirty = ints([75, 559, 4410, 51, 1001], torch.int32), ints([51, 64, 333, 4410, 52], torch.int32)
    hops_other = ints([4410, 75, 77, 1001, 64, 559], torch.int32)
    # 12 bins per octave (librosa's default 84 bins): the windows (2 uh + 1 = 187 taps) start ppad - uh = 19 words into a row, the least
    # of the geometries tested, and the stored range around a frame centre has the least slack over the taps that carry weight
    geos = (("", {}), (", 12 bins per octave, hop 512", dict(hop=512, n_bins=84, bpo=12)))
    cases = []
    for tag, geo in geos:
        for e in (1, 2, 3, 5):
            cases.append((f"logmag, engine {e}{tag}", lambda e=e, geo=geo: plan(engine=e, **geo),
                          {"test": lambda p: p.logmag(audio), "dirty": lambda p: p.logmag(dirty), "other": lambda p: p.logmag(other)}))
        for e in (3, 5):
            cases.append((f"ragged, engine {e}{tag}", lambda e=e, geo=geo: plan(engine=e, **geo),
                          {"test": lambda p: p.logmag(audio, lengths=lens), "dirty": lambda p: p.logmag(dirty, lengths=lens_dirty),
                           "other": lambda p: p.logmag(other, lengths=lens_other)}))
            cases.append((f"frames-major, engine {e}{tag}", lambda e=e, geo=geo: plan(engine=e, **geo),
                          {"test": lambda p: frames_major(p, audio), "dirty": lambda p: frames_major(p, dirty),
                           "other": lambda p: frames_major(p, other)}))
        hop_geo = dict(geo, hop=1)
        cases.append((f"logmag_hops{tag}", lambda hop_geo=hop_geo: plan(engine=3, **hop_geo),
                      {"test": lambda p: p.logmag_hops(audio, hops, lens, out_frames=592),
                       "dirty": lambda p: p.logmag_hops(dirty, hops_dirty, lens_dirty, out_frames=592),
                       "other": lambda p: p.logmag_hops(other, hops_other, lens_other, out_frames=500)}))
    return cases


def test_stale_workspace_content_is_never_read():
    """The ABI gives the workspace no content contract and the levels are stored sparsely (only near frame centres), so a sample that a
    call reads but did not store itself shows up exactly here: after a call with other audio, lengths and hops on the same workspace --
    of the same shape, and of another shape -- every entry point gives the bits it gives on a freshly zeroed workspace.  Real stale
    content only: part of the per-clip-hop workspace holds row indices, which arbitrary bit patterns would turn into wild addresses."""
    failed = []
    for label, make, calls in stale_cases():
        p = make()
        nbytes = 0
        for c in calls.values():                                           # the largest workspace any of the three asks for
            p._ws = None
            c(p)
            nbytes = max(nbytes, p._ws.numel())
        p._ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        fresh = calls["test"](p).clone()
        assert torch.isfinite(fresh).all(), label
        for how in ("dirty", "other"):
            p._ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
            calls[how](p)
            assert p._ws.numel() == nbytes, label
            again = calls["test"](p)
            if not torch.equal(fresh, again):
                moved = torch.nonzero((fresh != again).flatten(1).any(1)).flatten().tolist()
                failed.append((label, how, "clips", moved, float((fresh - again).abs().max())))
        p._ws = None
    print("\nstale workspace:", failed or "every entry point bit-identical")
    assert not failed, failed


# ---- frames-major ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", [3, 5])
def test_frames_major_equals_the_transposed_output(engine):
    """[clip][frame][bin] as the bank writes it against [clip][bin][frame] through the transpose: bit for bit, on the probe batch and at
    batch 17 (tests/test_gpu_pipeline.py has the one shape the pipeline uses, 64 x 15 s on engine 3)."""
    clips = list(probe_clips().values())
    p = plan(engine=engine)
    for ys in ([c.y for c in clips], [clips[(5 * i) % len(clips)].y for i in range(17)]):
        audio, _ = batch_of(ys)
        ref = p.logmag(audio)
        ws = torch.empty(_lib.lib().ake_cqt_workspace_bytes(p.handle, audio.shape[0], audio.shape[1]), dtype=torch.uint8, device=DEV)
        got = frames_major(p, audio, ws)
        assert torch.equal(got.transpose(1, 2), ref)
