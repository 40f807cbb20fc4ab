"""GPU: the tuning estimate and the retuner against their float64 models (ake_tuning_estimate_f32, ake_retune_f32 / ake_retune_pcm16_f32),
and ``tuning=`` through KeyEstimator.__call__ and KeyEstimator.track.

The three tolerances are four times the worst figure measured against the float64 models on these inputs (profiles/tuning.md):
    CENTS_TOL, STRENGTH_TOL   the estimate's two outputs; the sums run in double, so what is left is the float32 rounding of the outputs
    RETUNE_E                  the retuner's samples, as a share of sum|h| * max|x| (64 float32 fmaf per sample)
The issue's ceilings are asserted beside them: CENTS_TOL < 0.05 cents, RETUNE_E * sum|h| < 1e-5.
"""
import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics, synthetic
from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle
from test_gpu_pipeline import default_opt
from test_tuning_host import HOP, N15, SR, harmonic_clip, oracle_logmag
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AKE_ERR_INVALID, AKE_ERR_WORKSPACE, AKE_ERR_UNSUPPORTED = -1, -4, -5

CENTS_TOL = 4 * 1.61e-6          # measured worst 1.61e-06 cents (half a float32 ulp at 50 is 1.9e-06)
STRENGTH_TOL = 4 * 7.92e-9       # measured worst 7.92e-09
RETUNE_E = 4 * 3.30e-7           # measured worst 3.30e-07 of sum|h| * max|x| (sum|h| = 2.355)
NEW_KERNELS = ("tuning_sums_kernel", "tuning_finish_kernel", "retune_kernel", "retune_pcm16_kernel")
CHUNK = 64                       # frames per block of tuning_sums_kernel
TILE, BLOCK = 2048, 16384        # samples per staged tile and per workgroup of retune_kernel


def sum_abs_h():
    """max over the filter phases of sum_j |h(f - j)| on the retuner's table."""
    G = np.abs(metrics.retune_table().astype(np.float64))
    Z, R = metrics.RETUNE_ZEROS, metrics.RETUNE_RESOLUTION
    r = np.arange(R + 1)
    return float(max(sum(G[rr + m * R] for m in range(Z) if rr + m * R < len(G)) + sum(G[m * R - rr] for m in range(1, Z + 1)) for rr in r))


def test_the_tolerances_meet_the_ceilings():
    assert CENTS_TOL < 0.05 and RETUNE_E * sum_abs_h() < 1e-5, (CENTS_TOL, RETUNE_E * sum_abs_h())


@pytest.fixture(scope="module")
def net(gold_default):
    n = ake_amd.PitchClassNet(288, 12, 2, 7, default_opt())
    n.load_state_dict(golden_state_dict(gold_default), strict=True)
    return n.to(DEV).eval()


@pytest.fixture(scope="module")
def est(net):
    return ake_amd.KeyEstimator(net, SR, 5)


# ---- the estimate kernel against the model ----

def run_estimate(mel, frames_major, counts=None, min_strength=0.0, fill=0x5A, ws_bytes=None):
    """ake_tuning_estimate_f32 with guarded outputs and a guarded workspace of `fill` bytes -> (rc, cents, strength)."""
    L = ake_amd._lib.lib()
    B, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    need = L.ake_tuning_workspace_bytes(B, T)
    assert need > 0
    ws, ws_check = guarded(need if ws_bytes is None else ws_bytes, fill)
    cents, strength = GuardedTensor((B,)), GuardedTensor((B,))
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    rc = L.ake_tuning_estimate_f32(mel.data_ptr(), 1 if frames_major else 0, B, P, T, cnt.data_ptr() if cnt is not None else None,
                                   float(min_strength), cents.t.data_ptr(), strength.t.data_ptr(), ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)
    ws_check("tuning workspace"); cents.check("cents"); strength.check("strength")
    return rc, cents.t.clone(), strength.t.clone()


def check_estimate(mel_pt, counts, what):
    """mel_pt (B, P, T) float32 on the host: both layouts against the float64 model on the same float32 numbers."""
    want_c, want_s = metrics.estimate_tuning(mel_pt, counts)
    for fm in (False, True):
        mel = (mel_pt.transpose(1, 2) if fm else mel_pt).contiguous().to(DEV)
        rc, c, s = run_estimate(mel, fm, counts)
        assert rc == 0, ake_amd._lib.lib().ake_last_error()
        ec, es = float((c.cpu().double() - want_c).abs().max()), float((s.cpu().double() - want_s).abs().max())
        print(f"estimate {what} {'frames-major' if fm else 'pitch-major'}: cents {ec:.2e}, strength {es:.2e}")
        assert ec <= CENTS_TOL and es <= STRENGTH_TOL, (what, fm, ec, es)
        rc2, c2, s2 = run_estimate(mel, fm, counts, fill=0xFF)                          # a poisoned workspace, and a rerun
        assert rc2 == 0 and torch.equal(c, c2) and torch.equal(s, s2)
    return want_c, want_s


@pytest.mark.parametrize("P, T", [(288, 1), (288, 7), (288, 76), (288, CHUNK + 1), (288, 1501), (36, 76)])
def test_estimate_kernel_equals_the_model(P, T):
    g = torch.Generator().manual_seed(100 + T + P)
    mel = torch.rand((3, P, T), generator=g) * 3.0
    check_estimate(mel, None, f"{P}x{T}")
    _, s = check_estimate(mel, [T, (T + 1) // 2, 0], f"{P}x{T} ragged")
    assert float(s[2]) == 0.0


def test_estimate_kernel_on_a_real_transform(est):
    """Three detuned harmonic clips through the device CQT: the kernel against the model on that transform, and against the truth."""
    truth = (-38.0, 22.0, 47.0)
    audio = torch.from_numpy(np.stack([harmonic_clip(10 + i, c) for i, c in enumerate(truth)]).astype(np.float32)).to(DEV)
    mel = est.plan.logmag(audio).cpu()
    want_c, _ = check_estimate(mel, None, "real log-CQT")
    assert float((want_c - torch.tensor(truth, dtype=torch.float64)).abs().max()) <= 3.0
    c, s = ake_amd.estimate_tuning(mel.to(DEV))
    assert float((c.cpu().double() - want_c).abs().max()) <= CENTS_TOL
    c0, s0 = ake_amd.estimate_tuning(mel.to(DEV), min_strength=2.0)                      # nothing is that strong: every row reports 0
    assert not bool(c0.any()) and torch.equal(s0, s)


def test_min_strength_is_decided_per_row_on_the_device():
    """A threshold between the strengths of two rows: the rows below it report 0 cents, the others their estimate, as the model says;
    the strengths themselves do not change.  Uniform input (strengths of a few hundredths) and rows of hand-set power (up to 1)."""
    g = torch.Generator().manual_seed(77)
    mel = torch.rand((4, 288, 40), generator=g) * 3.0
    mel[2, 1::3] += 1.5                                                                  # a clearly sharp row
    mel[3, 0::3], mel[3, 2::3] = 0.0, 0.0                                                # all power on position 1: strength 1
    _, strength = metrics.estimate_tuning(mel)
    order = torch.argsort(strength)
    assert float(strength[order[0]]) < 0.1 and float(strength[order[-1]]) > 0.999
    for lo, hi in zip(order[:-1], order[1:]):
        thr = 0.5 * (float(strength[lo]) + float(strength[hi]))
        want_c, want_s = metrics.estimate_tuning(mel, min_strength=thr)
        assert int((want_c == 0).sum()) == int((strength < thr).sum()) > 0 and int((want_c != 0).sum()) > 0
        for fm in (False, True):
            rc, c, s = run_estimate((mel.transpose(1, 2) if fm else mel).contiguous().to(DEV), fm, min_strength=thr)
            assert rc == 0
            assert torch.equal(c.cpu() == 0, want_c == 0), (thr, c, want_c)
            assert float((c.cpu().double() - want_c).abs().max()) <= CENTS_TOL and float((s.cpu().double() - want_s).abs().max()) <= STRENGTH_TOL


def test_estimate_kernel_refusals():
    L = ake_amd._lib.lib()
    mel = torch.rand((3, 288, 76), device=DEV)
    need = L.ake_tuning_workspace_bytes(3, 76)
    rc, c, s = run_estimate(mel, False, ws_bytes=need - 256)
    assert rc == AKE_ERR_WORKSPACE and b"workspace" in L.ake_last_error()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(s).all())                    # nothing ran
    assert L.ake_tuning_workspace_bytes(0, 76) == 0 and L.ake_tuning_workspace_bytes(3, 0) == 0
    out = torch.zeros(3, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.ake_tuning_estimate_f32(mel.data_ptr(), 0, 3, 287, 76, None, 0.0, out.data_ptr(), out.data_ptr(), ws.data_ptr(), need, stream) == AKE_ERR_UNSUPPORTED
    assert L.ake_tuning_estimate_f32(None, 0, 3, 288, 76, None, 0.0, out.data_ptr(), out.data_ptr(), ws.data_ptr(), need, stream) == AKE_ERR_INVALID
    with pytest.raises(ValueError):
        ake_amd.estimate_tuning(torch.rand((1, 37, 8), device=DEV))


# ---- the retune kernel against the model ----

def run_retune(x, lengths, cents):
    """ake_retune_f32 / ake_retune_pcm16_f32 on x (B, n) into poisoned, guarded buffers -> (y (B, width), n_out (B,))."""
    L = ake_amd._lib.lib()
    B, n = x.shape
    width = L.ake_retune_out_len(n)
    y, n_out = GuardedTensor((B, width)), GuardedTensor((B,), dtype=torch.int64)
    len_d = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    cents_d = torch.tensor(cents, dtype=torch.float32, device=DEV)
    fn = L.ake_retune_pcm16_f32 if x.dtype == torch.int16 else L.ake_retune_f32
    rc = fn(x.data_ptr(), B, n, x.stride(0), len_d.data_ptr(), cents_d.data_ptr(), y.t.data_ptr(), width, n_out.t.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ake_last_error()
    y.check("retuned audio"); n_out.check("retuned lengths")
    return y.t.clone(), n_out.t.clone()


RETUNE_CASES = [((0, 1, 63), (33.3, 50.0, -50.0)), ((64, 65, 1), (-17.3, 50.0, -50.0)), ((TILE - 1, TILE + 1, TILE), (50.0, -50.0, 33.3)),
                ((BLOCK - 1, BLOCK + 1, BLOCK), (-17.3, 33.3, 0.0)), ((3 * BLOCK + 59, 30011, BLOCK + 1), (50.0, -50.0, 0.0)),
                ((777, 20000, 4099), (0.0, -17.3, 33.3))]


@pytest.fixture(scope="module")
def retune_inputs():
    """For every case: float32 rows (B, n_max) with 7.0 behind every row's end, and the model's output on them."""
    cases = []
    for i, (lengths, cents) in enumerate(RETUNE_CASES):
        c32 = np.array(cents, dtype=np.float32)
        for l, c in zip(lengths, c32):                                                   # no length may sit on a rounding edge
            v = l * 2.0 ** (float(c) / 1200.0)
            assert c == 0 or l == 0 or abs(v - round(v)) > 1e-6, (l, c)
        g = torch.Generator().manual_seed(700 + i)
        x = torch.rand((3, max(lengths)), generator=g) * 2.0 - 1.0
        for b, l in enumerate(lengths):
            x[b, l:] = 7.0
        want, want_n = metrics.retune_reference(x.double().numpy(), c32, lengths)
        cases.append((x, lengths, cents, want, want_n))
    return cases


@pytest.mark.parametrize("case", range(len(RETUNE_CASES)))
def test_retune_kernel_equals_the_model(retune_inputs, case):
    x, lengths, cents, want, want_n = retune_inputs[case]
    y, n_out = run_retune(x.to(DEV), lengths, cents)
    assert n_out.cpu().tolist() == want_n.tolist()
    assert y.shape == want.shape
    got = y.cpu().double().numpy()
    bound = sum_abs_h() * 1.0                                                             # max|x| <= 1
    for b, (l, c) in enumerate(zip(lengths, cents)):
        no = int(want_n[b])
        assert not got[b, no:].any(), (case, b)                                          # zeros up to the poisoned buffer's width
        err = float(np.abs(got[b, :no] - want[b, :no]).max()) / bound if no else 0.0
        print(f"retune n {l} at {c:+.1f} cents: {no} samples, error {err:.2e} of sum|h| max|x|")
        assert err <= RETUNE_E, (case, b, err)
        if c == 0.0:
            assert torch.equal(y[b, :l].cpu(), x[b, :l])                                 # 0 cents: the input, bit for bit
    y2, n2 = run_retune(x.to(DEV), lengths, cents)
    assert torch.equal(y, y2) and torch.equal(n_out, n2)


@pytest.mark.parametrize("case", [1, 3, 4])
def test_retune_pcm16_equals_the_float_route(case):
    """int16 rows of odd stride with 32767 behind every row's end: the float route's bits on pcm16_to_float."""
    lengths, cents = RETUNE_CASES[case]
    n = max(lengths) | 1                                                                  # an odd row length, so an odd row stride
    g = torch.Generator().manual_seed(800 + case)
    pcm = torch.randint(-32768, 32768, (3, n), generator=g).to(torch.int16)
    pcm[0, :2] = torch.tensor([-32768, 32767], dtype=torch.int16)
    for b, l in enumerate(lengths):
        pcm[b, l:] = 32767
    pcm = pcm.to(DEV)
    y_pcm, n_pcm = run_retune(pcm, lengths, cents)
    y_f32, n_f32 = run_retune(ake_amd.pcm16_to_float(pcm), lengths, cents)
    assert torch.equal(y_pcm, y_f32) and torch.equal(n_pcm, n_f32)
    a, la = ake_amd.retune(pcm, torch.tensor(cents), torch.tensor(lengths))               # the package-level call, the same bits
    assert torch.equal(a, y_pcm) and torch.equal(la, n_pcm)


def test_retune_refusals():
    L = ake_amd._lib.lib()
    x, c, y = torch.zeros((2, 100), device=DEV), torch.zeros(2, device=DEV), torch.zeros((2, 200), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.ake_retune_out_len(100) == 103 and L.ake_retune_out_len(0) == 1 and L.ake_retune_out_len(-1) == -1
    assert L.ake_retune_f32(x.data_ptr(), 2, 100, 100, None, c.data_ptr(), y.data_ptr(), 102, None, stream) == AKE_ERR_INVALID
    assert L.ake_retune_f32(x.data_ptr(), 2, 100, 99, None, c.data_ptr(), y.data_ptr(), 200, None, stream) == AKE_ERR_INVALID
    assert L.ake_retune_f32(x.data_ptr(), 2, 100, 100, None, None, y.data_ptr(), 200, None, stream) == AKE_ERR_INVALID
    out, n_out = ake_amd.retune(torch.zeros((2, 0), device=DEV), 10.0)
    assert out.shape == (2, 1) and not bool(out.any()) and n_out.tolist() == [0, 0]


# ---- tuning=None changes nothing ----

def _launched(fn):
    ake_amd._lib.prof_enable("", True)
    try:
        fn()
        return {k: v[1] for k, v in ake_amd._lib.prof_results().items()}
    finally:
        ake_amd._lib.prof_enable("", False)


def test_without_tuning_the_calls_launch_what_their_entry_points_launch(net, est):
    """A __call__ and a track without tuning launch exactly the kernels of ake_pipeline_forward_f32 / ake_pipeline_track_f32 called by
    hand, as often, and none of the new ones; with tuning="auto" the new ones do show (the timer sees them)."""
    L = ake_amd._lib.lib()
    audio = synthetic.make_batch_device(range(3), torch.device(DEV))[0]
    long_audio = torch.cat([audio, audio, audio], dim=1)[:2].contiguous()                # 45 s
    est(audio); est.track(long_audio); torch.cuda.synchronize()                           # (handles, workspaces and weights exist)
    stream = torch.cuda.current_stream().cuda_stream
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)

    def by_hand():
        B, n = audio.shape
        ws = torch.empty(L.ake_pipeline_workspace_bytes(est.plan.handle, net.handle, B, n), dtype=torch.uint8, device=DEV)
        ake_amd._lib.check(L.ake_pipeline_forward_f32(est.plan.handle, net.handle, audio.data_ptr(), B, n, audio.stride(0), f32(B, 12).data_ptr(),
                                                      f32(B, 12).data_ptr(), f32(B, 11).data_ptr(), ws.data_ptr(), ws.numel(), stream), "forward")

    def track_by_hand():
        R, n = long_audio.shape
        W = (1 + n // HOP - 76) // 25 + 1
        ws = torch.empty(L.ake_pipeline_track_workspace_bytes(est.plan.handle, net.handle, R, n, 76, 25), dtype=torch.uint8, device=DEV)
        outs = [f32(R, W, 12), f32(R, W, 12), f32(R, W, 11), i32(R, W), i32(R, W), i32(R, W), f32(R, W), i32(R)]
        ake_amd._lib.check(L.ake_pipeline_track_f32(est.plan.handle, net.handle, long_audio.data_ptr(), R, n, long_audio.stride(0), 76, 25,
                                                    *[o.data_ptr() for o in outs], ws.data_ptr(), ws.numel(), stream), "track")

    plain = _launched(lambda: est(audio))
    assert plain and plain == _launched(by_hand) and not set(plain) & set(NEW_KERNELS), sorted(plain)
    plain_track = _launched(lambda: est.track(long_audio))
    assert plain_track and plain_track == _launched(track_by_hand) and not set(plain_track) & set(NEW_KERNELS), sorted(plain_track)
    auto = _launched(lambda: est(audio, tuning="auto"))
    assert {k: auto.get(k) for k in NEW_KERNELS} == {"tuning_sums_kernel": 1, "tuning_finish_kernel": 1, "retune_kernel": 1, "retune_pcm16_kernel": None}
    given = _launched(lambda: est(audio, tuning=12.5))
    assert {k: given.get(k) for k in NEW_KERNELS} == {"tuning_sums_kernel": None, "tuning_finish_kernel": None, "retune_kernel": 1, "retune_pcm16_kernel": None}
    assert torch.equal(est(audio)[1], est(audio, tuning=None)[1])


# ---- end to end ----

E2E_CENTS = (-38.0, 22.0, 47.0)
E2E_LENGTHS = (N15, N15 - 30011, N15 - 77777)


def test_auto_tuning_end_to_end_against_the_float64_chain(net, est, gold_default):
    """Three ragged detuned 15 s clips: KeyEstimator(tuning="auto") against metrics.estimate_tuning on the oracle CQT ->
    metrics.retune_reference -> the oracle CQT -> the float64 net, within the 1e-3 of the other end-to-end comparisons; and the retuned
    clips land nearer the in-tune clips' outputs than the detuned ones do.

    Under the default wrap_mode the padded frames take part in the time-circular convolutions, so outputs are only comparable at one
    buffer width.  The asserted comparison therefore runs every arm in a buffer of the retuned batch's width (78 frames): the call
    with tuning="auto", the detuned clips with their own lengths, and the in-tune clips -- the same notes and phases at rho times the
    length, which is what a tape played rho times too fast was recorded from.  Only the tuning and the row lengths differ.  Key and
    tonic are also asserted at the detuned clips' own geometry (76-frame buffers for the detuned and the in-tune clips cut to the
    detuned lengths), where the compensated arm alone carries the wider buffer; the genre figure there is printed only."""
    rows = np.zeros((3, N15))
    tuned = np.zeros((3, N15))
    for i, (c, n) in enumerate(zip(E2E_CENTS, E2E_LENGTHS)):
        rows[i, :n] = harmonic_clip(20 + i, c, n)
        tuned[i, :n] = harmonic_clip(20 + i, 0.0, n)
    lengths = torch.tensor(E2E_LENGTHS)
    audio = torch.from_numpy(rows.astype(np.float32)).to(DEV)
    got = est(audio, lengths, tuning="auto")
    # the float64 chain, on the float32 audio the device was given
    x64 = rows.astype(np.float32).astype(np.float64)
    mel = oracle_logmag(x64)
    T_in = [1 + n // HOP for n in E2E_LENGTHS]
    cents, _ = metrics.estimate_tuning(mel, T_in)
    dev_cents, _ = est.estimate_tuning(audio, lengths)
    print("estimates: float64 chain", [f"{float(c):+.3f}" for c in cents], "device", [f"{float(c):+.3f}" for c in dev_cents.cpu()])
    y, n_out = metrics.retune_reference(x64, cents.numpy(), E2E_LENGTHS)
    assert all(50 < int(n) % HOP < HOP - 50 for n in n_out), n_out                       # no retuned length sits on a hop boundary
    mel2 = torch.from_numpy(oracle_logmag(y))
    seq = torch.tensor([1 + int(n) // HOP for n in n_out])
    for b in range(3):
        mel2[b, :, int(seq[b]):] = 0.0
    assert mel2.shape[2] == 1 + y.shape[1] // HOP
    sd = golden_state_dict(gold_default, torch.float64)
    ref = pcnet_oracle.pcnet_forward(sd, mel2[:, None], seq)
    for name, a, b in zip(("key", "tonic", "genre"), got, ref):
        e = rel_err(a.cpu(), b)
        print(f"tuning=auto {name}: rel err vs the float64 chain {e:.2e}")
        assert e < 1e-3, (name, e)
    width = y.shape[1]
    original, wide, wide_tuned = np.zeros((3, width)), np.zeros((3, width)), np.zeros((3, width))
    for i, n in enumerate(n_out):
        original[i, :int(n)] = harmonic_clip(20 + i, 0.0, int(n))
    wide[:, :N15], wide_tuned[:, :N15] = rows, tuned
    on_dev = lambda x: torch.from_numpy(x.astype(np.float32)).to(DEV)
    in_tune = est(on_dev(original), torch.from_numpy(n_out))                             # 78-frame buffer, retuned lengths
    plain_wide = est(on_dev(wide), lengths)                                              # 78-frame buffer, detuned clips as they are
    in_tune_cut = est(on_dev(wide_tuned), lengths)                                       # 78-frame buffer, in-tune clips cut to the detuned lengths
    same_length = est(on_dev(tuned), lengths)                                            # 76-frame buffers
    plain = est(audio, lengths)
    dist = lambda u, v: float((u - v).abs().max())
    figures = {}
    for k, name in enumerate(("key", "tonic", "genre")):
        figures[name] = f = (dist(got[k], in_tune[k]), dist(plain_wide[k], in_tune[k]), dist(got[k], in_tune_cut[k]), dist(plain_wide[k], in_tune_cut[k]),
                             dist(got[k], same_length[k]), dist(plain[k], same_length[k]))
        print(f"{name}: distance to the in-tune clips' outputs, one buffer width: compensated {f[0]:.3e}, uncompensated {f[1]:.3e}; to the in-tune "
              f"clips cut to the detuned lengths, one buffer width: {f[2]:.3e}, {f[3]:.3e}; at the detuned clips' own geometry (76-frame buffers, "
              f"the compensated arm in 78): {f[4]:.3e}, {f[5]:.3e}")
    for name, f in figures.items():
        assert f[0] < f[1], (name, f)
        if name != "genre":
            assert f[4] < f[5], (name, f)


@pytest.fixture(scope="module")
def detuned_recordings():
    """Two modulating recordings of 75 s and 52 s, 41 cents sharp and 27 cents flat, with their annotations."""
    arrays, segments = synthetic.modulating_batch_arrays((3, 8), (75.0, 52.0))
    detune = np.repeat(2.0 ** (np.array([41.0, -27.0]) / 1200.0), np.diff(arrays["offsets"]))
    arrays["cps"] = arrays["cps"] * detune
    audio = ake_amd.synth_partials(device=DEV, **arrays)
    ann = ake_amd.KeyAnnotations.from_segments([[(s / SR, k) for s, k in segs] for segs in segments], SR, DEV)
    return audio, torch.as_tensor(arrays["n"], device=DEV), ann


def _same_track(a, b):
    assert len(a._tensors()) == len(b._tensors())
    for x, y in zip(a._tensors(), b._tensors()):
        assert (x is None and y is None) or torch.equal(x, y)
    assert torch.equal(a.times, b.times)


@pytest.mark.parametrize("mode", ["float32", "int16", "streams", "given"])
def test_track_with_tuning_equals_the_manual_chain(net, est, detuned_recordings, mode):
    """track(tuning="auto", smooth=True, posteriors=True) = estimate_tuning, retune, track(lengths=...) by hand, tensor for tensor; its
    score is metrics.track_score on the moved boundaries."""
    audio, lengths, ann = detuned_recordings
    if mode == "int16":
        audio = (audio * 32767.0).round().to(torch.int16)
    e = ake_amd.KeyEstimator(net, SR, 5, streams=2) if mode == "streams" else est
    kw = dict(smooth=True, posteriors=True)
    cents, strength = est.estimate_tuning(audio, lengths)
    print(f"{mode}: estimates", [f"{float(c):+.2f}" for c in cents.cpu()], "strength", [f"{float(s):.3f}" for s in strength.cpu()])
    assert float((cents.cpu() - torch.tensor([41.0, -27.0])).abs().max()) <= 3.0
    retuned, len2 = ake_amd.retune(audio, cents, lengths)
    want = est.track(retuned, lengths=len2, **kw)
    got = e.track(audio, lengths, tuning=cents.clone() if mode == "given" else "auto", **kw)
    e.join()
    assert torch.equal(got.tuning_cents, cents)
    assert got.tuning_strength is None if mode == "given" else torch.equal(got.tuning_strength, strength)
    assert want.tuning_cents is None and len(got._tensors()) == len(want._tensors()) + (1 if mode == "given" else 2)
    want.tuning_cents, want.tuning_strength = got.tuning_cents, got.tuning_strength
    _same_track(got, want)
    assert int(got.counts.min()) > 0
    score = got.score(ann)
    ref = metrics.track_score(got.smooth_key_id, got.counts, ann.seg_start, ann.seg_key, ann.seg_count, got.hop, got.window_frames,
                              got.stride_frames, tuning_cents=got.tuning_cents)
    for a, b in zip((score.truth, score.category, score.tally, score.changes), ref):
        assert torch.equal(a, b)
    rho0 = 2.0 ** (float(cents[0]) / 1200.0)
    assert abs(got.segments(0)[-1][1] * rho0 - want.times[int(got.counts[0]) - 1].item() - want.window_seconds / 2) < 1e-9


# ---- tuning with the estimator's other modes ----

@pytest.fixture(scope="module")
def ragged_detuned():
    """Three ragged detuned 15 s clips on the device."""
    rows = np.zeros((3, N15), dtype=np.float32)
    for i, (c, n) in enumerate(zip(E2E_CENTS, E2E_LENGTHS)):
        rows[i, :n] = harmonic_clip(30 + i, c, n)
    return torch.from_numpy(rows).to(DEV), torch.tensor(E2E_LENGTHS, device=DEV)


@pytest.mark.parametrize("mode", ["true_end", "frames0", "frames0_wide"])
def test_call_with_tuning_in_other_modes_equals_the_manual_chain(net, ragged_detuned, mode):
    """wrap_mode="true_end", frames=0 and frames=0 with window_size > 592 (the estimate's transform is then W frames wide):
    __call__(tuning="auto") = estimate_tuning, retune, __call__(lengths=...) by hand, bit for bit; a given tensor likewise."""
    audio, lengths = ragged_detuned
    e = {"true_end": lambda: ake_amd.KeyEstimator(net, SR, 5, wrap_mode="true_end"), "frames0": lambda: ake_amd.KeyEstimator(net, SR, 0),
         "frames0_wide": lambda: ake_amd.KeyEstimator(net, SR, 0, window_size=640)}[mode]()
    cents, strength = e.estimate_tuning(audio, lengths)
    print(f"{mode}: estimates", [f"{float(c):+.2f}" for c in cents.cpu()], "strength", [f"{float(s):.3f}" for s in strength.cpu()])
    assert float((cents.cpu() - torch.tensor(E2E_CENTS)).abs().max()) <= 3.0
    retuned, len2 = ake_amd.retune(audio, cents, lengths)
    want = e(retuned, len2)
    for got in (e(audio, lengths, tuning="auto"), e(audio, lengths, tuning=cents)):
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(want[1], e(audio, lengths)[1])


def test_call_with_tuning_on_stereo_audio_at_another_rate(net, est):
    """rate= and channel=: 48 kHz stereo, mixed down and resampled first, then estimated and retuned: the manual chain, bit for bit."""
    n48, lens = 15 * 48000, (15 * 48000, 13 * 48000 + 321)
    stereo = np.zeros((2, 2, n48), dtype=np.float32)
    for i, (c, n) in enumerate(zip((31.0, -44.0), lens)):
        y = harmonic_clip(40 + i, c, n, sr=48000)
        stereo[i, 0, :n], stereo[i, 1, :n] = y, 0.5 * y
    audio, lengths = torch.from_numpy(stereo).to(DEV), torch.tensor(lens, device=DEV)
    mono, len_mono = ake_amd.get_resampler(48000, SR, DEV)(audio, channel=-1, lengths=lengths)
    cents, strength = est.estimate_tuning(mono, len_mono)
    got_c, got_s = est.estimate_tuning(audio, lengths, rate=48000, channel=-1)
    assert torch.equal(got_c, cents) and torch.equal(got_s, strength)
    assert float((cents.cpu() - torch.tensor([31.0, -44.0])).abs().max()) <= 3.0
    want = est(*ake_amd.retune(mono, cents, len_mono))
    got = est(audio, lengths, rate=48000, channel=-1, tuning="auto")
    assert all(bool(torch.isfinite(b).all()) and torch.equal(a, b) for a, b in zip(got, want))


def test_a_given_tensor_is_stored_as_the_kernel_reads_it(est, detuned_recordings):
    """NaN and values beyond +-50 in a tensor of cents: the track carries what the audio was resampled by (0 and +-50)."""
    audio, lengths, _ = detuned_recordings
    tr = est.track(audio, lengths, tuning=torch.tensor([float("nan"), 80.0]))
    assert tr.tuning_cents.cpu().tolist() == [0.0, 50.0]
    want = est.track(*ake_amd.retune(audio, torch.tensor([0.0, 50.0]), lengths))
    assert torch.equal(tr.key, want.key) and torch.equal(tr.counts, want.counts)
    with pytest.raises(ValueError):
        est(audio, lengths, tuning=51.0)
