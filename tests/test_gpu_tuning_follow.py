"""GPU: a tuning that drifts.  ake_tuning_track_f32 (csrc/tuning.hip) and ake_retune_curve_f32 / ake_retune_curve_pcm16_f32 /
ake_retune_curve_positions (csrc/audio.hip) against their float64 models (metrics.tuning_track, metrics.retune_curve_reference,
metrics.retune_curve_positions), and KeyEstimator's tuning="follow" against the manual chain and against the truth of two drifting
recordings.

Every tolerance is four times the worst deviation measured on these very inputs (the figures are in profiles/tuning_follow.md), under
the ceilings of test_the_tolerances_meet_the_ceilings."""
import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics
from conftest import golden_state_dict
from test_gpu_pipeline import default_opt
from test_gpu_tuning import _launched, _same_track, sum_abs_h
from test_tuning_follow_host import HOP, KNOT_FIRST, KNOT_STEP, SF, SR, WF, drifting_clip, ramp_cents, sine_cents, window_centre_seconds
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AKE_ERR_INVALID, AKE_ERR_WORKSPACE, AKE_ERR_UNSUPPORTED = -1, -4, -5

TRACK_CENTS_TOL = 4 * 1.91e-6     # measured worst 1.91e-06 cents (half a float32 ulp at 50 is 1.9e-06)
TRACK_STRENGTH_TOL = 4 * 2.97e-8  # measured worst 2.97e-08 (half a float32 ulp below 1 is 3.0e-08)
POSITION_TOL = 4 * 1.82e-12       # measured worst 1.82e-12 samples (an ulp of a position near 40 000 is 7.3e-12)
CURVE_E = 4 * 3.23e-7             # measured worst 3.23e-07 of sum|h| * max|x| (sum|h| = 2.355)
TILE, BLOCK = 2048, 16384         # outputs per staged tile and per workgroup of retune_curve_kernel
TRACK_KERNELS = ("tuning_frame_sums_kernel", "tuning_windows_kernel", "tuning_curve_kernel")
CURVE_KERNELS = ("retune_curve_prefix_kernel", "retune_curve_kernel", "retune_curve_pcm16_kernel", "retune_curve_positions_kernel")


def test_the_tolerances_meet_the_ceilings():
    assert TRACK_CENTS_TOL < 0.05 and TRACK_STRENGTH_TOL < 1e-6 and POSITION_TOL < 1e-6 and CURVE_E * sum_abs_h() < 1e-5


# ---- the track kernel against the model ----

TRACK_MIN_STRENGTH = 0.1
TRACK_SHAPES = [(288, 1, 5, 1, None), (288, 7, 5, 2, None), (288, 76, 25, 5, None), (288, 131, 25, 5, [131, 76, 24, 0]), (36, 65, 1, 1, None),
                (288, 10, 25, 5, None)]


def drifting_mel(P, T, seed):
    """(4, P, T) float32: uniform noise, and on top of it power that sits at a phase of the three bin positions which moves with the
    frame: row 0 sweeps -45 .. 70 cents (it leaves the semitone, so its curve saturates), row 1 stays near 30, row 2 goes quiet in
    its middle third (weak windows), row 3 is noise alone (every window weak)."""
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand((4, P, T), generator=g) * 1.5
    t = torch.arange(T, dtype=torch.float64) / max(T - 1, 1)
    cents = torch.stack([-45.0 + 115.0 * t, 30.0 + 10.0 * torch.sin(7.0 * t), 45.0 - 80.0 * t, torch.zeros(T, dtype=torch.float64)])
    gain = torch.ones((4, T), dtype=torch.float64)
    gain[2, T // 3:2 * T // 3 + (T > 2)] = 0.0
    gain[3] = 0.0
    for j in range(3):
        w = 1.0 + torch.cos(2 * np.pi * (cents / 100.0 - j / 3.0))
        mel[:, j::3, :] += (gain * w)[:, None, :].float()
    return mel


def held_margins(cents, strength, n_win, thr):
    """How far the model's own numbers lie from a decision of the curve: the least |strength - thr| over the live windows, and the least
    distance of a step between two held values from the seam (50 mod 100)."""
    ms, mw = float("inf"), float("inf")
    for b in range(cents.shape[0]):
        n = int(n_win[b])
        s = strength[b, :n]
        if n:
            ms = min(ms, float((s - thr).abs().min()))
        strong = (s >= thr).tolist()
        held = [float(cents[b, w]) for w in range(n) if strong[w]]
        for a, c in zip(held[:-1], held[1:]):
            d = (c - a) % 100.0
            mw = min(mw, abs(d - 50.0))
    return ms, mw


def run_track(mel, frames_major, wf, sf, counts=None, min_strength=0.0, fill=0x5A, ws_bytes=None):
    """ake_tuning_track_f32 with guarded outputs and a guarded workspace of `fill` bytes -> (rc, cents_raw, strength, curve, counts)."""
    L = ake_amd._lib.lib()
    B, P, T = (mel.shape[0], mel.shape[2], mel.shape[1]) if frames_major else mel.shape
    W = L.ake_tuning_track_windows(T, wf, sf)
    need = L.ake_tuning_track_workspace_bytes(B, T, wf, sf)
    assert need > 0 and W == metrics.tuning_track_windows(T, wf, sf)
    ws, ws_check = guarded(need if ws_bytes is None else ws_bytes, fill)
    outs = [GuardedTensor((B, W)), GuardedTensor((B, W)), GuardedTensor((B, W)), GuardedTensor((B,), dtype=torch.int32)]
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    rc = L.ake_tuning_track_f32(mel.data_ptr(), 1 if frames_major else 0, B, P, T, cnt.data_ptr() if cnt is not None else None, wf, sf,
                                float(min_strength), *[o.t.data_ptr() for o in outs], ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream)
    ws_check("tuning track workspace")
    for o, what in zip(outs, ("cents_raw", "strength", "curve", "window_counts")):
        o.check(what)
    return (rc,) + tuple(o.t.clone() for o in outs)


@pytest.mark.parametrize("P, T, wf, sf, counts", TRACK_SHAPES)
def test_track_kernel_equals_the_model(P, T, wf, sf, counts):
    mel_pt = drifting_mel(P, T, 300 + T + wf)
    want = metrics.tuning_track(mel_pt, wf, sf, counts, TRACK_MIN_STRENGTH)
    ms, mw = held_margins(want[0], want[1], want[3], TRACK_MIN_STRENGTH)
    assert ms > 2 * TRACK_STRENGTH_TOL and mw > 2 * TRACK_CENTS_TOL, (ms, mw)            # the model leaves no recording out
    T_i = counts if counts is not None else [T] * 4
    assert want[3].tolist() == [0 if t == 0 else 1 if t < wf else 1 + (t - wf) // sf for t in T_i]
    for fm in (False, True):
        mel = (mel_pt.transpose(1, 2) if fm else mel_pt).contiguous().to(DEV)
        rc, c, s, curve, n_win = run_track(mel, fm, wf, sf, counts, TRACK_MIN_STRENGTH)
        assert rc == 0, ake_amd._lib.lib().ake_last_error()
        assert n_win.cpu().tolist() == want[3].tolist()
        ec, es, ek = (float((g.cpu().double() - w).abs().max()) if g.numel() else 0.0 for g, w in zip((c, s, curve), want))
        print(f"track {P}x{T} wf {wf} sf {sf} {'frames-major' if fm else 'pitch-major'}: cents {ec:.2e}, strength {es:.2e}, curve {ek:.2e}")
        assert ec <= TRACK_CENTS_TOL and es <= TRACK_STRENGTH_TOL and ek <= TRACK_CENTS_TOL, (fm, ec, es, ek)
        for b in range(4):                                                                # behind a recording's windows: zeros, and the held value
            n = int(want[3][b])
            assert not bool(c[b, n:].any()) and not bool(s[b, n:].any())
            assert bool((curve[b, n:] == (curve[b, n - 1] if n else 0.0)).all())
        assert float(curve.abs().max()) <= 50.0
        rc2, *again = run_track(mel, fm, wf, sf, counts, TRACK_MIN_STRENGTH, fill=0xFF)   # a poisoned workspace, and a rerun
        assert rc2 == 0 and all(torch.equal(a, b) for a, b in zip(again, (c, s, curve, n_win)))
        got = ake_amd.tuning_track(mel, wf, sf, counts, TRACK_MIN_STRENGTH, frames_major=fm)
        assert all(torch.equal(a, b) for a, b in zip(got, (c, s, curve, n_win)))


def test_track_kernel_follows_a_sweep_across_the_seam():
    """Row 0 of the drifting input sweeps -45 .. 70 cents: its curve rises, saturates at 50 and never jumps down a semitone."""
    mel = drifting_mel(288, 131, 431).to(DEV)
    _, strength, curve, _ = ake_amd.tuning_track(mel, 25, 5, min_strength=TRACK_MIN_STRENGTH)
    row = curve[0].cpu()
    assert float(row[0]) < -20.0 and float(row[-1]) == 50.0 and float((row[1:] - row[:-1]).min()) >= -0.5
    assert float((row[1:] - row[:-1]).max()) < 20.0


def test_track_kernel_refusals():
    L = ake_amd._lib.lib()
    mel = torch.rand((4, 288, 76), device=DEV)
    need = L.ake_tuning_track_workspace_bytes(4, 76, 25, 5)
    rc, c, s, curve, n_win = run_track(mel, False, 25, 5, ws_bytes=need - 256)
    assert rc == AKE_ERR_WORKSPACE and b"workspace" in L.ake_last_error()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(curve).all()) and bool((n_win == -1).all())     # nothing ran
    assert L.ake_tuning_track_workspace_bytes(0, 76, 25, 5) == 0 and L.ake_tuning_track_workspace_bytes(4, 76, 0, 5) == 0
    assert L.ake_tuning_track_windows(76, 25, 0) == -1 and L.ake_tuning_track_windows(0, 25, 5) == 0
    out, cnt = torch.zeros((4, 11), device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda m, P, wf, sf: L.ake_tuning_track_f32(m, 0, 4, P, 76, None, wf, sf, 0.0, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                                       cnt.data_ptr(), ws.data_ptr(), need, stream)
    launched = _launched(lambda: [
        (call(mel.data_ptr(), 287, 25, 5) == AKE_ERR_UNSUPPORTED) or pytest.fail("287 bins"),
        (call(None, 288, 25, 5) == AKE_ERR_INVALID) or pytest.fail("null"),
        (call(mel.data_ptr(), 288, 0, 5) == AKE_ERR_INVALID) or pytest.fail("wf 0"),
        (call(mel.data_ptr(), 288, 25, 0) == AKE_ERR_INVALID) or pytest.fail("sf 0")])
    assert not set(launched) & set(TRACK_KERNELS)
    with pytest.raises(ValueError):
        ake_amd.tuning_track(torch.rand((1, 37, 8), device=DEV), 5, 1)


# ---- the curve's positions against the model ----

def curve_cents(name, K):
    i = np.arange(K, dtype=np.float64)
    return {"constant": np.full(K, 20.0), "ramp": -35.0 + 70.0 * i / max(K - 1, 1), "alternating": np.where(i % 2 == 0, 50.0, -50.0),
            "nan80": np.array([np.nan, 80.0, -80.0, 12.5] * (K // 4 + 1))[:K], "zero": np.zeros(K), "one": np.full(K, 33.3),
            "flat50": np.full(K, -50.0)}[name].astype(np.float32)


POSITION_CASES = [("constant", 9, 2205, 4410), ("ramp", 9, 2205, 4410), ("alternating", 9, 2205, 4410), ("one", 1, 1000, 300),
                  ("ramp", 3, 55125, 4410), ("nan80", 9, 2205, 4410), ("alternating", 627, 32, 64)]
POSITION_N = 40000


def run_positions(index, cents, first, step, fill=0x5A, ws_bytes=None):
    L = ake_amd._lib.lib()
    B, m = index.shape
    K = cents.shape[1]
    need = L.ake_retune_curve_workspace_bytes(B, K)
    assert need > 0
    ws, ws_check = guarded(need if ws_bytes is None else ws_bytes, fill)
    pos = GuardedTensor((B, m), dtype=torch.float64)
    rc = L.ake_retune_curve_positions(cents.data_ptr(), B, K, cents.stride(0), first, step, index.data_ptr(), m, pos.t.data_ptr(), ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream().cuda_stream)
    ws_check("curve workspace"); pos.check("positions")
    return rc, pos.t.clone()


@pytest.mark.parametrize("name, K, first, step", POSITION_CASES)
def test_positions_equal_the_model(name, K, first, step):
    """Indices 0, both sides of every knot's output index and the last output of a row of 40 000 samples."""
    cents = curve_cents(name, K)
    knots = metrics.retune_curve_forward(torch.tensor(first + step * np.arange(K, dtype=np.float64)), cents, first, step)
    last = int(np.floor(float(metrics.retune_curve_forward(torch.tensor([float(POSITION_N)], dtype=torch.float64), cents, first, step)[0]))) - 1
    sides = torch.cat([torch.floor(knots), torch.floor(knots) + 1, torch.ceil(knots) - 1]).to(torch.int64)
    index = torch.unique(torch.cat([torch.tensor([0, last]), sides.clamp_min(0)]))[None]
    want = metrics.retune_curve_positions(index.double(), cents, first, step)
    rc, got = run_positions(index.to(DEV), torch.from_numpy(cents)[None].to(DEV), first, step)
    assert rc == 0, ake_amd._lib.lib().ake_last_error()
    err = float((got.cpu() - want).abs().max())
    print(f"positions {name} K {K} first {first} step {step}: {index.numel()} indices, worst {err:.2e} samples")
    assert err <= POSITION_TOL
    pkg = ake_amd.retune_curve_positions(index[0].to(DEV), torch.from_numpy(cents).to(DEV), first, step)
    assert torch.equal(pkg, got[0])
    rc2, again = run_positions(index.to(DEV), torch.from_numpy(cents)[None].to(DEV), first, step, fill=0xFF)
    assert rc2 == 0 and torch.equal(again, got)


# ---- the curve retuner against the model ----

# (lengths, knot_first, knot_step, K, the curve of every row)
CURVE_CASES = [((0, 1, 63), 0, 64, 3, ("ramp", "alternating", "nan80")),
               ((5000, 20000, 63), 150, 300, 68, ("alternating", "ramp", "constant")),
               ((40000, 20000, 5000), 32, 64, 627, ("alternating", "ramp", "nan80")),
               ((40000, 5000, 20000), 2205, 4410, 10, ("ramp", "zero", "alternating")),
               ((20000, 5000, 1), 55125, 4410, 3, ("ramp", "constant", "alternating")),
               ((20000, 40000, 63), 1000, 300, 1, ("one", "flat50", "zero"))]


def run_curve(x, lengths, cents, first, step, fill=0x5A, ws_bytes=None, poison=True):
    """ake_retune_curve_f32 / _pcm16_f32 on x (B, n) into poisoned, guarded buffers -> (rc, y (B, width), n_out (B,))."""
    L = ake_amd._lib.lib()
    B, n = x.shape
    K = cents.shape[1]
    width = L.ake_retune_out_len(n)
    need = L.ake_retune_curve_workspace_bytes(B, K)
    ws, ws_check = guarded(need if ws_bytes is None else ws_bytes, fill)
    y, n_out = GuardedTensor((B, width)), GuardedTensor((B,), dtype=torch.int64)
    len_d = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    fn = L.ake_retune_curve_pcm16_f32 if x.dtype == torch.int16 else L.ake_retune_curve_f32
    rc = fn(x.data_ptr(), B, n, x.stride(0), len_d.data_ptr(), cents.data_ptr(), K, cents.stride(0), first, step, y.t.data_ptr(), width,
            n_out.t.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    ws_check("curve workspace"); y.check("retuned audio"); n_out.check("retuned lengths")
    return rc, y.t.clone(), n_out.t.clone()


@pytest.fixture(scope="module")
def curve_inputs():
    """For every case: float32 rows (3, n_max) with 7.0 behind every row's end, the curves, and the model's output on them."""
    cases = []
    for i, (lengths, first, step, K, names) in enumerate(CURVE_CASES):
        cents = np.stack([curve_cents(nm, K) for nm in names])
        for l, c in zip(lengths, cents):                                                 # no K(n) may sit on a rounding edge
            v = float(metrics.retune_curve_forward(torch.tensor([float(l)], dtype=torch.float64), c, first, step)[0])
            assert l == 0 or not c.any() or abs(v - round(v)) > 1e-6, (l, v)              # (an all-zero curve is a copy: n_out = n)
        g = torch.Generator().manual_seed(900 + i)
        x = torch.rand((3, max(lengths)), generator=g) * 2.0 - 1.0
        for b, l in enumerate(lengths):
            x[b, l:] = 7.0
        want, want_n = metrics.retune_curve_reference(x.double().numpy(), cents, first, step, lengths)
        cases.append((x, lengths, cents, first, step, names, want, want_n))
    return cases


@pytest.mark.parametrize("case", range(len(CURVE_CASES)))
def test_curve_kernel_equals_the_model(curve_inputs, case):
    x, lengths, cents, first, step, names, want, want_n = curve_inputs[case]
    cents_d = torch.from_numpy(cents).to(DEV)
    rc, y, n_out = run_curve(x.to(DEV), lengths, cents_d, first, step)
    assert rc == 0, ake_amd._lib.lib().ake_last_error()
    assert n_out.cpu().tolist() == want_n.tolist() and y.shape == want.shape
    got = y.cpu().double().numpy()
    bound = sum_abs_h() * 1.0                                                             # max|x| <= 1
    for b, (l, nm) in enumerate(zip(lengths, names)):
        no = int(want_n[b])
        assert not got[b, no:].any(), (case, b)                                          # zeros up to the poisoned buffer's width
        err = float(np.abs(got[b, :no] - want[b, :no]).max()) / bound if no else 0.0
        print(f"curve case {case} row {b}: n {l}, {nm}, step {step}: {no} samples, error {err:.2e} of sum|h| max|x|")
        assert err <= CURVE_E, (case, b, err)
        if nm == "zero":
            assert no == l and torch.equal(y[b, :l].cpu(), x[b, :l])                     # an all-zero curve: the input, bit for bit
        if nm in ("constant", "one", "flat50") and l:                                    # a constant curve: the one-ratio retuner
            one, n_one = ake_amd.retune(x[b:b + 1, :].to(DEV), float(cents[b, 0]), torch.tensor([l]))
            apart = float((one[0, :no] - y[b, :no]).abs().max()) / bound
            print(f"curve case {case} row {b}: against ake_amd.retune at {float(cents[b, 0]):+.1f} cents: {apart:.2e} of sum|h| max|x|")
            assert int(n_one[0]) == no and apart <= CURVE_E
    rc2, y2, n2 = run_curve(x.to(DEV), lengths, cents_d, first, step, fill=0xFF)          # a poisoned workspace, and a rerun
    assert rc2 == 0 and torch.equal(y, y2) and torch.equal(n_out, n2)
    a, la = ake_amd.retune_curve(x.to(DEV), cents_d, first, step, torch.tensor(lengths))
    assert torch.equal(a, y) and torch.equal(la, n_out)


def test_the_long_row_crosses_tile_and_workgroup_edges(curve_inputs):
    assert int(curve_inputs[2][7][0]) > 2 * BLOCK + TILE and int(curve_inputs[3][7][0]) > 2 * BLOCK


@pytest.mark.parametrize("case", [1, 2, 3])
def test_curve_pcm16_equals_the_float_route(case):
    """int16 rows of odd stride with 32767 behind every row's end: the float route's bits on pcm16_to_float."""
    lengths, first, step, K, names = CURVE_CASES[case]
    cents = torch.from_numpy(np.stack([curve_cents(nm, K) for nm in names])).to(DEV)
    n = max(lengths) | 1
    g = torch.Generator().manual_seed(950 + case)
    pcm = torch.randint(-32768, 32768, (3, n), generator=g).to(torch.int16)
    pcm[0, :2] = torch.tensor([-32768, 32767], dtype=torch.int16)
    for b, l in enumerate(lengths):
        pcm[b, l:] = 32767
    pcm = pcm.to(DEV)
    rc_p, y_pcm, n_pcm = run_curve(pcm, lengths, cents, first, step)
    rc_f, y_f32, n_f32 = run_curve(ake_amd.pcm16_to_float(pcm), lengths, cents, first, step)
    assert rc_p == 0 and rc_f == 0 and torch.equal(y_pcm, y_f32) and torch.equal(n_pcm, n_f32)
    a, la = ake_amd.retune_curve(pcm, cents, first, step, torch.tensor(lengths))
    assert torch.equal(a, y_pcm) and torch.equal(la, n_pcm)


def test_curve_refusals():
    """Each refusal returns its code and launches nothing."""
    L = ake_amd._lib.lib()
    x, y = torch.zeros((2, 100), device=DEV), torch.zeros((2, 200), device=DEV)
    c = torch.zeros((2, 4), device=DEV)
    idx, pos = torch.zeros((2, 5), dtype=torch.int64, device=DEV), torch.zeros((2, 5), dtype=torch.float64, device=DEV)
    need = L.ake_retune_curve_workspace_bytes(2, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert need > 0 and L.ake_retune_curve_workspace_bytes(0, 4) == 0 and L.ake_retune_curve_workspace_bytes(2, 0) == 0

    def call(x_ptr=x.data_ptr(), in_stride=100, c_ptr=c.data_ptr(), K=4, c_stride=4, first=0, step=64, out_stride=200, ws_bytes=need):
        return L.ake_retune_curve_f32(x_ptr, 2, 100, in_stride, None, c_ptr, K, c_stride, first, step, y.data_ptr(), out_stride, None, ws.data_ptr(),
                                      ws_bytes, stream)

    def positions(c_ptr=c.data_ptr(), K=4, step=64, first=0, idx_ptr=idx.data_ptr(), ws_bytes=need):
        return L.ake_retune_curve_positions(c_ptr, 2, K, 4, first, step, idx_ptr, 5, pos.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    codes = {}

    def refused():
        codes.update(null_in=call(x_ptr=None), null_cents=call(c_ptr=None), step=call(step=63), knots=call(K=0), first=call(first=-1),
                     in_stride=call(in_stride=99), out_stride=call(out_stride=102), cents_stride=call(c_stride=3), ws=call(ws_bytes=need - 256),
                     p_null=positions(idx_ptr=None), p_step=positions(step=63), p_knots=positions(K=0), p_first=positions(first=-1),
                     p_ws=positions(ws_bytes=need - 256))

    launched = _launched(refused)
    assert not set(launched) & set(CURVE_KERNELS), sorted(launched)
    want = dict.fromkeys(codes, AKE_ERR_INVALID)
    want.update(ws=AKE_ERR_WORKSPACE, p_ws=AKE_ERR_WORKSPACE)
    assert codes == want
    assert call() == 0 and positions() == 0
    with pytest.raises(ValueError):
        ake_amd.retune_curve(x, c, 0, 63)
    out, n_out = ake_amd.retune_curve(torch.zeros((2, 0), device=DEV), c, 0, 64)
    assert out.shape == (2, 1) and not bool(out.any()) and n_out.tolist() == [0, 0]


# ---- end to end: tuning="follow" on two recordings whose tuning drifts ----

@pytest.fixture(scope="module")
def net(gold_default):
    n = ake_amd.PitchClassNet(288, 12, 2, 7, default_opt())
    n.load_state_dict(golden_state_dict(gold_default), strict=True)
    return n.to(DEV).eval()


@pytest.fixture(scope="module")
def est(net):
    return ake_amd.KeyEstimator(net, SR, 5)


@pytest.fixture(scope="module")
def drifting():
    """40 s of sustained harmonic notes whose tuning ramps from -35 to +35 cents, and 40 s that sway by 25 cents around +5: float32 on
    the device, and the truth at the centres of the tuning track's windows."""
    x = np.stack([drifting_clip(0, ramp_cents), drifting_clip(1, sine_cents)])
    W = metrics.tuning_track_windows(1 + x.shape[1] // HOP, WF, SF)
    t = window_centre_seconds(W)
    return torch.from_numpy(x.astype(np.float32)).to(DEV), np.stack([ramp_cents(t), sine_cents(t)])


@pytest.fixture(scope="module")
def followed(est, drifting):
    """The manual chain: one transform, ake_amd.tuning_track, ake_amd.retune_curve."""
    audio, _ = drifting
    raw, strength, curve, n_win = ake_amd.tuning_track(est.plan.logmag(audio), WF, SF)
    retuned, lengths = ake_amd.retune_curve(audio, curve, KNOT_FIRST, KNOT_STEP)
    return raw, strength, curve, n_win, retuned, lengths


def test_track_follow_equals_the_manual_chain(est, drifting, followed):
    audio, truth = drifting
    raw, strength, curve, n_win, retuned, lengths = followed
    kw = dict(smooth=True, posteriors=True)
    got = est.track(audio, tuning="follow", **kw)
    want = est.track(retuned, lengths=lengths, **kw)
    assert got.tuning_cents is None and got.tuning_strength is None and want.tuning_curve is None
    assert torch.equal(got.tuning_curve, curve) and torch.equal(got.tuning_curve_strength, strength)
    assert (got.tuning_knot_first, got.tuning_knot_step) == (KNOT_FIRST, KNOT_STEP)
    assert len(got._tensors()) == len(want._tensors()) + 2
    want.tuning_curve, want.tuning_curve_strength = got.tuning_curve, got.tuning_curve_strength
    _same_track(got, want)
    assert int(got.counts.min()) > 0
    err = float(np.abs(got.tuning_curve.cpu().double().numpy() - truth).max())
    print(f"tuning_curve against the truth at the window centres: worst {err:.2f} cents")
    assert err <= 3.0
    # the last segment ends with the last window, in the recording's own time: through the curve, by the model
    for r in range(2):
        end_k = (float(want.times[int(got.counts[r]) - 1]) + want.window_seconds / 2) * SR
        own = float(metrics.retune_curve_positions(torch.tensor([end_k], dtype=torch.float64), curve[r].cpu(), KNOT_FIRST, KNOT_STEP)[0]) / SR
        end = got.segments(r)[-1][1]
        print(f"recording {r}: the track ends at {end:.6f} s of the recording ({end_k / SR:.6f} s of its retuned copy)")
        assert abs(end - own) <= 1e-6 and abs(end - audio.shape[1] / SR) < want.window_seconds


def test_following_leaves_no_detuning_and_one_number_does(est, drifting, followed):
    audio, _ = drifting
    *_, retuned, lengths = followed
    raw, strength, _, n_win = est.tuning_track(retuned, lengths)
    left = float(raw.abs().max())
    weakest = min(float(strength[r, :int(n_win[r])].min()) for r in range(2))
    cents, _ = est.estimate_tuning(audio)
    one, len_one = ake_amd.retune(audio, cents)
    raw_one, _, _, n_one = est.tuning_track(one, len_one)
    left_one = [float(raw_one[r, :int(n_one[r])].abs().max()) for r in range(2)]
    print(f"windowed detuning left after following: {left:.2f} cents (weakest window {weakest:.2f}); after tuning=\"auto\" "
          f"(estimates {[round(float(c), 2) for c in cents.cpu()]}): {[round(v, 2) for v in left_one]} cents")
    assert left <= 5.0
    assert min(left_one) > 20.0


def test_call_and_profile_key_follow_equal_the_manual_chain(est, drifting, followed):
    audio, _ = drifting
    *_, retuned, lengths = followed
    for a, b in zip(est(audio, tuning="follow"), est(retuned, lengths)):
        assert torch.equal(a, b)
    for a, b in zip(est.profile_key(audio, tuning="follow"), est.profile_key(retuned, lengths)):
        assert torch.equal(a, b)
    pcm = (audio * 32767.0).round().to(torch.int16)
    raw, strength, curve, _ = est.tuning_track(pcm)
    assert torch.equal(raw, est.tuning_track(ake_amd.pcm16_to_float(pcm))[0])
    prof = est.track(pcm, tuning="follow", method="profile", refine=True, smooth=True)
    assert torch.equal(prof.tuning_curve, curve) and prof.change_frame is not None
    for t, *_ in prof.change_points(0):
        assert 0.0 < t < audio.shape[1] / SR


def test_follow_refusals(net, est, drifting):
    audio, _ = drifting
    with pytest.raises(ValueError, match="frames=0"):
        ake_amd.KeyEstimator(net, SR, 0)(audio[:, :15 * SR], tuning="follow")
    with pytest.raises(ValueError, match="frames=0"):
        ake_amd.KeyEstimator(net, SR, 0).tuning_track(audio[:, :15 * SR])
    with pytest.raises(ValueError):
        est.stream(recordings=2, tuning="follow")
    with pytest.raises(ValueError):
        est(audio, tuning="following")


def test_the_other_tunings_launch_what_they_launched(est, drifting):
    """tuning=None and tuning="auto" launch none of the new kernels ("auto": the estimate's two and retune_kernel, once each, as
    before); tuning="follow" launches the track's three and the curve's two, once each, and none of the one-number path."""
    audio = drifting[0][:, :15 * SR].contiguous()
    est(audio); est(audio, tuning="auto"); est(audio, tuning="follow"); torch.cuda.synchronize()
    new, old = TRACK_KERNELS + CURVE_KERNELS, ("tuning_sums_kernel", "tuning_finish_kernel", "retune_kernel")
    plain = _launched(lambda: est(audio))
    assert plain and not set(plain) & set(new + old), sorted(plain)
    auto = _launched(lambda: est(audio, tuning="auto"))
    assert not set(auto) & set(new) and {k: auto.get(k) for k in old} == dict.fromkeys(old, 1)
    follow = _launched(lambda: est(audio, tuning="follow"))
    assert not set(follow) & set(old)
    assert {k: follow.get(k) for k in new} == dict(dict.fromkeys(TRACK_KERNELS, 1), retune_curve_prefix_kernel=1, retune_curve_kernel=1,
                                                   retune_curve_pcm16_kernel=None, retune_curve_positions_kernel=None)
    rest = lambda d: {k: v for k, v in d.items() if k not in new + old}
    assert rest(auto) == rest(follow)                                                    # one more transform than the plain call, both
    assert torch.equal(est(audio)[1], est(audio, tuning=None)[1])
