"""GPU: smooth key tracks -- the emission kernel (ake_key_emissions_f32), the Viterbi kernel (ake_viterbi_keys_f32) and
KeyEstimator.track(smooth=True).  The Viterbi checks are exact: metrics.viterbi_keys on the same float32 emissions on the CPU is the
kernel's recurrence operation for operation (additions, subtractions and comparisons only)."""
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


def device_viterbi(e, A, counts=None, prior=None, poison=True):
    """ake_viterbi_keys_f32 on float32 tensors given on the CPU -> int32 (R, W) path on the CPU."""
    L = _lib.lib()
    R, W, _ = e.shape
    e_d, A_d = e.to(DEV).contiguous(), A.to(DEV).contiguous()
    assert e_d.dtype == torch.float32 and A_d.dtype == torch.float32
    c_d = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    p_d = None if prior is None else prior.to(DEV).contiguous()
    nbytes = L.ake_viterbi_keys_workspace_bytes(R, W)
    assert nbytes >= R * W * 24
    ws = torch.full((nbytes,), 0xAB if poison else 0, dtype=torch.uint8, device=DEV)
    path = torch.full((R, W), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.ake_viterbi_keys_f32(e_d.data_ptr(), R, W, None if c_d is None else c_d.data_ptr(), A_d.data_ptr(),
                                      None if p_d is None else p_d.data_ptr(), path.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream), "ake_viterbi_keys_f32")
    torch.cuda.synchronize()
    return path.cpu()


def default_trans(stride=5.0):
    return metrics.key_transition_log(stay=math.exp(-stride / 60.0)).float()


def check_counts(path, counts):
    for r, c in enumerate(counts):
        assert bool(((path[r, :c] >= 0) & (path[r, :c] < 24)).all()) and bool((path[r, c:] == -1).all())


def test_viterbi_equals_the_host_recurrence_exactly():
    """R = 4, W = 40, counts (40, 17, 1, 0): seeded Gaussian emissions with a prior, then emissions and transitions drawn from small
    integers, where exact ties are frequent and the first-maximum rule decides."""
    counts = [40, 17, 1, 0]
    g = torch.Generator().manual_seed(21)
    e = torch.randn((4, 40, 24), generator=g) * 3
    A = metrics.key_transition_log(stay=0.7).float()
    prior = torch.randn(24, generator=g)
    for pr in (None, prior):
        want = metrics.viterbi_keys(e, A, log_prior=pr, counts=counts)
        got = device_viterbi(e, A, counts, pr)
        assert got.dtype == torch.int32 and torch.equal(got, want)
        check_counts(got, counts)
    assert len(set(got[0].tolist())) > 3                                                       # (a path that does move)
    ei = torch.randint(-2, 3, (4, 40, 24), generator=g).float()
    Ai = torch.randint(-2, 1, (24, 24), generator=g).float()
    cand = ei[0, 0][:, None] + Ai                                                              # ties among the 24 candidates of a step
    assert int((cand == cand.max(dim=0, keepdim=True).values).sum(dim=0).max()) > 1
    want = metrics.viterbi_keys(ei, Ai, counts=counts)
    got = device_viterbi(ei, Ai, counts)
    assert torch.equal(got, want)
    check_counts(got, counts)


@pytest.mark.parametrize("W", [1, 2])
def test_viterbi_one_and_two_windows(W):
    g = torch.Generator().manual_seed(22 + W)
    e = torch.randn((3, W, 24), generator=g) * 2
    A = default_trans()
    counts = [W, 1, 0]
    got = device_viterbi(e, A, counts)
    assert torch.equal(got, metrics.viterbi_keys(e, A, counts=counts))
    assert got[0, 0] >= 0 and got[2].tolist() == [-1] * W
    if W == 1:
        assert got[:2, 0].tolist() == np.argmax(e[:2, 0].numpy(), axis=1).tolist()


@pytest.mark.parametrize("chunks", [1, 2])
def test_viterbi_backtrace_crosses_chunk_boundaries(chunks):
    """W just above the backtrace's staging chunk and just above twice it, R = 2; the second recording ends one window behind a chunk
    boundary."""
    C = _lib.lib().ake_viterbi_chunk_windows()
    assert C >= 4 and C % 4 == 0
    W = chunks * C + 3 + chunks
    counts = [W, C + 1]
    g = torch.Generator().manual_seed(30 + chunks)
    e = torch.randn((2, W, 24), generator=g) * 3
    A = metrics.key_transition_log(stay=0.6).float()
    want = metrics.viterbi_keys(e, A, counts=counts)
    got = device_viterbi(e, A, counts)
    assert torch.equal(got, want)
    check_counts(got, counts)
    assert len(set(got[0].tolist())) > 10


def test_viterbi_zero_emissions_and_a_constant_matrix_give_key_0():
    e = torch.zeros((2, 50, 24))
    got = device_viterbi(e, torch.full((24, 24), -1.5))
    assert bool((got == 0).all())
    assert torch.equal(got, metrics.viterbi_keys(e, torch.full((24, 24), -1.5)))


def test_viterbi_null_counts_equal_full_counts():
    g = torch.Generator().manual_seed(40)
    e = torch.randn((3, 33, 24), generator=g) * 3
    A = default_trans(1.0)
    a, b = device_viterbi(e, A, None), device_viterbi(e, A, [33, 33, 33])
    assert torch.equal(a, b) and torch.equal(a, metrics.viterbi_keys(e, A))
    # counts beyond the tensor are clamped to it
    assert torch.equal(device_viterbi(e, A, [99, 33, -4]), metrics.viterbi_keys(e, A, counts=[33, 33, 0]))


def emission_bound(key64, tonic64, weight):
    """Per entry: 1e-5 * (1 + sum of the magnitudes of the 13 terms of e[k] as they enter it): the log-softmax term and the 12 clamped
    Bernoulli terms times weight / 12.  Each logf / log1pf is good to a few ulp (2^-23 ~ 1.2e-7) of its own magnitude."""
    inside, outside = torch.log(key64).clamp_min(-100).abs(), torch.log1p(-key64).clamp_min(-100).abs()
    S = metrics.KEY_SCALES
    mag = (S * inside[..., None, :] + (1 - S) * outside[..., None, :]).sum(dim=-1) * (abs(weight) / 12)
    ls = torch.log_softmax(tonic64, dim=-1).abs()
    return 1e-5 * (1 + mag + torch.cat([ls, ls], dim=-1))


def emission_inputs(rows, seed):
    g = torch.Generator().manual_seed(seed)
    key = torch.rand((rows, 12), generator=g)
    tonic = torch.randn((rows, 12), generator=g) * 4
    key[0, :3] = torch.tensor([0.0, 1.0, 1e-30])                                               # saturated memberships
    key[rows - 1, 9:] = torch.tensor([1.0, 1e-30, 0.0])
    if rows > 2:
        key[rows // 2] = torch.tensor([1.0, 0.0] * 6)
    return key, tonic


def device_emissions(key, tonic, weight, counts=None, windows=1):
    L = _lib.lib()
    rows = key.shape[0]
    k_d, t_d = key.to(DEV).contiguous(), tonic.to(DEV).contiguous()
    c_d = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    out = torch.full((rows, 24), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(L.ake_key_emissions_f32(k_d.data_ptr(), t_d.data_ptr(), rows, None if c_d is None else c_d.data_ptr(), windows, weight,
                                       out.data_ptr(), torch.cuda.current_stream().cuda_stream), "ake_key_emissions_f32")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("rows", [1, 63, 257])
def test_emissions_against_the_float64_model(rows):
    key, tonic = emission_inputs(rows, 50 + rows)
    for weight in (1.0, 3.0):
        got = device_emissions(key, tonic, weight)
        want = metrics.key_emissions(key.double(), tonic.double(), signature_weight=weight)
        assert bool(torch.isfinite(got).all())
        ratio = ((got.double() - want).abs() / emission_bound(key.double(), tonic.double(), weight)).max()
        print(f"emissions rows={rows} weight={weight}: largest |diff| / bound {float(ratio):.3f}")
        assert float(ratio) <= 1.0
    if rows == 63:                                                                             # 3 recordings of 21 windows, ragged
        counts = [21, 5, 0]
        got = device_emissions(key, tonic, 1.0, counts, 21).reshape(3, 21, 24)
        want = metrics.key_emissions(key.double().reshape(3, 21, 12), tonic.double().reshape(3, 21, 12), counts=counts)
        assert bool((got[1, 5:] == 0).all()) and bool((got[2] == 0).all()) and bool((got[0] != 0).all())
        bound = emission_bound(key.double(), tonic.double(), 1.0).reshape(3, 21, 24)
        assert bool(((got.double() - want).abs() <= bound).all())


def path_score(e64, A64, path):
    s = e64[0, path[0]]
    for w in range(1, len(path)):
        s = s + A64[path[w - 1], path[w]] + e64[w, path[w]]
    return float(s)


def test_device_path_is_optimal_in_float64_within_the_rounding_bound():
    """No tie assumptions: the device path's score, recomputed in float64 from the float64 emissions, lies within 3 * W * 2^-23 * max|d|
    of the float64 optimum; max|d| is the largest normalised score of the float64 host recurrence."""
    W = 40
    g = torch.Generator().manual_seed(60)
    e = torch.randn((4, W, 24), generator=g) * 3
    A = metrics.key_transition_log(stay=0.7).float()
    got = device_viterbi(e, A)
    e64, A64 = e.double(), A.double()
    best = metrics.viterbi_keys(e64, A64)
    for r in range(4):
        d = e64[r, 0] - e64[r, 0].max()
        dmax = float(d.abs().max())
        for w in range(1, W):                                                                  # the host recurrence, for max|d|
            d = (d[:, None] + A64).max(dim=0).values + e64[r, w]
            d = d - d.max()
            dmax = max(dmax, float(d.abs().max()))
        opt, mine = path_score(e64[r], A64, best[r].tolist()), path_score(e64[r], A64, got[r].tolist())
        bound = 3 * W * 2.0 ** -23 * dmax
        print(f"recording {r}: float64 optimum {opt:.6f}, device path {mine:.6f}, bound {bound:.2e}, max|d| {dmax:.1f}")
        assert opt - mine <= bound and mine <= opt + 1e-9


# ---- end to end: KeyEstimator.track(smooth=True) ----

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


@pytest.fixture(scope="module")
def smooth31(est, audio):
    tr = est.track(audio, stride_seconds=1.0, smooth=True)
    torch.cuda.synchronize()
    return tr


def check_smooth_track(tr, mean_key_seconds=60.0, weight=1.0):
    R, W = tr.key_id.shape
    counts = tr.counts.cpu().tolist()
    assert tr.emissions.shape == (R, W, 24) and tr.emissions.dtype == torch.float32
    assert tr.smooth_key_id.shape == (R, W) and tr.smooth_key_id.dtype == torch.int32
    key64, tonic64 = tr.key.cpu().double(), tr.tonic.cpu().double()
    want = metrics.key_emissions(key64, tonic64, signature_weight=weight, counts=counts)
    ratio = ((tr.emissions.cpu().double() - want).abs() / emission_bound(key64, tonic64, weight)).max() if W else 0.0
    print(f"track emissions: largest |diff| / bound {float(ratio):.3f}")
    assert float(ratio) <= 1.0
    A = metrics.key_transition_log(stay=math.exp(-tr.stride_seconds / mean_key_seconds)).float()
    path = tr.smooth_key_id.cpu()
    assert torch.equal(path, metrics.viterbi_keys(tr.emissions.cpu(), A, counts=counts))
    check_counts(path, counts)
    return path


def test_track_smooth_end_to_end(smooth31):
    tr = smooth31
    assert tr.key.shape == (3, 31, 12) and tr.counts.tolist() == [31] * 3 and tr.stride_seconds == pytest.approx(1.0)
    path = check_smooth_track(tr)
    segs = tr.segments(0)
    assert segs == tr.segments(0, smoothed=True) and all(s[2] >= 0 and s[3] != "unknown" for s in segs)
    assert segs[0][0] == 0.0 and segs[-1][1] == pytest.approx(37.5 + 7.6)
    assert [s[2] for s in segs] == [k for i, k in enumerate(path[0].tolist()) if i == 0 or k != path[0, i - 1]]
    assert len(tr.segments(0, smoothed=False)) >= 1


def test_smooth_false_changes_nothing(est, audio, smooth31):
    plain, off = est.track(audio, stride_seconds=1.0), est.track(audio, stride_seconds=1.0, smooth=False)
    assert plain.emissions is None and plain.smooth_key_id is None and off.emissions is None and off.smooth_key_id is None
    for x, y, z in zip(plain._tensors()[:8], off._tensors()[:8], smooth31._tensors()[:8]):
        assert torch.equal(x, y) and torch.equal(x, z)                                          # nor does smooth=True change the rest
    assert torch.equal(plain.times, off.times) and off.segments(0) == plain.segments(0)
    with pytest.raises(ValueError):
        plain.segments(0, smoothed=True)


def test_ragged_batch_with_a_recording_shorter_than_one_window(est, audio):
    lens = torch.tensor([N45, 500000, 22050 * 10])
    tr = est.track(audio, lengths=lens, stride_seconds=1.0, smooth=True, mean_key_seconds=20.0, signature_weight=2.0)
    assert tr.counts.tolist() == [31, 8, 0]
    path = check_smooth_track(tr, mean_key_seconds=20.0, weight=2.0)
    assert bool((tr.emissions[1, 8:] == 0).all()) and bool((tr.emissions[2] == 0).all())
    assert path[2].tolist() == [-1] * 31 and tr.segments(2) == []
    assert len(tr.segments(1)) >= 1 and tr.segments(1)[-1][1] == pytest.approx(float(tr.times[7]) + 7.6)
    # every recording shorter than one window: an empty smoothed track
    empty = est.track(audio[:, :22050 * 10], smooth=True)
    assert empty.emissions.shape == (3, 0, 24) and empty.smooth_key_id.shape == (3, 0) and empty.segments(0) == []


def test_two_streams_give_the_same_smoothed_track(net, est, audio, smooth31):
    est2 = ake_amd.KeyEstimator(net, 22050, 5, streams=2)
    lens = torch.tensor([N45, 500000, 22050 * 10], device=DEV)
    got = [est2.track(audio, stride_seconds=1.0, smooth=True), est2.track(audio, lens, smooth=True),
           est2.track(audio, stride_seconds=1.0, smooth=True)]
    est2.join()
    torch.cuda.synchronize()
    want = [smooth31, est.track(audio, lens, smooth=True), smooth31]
    for a, b in zip(got, want):
        assert a.emissions is not None and a.smooth_key_id is not None
        for x, y in zip(a._tensors(), b._tensors()):
            assert torch.equal(x, y)
    assert est2._slots[0]["stream"] is not None and est2._slots[1]["stream"] is not None


def test_a_user_transition_is_honoured_and_cached(est, audio, smooth31):
    """A uniform matrix makes the path the per-window first maximum of the emissions.  Exactly so for the uniform matrix of zeros: every
    step then computes max_i (d[i] + 0) = 0 and 0 + e[w][j] = e[w][j], the emissions themselves.  With log(1 / 24) in its place the
    float32 sum m + e[w][j] lands in a coarser binade than e (about -3.2 - 3.2 here) and rounds emissions one ulp apart -- this net's
    untrained key head scores the keys that close -- to the same value, so the first-maximum rule picks a smaller key there.  That
    matrix is held to the host recurrence instead, which rounds the same way."""
    uniform = torch.zeros((24, 24))
    before = len(est._transitions)
    tr = est.track(audio, stride_seconds=1.0, smooth=True, transition=uniform)
    assert torch.equal(tr.emissions, smooth31.emissions)
    first = np.argmax(tr.emissions.cpu().numpy(), axis=2)                                       # numpy: the first maximum
    assert np.array_equal(tr.smooth_key_id.cpu().numpy(), first)
    assert not torch.equal(tr.smooth_key_id, smooth31.smooth_key_id)                           # (the default matrix does smooth)
    normalised = torch.full((24, 24), math.log(1 / 24))
    tn = est.track(audio, stride_seconds=1.0, smooth=True, transition=normalised)
    assert torch.equal(tn.smooth_key_id.cpu(), metrics.viterbi_keys(tn.emissions.cpu(), normalised))
    before += 1
    again = est.track(audio, stride_seconds=1.0, smooth=True, transition=uniform)
    assert torch.equal(again.smooth_key_id, tr.smooth_key_id) and len(est._transitions) == before + 1
    cached = [v for v in est._transitions.values() if v[0] is uniform]
    assert len(cached) == 1 and cached[0][1].device.type == "cuda"
    est.track(audio, stride_seconds=1.0, smooth=True)                                          # the default of this stride: cached by smooth31
    assert len(est._transitions) == before + 1
    bad = uniform.clone()
    bad[0, 1] = -math.inf
    with pytest.raises(ValueError, match="large negative"):
        est.track(audio, smooth=True, transition=bad)
    with pytest.raises(ValueError, match="24, 24"):
        est.track(audio, smooth=True, transition=torch.zeros((12, 12)))
