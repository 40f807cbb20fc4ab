"""GPU: key changes to the frame inside key streams -- ake_stream_key_changes_f32 on a chroma ring that ake_stream_frame_stats_f32
filled, against the offline entry ake_key_changes_f32 on the joined frames and labels (to the bit) and against the float64 model
(metrics.key_changes, which metrics.stream_key_changes equals when joined: tests/test_stream_changes_host.py), its state and refusals,
and KeyEstimator.stream(refine=True) end to end.

Bounds.  Against the offline entry both kernels call csrc/changes.h on the same class sums (csrc/profile.h's prof_class_sum): torch.equal.
Against the model, as tests/test_gpu_key_changes.py: change_frame equal on every boundary whose model margin is >= 1e-9, gain and contrast
(double results rounded once to float32) within 1e-6 * max(1, |want|); at most 2 % of the boundaries may be left out for a small margin,
which the model alone is asserted to meet before the kernel is looked at.

Shapes: 36 bins, windows of 5 frames 2 apart, 12 to 40 windows, 1 and 3 recordings; the rings at their minimal lengths
(metrics.stream_changes_ring_frames, metrics.stream_changes_labels_carried + a call's labels), so both wrap several times."""
import json
from argparse import Namespace

import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from ake_amd.keyprofile import device_profiles
from ake_amd.pipeline import track_counts
from conftest import golden_state_dict, load_golden
from ws_guard import GuardedTensor, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, HOP, WF, SF = 22050, 4410, 76, 25
AKE_ERR_INVALID, AKE_ERR_WORKSPACE, AKE_ERR_UNSUPPORTED = -1, -4, -5
MIN_MARGIN, MAX_LEFT_OUT = 1e-9, 0.02
PATTERN = (1, 0, 3, 2, 7, 1)
COMPRESSIONS = metrics.PROFILE_COMPRESSIONS
OUT_NAMES = ("change_frame", "gain", "contrast")


def launched(fn):
    _lib.prof_enable("", True)
    try:
        _lib.prof_results()                                          # (start from an empty log)
        fn()
        return {k: v[1] for k, v in _lib.prof_results().items() if v[1]}
    finally:
        _lib.prof_enable("", False)


def user_profile():
    return torch.rand((2, 12), generator=torch.Generator().manual_seed(41), dtype=torch.float64) + 0.2


def as_kernel_reads(profiles):
    return metrics.key_profile_table(profiles).to(torch.float32).to(torch.float64)


def seeded_labels(seed, R, W):
    """Labels (R, W) with runs of one, two and more windows and the two kinds of "no key", -1 and 24."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda n: int(torch.randint(0, n, (1,), generator=g))
    rows = []
    for _ in range(R):
        row = []
        while len(row) < W:
            key = (-1, 24)[draw(2)] if draw(8) == 0 else draw(24)
            row += [key] * (1, 1, 2, 2, 3, 5)[draw(6)]
        rows.append(row[:W])
    return torch.tensor(rows, dtype=torch.int32)


def schedule_of(cuts, T, wf, sf, lag, flush_alone=True):
    """Pieces of `cuts` frames (cycled) with the labels trailing the windows by `lag` -> [(new frames, labels decided after, flush)]."""
    out, F, i = [], 0, 0
    while F < T:
        m = min(cuts[i % len(cuts)], T - F)
        F, i = F + m, i + 1
        out.append((m, max(track_counts(F, wf, sf) - lag, 0), False))
    W = track_counts(T, wf, sf)
    if flush_alone:
        return out + [(0, W, True)]
    return out[:-1] + [(out[-1][0], W, True)]


def rings_of(schedule, wf, sf, slack, lag):
    """The minimal rings of a schedule whose labels trail by `lag`."""
    most_frames = max(m for m, _, _ in schedule)
    most_labels = max(b[1] - a[1] for a, b in zip([(0, 0, False)] + schedule[:-1], schedule))
    return (metrics.stream_changes_ring_frames(wf, sf, slack, lag, most_frames),
            max(metrics.stream_changes_labels_carried(wf, sf, slack) + most_labels, 1))


def chroma_bytes(R, ring):
    return _lib.lib().ake_stream_profile_state_bytes(R, ring)


def label_bytes(R, label_ring):
    n = _lib.lib().ake_stream_key_changes_state_bytes(R, label_ring)
    assert n == (R * label_ring * 4 + 15) // 16 * 16
    return n


def run_entries(mel, labels, schedule, wf, sf, slack, ring, label_ring, compression=0, profiles="krumhansl", fill=None):
    """The stream's two entries over `mel` (R, P, T) float32 and `labels` (R, W) int32, both on the device, piece by piece: the chroma
    part of ake_stream_frame_stats_f32, then ake_stream_key_changes_f32 with the host's counts.  `fill`: the label state and the outputs
    sit in guarded buffers, the state filled with that byte, and the chroma state is held to be left as it was.  -> (the three joined
    outputs, the chroma state's defined bytes, the label state's)."""
    L_ = _lib.lib()
    R, P, T = mel.shape
    stream = torch.cuda.current_stream().cuda_stream
    chroma = torch.empty(chroma_bytes(R, ring), dtype=torch.uint8, device=DEV)
    nbytes = label_bytes(R, label_ring)
    state, state_check = guarded(nbytes, fill) if fill is not None else (torch.empty(nbytes, dtype=torch.uint8, device=DEV), lambda what: None)
    prof = device_profiles(profiles if isinstance(profiles, str) else as_kernel_reads(profiles), torch.device(DEV))
    F = L = B = 0
    joined = [[], [], []]
    for m, L_new, flush in schedule:
        rc = L_.ake_stream_frame_stats_f32(mel.data_ptr(), 0, R, P, T, F, m, F, ring, 1, compression, 0.0, chroma.data_ptr(), chroma.numel(), None, None, stream)
        assert rc == 0, L_.ake_last_error()
        F += m
        k = L_new - L
        B_new = metrics.stream_changes_ready(L_new, F, wf, sf, slack, flush)
        b = B_new - B
        shapes = ((R, b), torch.int32), ((R, b), torch.float32), ((R, b), torch.float32)
        if fill is not None:
            outs = [GuardedTensor(s, dtype=d, fill=0x7F if d == torch.int32 else 0xFF) for s, d in shapes]
            before = chroma.clone()
        else:
            outs = [Namespace(t=torch.empty(s, dtype=d, device=DEV), check=lambda what="": None) for s, d in shapes]
        new = labels[:, L:L_new].contiguous()
        rc = L_.ake_stream_key_changes_f32(chroma.data_ptr(), chroma.numel(), R, ring, F, new.data_ptr() if k else None, k, L, int(flush), wf, sf, slack,
                                           prof.data_ptr(), state.data_ptr(), state.numel(), label_ring, B, b,
                                           *[o.t.data_ptr() if b else None for o in outs], stream)
        assert rc == 0, L_.ake_last_error()
        for o, name in zip(outs, OUT_NAMES):
            o.check(name)
        state_check("label state")
        if fill is not None:
            assert torch.equal(chroma, before)                       # read only
        for j, o in zip(joined, outs):
            j.append(o.t.clone())
        L, B = L_new, B_new
    assert F == T and L == labels.shape[1] and B == max(L - 1, 0)
    torch.cuda.synchronize()
    return [torch.cat(j, dim=1) for j in joined], chroma[:R * ring * 96].clone(), state[:R * label_ring * 4].clone()


def offline(mel, labels, wf, sf, slack, compression=0, profiles="krumhansl"):
    return ake_amd.key_changes(mel, labels, wf, sf, slack_frames=slack, profiles=profiles if isinstance(profiles, str) else as_kernel_reads(profiles),
                               compression=COMPRESSIONS[compression])


def chunkings(T, wf, sf):
    """name -> (schedule, the lag its labels trail by)."""
    W = track_counts(T, wf, sf)
    return {"one window at a time": (schedule_of([wf] + [sf] * W, T, wf, sf, 0, flush_alone=False), 0),
            "irregular": (schedule_of(PATTERN, T, wf, sf, 2), 2),
            "irregular, a long lag": (schedule_of((3, 1, 4), T, wf, sf, 6), 6),
            "all in one call with the flush in it": ([(T, W, True)], 0),
            "k = 0 with the flush": ([(T, W, False), (0, W, True)], 0)}


def case(R, W, seed, wf=5, sf=2, extra=1):
    """-> (mel (R, 36, T) float32 on the host with a silent stretch, labels (R, W) int32): T holds W windows and `extra` frames more."""
    T = wf + (W - 1) * sf + extra
    mel = torch.rand((R, 36, T), generator=torch.Generator().manual_seed(seed)) * 3.0
    mel[R - 1, :, T // 3:T // 3 + 3] = 0.0
    return mel, seeded_labels(seed + 1, R, W)


# ---- 1. against the offline entry, under every chunking --------------------------------------------------------------------------------------

@pytest.mark.parametrize("slack", [0, 2, 7])
@pytest.mark.parametrize("R, W", [(1, 12), (3, 40), (3, 23)])
def test_entry_equals_the_offline_entry_under_every_chunking(R, W, slack):
    wf, sf = 5, 2
    host, labels_host = case(R, W, 100 * W + 10 * R + slack)
    T = host.shape[2]
    assert any((labels_host[r, 1:-1] != labels_host[r, :-2]).logical_and(labels_host[r, 1:-1] != labels_host[r, 2:]).any() for r in range(R))   # one-window runs
    assert bool((labels_host[:, 1:] == labels_host[:, :-1]).any())
    mel, labels = host.to(DEV), labels_host.to(DEV)
    n_there = 0
    for compression, profiles in ((0, "krumhansl"), (1, "krumhansl"), (2, "krumhansl"), (1, user_profile())):
        want = offline(mel, labels, wf, sf, slack, compression, profiles)
        n_there += int((want[0] >= 0).sum())
        big = None
        for name, (schedule, lag) in chunkings(T, wf, sf).items():
            what = (name, compression, isinstance(profiles, str))
            # rings that hold everything: the same state bytes whatever the chunking
            got, chroma, state = run_entries(mel, labels, schedule, wf, sf, slack, T + wf, W + 3, compression, profiles)
            for out_name, a, b in zip(OUT_NAMES, got, want):
                assert a.shape == b.shape and torch.equal(a, b), (out_name,) + what
            if big is None:
                big = (chroma, state)
                assert torch.equal(state.view(torch.int32).view(R, W + 3)[:, :W], labels) and bool((state.view(torch.int32).view(R, W + 3)[:, W:] == -1).all())
            assert torch.equal(chroma, big[0]) and torch.equal(state, big[1]), what
            if len(schedule) <= 2:
                continue
            # the minimal rings: they wrap several times, and hold the last frames' rows and the last windows' labels by index
            ring, label_ring = rings_of(schedule, wf, sf, slack, lag)
            assert W < 23 or (ring < T / 1.5 and label_ring < W / 2)
            got, chroma, state = run_entries(mel, labels, schedule, wf, sf, slack, ring, label_ring, compression, profiles)
            for out_name, a, b in zip(OUT_NAMES, got, want):
                assert torch.equal(a, b), (out_name, "minimal rings") + what
            rows, small = big[0].view(torch.float64).view(R, T + wf, 12), chroma.view(torch.float64).view(R, ring, 12)
            for t in range(T - ring, T):
                assert torch.equal(small[:, t % ring], rows[:, t]), t
            slots = state.view(torch.int32).view(R, label_ring)
            for v in range(W - label_ring, W):
                assert torch.equal(slots[:, v % label_ring], labels[:, v]), v
    assert n_there > 0
    same_profile = offline(mel, labels, wf, sf, slack, 1)
    assert not torch.equal(same_profile[1], offline(mel, labels, wf, sf, slack, 1, user_profile())[1])       # the user's profile reached the kernel


def test_the_span_cap():
    """stride_frames + 2 * slack_frames = 1024 frames is the longest span; boundary 1 of the labels a a b b has exactly that many."""
    wf, sf, slack = 16, 1000, 12
    T = 3 * sf + wf + 30
    host = torch.rand((1, 36, T), generator=torch.Generator().manual_seed(77)) * 3.0
    labels_host = torch.tensor([[3, 3, 17, 17]], dtype=torch.int32)
    want = metrics.key_changes(host, labels_host, wf, sf, slack_frames=slack, profiles=as_kernel_reads("krumhansl"))
    assert want[0][0].tolist()[0] == want[0][0].tolist()[2] == -1 and 1008 - 12 <= int(want[0][0, 1]) <= 2008 + 12
    assert float(want[3][0, 1]) >= MIN_MARGIN
    mel, labels = host.to(DEV), labels_host.to(DEV)
    for cuts, lag in (((600,), 0), ((600,), 1), ((T,), 0)):
        schedule = schedule_of(cuts, T, wf, sf, lag)
        ring, label_ring = rings_of(schedule, wf, sf, slack, lag)
        got, _, _ = run_entries(mel, labels, schedule, wf, sf, slack, ring, label_ring)
        assert all(torch.equal(a, b) for a, b in zip(got, offline(mel, labels, wf, sf, slack)))
        assert torch.equal(got[0].cpu(), want[0])
        for g, w in zip(got[1:], want[1:3]):
            assert float(((g.cpu().double() - w).abs() / w.abs().clamp_min(1.0)).max()) <= 1e-6
    with pytest.raises(ValueError, match="1024"):
        ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288).stream(1, method="profile", refine=True, refine_slack_seconds=100.0)


# ---- 2. against the float64 model -----------------------------------------------------------------------------------------------------------

def test_entry_against_the_float64_model():
    wf, sf = 5, 2
    total = left_out = 0
    worst = {"gain": 0.0, "contrast": 0.0}
    for R, W, slack, compression, profiles, seed in ((3, 40, 2, 0, "krumhansl", 1), (3, 40, 7, 1, "krumhansl", 2), (1, 12, 0, 2, "krumhansl", 3),
                                                     (3, 23, 2, 1, user_profile(), 4), (3, 40, 7, 2, user_profile(), 5)):
        host, labels_host = case(R, W, 7000 + seed)
        T = host.shape[2]
        want = metrics.key_changes(host, labels_host, wf, sf, slack_frames=slack, profiles=as_kernel_reads(profiles), compression=COMPRESSIONS[compression])
        there = want[0] >= 0
        sure = there & (want[3] >= MIN_MARGIN)
        total, left_out = total + int(there.sum()), left_out + int((there & ~sure).sum())
        schedule = schedule_of(PATTERN, T, wf, sf, 2)
        ring, label_ring = rings_of(schedule, wf, sf, slack, 2)
        got, _, _ = run_entries(host.to(DEV), labels_host.to(DEV), schedule, wf, sf, slack, ring, label_ring, compression, profiles)
        frame, gain, contrast = (g.cpu() for g in got)
        assert torch.equal(frame[sure], want[0][sure]) and torch.equal(frame < 0, ~there)
        for name, g, w in (("gain", gain, want[1]), ("contrast", contrast, want[2])):
            err = float(((g.double() - w).abs() / w.abs().clamp_min(1.0)).max())
            worst[name] = max(worst[name], err)
            assert err <= 1e-6, (name, seed, err)
        assert not bool(gain[~there].any()) and not bool(contrast[~there].any())              # exact zeros where there is no boundary
        assert bool((gain >= 0).all()) and bool((contrast.abs() <= 2).all())
    print(f"\n  STREAM changes against the model: {total} boundaries, {left_out} left out for a margin below {MIN_MARGIN:g}; gain {worst['gain']:.2e}, "
          f"contrast {worst['contrast']:.2e} (bound 1e-6)")
    assert total >= 120 and left_out <= MAX_LEFT_OUT * total          # (the model alone: seeds chosen on the CPU)


# ---- 3. state, guards and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x77])
def test_guarded_state_and_outputs_over_a_poisoned_fresh_state(fill):
    """labels_before == 0 reads nothing of the label state and writes it whole: three fill bytes give the same outputs and the same state,
    and no call writes outside the bytes it was given or into the chroma state."""
    wf, sf, slack = 5, 2, 2
    host, labels_host = case(3, 23, 31)
    T, W = host.shape[2], 23
    mel, labels = host.to(DEV), labels_host.to(DEV)
    want = offline(mel, labels, wf, sf, slack)
    for schedule, lag in (chunkings(T, wf, sf)["irregular"], ([(0, 0, False), (T, W - 4, False), (0, W, True)], 0)):
        ring, label_ring = (rings_of(schedule, wf, sf, slack, lag)[0], W + 9) if lag == 0 else rings_of(schedule, wf, sf, slack, lag)
        got, _, state = run_entries(mel, labels, schedule, wf, sf, slack, ring, label_ring, fill=fill)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        clean = run_entries(mel, labels, schedule, wf, sf, slack, ring, label_ring)
        assert torch.equal(state, clean[2])
        if lag == 0:                                                 # the slots no window has reached: -1 whatever the fill
            assert bool((state.view(torch.int32).view(3, label_ring)[:, W:] == -1).all())


def _call(chroma, state, R=1, ring=32, frames=16, k=4, before=0, flush=0, wf=5, sf=2, slack=2, label_ring=8, first=0, n=1, labels=None, outs=None,
          chroma_nbytes=None, nbytes=None, null=()):
    prof = device_profiles("krumhansl", torch.device(DEV))
    labels = torch.tensor([[1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]], dtype=torch.int32, device=DEV) if labels is None else labels
    outs = [torch.full((4, 16), 7, dtype=torch.int32, device=DEV), torch.full((4, 16), 7.0, device=DEV), torch.full((4, 16), 7.0, device=DEV)] if outs is None else outs
    ptr = lambda name, t: None if name in null else t.data_ptr()
    rc = _lib.lib().ake_stream_key_changes_f32(ptr("chroma", chroma), chroma.numel() if chroma_nbytes is None else chroma_nbytes, R, ring, frames,
                                               ptr("labels", labels), k, before, flush, wf, sf, slack, ptr("profiles", prof), ptr("state", state),
                                               state.numel() if nbytes is None else nbytes, label_ring, first, n,
                                               ptr("change_frame", outs[0]), ptr("gain", outs[1]), ptr("contrast", outs[2]),
                                               torch.cuda.current_stream().cuda_stream)
    return rc, outs


def test_refusals_launch_nothing():
    L = _lib.lib()
    assert L.ake_stream_key_changes_state_bytes(0, 8) == 0 and L.ake_stream_key_changes_state_bytes(65536, 8) == 0 and L.ake_stream_key_changes_state_bytes(1, 0) == 0
    chroma = torch.zeros(chroma_bytes(1, 32), dtype=torch.uint8, device=DEV)
    state = torch.full((label_bytes(1, 8),), 0x5A, dtype=torch.uint8, device=DEV)
    codes, kept = [], []

    def all_refusals():
        def c(want, **kw):
            rc, outs = _call(chroma, state, **kw)
            codes.append((kw, want, rc))
            kept.extend(outs)
        for null in ("chroma", "profiles", "state", "labels", "change_frame", "gain", "contrast"):
            c(AKE_ERR_INVALID, null=(null,))
        for kw in (dict(R=0), dict(R=65536), dict(ring=0), dict(label_ring=0), dict(wf=0), dict(sf=0), dict(slack=-1), dict(k=-1), dict(n=-1), dict(first=-1),
                   dict(before=-1), dict(frames=-1), dict(frames=2 ** 31), dict(k=65536), dict(n=65536),
                   dict(frames=10),                                  # window 3 ends at frame 11: a label whose frames have not arrived
                   dict(n=3),                                        # boundary 2 needs the label of window 4, and 4 windows are decided
                   dict(k=2),                                        # boundary 0 needs the label of window 2
                   dict(flush=1, n=4),                               # also at the flush boundary 3 needs window 4
                   dict(k=6, frames=15, n=4, slack=7),               # boundary 3 reads up to frame 4 * 2 + 2 + 7 = 17: not yet arrived
                   dict(before=4, k=4, frames=30, first=2, n=4, slack=0, ring=16),      # boundary 2 reads from frame 6, a ring of 16 holds 14 on
                   dict(k=9, frames=30),                             # more new labels than slots
                   dict(before=6, k=4, frames=30, first=2, n=6)):    # window 1's label shares its slot with window 9's, which this call brings
            c(AKE_ERR_INVALID, **kw)
        c(AKE_ERR_UNSUPPORTED, sf=1000, slack=13, frames=4000)
        c(AKE_ERR_UNSUPPORTED, sf=1025, slack=0, frames=4000)
        c(AKE_ERR_WORKSPACE, nbytes=state.numel() - 1)
        c(AKE_ERR_WORKSPACE, chroma_nbytes=chroma.numel() - 1)

    assert launched(all_refusals) == {}
    for kw, want, rc in codes:
        assert rc == want, (kw, rc, L.ake_last_error())
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all()) and all(bool((t == 7).all()) for t in kept)        # and nothing was written


def test_the_empty_call_launches_nothing_and_a_label_call_launches_one():
    chroma = torch.zeros(chroma_bytes(1, 32), dtype=torch.uint8, device=DEV)
    state = torch.full((label_bytes(1, 8),), 0x5A, dtype=torch.uint8, device=DEV)
    codes = []
    assert launched(lambda: codes.extend([_call(chroma, state, k=0, n=0)[0], _call(chroma, state, k=0, n=0, frames=0)[0],
                                          _call(chroma, state, k=0, n=0, before=4, flush=1, null=("labels", "change_frame", "gain", "contrast"))[0]])) == {}
    assert codes == [0, 0, 0]
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all())
    # labels without a boundary: one launch that only writes them; then a boundary over silent frames (a zero ring): a frame, not -1
    ok = []
    assert launched(lambda: ok.append(_call(chroma, state, k=2, n=0, null=("change_frame", "gain", "contrast"))[0])) == {"stream_key_changes_kernel": 1}
    assert state[:32].view(torch.int32).tolist() == [1, 1, -1, -1, -1, -1, -1, -1]
    out = []
    assert launched(lambda: out.append(_call(chroma, state, labels=torch.tensor([[2, 2]], dtype=torch.int32, device=DEV), before=2, k=2, first=1))) == {"stream_key_changes_kernel": 1}
    rc, (frame, gain, contrast) = out[0]
    assert ok == [0] and rc == 0 and state[:32].view(torch.int32).tolist() == [1, 1, 2, 2, -1, -1, -1, -1]
    assert int(frame[0, 0]) == 2 and float(gain[0, 0]) == 0.0 and float(contrast[0, 0]) == 0.0        # (every C_j is 0: the first maximum, at lo = m_1 - slack)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------

SECONDS = 75.0


@pytest.fixture(scope="module")
def recordings():
    audio, ann = synthetic.make_modulating_batch_device((3, 8), SECONDS, DEV)
    return audio.contiguous(), ann


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


def chunks_of(n):
    out, left = [1, 4409, 4410, 4411, 0, 100000], n - 113231
    while left > 0:
        out.append(min(3 * SR, left))
        left -= out[-1]
    return out


def run_stream(s, audio, schedule):
    ups, counts, at = [], [], 0
    for m in schedule:
        ups.append(s.push(audio[:, at:at + m]))
        counts.append((s.F, s.L))
        at += m
    assert at == audio.shape[1]
    ups.append(s.finish())
    counts.append((s.F, s.L))
    torch.cuda.synchronize()
    return ups, counts


def joined(ups, name):
    return torch.cat([getattr(u, name) for u in ups], dim=1)


def check_refined_stream(s, ups, counts, slack, **kw):
    """The five fields of every update: the counts by the rule, and joined, ake_amd.key_changes on the stream's own frames and labels."""
    labels = joined(ups, "smooth_key_id" if s.smooth else "key_id")
    W = labels.shape[1]
    B = L0 = 0
    for u, (F, L) in zip(ups, counts):
        fin = u is ups[-1]
        assert u.change_first_boundary == B and L - L0 == (u.smooth_key_id if s.smooth else u.key_id).shape[1]
        b = metrics.stream_changes_ready(L, F, WF, SF, slack, fin) - B
        for name, dtype in (("change_frame", torch.int32), ("change_gain", torch.float32), ("change_contrast", torch.float32), ("change_times", torch.float64)):
            t = getattr(u, name)
            assert tuple(t.shape) == (s.R, b) and t.dtype == dtype, name
        B, L0 = B + b, L
    assert B == W - 1 and W == track_counts(s.frames.shape[2], WF, SF)
    want = ake_amd.key_changes(s.frames, labels, WF, SF, slack_frames=slack, **kw)
    for name, t in zip(("change_frame", "change_gain", "change_contrast"), want):
        assert torch.equal(joined(ups, name), t), name
    assert torch.equal(joined(ups, "change_times"), want[0].to(torch.float64) * HOP / SR / s.rho)
    one = ake_amd.stream.StreamUpdate.concat(ups)
    assert one.change_first_boundary == 0 and torch.equal(one.change_frame, want[0]) and torch.equal(one.change_times, joined(ups, "change_times"))
    return want


@pytest.mark.parametrize("method, smooth, mode", [("profile", True, "float"), ("profile", False, "int16"), ("net", True, "retune"), ("net", False, "float")])
def test_refined_stream_equals_key_changes_on_its_own_frames(est_none, est_net, recordings, method, smooth, mode):
    audio, ann = recordings
    est = est_none if method == "profile" else est_net
    kw = dict(profiles="temperley", compression="magnitude") if mode == "int16" else {}
    extra = dict(retune_cents=12.5) if mode == "retune" else {}
    slack_seconds, slack = (2.0, 10) if mode == "int16" else (None, SF)
    s = est.stream(2, method=method, smooth=smooth, lag_windows=3, keep_frames=True, refine=True, refine_slack_seconds=slack_seconds, **kw, **extra)
    assert s.ring_frames == max(metrics.stream_changes_ring_frames(WF, SF, slack, 3 if smooth else 0, s.max_mel),
                                metrics.stream_profile_ring_frames(WF, s.max_mel) if method == "profile" else 1)
    src = (audio * 32767.0).round().to(torch.int16) if mode == "int16" else audio
    ups, counts = run_stream(s, src, chunks_of(audio.shape[1]))
    want = check_refined_stream(s, ups, counts, slack, **kw)
    assert (s.rho != 1.0) == (mode == "retune")
    assert any(u.change_frame.shape[1] for u in ups[:-1]) and ups[-1].change_frame.shape[1] >= 1          # boundaries while it runs, and the rest at the end
    if method == "profile" and smooth:
        # a modulating recording: the stream finds changes, and places them where key_changes places them on its frames (above); their
        # distance to the annotations is reported, not judged (profiles/track_stream_refine.md has it beside the offline figure)
        frames, starts, n_seg = want[0].cpu().tolist(), ann.seg_start.cpu().tolist(), ann.seg_count.cpu().tolist()
        dist = sorted(min(abs(f - st / HOP) for st in starts[r][1:n_seg[r]]) for r in range(2) for f in frames[r] if f >= 0)
        assert len(dist) >= 2
        print(f"\n  STREAM refine: {len(dist)} streamed boundaries, median {dist[len(dist) // 2]:.2f} and worst {dist[-1]:.2f} frames from the nearest annotated change")


def test_stream_refusals(est_none):
    for kw in (dict(refine_slack_seconds=-1.0), dict(refine_slack_seconds=101.0), dict(compression="sqrt"), dict(profiles="nobody")):
        with pytest.raises(ValueError):
            est_none.stream(1, method="profile", refine=True, **kw)
    s = est_none.stream(1, method="profile", refine=True)                                          # a stream that never gets a window
    u = ake_amd.stream.StreamUpdate.concat([s.push(torch.zeros((1, SR), device=DEV)), s.finish()])
    assert u.change_first_boundary == 0 and tuple(u.change_frame.shape) == tuple(u.change_times.shape) == (1, 0)


# ---- 5. launch sets --------------------------------------------------------------------------------------------------------------------------

UPDATE_TENSORS = ("key", "tonic", "genre", "key_id", "signature_id", "tonic_id", "confidence", "times", "emissions", "filtered", "smooth_key_id", "posteriors",
                  "smooth_confidence", "log_likelihood", "tuning_cents", "tuning_strength")
CHANGE_FIELDS = ("change_first_boundary", "change_frame", "change_gain", "change_contrast", "change_times")


@pytest.mark.parametrize("method", ["net", "profile"])
def test_launch_sets_with_and_without_refine(est_net, est_none, recordings, method):
    audio = recordings[0][:, :60 * SR]
    est = est_net if method == "net" else est_none
    schedule = [10 * SR, 0, 10 * SR, 100, 10 * SR - 100, 5 * SR, 5 * SR, 10 * SR, 10 * SR]
    kw = dict(method=method, lag_windows=1, posteriors=True, tuning_meter=method == "profile")
    runs = {}
    for name, more in (("as before", {}), ("off", dict(refine=False)), ("on", dict(refine=True))):
        s = est.stream(2, **kw, **more)                               # ("as before": opened the way a caller did before the keyword existed)
        out = {}
        runs[name] = (launched(lambda: out.update(r=run_stream(s, audio, schedule))), out["r"][0], out["r"][1], s)
    before, off, on = runs["as before"], runs["off"], runs["on"]
    # without refine: the same launches and the same bits, and none of the new fields
    assert before[0] == off[0] and "stream_key_changes_kernel" not in off[0] and (method == "profile" or "stream_frame_stats_kernel" not in off[0])
    assert off[3].label_state is None and (method == "profile" or off[3].stats_state is None)
    for a, b, c in zip(before[1], off[1], on[1]):
        assert all(getattr(a, f) is None and getattr(b, f) is None and getattr(c, f) is not None for f in CHANGE_FIELDS)
        for f in UPDATE_TENSORS:
            x, y, z = getattr(a, f), getattr(b, f), getattr(c, f)
            assert (x is None and y is None and z is None) or (torch.equal(x, y) and torch.equal(x, z)), f       # refine changes nothing else
        assert (a.first_window, a.windows, a.smooth_first_window) == (b.first_window, b.windows, b.smooth_first_window)
    # with refine: one stream_key_changes_kernel per piece that brings labels or completes a boundary -- a piece that does neither adds
    # nothing but, on a net stream, the frame launch -- and on a net stream one stream_frame_stats_kernel per piece that has new frames
    counts = on[2]
    with_frames = sum(1 for a, b in zip([(0, 0)] + counts[:-1], counts) if b[0] > a[0])
    with_labels = sum(1 for u in on[1] if u.smooth_key_id.shape[1])
    with_boundaries = sum(1 for u in on[1] if u.change_frame.shape[1])
    assert 0 < with_boundaries <= with_labels < len(on[1]) and 0 < with_frames < len(counts)
    assert all(u.smooth_key_id.shape[1] for u in on[1] if u.change_frame.shape[1])                 # (here every boundary waited for a label)
    want = dict(off[0], stream_key_changes_kernel=with_labels)
    if method == "net":
        want["stream_frame_stats_kernel"] = with_frames
    assert on[0] == want, (sorted(on[0].items()), sorted(want.items()))
