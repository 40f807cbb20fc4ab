"""GPU: the track score (ake_track_score_i32, KeyTrack.score) against metrics.track_score on the CPU.  Integers only, so every check is
torch.equal.  No accuracy is asserted anywhere: the end-to-end net has seeded weights, not trained ones."""
import json
from argparse import Namespace

import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, WF, SF = 4410, 76, 25
CENTRE0 = (WF - 1) * HOP // 2


def device_score(pred, counts, start, key, count, hop=HOP, wf=WF, sf=SF, want_truth=True, want_category=True):
    """ake_track_score_i32 on CPU tensors, every output poisoned first -> (truth | None, category | None, tally, changes) on the CPU."""
    R, W = pred.shape
    d = lambda t, dt: None if t is None else torch.as_tensor(t).to(device=DEV, dtype=dt).contiguous()
    pred_d, counts_d = d(pred, torch.int32), d(counts, torch.int32)
    start_d, key_d, count_d = d(start, torch.int64), d(key, torch.int32), d(count, torch.int32)
    poison = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=DEV)
    truth, cat, tally, changes = poison(R, W) if want_truth else None, poison(R, W) if want_category else None, poison(R, 2, 6), poison(R, 2)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().ake_track_score_i32(pred_d.data_ptr(), ptr(counts_d), start_d.data_ptr(), key_d.data_ptr(), count_d.data_ptr(), R, W,
                                              start.shape[1], hop, wf, sf, ptr(truth), ptr(cat), tally.data_ptr(), changes.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "ake_track_score_i32")
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (truth, cat, tally, changes))


def same(pred, counts, start, key, count, **geom):
    """Kernel == host restatement on every output; also with null truth / category pointers."""
    hop, wf, sf = geom.get("hop", HOP), geom.get("wf", WF), geom.get("sf", SF)
    want = metrics.track_score(pred, counts, start, key, count, hop, wf, sf)
    got = device_score(pred, counts, start, key, count, **geom)
    for name, g, w in zip(("truth", "category", "tally", "changes"), got, want):
        assert g.dtype == torch.int32 and torch.equal(g, w), name
    bare = device_score(pred, counts, start, key, count, want_truth=False, want_category=False, **geom)
    assert torch.equal(bare[2], want[2]) and torch.equal(bare[3], want[3])
    return got


def random_annotations(g, R, S, span):
    """Ascending random starts (segment 0 at 0) with random keys, some unlabelled, padded as KeyAnnotations pads; seg_count 1..S."""
    count = torch.randint(1, S + 1, (R,), generator=g, dtype=torch.int32)
    start = torch.full((R, S), 2 ** 63 - 1, dtype=torch.int64)
    key = torch.full((R, S), -1, dtype=torch.int32)
    for r in range(R):
        c = int(count[r])
        gaps = torch.randint(1, max(2, 2 * span // S), (c - 1,), generator=g, dtype=torch.int64)          # strictly ascending starts
        start[r, :c] = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(gaps, dim=0)])
        key[r, :c] = torch.randint(-1, 24, (c,), generator=g, dtype=torch.int32)
    return start, key, count


@pytest.mark.parametrize("W", [1, 17, 300])
def test_score_equals_the_host_restatement(W):
    """R = 3, up to 9 segments, random predictions with -1 among them; 300 windows are more than the block's threads."""
    g = torch.Generator().manual_seed(100 + W)
    span = (W * SF + WF) * HOP
    start, key, count = random_annotations(g, 3, 9, span)
    count[0] = 9
    pred = torch.randint(-1, 24, (3, W), generator=g, dtype=torch.int32)
    # make half of the predictions right or related, so that every category occurs
    truth, _ = metrics.window_truth(start, key, count, W, HOP, WF, SF)
    rel = torch.tensor([[k, *synthetic._related_keys(k)] for k in range(24)])
    pick = rel[truth.clamp_min(0).long(), torch.randint(0, 5, (3, W), generator=g)].to(torch.int32)
    pred = torch.where(torch.rand((3, W), generator=g) < 0.5, pick, pred)
    for counts in (None, [W, max(W // 2, 1), 0], [W + 5, 1, -3]):
        got = same(pred, counts, start, key, count)
    if W == 300:
        assert set(got[1].unique().tolist()) == {-1, 0, 1, 2, 3, 4, 5} and int(got[2][0, 1].sum()) > 0
    # another geometry: an odd hop, an even window, a stride of one frame
    start2, key2, count2 = random_annotations(g, 3, 9, (W + 6) * 441)
    same(pred, None, start2, key2, count2, hop=441, wf=6, sf=1)


def test_seg_count_zero_and_one_and_unlabelled_stretches():
    start = torch.tensor([[0, 2 ** 63 - 1, 2 ** 63 - 1], [0, 5, 9], [0, SF * HOP * 2, SF * HOP * 4], [0, 100, 200]], dtype=torch.int64)
    key = torch.tensor([[4, -1, -1], [7, 8, 9], [3, -1, 5], [-1, -1, -1]], dtype=torch.int32)
    count = torch.tensor([1, 0, 3, 3], dtype=torch.int32)
    g = torch.Generator().manual_seed(7)
    pred = torch.randint(-1, 24, (4, 8), generator=g, dtype=torch.int32)
    truth, cat, tally, changes = same(pred, [8, 8, 8, 8], start, key, count)
    assert truth[0].tolist() == [4] * 8 and truth[1].tolist() == [-1] * 8 and truth[2].tolist() == [3, -1, -1, 5, 5, 5, 5, 5]
    assert int(tally[1].abs().sum()) == 0 and changes[1].tolist() == [0, 0] and int(tally[3].abs().sum()) == 0
    assert bool((cat[1] == -1).all()) and bool((cat[3] == -1).all()) and int(tally[0, 0].sum()) == 8
    # seg_count beyond the array is clamped to it
    same(pred, None, start, key, torch.tensor([1, 0, 99, -2], dtype=torch.int32))


@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_a_boundary_on_and_beside_the_centre_sample(offset):
    start = torch.tensor([[0, CENTRE0 + offset, 2 ** 63 - 1], [0, CENTRE0 - 10, CENTRE0 + 10]], dtype=torch.int64)
    key = torch.tensor([[3, 7, -1], [3, 7, 3]], dtype=torch.int32)
    count = torch.tensor([2, 3], dtype=torch.int32)
    pred = torch.tensor([[7, 7], [3, 3]], dtype=torch.int32)
    truth, cat, tally, _ = same(pred, None, start, key, count)
    assert truth[0, 0] == (3 if offset > 0 else 7) and truth[1].tolist() == [7, 3]
    # recording 1: window 0 spans two boundaries back to the same key, window 1 lies across both: neither is pure
    assert tally[1, 0].tolist() == [1, 0, 0, 0, 1, 0] and tally[1, 1].tolist() == [0] * 6


# ---- end to end: track a modulating batch and score it ----

@pytest.fixture(scope="module")
def net(gold_default):
    opt = Namespace(**json.loads(str(gold_default["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold_default), strict=True)
    return net.to(DEV).eval()


def test_score_a_tracked_modulating_batch(net):
    """2 modulating recordings of 40 s, window 15 s, stride 5 s: 6 windows each.  The tallies add up to the scored windows and equal
    the host function on the track's own tensors, for both sources."""
    est = ake_amd.KeyEstimator(net, 22050, 5)
    audio, ann = synthetic.make_modulating_batch_device([0, 1], 40.0, DEV, min_seconds=5.0, mean_seconds=8.0)
    track = est.track(audio, window_seconds=15.0, stride_seconds=5.0, smooth=True)
    assert (track.hop, track.window_frames, track.stride_frames, track.sample_rate) == (4410, 76, 25, 22050)
    assert track.counts.tolist() == [6, 6]
    scores = {sm: track.score(ann, smoothed=sm) for sm in (False, True, None)}
    torch.cuda.synchronize()
    cpu = lambda t: t.cpu()
    for sm, source in ((False, track.key_id), (True, track.smooth_key_id)):
        s = scores[sm]
        assert isinstance(s, ake_amd.TrackScore) and s.truth.device.type == "cuda"
        want = metrics.track_score(cpu(source), cpu(track.counts), cpu(ann.seg_start), cpu(ann.seg_key), cpu(ann.seg_count), 4410, 76, 25)
        for g, w in zip((s.truth, s.category, s.tally, s.changes), want):
            assert torch.equal(cpu(g), w)
        assert s.tally[:, 0].sum(dim=1).tolist() == [6, 6] and int((s.truth >= 0).sum()) == 12          # every window is annotated
        assert bool((s.tally[:, 1] <= s.tally[:, 0]).all())
        centres = (track.times * 22050).round().long()                                                    # the truth sits at KeyTrack.times
        for r in range(2):
            segs = [(int(a), int(k)) for a, k in zip(ann.seg_start[r, :int(ann.seg_count[r])].tolist(), ann.seg_key[r].tolist())]
            assert s.truth[r].tolist() == [[k for a, k in segs if a <= int(c)][-1] for c in centres]
        per, pooled = s.weighted()
        assert per.shape == (2,) and 0.0 <= pooled <= 1.0 and s.fractions()[0].shape == (2, 6)
    assert int(scores[True].tally[:, 0, 5].sum()) == 0                                                    # the smoothed path always names a key
    assert all(torch.equal(a, b) for a, b in zip((scores[None].tally, scores[None].changes), (scores[True].tally, scores[True].changes)))
    plain = est.track(audio, window_seconds=15.0, stride_seconds=5.0)
    assert torch.equal(plain.score(ann).tally, scores[False].tally)
    with pytest.raises(ValueError):
        plain.score(ann, smoothed=True)
    bare = ake_amd.KeyTrack(plain.key, plain.tonic, plain.genre, plain.key_id, plain.sig, plain.tonic_id, plain.confidence, plain.counts, plain.times)
    with pytest.raises(ValueError):
        bare.score(ann)
    assert len(plain._tensors()) == 8                                                                     # (the geometry fields are no tensors)
