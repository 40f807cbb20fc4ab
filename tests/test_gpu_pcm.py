"""PARITY (GPU): 16-bit PCM audio through every layer.  A sample s means float(s) * 2^-15, which is exact, so every PCM route is held to
bit identity (torch.equal) with the float32 route on ``pcm16_to_float(pcm)``."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, synthetic
from ake_amd.cqt import hop_for_window
from conftest import golden_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
to_f = ake_amd.pcm16_to_float


def pcm_clip(i, n, sr=SR):
    """Clip i of the synthetic set as 16-bit PCM (CPU, (n,) int16)."""
    w = synthetic.make_clip(i, n, sr)[0]
    return torch.from_numpy(np.clip(np.rint(w * 32767.0), -32768, 32767).astype(np.int16))


def padded_rows(clips, fill=32767, extra=0):
    """Clips of any lengths as the rows of one (B, n_max + extra) int16 tensor on the device, `fill` behind every clip's end."""
    n = max(c.numel() for c in clips)
    rows = torch.full((len(clips), n + extra), fill, dtype=torch.int16)
    for r, c in zip(rows, clips):
        r[:c.numel()] = c
    return rows.to(DEV)


def float_rows(rows, lens):
    """The float comparand of padded_rows: converted samples, zeros behind every clip's end."""
    f = to_f(rows)
    for r, n in zip(f, lens):
        r[n:] = 0.0
    return f


@pytest.fixture(scope="module")
def plan():
    return ake_amd.get_plan(SR, 4410, 288, 36, DEV)


@pytest.fixture(scope="module")
def net(gold_default):
    n = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True))
    n.load_state_dict(golden_state_dict(gold_default), strict=True)
    return n.to(DEV).eval()


def c_logmag(plan, audio, row_stride, frames_major):
    """The C entries directly, equal-length rows: (return code, output).  int16 -> ake_cqt_logmag_pcm16_f32, float32 -> the float entry."""
    L = _lib.lib()
    B, n = audio.shape
    T = plan.num_frames(n)
    out = torch.full((B, T, plan.n_bins) if frames_major else (B, plan.n_bins, T), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(int(L.ake_cqt_workspace_bytes(plan.handle, B, n)), 256), dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    if audio.dtype == torch.int16:
        rc = L.ake_cqt_logmag_pcm16_f32(plan.handle, audio.data_ptr(), B, n, row_stride, None, None, out.data_ptr(), T, int(frames_major),
                                        ws.data_ptr(), ws.numel(), s)
    elif frames_major:
        rc = L.ake_cqt_logmag_frames_major_f32(plan.handle, audio.data_ptr(), B, n, row_stride, out.data_ptr(), ws.data_ptr(), ws.numel(), s)
    else:
        rc = L.ake_cqt_logmag_f32(plan.handle, audio.data_ptr(), B, n, row_stride, out.data_ptr(), T, ws.data_ptr(), ws.numel(), s)
    return rc, out


# ---- 1. CQT ---------------------------------------------------------------------------------------------------------------------------

def test_cqt_ragged_rows_with_foreign_samples_behind_their_ends(plan):
    lens = [SR * 6 + 1, SR * 6 + 2, 7, 1]
    clips = [pcm_clip(i, n) for i, n in enumerate(lens)]
    clips[0][100], clips[0][101] = -32768, 32767                       # the extreme values are present
    rows = padded_rows(clips)                                           # (4, 6 s + 2): even stride, read in place
    assert rows.stride(0) % 2 == 0
    got = plan.logmag(rows, lengths=torch.tensor(lens))
    ref = plan.logmag(float_rows(rows, lens), lengths=torch.tensor(lens))
    assert torch.equal(got, ref) and float(ref.abs().max()) > 0.1


@pytest.mark.parametrize("frames_major", [False, True])
def test_cqt_equal_rows_of_odd_length(plan, frames_major):
    n = SR * 6 + 3                                                      # odd, and no multiple of 4: every row's last sample shares its
    rows = padded_rows([pcm_clip(i, n) for i in range(4)], extra=1)     # 4-byte word with a foreign 32767
    pcm = rows[:, :n]
    assert pcm.stride(0) % 2 == 0 and int(rows[0, n]) == 32767
    rc, got = c_logmag(plan, pcm, pcm.stride(0), frames_major)
    assert rc == 0
    fl = to_f(pcm).contiguous()
    rc, ref = c_logmag(plan, fl, fl.stride(0), frames_major)
    assert rc == 0
    assert torch.equal(got, ref) and torch.isfinite(ref).all()
    if not frames_major:
        assert torch.equal(plan.logmag(pcm), ref)                       # the Python layer takes the same strided view in place


@pytest.mark.parametrize("frames_major", [False, True])
def test_cqt_one_long_clip_over_several_cascade_segments(plan, frames_major):
    pcm = pcm_clip(3, synthetic.N_SAMPLES)[None].to(DEV)                # 15 s
    pcm[0, 5000], pcm[0, 5001], pcm[0, -1] = -32768, 32767, -32768
    rc, got = c_logmag(plan, pcm, pcm.stride(0), frames_major)
    assert rc == 0
    fl = to_f(pcm)
    assert float(fl.min()) == -1.0 and float(fl.max()) == 32767.0 / 32768.0
    rc, ref = c_logmag(plan, fl, fl.stride(0), frames_major)
    assert rc == 0 and torch.equal(got, ref)


def test_cqt_whole_song_hops():
    hplan = ake_amd.get_any_hop_plan(SR, 288, 36, DEV)
    lens = [SR * 7, SR * 9]
    rows = padded_rows([pcm_clip(i, n) for i, n in enumerate(lens)])
    lengths = torch.tensor(lens, device=DEV)
    hops = hop_for_window(lengths).to(torch.int32)
    got = hplan.logmag_hops(rows, hops, lengths, out_frames=592)
    ref = hplan.logmag_hops(float_rows(rows, lens), hops, lengths, out_frames=592)
    assert torch.equal(got, ref) and float(ref.abs().max()) > 0.1


@pytest.mark.parametrize("engine", [1, 2, 5])
def test_cqt_other_engines_refuse_pcm_by_name(engine):
    p = ake_amd.CQTPlan(SR, 4410, 216, 36, device=DEV, engine=engine)
    pcm = pcm_clip(0, SR * 2)[None].to(DEV)
    with pytest.raises(_lib.AkeError, match=r"\(-5\).*engine 3"):       # AKE_ERR_UNSUPPORTED, and the message names the engine that can
        p.logmag(pcm)


def test_cqt_entry_refuses_an_odd_stride(plan):
    pcm = padded_rows([pcm_clip(i, 4411) for i in range(2)])            # contiguous (2, 4411): row 1 starts in the middle of a word
    rc, _ = c_logmag(plan, pcm, pcm.stride(0), False)
    assert rc == -1                                                     # AKE_ERR_INVALID
    assert b"4-byte aligned" in _lib.lib().ake_last_error()


def test_cqt_copy_path_for_a_contiguous_tensor_of_odd_length(plan):
    pcm = padded_rows([pcm_clip(i, 132301) for i in range(3)])
    assert pcm.is_contiguous() and pcm.shape == (3, 132301)
    assert torch.equal(plan.logmag(pcm), plan.logmag(to_f(pcm)))


# ---- 2. resampler ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stereo():
    """(3, 2, 30011) int16, planar, with the extreme values in it."""
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-32768, 32768, (3, 2, 30011), generator=g, dtype=torch.int32).to(torch.int16)
    x[0, 0, 0], x[0, 1, 0] = -32768, 32767
    return x.to(DEV)


@pytest.mark.parametrize("rate_in", [48000, 44100])
def test_resampler_planar_and_interleaved(stereo, rate_in):
    rs = ake_amd.Resampler(rate_in, SR, DEV)
    inter = stereo.transpose(1, 2).contiguous().transpose(1, 2)         # (B, n, C) storage as the zero-copy (B, C, n) view
    assert inter.stride() == (2 * 30011, 1, 2) and torch.equal(inter, stereo)
    for channel in (0, 1, -1):
        ref, ref_len = rs(to_f(stereo), channel=channel)
        for x in (stereo, inter):
            got, got_len = rs(x, channel=channel)
            assert torch.equal(got, ref) and torch.equal(got_len, ref_len), (rate_in, channel)


def test_resampler_identity_and_ragged(stereo):
    same, _ = ake_amd.Resampler(SR, SR, DEV)(stereo, channel=0)
    assert torch.equal(same, to_f(stereo[:, 0]))
    lens = [20000, 12345, 7, 19999]
    rows = padded_rows([pcm_clip(i, n) for i, n in enumerate(lens)])[:, None, :]
    rs = ake_amd.Resampler(48000, SR, DEV)
    got, got_len = rs(rows, lengths=torch.tensor(lens))
    ref, ref_len = rs(float_rows(rows[:, 0], lens)[:, None, :], lengths=torch.tensor(lens))
    assert torch.equal(got, ref) and torch.equal(got_len, ref_len)


# ---- 3. pipeline ----------------------------------------------------------------------------------------------------------------------

def same_outputs(a, b):
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_pipeline_equal_and_ragged(net):
    est = ake_amd.KeyEstimator(net, SR, 5)
    eq = padded_rows([pcm_clip(i, SR * 7) for i in range(3)])
    same_outputs(est(eq), est(to_f(eq)))
    # the old silent route read the samples unscaled, 32 768 times too loud: what an int16 batch gives has changed, on purpose
    assert not torch.equal(est(eq)[0], est(eq.float())[0])
    lens = [SR * 6 + 1, SR * 9, SR * 15 // 2 + 3]
    rows = padded_rows([pcm_clip(i, n) for i, n in enumerate(lens)])
    same_outputs(est(rows, lengths=torch.tensor(lens)), est(float_rows(rows, lens), lengths=torch.tensor(lens)))
    true_end = ake_amd.KeyEstimator(net, SR, 5, wrap_mode="true_end")
    same_outputs(true_end(rows, lengths=torch.tensor(lens)), true_end(float_rows(rows, lens), lengths=torch.tensor(lens)))


def test_pipeline_side_streams_and_join(net):
    est = ake_amd.KeyEstimator(net, SR, 5, streams=2)
    a = padded_rows([pcm_clip(i, SR * 6) for i in range(3)])
    b = padded_rows([pcm_clip(i + 3, SR * 8) for i in range(3)])
    got_a, got_b = est(a), est(b)
    est.join()
    ref = ake_amd.KeyEstimator(net, SR, 5)
    same_outputs(got_a, ref(to_f(a)))
    same_outputs(got_b, ref(to_f(b)))


def test_pipeline_interleaved_stereo_at_48k(net):
    n = 48000 * 6 + 1
    planar = torch.stack([torch.stack([pcm_clip(2 * b + c, n, 48000) for c in range(2)]) for b in range(2)]).to(DEV)   # (2, 2, n)
    inter = planar.transpose(1, 2).contiguous().transpose(1, 2)
    est = ake_amd.KeyEstimator(net, SR, 5)
    same_outputs(est(inter, rate=48000, channel=-1), est(to_f(planar), rate=48000, channel=-1))


def test_pipeline_whole_song_estimator(net):
    est = ake_amd.KeyEstimator(net, SR, 0)
    lens = [SR * 7, SR * 9]
    rows = padded_rows([pcm_clip(i, n) for i, n in enumerate(lens)])
    same_outputs(est(rows, lengths=torch.tensor(lens)), est(float_rows(rows, lens), lengths=torch.tensor(lens)))


# ---- 4. track -------------------------------------------------------------------------------------------------------------------------

def same_tracks(a, b):
    ta, tb = a._tensors(), b._tensors()
    assert len(ta) == len(tb)
    for x, y in zip(ta, tb):
        assert (x is None and y is None) or torch.equal(x, y)
    assert torch.equal(a.times, b.times)


def test_track_ragged_recordings_smooth_with_posteriors(net):
    est = ake_amd.KeyEstimator(net, SR, 5)
    lens = [SR * 40, SR * 33]
    rows = padded_rows([pcm_clip(i, n) for i, n in enumerate(lens)])
    kw = dict(lengths=torch.tensor(lens), window_seconds=15.0, stride_seconds=5.0, smooth=True, posteriors=True)
    got, ref = est.track(rows, **kw), est.track(float_rows(rows, lens), **kw)
    assert got.posteriors is not None and len(got._tensors()) == 13 and got.counts.tolist() == [6, 4]
    same_tracks(got, ref)
    same_tracks(est.track(rows[:1, :lens[0]]), est.track(to_f(rows[:1, :lens[0]])))   # equal-length form (frames-major route)


# ---- 5. HostFeeder --------------------------------------------------------------------------------------------------------------------

def test_host_feeder_matches_direct_calls_in_order(net):
    est = ake_amd.KeyEstimator(net, SR, 5)
    sizes, lens = [3, 5, 2, 5, 1], [SR * 6, SR * 8 + 1, SR * 9 + 2, SR * 7 + 3, SR * 6 - 5]      # the buffers grow, then are reused
    batches = []
    for k, (B, n) in enumerate(zip(sizes, lens)):
        pcm = torch.stack([pcm_clip(10 * k + i, n) for i in range(B)])
        batches.append(pcm if k % 2 == 0 else to_f(pcm))                # int16, float32, int16, float32, int16
    batches[2] = batches[2].pin_memory()
    # (every row is a clip of several seconds: a row of a few samples has one frame, which the net's time pooling halves to none, and
    # the mean over no frame is NaN, as the reference's torch.mean is -- equal on both routes, but not torch.equal)
    ragged = torch.tensor([lens[3], lens[3] - 4411, SR * 6 + 7, lens[3] - 1, SR * 6])
    batches[3] = (batches[3], ragged)
    results = list(ake_amd.HostFeeder(est, depth=2)(batches))
    assert len(results) == 5
    for item, got in zip(batches, results):
        x, l = item if isinstance(item, tuple) else (item, None)
        same_outputs(got, est(x.to(DEV), lengths=l))


def test_host_feeder_interleaved_stereo_and_track(net):
    est = ake_amd.KeyEstimator(net, SR, 5)
    n = 48000 * 6 + 1
    inter = torch.stack([torch.stack([pcm_clip(2 * b + c, n, 48000) for c in range(2)]) for b in range(2)]).transpose(1, 2).contiguous().transpose(1, 2)
    (got,) = list(ake_amd.HostFeeder(est, depth=2, rate=48000, channel=-1)([inter]))
    same_outputs(got, est(inter.to(DEV), rate=48000, channel=-1))
    recs = [pcm_clip(0, SR * 33)[None], to_f(pcm_clip(1, SR * 26 + 1))[None]]
    tracks = list(ake_amd.HostFeeder(est, depth=2, track=True, smooth=True)(recs))
    for x, got in zip(recs, tracks):
        same_tracks(got, est.track(x.to(DEV), smooth=True))


def test_host_feeder_refuses_bad_arguments(net):
    est = ake_amd.KeyEstimator(net, SR, 5)
    with pytest.raises(ValueError):
        ake_amd.HostFeeder(est, depth=0)
    with pytest.raises(ValueError):
        list(ake_amd.HostFeeder(est)([torch.zeros((1, SR), dtype=torch.int16, device=DEV)]))


# ---- 6. KeyDataset --------------------------------------------------------------------------------------------------------------------

def test_keydataset_takes_int16_waveforms():
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5, octaves=8,
                    local=False, only_semitones=False, multi_scale=False)
    waves = [pcm_clip(i, n).numpy() for i, n in enumerate((SR * 4, SR * 4, SR * 5 + 1))]
    items = []
    for ws in (waves, [w.astype(np.float32) / 32768.0 for w in waves]):
        ds = ake_amd.KeyDataset(False, opt)
        ds.import_data(ake_amd.WaveformLoader("clips", ws, [3, 14, 20], SR), shuffle=False)
        items.append([ds[i]["mel"] for i in range(3)])
    for a, b in zip(*items):
        assert torch.equal(a, b) and float(a.abs().max()) > 0.1
