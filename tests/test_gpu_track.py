"""GPU: key tracking -- one CQT per recording, the net on sliding windows of its frames, the decode to key labels
(ake_pcnet_forward_windows_f32, ake_decode_keys_f32, ake_pipeline_track_f32 / KeyEstimator.track)."""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics, synthetic
from conftest import golden_state_dict, rel_err
from oracle import cqt_oracle, pcnet_oracle
from test_track_host import GAP, signature_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WF, SF = 76, 25                      # 15 s windows, 5 s stride at 5 frames per second
N45 = 992250                         # 45 s at 22.05 kHz: 226 frames, 7 windows


def make_net(gold):
    opt = Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(golden_state_dict(gold), strict=True)
    return net.to(DEV).eval(), opt


@pytest.fixture(scope="module")
def net(gold_default):
    return make_net(gold_default)[0]


@pytest.fixture(scope="module")
def est(net):
    return ake_amd.KeyEstimator(net, 22050, 5)


@pytest.fixture(scope="module")
def recordings():
    """2 recordings of 45 s whose key changes: three 15 s clips of different keys each, concatenated."""
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7))]
    audio = np.stack(rows).astype(np.float32)
    assert audio.shape == (2, N45)
    return audio


@pytest.fixture(scope="module")
def track45(est, recordings):
    tr = est.track(torch.from_numpy(recordings).to(DEV))
    torch.cuda.synchronize()
    return tr


def forward_windows(net, mel, frames_major, wf, sf):
    """ake_pcnet_forward_windows_f32 on mel (R, T, P) [frames_major] or (R, P, T)."""
    L = ake_amd._lib.lib()
    net._sync_weights(torch.device(DEV), for_eval=True)
    R = mel.shape[0]
    T = mel.shape[1] if frames_major else mel.shape[2]
    W = (T - wf) // sf + 1
    outs = [torch.full((R, W, n), float("nan"), dtype=torch.float32, device=DEV) for n in (12, 12, 11)]
    nbytes = L.ake_pcnet_forward_windows_workspace_bytes(net._h, R, T, wf, sf)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ake_amd._lib.check(L.ake_pcnet_forward_windows_f32(net._h, mel.data_ptr(), 1 if frames_major else 0, R, T, wf, sf, outs[0].data_ptr(),
                                                       outs[1].data_ptr(), outs[2].data_ptr() if net.genre else None, ws.data_ptr(), ws.numel(),
                                                       torch.cuda.current_stream().cuda_stream), "ake_pcnet_forward_windows_f32")
    return outs if net.genre else outs[:2]


def materialised(net, mel_rows, wf, sf, chunk=None):
    """ake_pcnet_forward_f32 on the windows of mel_rows (R, P, T) cut with unfold(...).contiguous(); `chunk`: windows per call."""
    R, Pn, T = mel_rows.shape
    win = mel_rows.unfold(2, wf, sf).permute(0, 2, 1, 3).contiguous()                # (R, W, P, wf)
    W = win.shape[1]
    x = win.reshape(R * W, 1, Pn, wf)
    seq = torch.full((R * W,), wf, device=DEV)
    parts = [net(x[c:c + (chunk or R * W)], seq[c:c + (chunk or R * W)]) for c in range(0, R * W, chunk or R * W)]
    return [torch.cat([p[i] for p in parts]).reshape(R, W, -1) for i in range(len(parts[0]))]


def test_windows_equal_materialised_slices_bit_for_bit(net):
    """Frames-major mel, 2 recordings x 226 frames, window 76, stride 25 (7 windows each): the windows forward changes where the net's
    input is read from, not what is computed."""
    g = torch.Generator().manual_seed(7)
    mel_fm = (torch.rand((2, 226, 288), generator=g) * 3).to(DEV)
    got = forward_windows(net, mel_fm, True, WF, SF)
    want = materialised(net, mel_fm.transpose(1, 2).contiguous(), WF, SF)
    assert got[0].shape == (2, 7, 12) and got[2].shape == (2, 7, 11)
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert (got[1][0, 0] - got[1][0, 1]).abs().max() > 0                             # the windows do differ


def test_gather_path_row_major_and_variant_net_bit_for_bit(net, gold_staysixth):
    g = torch.Generator().manual_seed(8)
    mel = (torch.rand((2, 288, 226), generator=g) * 3).to(DEV)                       # [recording][bin][frame], as the ragged CQT leaves it
    for a, b in zip(forward_windows(net, mel, False, WF, SF), materialised(net, mel, WF, SF)):
        assert torch.equal(a, b)
    var, opt = make_net(gold_staysixth)
    assert var.stay_sixth
    Pn = opt.octaves * 36
    mel_v = (torch.rand((2, 226, Pn), generator=g) * 3).to(DEV)
    want = materialised(var, mel_v.transpose(1, 2).contiguous(), WF, SF)
    for fm, m in ((True, mel_v), (False, mel_v.transpose(1, 2).contiguous())):
        got = forward_windows(var, m, fm, WF, SF)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_windows_run_in_chunks_across_recordings(net):
    """3 recordings x 100 windows: the forward runs 256 windows at a time, and the second call starts inside recording 2."""
    g = torch.Generator().manual_seed(9)
    mel_fm = (torch.rand((3, 76 + 99 * 5, 288), generator=g) * 3).to(DEV)
    got = forward_windows(net, mel_fm, True, WF, 5)
    want = materialised(net, mel_fm.transpose(1, 2).contiguous(), WF, 5, chunk=256)
    assert got[0].shape == (3, 100, 12)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_single_window_track_equals_the_clip_call(est):
    audio = synthetic.make_batch_device(range(5), torch.device(DEV))[0]
    assert audio.shape[1] == 330750
    tr = est.track(audio)
    key, tonic, genre = est(audio)
    assert tr.key.shape == (5, 1, 12) and tr.counts.tolist() == [1] * 5 and tr.times.tolist() == [7.5]
    assert torch.equal(tr.key[:, 0], key) and torch.equal(tr.tonic[:, 0], tonic) and torch.equal(tr.genre[:, 0], genre)


def test_track_end_to_end_against_the_oracle(track45, recordings, gold_default):
    tr = track45
    assert tr.key.shape == (2, 7, 12) and tr.tonic.shape == (2, 7, 12) and tr.genre.shape == (2, 7, 11)
    assert tr.counts.tolist() == [7, 7] and tr.times.tolist() == pytest.approx([7.5 + 5 * w for w in range(7)])
    sd = golden_state_dict(gold_default, torch.float64)
    with torch.no_grad():
        mel = cqt_oracle.FastDirectCQT(22050, 4410, dtype=torch.float64)(recordings)          # (2, 288, 226): ONE transform per recording
        assert mel.shape == (2, 288, 226)
        win = mel.unfold(2, WF, SF).permute(0, 2, 1, 3).reshape(14, 1, 288, WF)
        ref = pcnet_oracle.pcnet_forward(sd, win, torch.full((14,), WF))
    for name, a, b in zip(("key", "tonic", "genre"), (tr.key, tr.tonic, tr.genre), ref):
        err = rel_err(a.cpu().reshape(14, -1), b)
        print(f"track {name}: rel err vs oracle {err:.2e}")
        assert err < 1e-3, name
    segs = tr.segments(0)                                                                     # (reads the device tensors)
    assert segs[0][0] == 0.0 and segs[-1][1] == pytest.approx(37.5 + 7.6) and all(a[1] == pytest.approx(b[0]) for a, b in zip(segs, segs[1:]))
    assert (tr.tonic[0, 0] - tr.tonic[0, 6]).abs().max() > 0                                  # the track does change


def test_ragged_batch_counts_and_padding_windows(est, recordings):
    lens = [N45, 500000]
    rows = torch.from_numpy(recordings).clone()
    rows[1, lens[1]:] = 7.0                                                                    # never read
    tr = est.track(rows.to(DEV), lengths=torch.tensor(lens))
    assert tr.counts.tolist() == [7, 2] and tr.key.shape == (2, 7, 12)
    alone = est.track(torch.from_numpy(recordings[1:2, :lens[1]].copy()).to(DEV))
    assert alone.counts.tolist() == [2] and alone.key.shape == (1, 2, 12)
    assert (tr.key[1, :2] - alone.key[0]).abs().max() < 1e-5
    assert rel_err(tr.tonic[1, :2].cpu(), alone.tonic[0].cpu()) < 2e-5 and rel_err(tr.genre[1, :2].cpu(), alone.genre[0].cpu()) < 2e-5
    for t in (tr.key_id, tr.sig, tr.tonic_id):
        assert t.dtype == torch.int32 and bool((t[1, 2:] == -1).all())                        # windows at index >= count decode to -1
    assert bool((tr.confidence[1, 2:] == 0).all())
    assert bool((tr.sig[0] >= 0).all()) and bool((tr.sig[1, :2] >= 0).all()) and bool((tr.tonic_id[1, :2] >= 0).all())
    assert (tr.confidence[1, :2] - alone.confidence[0]).abs().max() < 1e-5
    assert len(tr.segments(1)) >= 1 and tr.segments(1)[-1][1] == pytest.approx(float(tr.times[1]) + 7.6)


def test_device_decode_equals_host_decode(recordings, track45, gold_default):
    """ake_decode_keys_f32 against metrics.decode_keys and the float64 restatement, on the outputs of track() at a 1 s stride (31
    windows per recording).  A window whose two best distinct table rows are closer than 1e-5 in float64 has no defined float32
    winner and is left out of the sig comparison; the test fails if that is more than 5 % of the windows.

    The fixture's seeded (untrained) weights give a key output that is flat over the pitch classes (0.52506 +- 1e-5: every window
    would be left out), so this net is the fixture's with its last key-head convolution scaled by 2e4 around the flat logit
    (weight * s, bias -> s * (bias - mean logit)): the same map, amplified until the pitch classes differ."""
    s = 2e4
    m = float(torch.logit(track45.key.double()).mean())
    sd = golden_state_dict(gold_default)
    sd["key_classifier.3.conv2d.bias"] = (sd["key_classifier.3.conv2d.bias"].double() - m).mul(s).float()
    sd["key_classifier.3.conv2d.weight"] = sd["key_classifier.3.conv2d.weight"] * s
    opt = Namespace(**json.loads(str(gold_default["opt"])))
    net2 = ake_amd.PitchClassNet(288, 12, opt.num_layers, opt.kernel_size, opt)
    net2.load_state_dict(sd, strict=True)
    est2 = ake_amd.KeyEstimator(net2.to(DEV).eval(), 22050, 5)
    tr = est2.track(torch.from_numpy(recordings).to(DEV), stride_seconds=1.0)
    assert tr.key.shape == (2, 31, 12)
    spread = float((tr.key.max(dim=2).values - tr.key.min(dim=2).values).median())
    print(f"decode: median spread of a window's key outputs {spread:.3f}")
    assert spread > 0.05
    key, tonic = tr.key.reshape(-1, 12), tr.tonic.reshape(-1, 12)
    want_sig, want_conf, gap = signature_reference(key.cpu().numpy())
    keep = gap >= GAP
    print(f"decode: {int((~keep).sum())} of {len(keep)} windows left out ({100.0 * (~keep).mean():.1f} %), smallest gap {gap.min():.2e}")
    assert (~keep).mean() <= 0.05
    h_key_id, h_sig, h_tonic, h_conf = metrics.decode_keys(key.cpu(), tonic.cpu())
    d_sig, d_tonic, d_key_id = (t.reshape(-1).cpu().numpy() for t in (tr.sig, tr.tonic_id, tr.key_id))
    assert np.array_equal(d_sig[keep], h_sig.numpy()[keep]) and np.array_equal(d_sig[keep], want_sig[keep])
    assert np.array_equal(d_tonic, h_tonic.numpy())            # (distinct float32 logits: the argmax is exact on both sides)
    assert np.array_equal(d_key_id[keep], h_key_id.numpy()[keep])
    assert np.abs(tr.confidence.reshape(-1).cpu().numpy() - want_conf).max() < 1e-5
    # the same decode on the device through torch ops
    g_key_id, g_sig, g_tonic, _ = metrics.decode_keys(key, tonic)
    assert np.array_equal(g_sig.cpu().numpy()[keep], d_sig[keep]) and np.array_equal(g_tonic.cpu().numpy(), d_tonic)
    # the entry point on its own, with counts
    L = ake_amd._lib.lib()
    counts = torch.tensor([31, 4], dtype=torch.int32, device=DEV)
    outs = [torch.empty(62, dtype=torch.int32, device=DEV) for _ in range(3)] + [torch.empty(62, dtype=torch.float32, device=DEV)]
    ake_amd._lib.check(L.ake_decode_keys_f32(key.data_ptr(), tonic.data_ptr(), 62, counts.data_ptr(), 31, *(o.data_ptr() for o in outs),
                                             torch.cuda.current_stream().cuda_stream), "ake_decode_keys_f32")
    assert torch.equal(outs[1][:35], tr.sig.reshape(-1)[:35]) and bool((outs[1][35:] == -1).all()) and bool((outs[0][35:] == -1).all())
    assert torch.equal(outs[0][:35], tr.key_id.reshape(-1)[:35]) and bool((outs[2][35:] == -1).all())


def test_two_streams_give_the_same_track(net, est, recordings):
    est2 = ake_amd.KeyEstimator(net, 22050, 5, streams=2)
    audio = torch.from_numpy(recordings).to(DEV)
    lengths = torch.tensor([N45, 500000], device=DEV)
    got = [est2.track(audio), est2.track(audio, lengths), est2.track(audio, stride_seconds=1.0)]
    est2.join()
    torch.cuda.synchronize()
    want = [est.track(audio), est.track(audio, lengths), est.track(audio, stride_seconds=1.0)]
    for a, b in zip(got, want):
        for x, y in zip(a._tensors(), b._tensors()):
            assert torch.equal(x, y)
        assert torch.equal(a.times, b.times)
    assert est2._slots[0]["stream"] is not None and est2._slots[1]["stream"] is not None


def test_sample_rate_and_channels_go_through_the_resampler(est, recordings):
    rs = ake_amd.get_resampler(44100, 22050, torch.device(DEV))
    g = torch.Generator().manual_seed(3)
    stereo = (torch.rand((2, 2, 2 * N45), generator=g) - 0.5).to(DEV)
    tr = est.track(stereo, rate=44100, channel=1)
    assert tr.key.shape == (2, 7, 12) and tr.counts.tolist() == [7, 7]
    for t in (tr.key, tr.tonic, tr.genre, tr.confidence):
        assert bool(torch.isfinite(t).all())
    pre, _ = rs(stereo, channel=1, lengths=None)
    want = est.track(pre)
    for x, y in zip(tr._tensors(), want._tensors()):
        assert torch.equal(x, y)


def test_long_recordings_split_into_more_cascade_segments_bit_for_bit(est, recordings):
    """A small batch of long recordings runs the decimator cascade in more segments per recording than a full batch does (12 against 4
    for 45 s); every segment warms up on its own history, so the split must not change a value."""
    one = torch.from_numpy(recordings[:1]).to(DEV)
    alone = est.plan.logmag(one)                                      # 1 recording: 244 ticks, 12 segments
    many = est.plan.logmag(one.repeat(256, 1))                        # 256 recordings: 4 segments each
    assert alone.shape == (1, 288, 226) and torch.equal(many[0], alone[0]) and torch.equal(many[255], alone[0])


def test_recordings_shorter_than_one_window_give_an_empty_track(est):
    audio = synthetic.make_batch_device(range(2), torch.device(DEV), n_samples=22050 * 10)[0]
    tr = est.track(audio)
    assert tr.key.shape == (2, 0, 12) and tr.key_id.shape == (2, 0) and tr.counts.tolist() == [0, 0] and len(tr.times) == 0
    assert tr.segments(0) == [] and tr.segments(1) == []
