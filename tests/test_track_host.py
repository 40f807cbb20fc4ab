"""Key tracking, the parts that need no GPU: the decode (``metrics.decode_keys``), the window arithmetic, ``KeyTrack.segments`` and the
refusals of ``KeyEstimator.track`` / ``ake_pcnet_forward_windows_f32``."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics
from ake_amd import pipeline as P
from ake_amd.KeyDataset import SIGNATURE
from oracle import mirex_oracle

GAP = 1e-5      # a row whose two best DISTINCT table rows are closer than this in float64 has no defined float32 winner


def signature_reference(key_preds):
    """float64 numpy restatement of models.py:1065-1083 for every row: (first-maximum row index over the 21-row table, that cosine,
    gap between the best and the second best of the 12 distinct rows -- the 15 circle-of-fifths rows hold 12 distinct scales)."""
    table = mirex_oracle.key_signature_map().astype(np.float64)
    distinct = np.unique(table, axis=0)
    assert distinct.shape == (12, 12)
    kp = np.asarray(key_preds, np.float64)
    sig, conf, gap = [], [], []
    for row in kp:
        pn = max(np.sqrt((row * row).sum()), 1e-8)
        sims = (table * row).sum(1) / (pn * np.maximum(np.sqrt((table * table).sum(1)), 1e-8))
        sig.append(int(np.argmax(sims)))                       # numpy's argmax is the first maximum
        conf.append(float(sims.max()))
        top = np.sort((distinct * row).sum(1) / (pn * np.sqrt(7.0)))
        gap.append(float(top[-1] - top[-2]))
    return np.array(sig), np.array(conf), np.array(gap)


def test_decode_sig_equals_the_float64_restatement_on_the_fixture(gold_mirex):
    kp, tp = gold_mirex["key_preds"], gold_mirex["tonic_preds"]
    assert kp.shape == (96, 12) and tp.shape == (96, 12)
    want, conf, gap = signature_reference(kp)
    keep = gap >= GAP
    print(f"smallest top-two gap {gap.min():.3e}; rows left out: {int((~keep).sum())} of {len(keep)}")
    assert keep.all()                                          # the fixture's smallest gap is 1.4e-4: nothing is left out
    key_id, sig, tonic_id, confidence = metrics.decode_keys(torch.from_numpy(kp), torch.from_numpy(tp))
    assert sig.dtype == torch.int32 and key_id.dtype == torch.int32 and tonic_id.dtype == torch.int32
    assert np.array_equal(sig.numpy()[keep], want[keep])
    assert np.array_equal(tonic_id.numpy(), np.argmax(tp, axis=1))      # (numpy: first maximum)
    assert np.abs(confidence.numpy() - conf).max() < 1e-6
    # leading dimensions are kept
    k3 = metrics.decode_keys(torch.from_numpy(kp).reshape(8, 12, 12), torch.from_numpy(tp).reshape(8, 12, 12))
    assert k3[0].shape == (8, 12) and torch.equal(k3[0].reshape(-1), key_id) and torch.equal(k3[3].reshape(-1), confidence)


def test_key_id_rule_on_the_circle_of_fifths():
    table = metrics.KEY_SIGNATURE_MAP
    for row in range(15):
        major = (7 * (row - 7)) % 12
        minor = (major + 9) % 12
        key = table[row][None].repeat(12, 1) * 0.9 + 0.05           # the scale's own row is the unique best match
        tonic = torch.eye(12)
        key_id, sig, tonic_id, conf = metrics.decode_keys(key, tonic)
        first = int(torch.nonzero((table == table[row]).all(1))[0])  # rows 0/12, 1/13, 2/14 are the same scale: the first one wins
        assert sig.tolist() == [first] * 12 and tonic_id.tolist() == list(range(12))
        for t in range(12):
            want = 12 + t if t == major else t if t == minor else -1
            assert int(key_id[t]) == want, (row, t)
        assert metrics.KEY_NAMES[12 + major].endswith("major") and metrics.KEY_NAMES[minor].endswith("minor")
    assert len(metrics.KEY_NAMES) == 24 and metrics.KEY_NAMES[9] == "A minor" and metrics.KEY_NAMES[12] == "C major"
    assert list(metrics.KEY_NAMES) == list(SIGNATURE)
    # C major scale, tonic C -> "C major"; tonic A -> "A minor"; tonic D -> no key
    c_major = table[7][None]
    ids = [int(metrics.decode_keys(c_major, torch.eye(12)[t][None])[0]) for t in (0, 9, 2)]
    assert ids == [12, 9, -1]


def test_window_arithmetic_against_a_brute_force_loop():
    assert P.track_window_frames(330750, 4410) == 76                # 15 s at 22.05 kHz, 5 frames per second: the benchmarked shape
    assert P.track_window_frames(round(15.0 * 44100), 8820) == 76
    assert P.track_stride_frames(5.0, 5) == 25 and P.track_stride_frames(1.0, 5) == 5 and P.track_stride_frames(0.01, 5) == 1
    assert P.track_stride_frames(0.5, 5) == round(2.5)              # Python's round: half to even
    for wf in (1, 7, 76):
        for sf in (1, 5, 25, 76, 100):
            for T in list(range(0, 200)) + [1501]:
                brute = sum(1 for w in range(T + 1) if w * sf + wf <= T)
                assert P.track_counts(T, wf, sf) == brute, (T, wf, sf)
            Ts = torch.arange(0, 300)
            assert P.track_counts(Ts, wf, sf).tolist() == [P.track_counts(int(t), wf, sf) for t in Ts]
    assert P.track_counts(75, 76, 25) == 0 and P.track_counts(76, 76, 25) == 1
    assert P.track_counts(1 + 992250 // 4410, 76, 25) == 7 and P.track_counts(1 + 500000 // 4410, 76, 25) == 2


def _track(key_id, counts, wf=76, sf=25, hop=4410, sr=22050):
    key_id = torch.tensor(key_id, dtype=torch.int32)
    R, W = key_id.shape
    z = torch.zeros((R, W, 12))
    times = (torch.arange(W, dtype=torch.float64) * sf + (wf - 1) / 2) * hop / sr
    return P.KeyTrack(z, z, None, key_id, key_id, key_id, torch.zeros((R, W)), torch.tensor(counts, dtype=torch.int32), times,
                      wf * hop / sr, sf * hop / sr)


def test_segments_run_length_encode_key_id():
    tr = _track([[9, 9, 9, 12, 12, -1, 9], [0, 0, -1, -1, -1, -1, -1]], [7, 2])
    assert tr.times.tolist() == pytest.approx([7.5 + 5 * w for w in range(7)])
    segs = tr.segments(0)
    assert [(s[2], s[3]) for s in segs] == [(9, "A minor"), (12, "C major"), (-1, "unknown"), (9, "A minor")]
    # a window stands for the stride around its centre; the first segment starts at 0, the last ends with the last window (30 + 15.2 s)
    assert [s[0] for s in segs] == pytest.approx([0.0, 20.0, 30.0, 35.0])
    assert [s[1] for s in segs] == pytest.approx([20.0, 30.0, 35.0, 37.5 + 7.6])
    for a, b in zip(segs, segs[1:]):
        assert a[1] == pytest.approx(b[0])
    assert tr.segments(1) == [(0.0, pytest.approx(12.5 + 7.6), 0, "C minor")]      # only the first counts[1] = 2 windows
    assert _track([[-1, -1]], [0]).segments(0) == []


def _bare_estimator(frames=5, wrap_mode="dataset_max", local=False):
    est = P.KeyEstimator.__new__(P.KeyEstimator)                   # (the constructor uploads the CQT tables: it needs a GPU)
    est.frames, est.wrap_mode, est.sample_rate = frames, wrap_mode, 22050
    est.net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True, local=local, frames=5, loc_window_size=10))
    return est


def test_track_refuses_what_it_cannot_do():
    audio = torch.zeros((1, 330750))
    with pytest.raises(ValueError, match="frames=0"):
        _bare_estimator(frames=0).track(audio)
    with pytest.raises(ValueError, match="true_end"):
        _bare_estimator(wrap_mode="true_end").track(audio)
    with pytest.raises(ValueError, match="--local"):
        _bare_estimator(local=True).track(audio)


def test_the_library_refuses_a_local_net_by_name():
    lib = _lib.lib()
    p = _lib.PcnetConfig()
    lib.ake_pcnet_default_config(C.byref(p), 8, 1)
    p.local = 38
    h = C.c_void_p()
    assert lib.ake_pcnet_create(C.byref(p), C.byref(h)) == 0
    assert lib.ake_pcnet_forward_windows_workspace_bytes(h, 2, 226, 76, 25) == 0
    rc = lib.ake_pcnet_forward_windows_f32(h, 16, 1, 2, 226, 76, 25, 16, 16, 16, 16, 1 << 30, None)     # refused before anything is read
    assert rc == -5 and b"--local" in lib.ake_last_error()
    lib.ake_pcnet_destroy(h)
    # the default net sizes its workspace by the 256-window chunk, not by the number of windows
    lib.ake_pcnet_default_config(C.byref(p), 8, 1)
    assert lib.ake_pcnet_create(C.byref(p), C.byref(h)) == 0
    one = lib.ake_pcnet_forward_windows_workspace_bytes(h, 1, 76 + 255 * 5, 76, 5)        # 256 windows
    many = lib.ake_pcnet_forward_windows_workspace_bytes(h, 8, 1501, 76, 5)               # 8 x 286 windows
    assert 0 < one == many
    assert lib.ake_pcnet_forward_windows_workspace_bytes(h, 1, 75, 76, 5) == 0            # shorter than one window
    lib.ake_pcnet_destroy(h)
