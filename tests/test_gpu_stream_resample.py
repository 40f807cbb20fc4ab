"""GPU: the polyphase resampler on audio that arrives in chunks -- ake_stream_resample_f32 / ake_stream_resample_pcm16_f32,
ake_amd.StreamResampler and KeyEstimator.stream(source_rate=..., source_channels=..., channel=...).

The contract is bit identity with the offline resampler (ake_amd.Resampler) on the joined audio for every way of cutting it, so every
comparison of samples here is torch.equal and there is no tolerance to choose.  The end-to-end part compares a stream with a source format
against a plain stream fed the resampler's own pieces (torch.equal again), and against track on the whole audio within test_gpu_stream.py's
BUDGET, on that file's two recordings read as the two channels of 48 kHz audio."""
import ctypes as C
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict, load_golden, rel_err
from ws_guard import Guarded, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
N_IN = 20011                                   # odd, no multiple of anything in sight
SCHEDULE = (0, 1, 7, 43, 44, 45, 1000, 3, 4096)            # then the rest: pieces shorter than, as long as and longer than the tails (40, 43)
GAP = 8                                        # floats of poison between two calls' outputs
BUDGET = 1e-3                                  # test_gpu_stream.py's
INVALID, WORKSPACE = -1, -4


def schedules(n):
    return {"irregular": list(SCHEDULE) + [n - sum(SCHEDULE)], "at once": [n], "single samples": [1] * 200 + [n - 200]}


_audio, _handles, _refs = {}, {}, {}


def audio_f32(R, Cn):
    """(R, Cn, N_IN) float32 in [-1, 1), every recording and channel its own noise; shared and left unchanged."""
    if (R, Cn) not in _audio:
        g = torch.Generator().manual_seed(100 * R + Cn)
        _audio[R, Cn] = (torch.rand((R, Cn, N_IN), generator=g) * 2 - 1).to(DEV)
    return _audio[R, Cn]


def source(form, R, Cn):
    """The audio as the entry point is to read it: (R, Cn, N_IN) float32 planar, int16 planar, or int16 as a view of interleaved
    (R, N_IN, Cn + 1) storage whose last slot holds 32767 and belongs to no channel."""
    x = audio_f32(R, Cn)
    if form == "f32":
        return x
    pcm = (x * 32767).round().to(torch.int16)
    pcm[:, :, 5], pcm[:, :, 6] = -32768, 32767
    if form == "i16 planar":
        return pcm
    buf = torch.full((R, N_IN, Cn + 1), 32767, dtype=torch.int16, device=DEV)
    buf[:, :, :Cn] = pcm.transpose(1, 2)
    return buf[:, :, :Cn].transpose(1, 2)


def handle(rate):
    if rate not in _handles:
        _handles[rate] = ake_amd.get_resampler(rate, SR, DEV)
    return _handles[rate]


def offline(rate, form, R, Cn, channel):
    """ake_amd.Resampler on the whole audio, once per case."""
    key = (rate, form, R, Cn, channel)
    if key not in _refs:
        _refs[key] = handle(rate)(source(form, R, Cn), channel=channel)[0]
    return _refs[key]


def entry_call(rs, chunk, R, Cn, channel, n_before, flush, state, state_bytes, out_ptr, out_stride, k_out, over=None):
    """One call of the entry point for `chunk` (R, Cn, m) or None; `over` replaces arguments by name."""
    L = _lib.lib()
    m = 0 if chunk is None else chunk.shape[2]
    a = dict(r=rs._h, chunk=chunk.data_ptr() if m else None, R=R, Cn=Cn, m=m, rec=chunk.stride(0) if m else 0, ch=chunk.stride(1) if m else 0,
             smp=chunk.stride(2) if m else 1, channel=channel, before=n_before, flush=flush, state=state, state_bytes=state_bytes, out=out_ptr,
             out_stride=out_stride, k_out=C.byref(k_out) if k_out is not None else None)
    a.update(over or {})
    stream = torch.cuda.current_stream().cuda_stream
    if chunk is not None and chunk.dtype == torch.int16:
        return L.ake_stream_resample_pcm16_f32(a["r"], a["chunk"], a["R"], a["Cn"], a["m"], a["rec"], a["ch"], a["smp"], a["channel"], a["before"],
                                               a["flush"], a["state"], a["state_bytes"], a["out"], a["out_stride"], a["k_out"], stream)
    assert a["smp"] == 1
    return L.ake_stream_resample_f32(a["r"], a["chunk"], a["R"], a["Cn"], a["m"], a["rec"], a["ch"], a["channel"], a["before"], a["flush"],
                                     a["state"], a["state_bytes"], a["out"], a["out_stride"], a["k_out"], stream)


def streamed(rate, src, channel, pieces, fill, flush_alone=True):
    """The entry point over `src` (R, Cn, n) cut into `pieces`, then a flush of its own (or the last piece flushes) -> (R, n_out)
    float32.  The state is a guarded buffer filled with `fill`; every call writes to its own place in one guarded, poisoned output buffer,
    GAP floats behind the last call's, and whatever lies between and behind the pieces must still be poison at the end."""
    if flush_alone:
        pieces = list(pieces) + [0]
    L, rs = _lib.lib(), handle(rate)
    R, Cn, n = src.shape
    nbytes = L.ake_stream_resample_state_bytes(rs._h, R)
    assert nbytes > 0 and nbytes % 16 == 0
    state, state_check = guarded(nbytes, fill, 1 << 12)
    total = rs.out_len(n)
    width = total + GAP * (len(pieces) + 2)
    og = Guarded(R * width * 4, 0xFF, 1 << 12, pad_to=1, align=16)
    out = og.view.view(torch.float32).view(R, width)
    at, col, spans = 0, 0, []
    for i, m in enumerate(pieces):
        flush = int(i == len(pieces) - 1)
        chunk = src[:, :, at:at + m] if m else None
        want = L.ake_stream_resample_out_count(rs._h, at + m, flush) - L.ake_stream_resample_out_count(rs._h, at, 0)
        k_out = C.c_int64(-7)
        rc = entry_call(rs, chunk, R, Cn, channel, at, flush, state.data_ptr(), nbytes, out.data_ptr() + 4 * col, width, k_out)
        assert rc == 0, L.ake_last_error()
        assert k_out.value == want >= 0
        spans.append((col, want))
        col += want + GAP
        at += m
    assert at == n and sum(k for _, k in spans) == total
    state_check("state")
    og.check("output")
    written = torch.zeros(width, dtype=torch.bool, device=DEV)
    for c, k in spans:
        written[c:c + k] = True
    assert bool(torch.isnan(out[:, ~written]).all()), "a call wrote behind its k_out outputs"
    return torch.cat([out[:, c:c + k] for c, k in spans], dim=1)


CASES = [(rate, Cn, channel) for rate in (44100, 48000, 16000) for Cn, channel in ((1, 0), (2, 0), (2, 1), (2, -1))] + [(SR, 2, 0), (SR, 2, 1), (SR, 2, -1)]


@pytest.mark.parametrize("form", ["f32", "i16 planar", "i16 interleaved"])
@pytest.mark.parametrize("rate,Cn,channel", CASES)
def test_any_cut_equals_the_offline_resampler_on_the_whole(rate, Cn, channel, form):
    for R in (1, 3):
        src, ref = source(form, R, Cn), offline(rate, form, R, Cn, channel)
        assert ref.shape == (R, handle(rate).out_len(N_IN)) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
        for (name, pieces), fill in zip(schedules(N_IN).items(), (0x00, 0xFF, 0x77)):
            got = streamed(rate, src, channel, pieces, fill, flush_alone=name != "at once")     # "at once": one call, flushing
            assert got.shape == ref.shape, (R, name)
            assert torch.equal(got, ref), (R, name, int((got != ref).sum()), float((got - ref).abs().max()))


def test_pcm_and_float_streams_carry_the_same_values():
    """A stream may change its sample format from push to push: the state holds float32 sums whatever they came from."""
    rate, R, Cn, channel = 48000, 2, 2, -1
    pcm = source("i16 planar", R, Cn)
    flt = ake_amd.pcm16_to_float(pcm)
    ref = handle(rate)(pcm, channel=channel)[0]
    s = ake_amd.StreamResampler(rate, SR, R, Cn, channel, DEV)
    outs, at = [], 0
    for i, m in enumerate(schedules(N_IN)["irregular"]):
        outs.append(s.push((pcm if i % 2 else flt)[:, :, at:at + m]))
        at += m
    outs.append(s.finish())
    assert torch.equal(torch.cat(outs, dim=1), ref)


def test_the_python_stream_resampler():
    rate, R, Cn = 44100, 3, 2
    src = source("i16 interleaved", R, Cn)
    ref = offline(rate, "i16 interleaved", R, Cn, 1)
    s = ake_amd.StreamResampler(rate, SR, R, Cn, 1, DEV, max_chunk_samples=3000)      # the 4096 and the rest go in pieces
    outs, at = [], 0
    for m in schedules(N_IN)["irregular"]:
        outs.append(s.push(src[:, :, at:at + m]))
        assert outs[-1].shape == (R, s.out_count(at + m) - s.out_count(at)) and outs[-1].dtype == torch.float32
        at += m
    outs.append(s.finish())
    assert torch.equal(torch.cat(outs, dim=1), ref)
    up, down, half = metrics.resample_ratio(rate, SR)
    assert all(s.out_count(n, f) == metrics.resampled_final(n, up, down, half, f) for n in (0, 1, 19, 20, 21, 5000) for f in (False, True))
    with pytest.raises(ValueError):
        s.push(src[:, :, :10])
    with pytest.raises(ValueError):
        s.finish()
    mono = ake_amd.StreamResampler(rate, SR, R, 1, 0, DEV)
    assert mono.push(audio_f32(R, 1)[:, 0, :100]).shape == (R, 40)                    # (R, m) with one channel; 100 - 20 inputs are under no tap
    for bad in (audio_f32(R, 2)[:, :, :10], audio_f32(1, 1)[:, :, :10], audio_f32(R, 1)[:, :, :10].double()):
        with pytest.raises(ValueError):
            mono.push(bad)
    for kw in (dict(recordings=0), dict(channels=0), dict(channel=2), dict(channel=-2), dict(max_chunk_samples=0)):
        with pytest.raises(ValueError):
            ake_amd.StreamResampler(rate, SR, **{**dict(recordings=1, channels=2, channel=0, device=DEV), **kw})


def test_calls_with_nothing_to_do_launch_nothing():
    L, rs = _lib.lib(), handle(48000)
    R, Cn = 2, 2
    nbytes = L.ake_stream_resample_state_bytes(rs._h, R)
    state, state_check = guarded(nbytes, 0x77, 1 << 12)
    og = Guarded(R * 64 * 4, 0xFF, 1 << 12, pad_to=1, align=16)
    k_out = C.c_int64(-7)
    src = source("f32", R, Cn)
    _lib.prof_enable("", True)
    try:
        # a flush of a stream that got nothing; an empty push in front of and behind 30 samples that are under no output's last tap yet
        assert entry_call(rs, None, R, Cn, 0, 0, 1, state.data_ptr(), nbytes, og.view.data_ptr(), 64, k_out) == 0 and k_out.value == 0
        assert entry_call(rs, None, R, Cn, 0, 0, 0, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert entry_call(rs, None, R, Cn, 0, 30, 0, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert set(_lib.prof_results()) == set()
        state_check("state")
        # 10 samples: nothing final yet (k * 320 + 3200 < 10 * 147 for no k), but they must be carried: the tail launch alone
        assert entry_call(rs, src[:, :, :10], R, Cn, 0, 0, 0, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert set(_lib.prof_results()) == {"stream_resample_tail_kernel"}
        # a flush behind them: outputs, and nothing to carry
        assert entry_call(rs, None, R, Cn, 0, 10, 1, state.data_ptr(), nbytes, og.view.data_ptr(), 64, k_out) == 0 and k_out.value == 5
        assert set(_lib.prof_results()) == {"stream_resample_kernel"}
        # the same rate: a mix, never a tail
        same = handle(SR)
        assert entry_call(same, src[:, :, :10], R, Cn, -1, 0, 0, state.data_ptr(), nbytes, og.view.data_ptr(), 64, k_out) == 0 and k_out.value == 10
        assert set(_lib.prof_results()) == {"stream_resample_kernel"}
    finally:
        _lib.prof_enable("", False)
    og.check("output")
    got = og.view.view(torch.float32).view(R, 64)
    assert torch.equal(got[:, :10], (src[:, 0, :10] + src[:, 1, :10]) * 0.5) and bool(torch.isnan(got[:, 10:]).all())


def test_entry_errors():
    L, rs = _lib.lib(), handle(48000)
    R, Cn, m = 2, 2, 500
    nbytes = L.ake_stream_resample_state_bytes(rs._h, R)
    assert nbytes == R * 4 * ((2 * 3200 // 147 + 1 + 3) // 4 * 4)
    assert L.ake_stream_resample_state_bytes(None, R) == 0 and L.ake_stream_resample_state_bytes(rs._h, 0) == 0
    assert L.ake_stream_resample_state_bytes(rs._h, 65536) == 0
    assert L.ake_stream_resample_out_count(None, 5, 0) == -1 and L.ake_stream_resample_out_count(rs._h, -1, 0) == -1
    state, state_check = guarded(nbytes + 16, 0x77, 1 << 12)
    src, pcm = source("f32", R, Cn)[:, :, :m], source("i16 interleaved", R, Cn)[:, :, :m]
    want = L.ake_stream_resample_out_count(rs._h, m, 1)
    og = Guarded(R * want * 4, 0xFF, 1 << 12, pad_to=1, align=16)
    k_out = C.c_int64(-7)
    _lib.prof_enable("", True)
    try:
        def call(data=src, **over):
            return entry_call(rs, data, R, Cn, 0, 0, 1, state.data_ptr(), nbytes, og.view.data_ptr(), want, k_out, over)

        assert call(state_bytes=nbytes - 1) == WORKSPACE and b"state" in L.ake_last_error()
        for bad in (dict(r=None), dict(chunk=None), dict(state=None), dict(k_out=None), dict(out=None), dict(R=0), dict(R=65536), dict(Cn=0),
                    dict(channel=2), dict(channel=-2), dict(m=-1), dict(before=-1), dict(rec=-1), dict(ch=-1), dict(out_stride=want - 1),
                    dict(state=state.data_ptr() + 4)):
            assert call(**bad) == INVALID, bad
        assert call(pcm, smp=0) == INVALID
        assert call(pcm, state_bytes=nbytes - 1) == WORKSPACE
        assert set(_lib.prof_results()) == set()                                       # none of them launched anything
        state_check("state")
        og.check("output")
        assert bool(torch.isnan(og.view.view(torch.float32)).all())
        assert call() == 0 and k_out.value == want
        assert call(pcm) == 0 and k_out.value == want
        assert set(_lib.prof_results()) == {"stream_resample_kernel", "stream_resample_tail_kernel"}
    finally:
        _lib.prof_enable("", False)
    og.check("output")
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------

SRC_RATE = 48000


@pytest.fixture(scope="module")
def est():
    gold = load_golden("pcnet_trained.npz")
    sd32, opt = golden_state_dict(gold), Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(sd32, strict=True)
    return ake_amd.KeyEstimator(net.to(DEV).eval(), SR, 5)


@pytest.fixture(scope="module")
def interleaved():
    """test_gpu_stream.py's two 45 s recordings, read as 48 kHz audio (20.7 s): recording r has rows r and 1 - r as its two channels.
    int16, interleaved (R, n, 2) storage -> the (R, 2, n) view a stream takes."""
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7))]
    a = torch.from_numpy(np.stack(rows).astype(np.float32))
    planar = torch.stack([a, a.flip(0)], dim=1)                                       # (2, 2, n)
    buf = (planar * 32767).round().to(torch.int16).transpose(1, 2).contiguous().to(DEV)
    return buf.transpose(1, 2)


FIELDS = ("key", "tonic", "genre", "key_id", "signature_id", "tonic_id", "confidence", "times", "emissions", "filtered", "smooth_key_id",
          "posteriors", "smooth_confidence", "log_likelihood")


def assert_same_update(a, b, where):
    assert (a.first_window, a.windows, a.smooth_first_window) == (b.first_window, b.windows, b.smooth_first_window), where
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (where, name)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), (where, name)


@pytest.mark.parametrize("posteriors", [False, True])
def test_a_stream_with_a_source_format_end_to_end(est, interleaved, posteriors):
    R, _, n = interleaved.shape
    pieces = [1, 47999, 0, 100000, 5]
    while sum(pieces) < n:
        pieces.append(min(SRC_RATE, n - sum(pieces)))
    assert sum(pieces) == n and len(pieces) > 20
    a = est.stream(R, source_rate=SRC_RATE, source_channels=2, channel=-1, stride_seconds=1.0, lag_windows=2, posteriors=posteriors)
    b = est.stream(R, stride_seconds=1.0, lag_windows=2, posteriors=posteriors)
    rs = ake_amd.StreamResampler(SRC_RATE, SR, R, 2, -1, DEV)
    ups, at = [], 0
    for i, m in enumerate(pieces):
        chunk = interleaved[:, :, at:at + m]
        ups.append(a.push(chunk))
        assert_same_update(ups[-1], b.push(rs.push(chunk)), i)
        at += m
    ups.append(a.finish())
    assert_same_update(ups[-1], ake_amd.StreamUpdate.concat([b.push(rs.finish()), b.finish()]), "finish")
    with pytest.raises(ValueError):
        a.push(interleaved[:, :, :10])
    # the windows track gives on the whole audio, and its outputs within the budget one schedule is held to against another
    tr = est.track(interleaved, rate=SRC_RATE, channel=-1, stride_seconds=1.0)
    W = tr.key.shape[1]
    frames = 1 + handle(SRC_RATE).out_len(n) // 4410
    assert W == (frames - 76) // 5 + 1 >= 4 and sum(u.windows for u in ups) == W
    key, tonic = (torch.cat([getattr(u, name) for u in ups], dim=1) for name in ("key", "tonic"))
    e = (rel_err(key, tr.key), rel_err(tonic, tr.tonic))
    print(f"\n  STREAM RESAMPLE end to end | {W} windows; key / tonic against track on the whole: {e[0]:.1e} {e[1]:.1e}")
    assert max(e) < BUDGET, e
    assert torch.equal(torch.cat([u.times for u in ups]), tr.times)
    # max_chunk_samples counts source samples: the 100000 go in two pieces, which moves the re-transforms and so is no matter of bits
    c = est.stream(R, source_rate=SRC_RATE, source_channels=2, channel=-1, stride_seconds=1.0, lag_windows=2, posteriors=posteriors, max_chunk_samples=60000)
    assert c.resampled.shape[1] < 30000 and c.hist_cap < a.hist_cap
    ups_c, at = [], 0
    for m in pieces:
        ups_c.append(c.push(interleaved[:, :, at:at + m]))
        at += m
    ups_c.append(c.finish())
    assert sum(u.windows for u in ups_c) == W
    for name, whole in (("key", key), ("tonic", tonic)):
        assert rel_err(torch.cat([getattr(u, name) for u in ups_c], dim=1), whole) < BUDGET, name


def test_only_a_stream_with_a_source_format_launches_the_resampler(est, interleaved):
    mono = ake_amd.pcm16_to_float(interleaved[:, 0, :15 * SR]).contiguous()
    names = {}
    for kind, kw in (("plain", {}), ("same format", dict(source_rate=SR, source_channels=1)), ("source", dict(source_rate=SRC_RATE))):
        _lib.prof_enable("", True)
        try:
            _lib.prof_results()                                                      # (whatever an earlier test left behind)
            s = est.stream(2, smooth=False, **kw)
            for at in range(0, mono.shape[1], 5 * SR):
                s.push(mono[:, at:at + 5 * SR])
            s.finish()
            torch.cuda.synchronize()
            names[kind] = set(_lib.prof_results())
        finally:
            _lib.prof_enable("", False)
    assert {"stream_history_kernel", "decode_keys_kernel"} <= names["plain"]
    assert not any("resample" in name for name in names["plain"]), names["plain"]
    assert names["same format"] == names["plain"]
    assert names["source"] - names["plain"] == {"stream_resample_kernel", "stream_resample_tail_kernel"}


def test_what_a_stream_still_refuses(est):
    for kw in (dict(rate=44100), dict(tuning="auto"), dict(source_channels=0), dict(source_channels=2, channel=2), dict(source_rate=0)):
        with pytest.raises(ValueError):
            est.stream(1, **kw)
    with pytest.raises(ValueError, match="source_rate"):
        est.stream(1, rate=44100)
    s = est.stream(2)
    with pytest.raises(ValueError):
        s.push(torch.zeros((2, 2, 100), device=DEV))
    s2 = est.stream(2, source_channels=2)
    with pytest.raises(ValueError):
        s2.push(torch.zeros((2, 100), device=DEV))
    u = s2.push(torch.zeros((2, 2, 100), device=DEV))
    assert u.windows == 0 and s2.finish().windows == 0
    torch.cuda.synchronize()
