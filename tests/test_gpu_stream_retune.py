"""GPU: the retuner on audio that arrives in chunks -- ake_retune_ratio, ake_stream_retune_f32 / ake_stream_retune_pcm16_f32,
ake_amd.StreamRetuner and KeyEstimator.stream(retune_cents=...).

The contract is bit identity with the offline retuner (ake_amd.retune) on the joined audio for every way of cutting it, so every comparison
of samples here is torch.equal and there is no tolerance to choose.  The end-to-end part compares a retuning stream against a plain stream
fed the retuner's own pieces (torch.equal again, `times` apart: they are the plain stream's divided by rho), and against track(tuning=c) on
the whole audio within test_gpu_stream.py's BUDGET.  The meter's 3 cents are tests/test_tuning_host.py's limit for the estimate."""
import ctypes as C
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import _lib, metrics, synthetic
from conftest import golden_state_dict, load_golden, rel_err
from test_tuning_host import harmonic_clip
from ws_guard import Guarded, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
N_IN = 20011                                   # odd, no multiple of anything in sight
CENTS = (-50.0, -17.3, 0.0, 33.3, 50.0)
SCHEDULE = (0, 1, 7, 62, 63, 64, 65, 1000, 3, 4096)        # then the rest: pieces shorter than, as long as and longer than the ring
GAP = 8                                        # floats of poison between two calls' outputs
PAD = 5                                        # 32767s behind every int16 row, which the row stride skips
BUDGET = 1e-3                                  # test_gpu_stream.py's
METER_CENTS = 3.0                              # tests/test_tuning_host.py's
INVALID, WORKSPACE = -1, -4


def schedules(n):
    return {"irregular": list(SCHEDULE) + [n - sum(SCHEDULE)], "at once": [n], "single samples": [1] * 200 + [n - 200]}


_audio, _refs, _rhos = {}, {}, {}


def audio_f32(R):
    """(R, N_IN) float32 in [-1, 1), every recording its own noise; shared and left unchanged."""
    if R not in _audio:
        g = torch.Generator().manual_seed(700 + R)
        _audio[R] = (torch.rand((R, N_IN), generator=g) * 2 - 1).to(DEV)
    return _audio[R]


def source(form, R):
    """The audio as the entry point is to read it: (R, N_IN) float32, or int16 as a view of (R, N_IN + PAD) storage whose last PAD
    columns hold 32767 and belong to no recording."""
    x = audio_f32(R)
    if form == "f32":
        return x
    buf = torch.full((R, N_IN + PAD), 32767, dtype=torch.int16, device=DEV)
    buf[:, :N_IN] = (x * 32767).round().to(torch.int16)
    buf[:, 5], buf[:, 6] = -32768, 32767
    return buf[:, :N_IN]


def device_rho(cents):
    """ake_retune_ratio, once per value."""
    if cents not in _rhos:
        rho = C.c_double(-1.0)
        assert _lib.lib().ake_retune_ratio(cents, C.byref(rho), torch.cuda.current_stream().cuda_stream) == 0, _lib.lib().ake_last_error()
        _rhos[cents] = rho.value
    return _rhos[cents]


def offline(form, R, cents):
    """ake_amd.retune on the whole audio, once per case -> (the samples (R, n_out), n_out)."""
    key = (form, R, cents)
    if key not in _refs:
        y, lengths = ake_amd.retune(source(form, R), cents)
        n_out = lengths.cpu().tolist()
        assert len(set(n_out)) == 1
        _refs[key] = (y[:, :n_out[0]].clone(), n_out[0])
    return _refs[key]


def entry_call(chunk, R, cents, rho, n_before, flush, state, state_bytes, out_ptr, out_stride, k_out, over=None):
    """One call of the entry point for `chunk` (R, m) or None; `over` replaces arguments by name."""
    L = _lib.lib()
    m = 0 if chunk is None else chunk.shape[1]
    a = dict(chunk=chunk.data_ptr() if m else None, R=R, m=m, rec=(chunk.stride(0) if R > 1 else m) if m else 0, cents=cents, rho=rho,
             before=n_before, flush=flush, state=state, state_bytes=state_bytes, out=out_ptr, out_stride=out_stride,
             k_out=C.byref(k_out) if k_out is not None else None)
    a.update(over or {})
    fn = L.ake_stream_retune_pcm16_f32 if chunk is not None and chunk.dtype == torch.int16 else L.ake_stream_retune_f32
    return fn(a["chunk"], a["R"], a["m"], a["rec"], a["cents"], a["rho"], a["before"], a["flush"], a["state"], a["state_bytes"], a["out"],
              a["out_stride"], a["k_out"], torch.cuda.current_stream().cuda_stream)


def streamed(src, cents, pieces, fill, flush_alone=True):
    """The entry point over `src` (R, n) cut into `pieces`, then a flush of its own (or the last piece flushes) -> ((R, n_out) float32,
    the summed k_out).  The state is a guarded buffer filled with `fill`; every call writes to its own place in one guarded, poisoned
    output buffer, GAP floats behind the last call's, and whatever lies between and behind the pieces must still be poison at the end."""
    if flush_alone:
        pieces = list(pieces) + [0]
    L, rho = _lib.lib(), device_rho(cents)
    R, n = src.shape
    nbytes = L.ake_stream_retune_state_bytes(R)
    assert nbytes == R * 64 * 4
    state, state_check = guarded(nbytes, fill, 1 << 12)
    total = L.ake_stream_retune_out_count(cents, rho, n, 1)
    assert total == metrics.retune_final(n, rho, True, copy=cents == 0.0)
    width = total + GAP * (len(pieces) + 2)
    og = Guarded(R * width * 4, 0xFF, 1 << 12, pad_to=1, align=16)
    out = og.view.view(torch.float32).view(R, width)
    at, col, spans = 0, 0, []
    for i, m in enumerate(pieces):
        flush = int(i == len(pieces) - 1)
        chunk = src[:, at:at + m] if m else None
        want = L.ake_stream_retune_out_count(cents, rho, at + m, flush) - L.ake_stream_retune_out_count(cents, rho, at, 0)
        assert want == metrics.retune_final(at + m, rho, bool(flush), copy=cents == 0.0) - metrics.retune_final(at, rho, copy=cents == 0.0)
        k_out = C.c_int64(-7)
        rc = entry_call(chunk, R, cents, rho, at, flush, state.data_ptr(), nbytes, out.data_ptr() + 4 * col, width, k_out)
        assert rc == 0, L.ake_last_error()
        assert k_out.value == want >= 0
        spans.append((col, want))
        col += want + GAP
        at += m
    assert at == n
    state_check("state")
    og.check("output")
    written = torch.zeros(width, dtype=torch.bool, device=DEV)
    for c, k in spans:
        written[c:c + k] = True
    assert bool(torch.isnan(out[:, ~written]).all()), "a call wrote behind its k_out outputs"
    return torch.cat([out[:, c:c + k] for c, k in spans], dim=1), sum(k for _, k in spans)


@pytest.mark.parametrize("form", ["f32", "i16"])
@pytest.mark.parametrize("cents", CENTS)
def test_any_cut_equals_the_offline_retuner_on_the_whole(cents, form):
    for R in (1, 3):
        src = source(form, R)
        ref, n_out = offline(form, R, cents)
        assert ref.shape == (R, n_out) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
        if form == "i16":                                                               # = the float32 results on pcm16_to_float(pcm)
            ref_f, n_f = ake_amd.retune(ake_amd.pcm16_to_float(src), cents)
            assert int(n_f[0]) == n_out and torch.equal(ref_f[:, :n_out], ref)
        for (name, pieces), fill in zip(schedules(N_IN).items(), (0x00, 0xFF, 0x77)):
            got, total = streamed(src, cents, pieces, fill, flush_alone=name != "at once")     # "at once": one call, flushing
            assert total == n_out, (R, name)                                            # the summed k_out = the offline lengths
            assert got.shape == ref.shape, (R, name)
            assert torch.equal(got, ref), (R, name, int((got != ref).sum()), float((got - ref).abs().max()))


def test_the_ratio_entry():
    L = _lib.lib()
    assert device_rho(50.0) == metrics.RETUNE_MAX_RATIO == device_rho(70.0) == device_rho(float("inf"))
    assert device_rho(-50.0) == 1.0 / metrics.RETUNE_MAX_RATIO == device_rho(-1e9)
    rho = C.c_double(-1.0)
    assert L.ake_retune_ratio(float("nan"), C.byref(rho), None) == 0 and rho.value == 1.0                # NaN reads as 0
    assert device_rho(0.0) == 1.0
    for cents in (-49.99, -17.3, -0.01, 0.01, 12.5, 33.3, 49.99):
        c32 = float(np.float32(cents))
        want = 2.0 ** (c32 / 1200.0)
        # a last-place difference between the device's exp2 and the host's power is allowed, and no more: two such operations on the
        # same double cannot lie further apart.  (Bit identity with the offline kernel, above, is the check of the ratio itself.)
        assert abs(device_rho(c32) - want) <= 2.0 ** -50 * want, (cents, device_rho(c32), want)
    assert L.ake_retune_ratio(3.0, None, None) == INVALID
    assert L.ake_stream_retune_out_count(3.0, 0.9, 100, 0) == -1 and L.ake_stream_retune_out_count(3.0, float("nan"), 100, 0) == -1
    assert L.ake_stream_retune_out_count(3.0, device_rho(3.0), -1, 0) == -1
    assert L.ake_stream_retune_state_bytes(0) == 0 and L.ake_stream_retune_state_bytes(65536) == 0


def test_calls_with_nothing_to_do_launch_nothing():
    L, R, cents = _lib.lib(), 2, 33.3
    rho = device_rho(cents)
    nbytes = L.ake_stream_retune_state_bytes(R)
    state, state_check = guarded(nbytes, 0x77, 1 << 12)
    og = Guarded(R * 64 * 4, 0xFF, 1 << 12, pad_to=1, align=16)
    k_out = C.c_int64(-7)
    src = source("f32", R)
    ake_amd.retune(src[:, :100], cents)                                                 # (the table's upload is no launch of these calls)
    _lib.prof_enable("", True)
    try:
        _lib.prof_results()
        # a flush of a stream that got nothing; an empty push at the start and in mid-stream
        assert entry_call(None, R, cents, rho, 0, 1, state.data_ptr(), nbytes, og.view.data_ptr(), 64, k_out) == 0 and k_out.value == 0
        assert entry_call(None, R, cents, rho, 0, 0, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert entry_call(None, R, cents, rho, 30, 0, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert entry_call(None, R, 0.0, 1.0, 30, 1, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert set(_lib.prof_results()) == set()
        state_check("state")
        # 32 samples: output 0 reads input 32, so nothing is final, but they must be carried: the tail launch alone
        assert entry_call(src[:, :32], R, cents, rho, 0, 0, state.data_ptr(), nbytes, None, 0, k_out) == 0 and k_out.value == 0
        assert set(_lib.prof_results()) == {"stream_retune_tail_kernel"}
        # a flush behind them: outputs, and nothing to carry
        want = int(np.floor(32 * rho))
        assert entry_call(None, R, cents, rho, 32, 1, state.data_ptr(), nbytes, og.view.data_ptr(), 64, k_out) == 0 and k_out.value == want
        assert set(_lib.prof_results()) == {"stream_retune_kernel"}
        got = og.view.view(torch.float32).view(R, 64)[:, :want].clone()
        # zero cents: a copy, never a tail
        assert entry_call(src[:, :10], R, 0.0, 1.0, 0, 0, state.data_ptr(), nbytes, og.view.data_ptr(), 64, k_out) == 0 and k_out.value == 10
        assert entry_call(src[:, 10:20], R, float("nan"), 1.0, 10, 1, state.data_ptr(), nbytes, og.view.data_ptr() + 40, 64, k_out) == 0
        assert k_out.value == 10 and set(_lib.prof_results()) == {"stream_retune_kernel"}
        # the 33rd sample makes outputs 0 and 1 final (floor(1 / rho) = 0: they read the same 64 inputs): both launches
        assert metrics.retune_final(33, rho) == 2
        assert entry_call(src[:, :33], R, cents, rho, 0, 0, state.data_ptr(), nbytes, og.view.data_ptr() + 128, 64, k_out) == 0 and k_out.value == 2
        assert set(_lib.prof_results()) == {"stream_retune_kernel", "stream_retune_tail_kernel"}
    finally:
        _lib.prof_enable("", False)
    og.check("output")
    state_check("state")
    out = og.view.view(torch.float32).view(R, 64)
    assert torch.equal(got, ake_amd.retune(src[:, :32].contiguous(), cents)[0][:, :want])
    assert torch.equal(out[:, :20], src[:, :20]) and torch.equal(out[:, 20:want], got[:, 20:]) and bool(torch.isnan(out[:, 34:]).all())
    assert torch.equal(out[:, 32:34], ake_amd.retune(src[:, :100].contiguous(), cents)[0][:, :2])  # final after 33 samples, whatever follows


def test_entry_errors():
    L, R, m, cents = _lib.lib(), 2, 500, -17.3
    rho = device_rho(cents)
    nbytes = L.ake_stream_retune_state_bytes(R)
    state, state_check = guarded(nbytes + 16, 0x77, 1 << 12)
    src, pcm = source("f32", R)[:, :m], source("i16", R)[:, :m]
    want = L.ake_stream_retune_out_count(cents, rho, m, 1)
    assert want == int(np.floor(m * rho))
    og = Guarded(R * want * 4, 0xFF, 1 << 12, pad_to=1, align=16)
    k_out = C.c_int64(-7)
    ake_amd.retune(src.contiguous(), cents)
    _lib.prof_enable("", True)
    try:
        _lib.prof_results()

        def call(data=src, **over):
            return entry_call(data, R, cents, rho, 0, 1, state.data_ptr(), nbytes, og.view.data_ptr(), want, k_out, over)

        assert call(state_bytes=nbytes - 1) == WORKSPACE and b"state" in L.ake_last_error()
        for bad in (dict(chunk=None), dict(state=None), dict(k_out=None), dict(out=None), dict(R=0), dict(R=65536), dict(m=-1), dict(before=-1),
                    dict(rec=-1), dict(out_stride=want - 1), dict(state=state.data_ptr() + 4), dict(rho=float("nan")), dict(rho=0.5),
                    dict(rho=1.03), dict(rho=0.0)):
            assert call(**bad) == INVALID, bad
        assert call(pcm, state_bytes=nbytes - 1) == WORKSPACE
        assert call(pcm, rec=-1) == INVALID
        assert set(_lib.prof_results()) == set()                                       # none of them launched anything
        state_check("state")
        og.check("output")
        assert bool(torch.isnan(og.view.view(torch.float32)).all())
        assert call() == 0 and k_out.value == want
        assert set(_lib.prof_results()) == {"stream_retune_kernel"}                    # (a flushing call carries nothing)
        assert call(pcm, flush=0) == 0 and k_out.value == L.ake_stream_retune_out_count(cents, rho, m, 0)
        assert set(_lib.prof_results()) == {"stream_retune_kernel", "stream_retune_tail_kernel"}
    finally:
        _lib.prof_enable("", False)
    og.check("output")
    state_check("state")


def test_a_stream_that_changes_its_sample_format():
    """The ring holds float32 whatever the samples came from."""
    R, cents = 2, 33.3
    pcm = source("i16", R)
    flt = ake_amd.pcm16_to_float(pcm)
    ref, n_out = offline("i16", R, cents)
    s = ake_amd.StreamRetuner(cents, R, DEV)
    outs, at = [], 0
    for i, m in enumerate(schedules(N_IN)["irregular"]):
        outs.append(s.push((pcm if i % 2 else flt)[:, at:at + m]))
        at += m
    outs.append(s.finish())
    assert torch.equal(torch.cat(outs, dim=1), ref)


def test_the_python_stream_retuner():
    R, cents = 3, -17.3
    src = source("i16", R)
    ref, n_out = offline("i16", R, cents)
    s = ake_amd.StreamRetuner(cents, R, DEV, max_chunk_samples=3000)                  # the 4096 and the rest go in pieces
    assert s.rho == device_rho(float(np.float32(cents))) and s.cents == float(np.float32(cents))
    outs, at = [], 0
    for m in schedules(N_IN)["irregular"]:
        outs.append(s.push(src[:, at:at + m]))
        assert outs[-1].shape == (R, s.out_count(at + m) - s.out_count(at)) and outs[-1].dtype == torch.float32
        at += m
    outs.append(s.finish())
    assert torch.equal(torch.cat(outs, dim=1), ref)
    assert all(s.out_count(n, f) == metrics.retune_final(n, s.rho, f) for n in (0, 1, 32, 33, 34, 95, 96, 5000, 10 ** 6 + 7) for f in (False, True))
    with pytest.raises(ValueError):
        s.push(src[:, :10])
    with pytest.raises(ValueError):
        s.finish()
    zero = ake_amd.StreamRetuner(0, R, DEV)
    assert zero.rho == 1.0 and torch.equal(zero.push(audio_f32(R)[:, :100]), audio_f32(R)[:, :100]) and zero.finish().shape == (R, 0)
    t = ake_amd.StreamRetuner(torch.tensor(12.5), R, DEV)
    assert t.push(audio_f32(R)[:, :100]).shape == (R, t.out_count(100)) and t.out_count(100) == metrics.retune_final(100, t.rho)
    for bad in (audio_f32(1)[:, :10], audio_f32(R)[:, :10].double(), audio_f32(R)[:, None, :10]):
        with pytest.raises(ValueError):
            t.push(bad)
    for kw in (dict(cents=50.5), dict(cents=-60), dict(cents=float("nan")), dict(cents=torch.zeros(3)), dict(recordings=0), dict(recordings=65536),
               dict(max_chunk_samples=0)):
        with pytest.raises(ValueError):
            ake_amd.StreamRetuner(**{**dict(cents=10.0, recordings=1, device=DEV), **kw})


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------

E2E_CENTS = 33.3
N30 = 30 * SR


@pytest.fixture(scope="module")
def est():
    gold = load_golden("pcnet_trained.npz")
    sd32, opt = golden_state_dict(gold), Namespace(**json.loads(str(gold["opt"])))
    net = ake_amd.PitchClassNet(opt.octaves * 36, 12, opt.num_layers, opt.kernel_size, opt)
    net.load_state_dict(sd32, strict=True)
    return ake_amd.KeyEstimator(net.to(DEV).eval(), SR, 5)


@pytest.fixture(scope="module")
def recordings():
    """test_gpu_stream.py's two 45 s recordings; all but the 48 kHz case, which reads them as 20.7 s, take the first 30 s."""
    rows = [np.concatenate([synthetic.make_clip(i)[0] for i in ids]) for ids in ((0, 1, 2), (5, 6, 7))]
    return torch.from_numpy(np.stack(rows).astype(np.float32)).to(DEV)


FIELDS = ("key", "tonic", "genre", "key_id", "signature_id", "tonic_id", "confidence", "emissions", "filtered", "smooth_key_id", "posteriors",
          "smooth_confidence", "log_likelihood", "tuning_cents", "tuning_strength")


def assert_same_update(a, b, rho, where):
    assert (a.first_window, a.windows, a.smooth_first_window) == (b.first_window, b.windows, b.smooth_first_window), where
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (where, name)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), (where, name)
    assert torch.equal(a.times, b.times / rho), where                                 # seconds of the recording as it was


def pieces_of(n, first=(1, 4409, 0, 100000, 5), step=SR):
    pieces = list(first)
    while sum(pieces) < n:
        pieces.append(min(step, n - sum(pieces)))
    assert sum(pieces) == n
    return pieces


@pytest.mark.parametrize("case", ["plain", "posteriors", "profile", "int16", "48k stereo"])
def test_a_retuning_stream_end_to_end(est, recordings, case):
    if case != "48k stereo":
        recordings = recordings[:, :N30].contiguous()
    R, n = recordings.shape
    kw = dict(stride_seconds=1.0, lag_windows=2, tuning_meter=True)
    kw.update({"posteriors": dict(posteriors=True), "profile": dict(method="profile")}.get(case, {}))
    src, src_kw, rs = recordings, {}, None
    if case == "int16":
        src = (recordings * 32767).round().to(torch.int16)
    if case == "48k stereo":                                                          # the recordings read as 48 kHz audio; channel 1 the other's
        src = torch.stack([recordings, recordings.flip(0)], dim=1)
        src_kw = dict(source_rate=48000, source_channels=2, channel=-1)
        rs = ake_amd.StreamResampler(48000, SR, R, 2, -1, DEV)
    a = est.stream(R, retune_cents=E2E_CENTS, **src_kw, **kw)
    b = est.stream(R, **kw)
    rt = ake_amd.StreamRetuner(E2E_CENTS, R, DEV)
    assert a.rho == rt.rho == device_rho(float(np.float32(E2E_CENTS))) and a.retuner is not None and b.retuner is None
    ups, at = [], 0
    for i, m in enumerate(pieces_of(n, step=48000 if rs else SR)):
        chunk = src[..., at:at + m]
        ups.append(a.push(chunk))
        assert ups[-1].retune_cents == rt.cents
        assert_same_update(ups[-1], b.push(rt.push(rs.push(chunk) if rs else chunk)), rt.rho, i)
        at += m
    ups.append(a.finish())
    rest = [b.push(rt.push(rs.finish()))] if rs else []
    assert_same_update(ups[-1], ake_amd.StreamUpdate.concat(rest + [b.push(rt.finish()), b.finish()]), rt.rho, "finish")
    with pytest.raises(ValueError):
        a.push(src[..., :10])
    assert sum(u.windows for u in ups) >= 4 and b.N == rt.out_count(rt.n, True) == a.N
    if case in ("plain", "profile"):
        # the windows track(tuning=c) gives on the whole audio, and its outputs within the budget one schedule is held to against another
        tr = est.track(recordings, tuning=E2E_CENTS, stride_seconds=1.0, **({"method": "profile"} if case == "profile" else {}))
        counts = tr.counts.cpu().tolist()                                             # (the retuned batch is ragged in a wider buffer)
        W = counts[0]
        assert counts == [W] * R and W == (1 + a.N // 4410 - 76) // 5 + 1 == sum(u.windows for u in ups)
        key, tonic = (torch.cat([getattr(u, name) for u in ups], dim=1) for name in ("key", "tonic"))
        e = (rel_err(key, tr.key[:, :W]), rel_err(tonic, tr.tonic[:, :W]))
        print(f"\n  STREAM RETUNE end to end ({case}) | {W} windows; key / tonic against track(tuning=c) on the whole: {e[0]:.1e} {e[1]:.1e}")
        assert max(e) < BUDGET, e
        assert torch.equal(torch.cat([u.times for u in ups]), tr.times[:W] / rt.rho)


def test_without_retune_cents_a_stream_is_what_it_was(est, recordings):
    src = recordings[:, :20 * SR]
    names, ups = {}, {}
    for kind, kw in (("without", {}), ("none", dict(retune_cents=None)), ("zero", dict(retune_cents=0)), ("retuned", dict(retune_cents=E2E_CENTS))):
        _lib.prof_enable("", True)
        try:
            _lib.prof_results()                                                      # (whatever an earlier test left behind)
            s = est.stream(2, smooth=False, **kw)
            ups[kind] = [s.push(src[:, at:at + 5 * SR]) for at in range(0, src.shape[1], 5 * SR)] + [s.finish()]
            torch.cuda.synchronize()
            names[kind] = {name: count for name, (_, count) in _lib.prof_results().items()}
        finally:
            _lib.prof_enable("", False)
    assert {"stream_history_kernel", "decode_keys_kernel"} <= set(names["without"])
    assert not any("retune" in name for name in names["without"]), names["without"]
    assert names["none"] == names["zero"] == names["without"]
    # the ratio is read off the device once, when the stream is opened; four pushes and the finish retune
    assert set(names["retuned"]) - set(names["without"]) == {"retune_ratio_kernel", "stream_retune_kernel", "stream_retune_tail_kernel"}
    assert (names["retuned"]["retune_ratio_kernel"], names["retuned"]["stream_retune_kernel"], names["retuned"]["stream_retune_tail_kernel"]) == (1, 5, 4)
    for kind in ("none", "zero"):
        for i, (u, v) in enumerate(zip(ups[kind], ups["without"])):
            assert u.retune_cents == (None if kind == "none" else 0.0)
            assert_same_update(u, v, 1.0, (kind, i))
    assert sum(u.windows for u in ups["without"]) == 2


def test_the_meter_sees_the_retuned_audio(est):
    """A harmonic clip 30 cents sharp, as the tuning tests make theirs: the plain stream's meter ends at +30, the retuned stream's at 0."""
    clip = torch.from_numpy(harmonic_clip(50, 30.0).astype(np.float32))[None].to(DEV)
    ends = {}
    for kind, kw in (("plain", {}), ("retuned", dict(retune_cents=30))):
        s = est.stream(1, method="profile", tuning_meter=True, **kw)
        for at in range(0, clip.shape[1], SR):
            s.push(clip[:, at:at + SR])
        ends[kind] = float(s.finish().tuning_cents[0])
    print(f"\n  STREAM RETUNE meter | a clip 30 cents sharp: plain {ends['plain']:+.2f}, with retune_cents=30 {ends['retuned']:+.2f} cents")
    assert abs(ends["plain"] - 30.0) <= METER_CENTS and abs(ends["retuned"]) <= METER_CENTS, ends


def test_what_a_stream_refuses(est):
    for kw in (dict(retune_cents=50.5), dict(retune_cents=-51), dict(retune_cents=float("nan")), dict(retune_cents="auto"),
               dict(retune_cents=torch.tensor([3.0])), dict(retune_cents=True), dict(tuning="auto"), dict(tuning=3.0, retune_cents=3.0)):
        with pytest.raises(ValueError):
            est.stream(1, **kw)
    with pytest.raises(ValueError, match="tuning_meter"):
        est.stream(1, tuning=3.0)
    # the retuner keeps 0.94 of the Nyquist frequency: at 17 kHz the 288 bins' top (8210 Hz) lies above 0.94 * 8500 Hz
    high = ake_amd.KeyEstimator(None, 17000, 5, device=DEV, pitches=288)
    with pytest.raises(ValueError, match="Nyquist"):
        high.stream(1, method="profile", retune_cents=10.0)
    assert high.stream(1, method="profile", retune_cents=0).retuner is None              # nothing is filtered: nothing to refuse
    s = est.stream(2, retune_cents=-12.5, max_chunk_samples=5000)
    assert s.retuned.shape == (2, metrics.retune_out_len(5000) + 64) and s.max_chunk == s.retuned.shape[1]
    with pytest.raises(ValueError):
        s.push(torch.zeros((2, 2, 100), device=DEV))
    u = s.push(torch.zeros((2, 12000), device=DEV))                                    # three pieces
    assert u.windows == 0 and s.retuner.n == 12000 and s.N == s.retuner.out_count(12000)
    assert s.finish().windows == 0 and s.N == int(np.floor(12000 * s.rho))
    torch.cuda.synchronize()
