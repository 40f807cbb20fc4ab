"""Key tracking on audio as it arrives: what a KeyStream.push costs, against calling track again on a rolling buffer -> one JSON line.

  push      : est.stream(R, stride 5 s, lag 6) fed white noise (no side's cost depends on the content) in chunks of one hop (0.2 s) and of
              1 s, float32 and 16-bit PCM, R = 1, 16, 256.  After 30 s of warm-up every push is timed with events on the stream: median, 95th
              percentile and maximum over --pushes pushes, and the median of the pushes that completed a window.
  split     : the same pushes once more under the library's kernel timer, per push on average: transform (history, cascade, bank, frame
              cache), net (gather and the net's kernels), smoother (decode, emissions, step); launch_share = 1 - kernels / mean push.
  baseline  : the parent commit's only way -- est.track(smooth=True) on a 60 s buffer of the same R and dtype, once per push (rolling the
              buffer is not timed); median over --baseline-reps calls.
  smoother  : ake_key_stream_step_f32 alone, 8 recordings x 2000 windows in one call at lags 3, 12, 255, per window; and one window per
              call (a push's shape).
  support   : H of the default plan, and the latency it gives from audio to raw label and to smoothed label.
  frames    : streamed against offline frames, the re-transform's start s0 on the decimation grid (a multiple of 2^(octaves-1)) and off it.
  --accuracy: tools/track_accuracy.py's net and modulating recordings (one run on sine mixes): the fixed-lag path at lags 0, 3, 6, 12 scored
              as KeyTrack.score scores, beside the raw labels and the offline Viterbi path, at a 5 s stride.

  --posteriors: this section alone.  est.stream(R, posteriors=True) at strides of 15 / 5 / 1 s and lags 6 and 30, fed 1 s chunks; once
              every sweep runs its whole lag, --pushes pushes under the library's kernel timer: the two added launches
              (key_stream_sweep_kernel, key_stream_loglik_kernel) per launch, beside key_stream_step_kernel's; and the host route on the
              same pushes -- the emissions copied to the CPU, then metrics.key_stream_posteriors with its carried state -- per push that
              completed a window, by the host clock.

  --source-rate HZ [--source-channels C]: this section alone.  est.stream(R, source_rate=HZ, source_channels=C, channel=-1) fed interleaved
              int16 chunks of 0.2 s and 1 s, beside a plain stream fed the same seconds of mono int16 audio at the estimator's rate (the only
              push there was before the carried resampler): per push by events on the stream, median and 95th percentile; and the two
              added launches (stream_resample_kernel, stream_resample_tail_kernel) per launch under the library's kernel timer.

  --method profile [--tuning-meter]: this section alone.  est.stream(R, method="profile") on an estimator without a net beside
              est.stream(R) with the net, both fed 0.5 s float32 chunks, at strides of 5 s and 1 s (15 s windows): per push by events on
              the stream, median and 95th percentile; the two added launches (stream_frame_stats_kernel, stream_profile_score_kernel) per
              launch under the library's kernel timer; and, on synthesised recordings, how many of a profile stream's key labels are those
              of track(method="profile") on the whole audio.  --tuning-meter (also with --method net) opens the streams with the meter.

  --retune-cents C: this section alone.  est.stream(R, retune_cents=C) beside est.stream(R), both fed float32 chunks of 0.1 s and 1 s: three
              rounds of --pushes pushes each, the two streams taking turns; per push by events on the stream, the median of each round, and
              over the rounds their median and spread; and the two added launches (stream_retune_kernel, stream_retune_tail_kernel) per
              launch under the library's kernel timer.

  --refine: this section alone.  est.stream(R, refine=True) beside est.stream(R), with the net and with method="profile", both fed float32
              chunks of one hop and of 1 s: three rounds of --pushes pushes each, the two streams taking turns; per push by events on the
              stream, the median of each round, over the rounds their median and spread, and what refine adds at the median; the launches
              it adds (stream_key_changes_kernel, and on a net stream stream_frame_stats_kernel) per launch under the library's kernel
              timer.  And the two change-point kernels per boundary on the same spans: alternating labels on 40 windows at the default
              geometry (76 frames, 25 apart, slack 25: spans of 75 frames), key_changes_kernel on the log-CQT beside
              stream_key_changes_kernel on the chroma ring, all boundaries in one call and one boundary a call (a push's shape).

Usage: python tools/stream_bench.py [--pushes 200] [--accuracy] [--posteriors] [--source-rate 48000 --source-channels 2]
                                    [--method profile] [--tuning-meter] [--retune-cents 33.3] [--refine]"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time
from argparse import Namespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ake_amd  # noqa: E402
from ake_amd import _lib, metrics  # noqa: E402
from ake_amd.pipeline import KeyTrack  # noqa: E402

SR, DEV, HOP = 22050, "cuda:0", 4410
GROUPS = {"transform": ("stream_history", "stream_frames", "cqt_", "decim", "transpose", "logmag"),
          "smoother": ("decode_keys", "key_emissions", "key_stream_step")}


def group_of(kernel):
    for g, prefixes in GROUPS.items():
        if any(kernel.startswith(p) or p in kernel for p in prefixes):
            return g
    return "net"


def percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def push_row(est, R, chunk, dtype, pushes, baseline_reps):
    src = torch.randn((R, chunk * 8), device=DEV) * 0.3
    if dtype == torch.int16:
        src = (src.clamp(-1, 1) * 32767).to(torch.int16)
    pieces = [src[:, i * chunk:(i + 1) * chunk] for i in range(8)]
    s = est.stream(R)
    for i in range(30 * SR // chunk + 1):                                            # warm: windows are being emitted
        s.push(pieces[i % 8])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(pushes)]
    emitted = []
    for i, (a, b) in enumerate(ev):
        a.record()
        u = s.push(pieces[i % 8])
        b.record()
        emitted.append(u.windows)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    _lib.prof_enable("", True)
    for i in range(pushes):
        s.push(pieces[i % 8])
    split = {"transform": 0.0, "net": 0.0, "smoother": 0.0}
    for name, (total, _) in _lib.prof_results().items():
        split[group_of(name)] += total / pushes
    _lib.prof_enable("", False)
    buf = torch.randn((R, 60 * SR), device=DEV) * 0.3
    if dtype == torch.int16:
        buf = (buf.clamp(-1, 1) * 32767).to(torch.int16)
    for _ in range(2):
        est.track(buf, smooth=True)
    torch.cuda.synchronize()
    base = []
    for _ in range(baseline_reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        est.track(buf, smooth=True)
        b.record()
        b.synchronize()
        base.append(a.elapsed_time(b))
    del buf, s
    torch.cuda.empty_cache()
    with_window = [m for m, k in zip(ms, emitted) if k]
    mean = statistics.fmean(ms)
    return {"recordings": R, "chunk_s": round(chunk / SR, 3), "dtype": "int16" if dtype == torch.int16 else "float32",
            "push_ms": {"median": round(statistics.median(ms), 4), "p95": round(percentile(ms, 0.95), 4), "max": round(max(ms), 4),
                        "mean": round(mean, 4), "median_with_window": round(statistics.median(with_window), 4) if with_window else None,
                        "pushes_with_window": len(with_window)},
            "kernels_ms_per_push": {k: round(v, 4) for k, v in split.items()},
            "launch_share": round(1.0 - sum(split.values()) / mean, 3),
            "baseline_track_60s_ms": round(statistics.median(base), 4),
            "baseline_over_push_p95": round(statistics.median(base) / percentile(ms, 0.95), 1)}


def smoother_rows():
    L = _lib.lib()
    R, K = 8, 2000
    e = torch.randn((R, K, 24), device=DEV) * 3
    A = metrics.key_transition_log(0.92).float().to(DEV)
    out, path, k_out = torch.empty_like(e), torch.empty((R, K), dtype=torch.int32, device=DEV), C.c_int(0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for lag in (3, 12, 255):
        state = torch.zeros(L.ake_key_stream_state_bytes(R, lag), dtype=torch.uint8, device=DEV)

        def call(k, before):
            _lib.check(L.ake_key_stream_step_f32(e.data_ptr(), R, k, before, lag, 0, A.data_ptr(), None, state.data_ptr(), state.numel(), out.data_ptr(),
                                                 path.data_ptr(), C.byref(k_out), stream), "ake_key_stream_step_f32")

        res = {}
        for name, k, before, reps in (("all_at_once", K, 0, 10), ("one_per_call", 1, 1000, 200)):
            call(k, before)
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(k, before)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            res[name] = statistics.median(ms)
        rows.append({"lag": lag, "us_per_window": round(1e3 * res["all_at_once"] / K, 4), "one_window_call_us": round(1e3 * res["one_per_call"], 2)})
    return rows


def posteriors_rows(est, recordings, pushes):
    rows = []
    chunk = torch.randn((max(recordings), SR), device=DEV) * 0.3
    names = ("key_stream_step_kernel", "key_stream_sweep_kernel", "key_stream_loglik_kernel")
    for R in recordings:
        for stride in (15.0, 5.0, 1.0):
            for lag in (6, 30):
                s = est.stream(R, stride_seconds=stride, lag_windows=lag, posteriors=True)
                A = s.trans.cpu()
                state = None
                for _ in range(int(15 + (lag + 2) * stride) + 1):                    # warm: every sweep runs its whole lag from here on
                    u = s.push(chunk[:R])
                    if u.windows:
                        *_, state = metrics.key_stream_posteriors(u.emissions.cpu(), A, lag=lag, state=state, flush=False, return_state=True)
                torch.cuda.synchronize()
                _lib.prof_enable("", True)
                ups = [s.push(chunk[:R]) for _ in range(pushes)]
                prof = _lib.prof_results()
                _lib.prof_enable("", False)
                host, worst = [], 0.0
                for u in ups:
                    if not u.windows:
                        continue
                    t0 = time.perf_counter()
                    post, ll, state = metrics.key_stream_posteriors(u.emissions.cpu(), A, lag=lag, state=state, flush=False, return_state=True)
                    host.append(1e3 * (time.perf_counter() - t0))
                    worst = max(worst, float((post - u.posteriors.cpu()).abs().max()))
                rows.append({"recordings": R, "stride_s": stride, "lag": lag, "pushes_with_window": len(host),
                             "windows_per_such_push": round(sum(u.windows for u in ups) / max(1, len(host)), 2),
                             "kernel_us_per_launch": {n: round(1e3 * prof[n][0] / prof[n][1], 2) for n in names if n in prof},
                             "host_route_ms_per_push": round(statistics.median(host), 3) if host else None,
                             "max_abs_diff_to_host_float32": worst})
                del s
    return rows


def timed_pushes(s, pieces, pushes, warm):
    """Milliseconds of each of `pushes` pushes, by events on the stream, after `warm` pushes."""
    for i in range(warm):
        s.push(pieces[i % len(pieces)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(pushes)]
    for i, (a, b) in enumerate(ev):
        a.record()
        s.push(pieces[i % len(pieces)])
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def source_rows(est, recordings, pushes, rate, channels):
    """A push of int16 audio at `rate` Hz with `channels` interleaved channels (their mean taken) through the carried resampler, beside a
    push of the same seconds of mono int16 audio at the estimator's rate -- the only push there was before --, and the two added
    launches on their own."""
    rows = []
    for R in recordings:
        for seconds in (0.2, 1.0):
            m_src, m = int(round(seconds * rate)), int(round(seconds * SR))
            noise = lambda *shape: (torch.randn(shape, device=DEV) * 0.3).clamp(-1, 1).mul(32767).to(torch.int16)   # noqa: E731
            src = [noise(R, m_src, channels).transpose(1, 2) for _ in range(8)]            # interleaved storage, read in place
            mono = [noise(R, m) for _ in range(8)]
            warm = int(30 / seconds) + 1
            kw = dict(source_rate=rate, source_channels=channels, channel=-1 if channels > 1 else 0)
            ms_src = timed_pushes(est.stream(R, **kw), src, pushes, warm)
            ms_mono = timed_pushes(est.stream(R), mono, pushes, warm)
            s = est.stream(R, **kw)
            for i in range(warm):
                s.push(src[i % 8])
            torch.cuda.synchronize()
            _lib.prof_enable("stream_resample", True)
            for i in range(pushes):
                s.push(src[i % 8])
            prof = _lib.prof_results()
            _lib.prof_enable("", False)
            stat = lambda ms: {"median": round(statistics.median(ms), 4), "p95": round(percentile(ms, 0.95), 4)}   # noqa: E731
            rows.append({"recordings": R, "chunk_s": seconds, "source": f"{rate} Hz x {channels} int16 interleaved", "push_ms_source": stat(ms_src),
                         "push_ms_mono_int16_at_the_estimators_rate": stat(ms_mono),
                         "added_ms_median": round(statistics.median(ms_src) - statistics.median(ms_mono), 4),
                         "kernel_us_per_launch": {n: round(1e3 * t / k, 2) for n, (t, k) in prof.items()}})
            del s, src, mono
    return rows


def method_rows(est, recordings, pushes, method, meter):
    """A push of a stream opened with `method` (and the tuning meter) beside a push of the net's stream without it, 0.5 s chunks."""
    free = ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)
    chunk = SR // 2
    stat = lambda ms: {"median": round(statistics.median(ms), 4), "p95": round(percentile(ms, 0.95), 4), "mean": round(statistics.fmean(ms), 4)}   # noqa: E731
    rows = []
    for R in recordings:
        pieces = [torch.randn((R, chunk), device=DEV) * 0.3 for _ in range(8)]
        for stride in (5.0, 1.0):
            warm = 30 * SR // chunk + 1
            kw = dict(stride_seconds=stride, method=method, tuning_meter=meter)
            owner = free if method == "profile" else est
            ms_new = timed_pushes(owner.stream(R, **kw), pieces, pushes, warm)
            ms_net = timed_pushes(est.stream(R, stride_seconds=stride), pieces, pushes, warm)
            s = owner.stream(R, **kw)
            for i in range(warm):
                s.push(pieces[i % 8])
            torch.cuda.synchronize()
            _lib.prof_enable("", True)
            for i in range(pushes):
                s.push(pieces[i % 8])
            prof = _lib.prof_results()
            _lib.prof_enable("", False)
            rows.append({"recordings": R, "chunk_s": 0.5, "window_s": 15, "stride_s": stride, "method": method, "tuning_meter": meter,
                         "push_ms": stat(ms_new), "push_ms_net_stream": stat(ms_net),
                         "kernel_us_per_launch": {n: round(1e3 * t / k, 2) for n, (t, k) in prof.items() if n.startswith("stream_") and k},
                         "launches_per_push": round(sum(k for _, k in prof.values()) / pushes, 2),
                         "kernels_ms_per_push": round(sum(t for t, _ in prof.values()) / pushes, 4)})
            del s
    return rows


def retune_rows(est, recordings, pushes, cents, rounds=3):
    """A push of est.stream(R, retune_cents=cents) beside a push of est.stream(R), float32 chunks of 0.1 s and 1 s: `rounds` rounds of
    `pushes` pushes each, the two streams taking turns in one process; per round the median, and over the rounds the median of those and
    their spread (largest - smallest).  And the two added launches on their own, under the library's kernel timer."""
    rows = []
    for R in recordings:
        for seconds in (0.1, 1.0):
            m = int(round(seconds * SR))
            pieces = [torch.randn((R, m), device=DEV) * 0.3 for _ in range(8)]
            warm = int(30 / seconds) + 1
            meds = {"retuned": [], "plain": []}
            for _ in range(rounds):
                for kind, kw in (("retuned", dict(retune_cents=cents)), ("plain", {})):
                    meds[kind].append(statistics.median(timed_pushes(est.stream(R, **kw), pieces, pushes, warm)))
            s = est.stream(R, retune_cents=cents)
            for i in range(warm):
                s.push(pieces[i % 8])
            torch.cuda.synchronize()
            _lib.prof_enable("stream_retune", True)
            for i in range(pushes):
                s.push(pieces[i % 8])
            prof = _lib.prof_results()
            _lib.prof_enable("", False)
            stat = lambda xs: {"median_of_rounds": round(statistics.median(xs), 4), "spread": round(max(xs) - min(xs), 4),   # noqa: E731
                               "rounds": [round(x, 4) for x in xs]}
            rows.append({"recordings": R, "chunk_s": seconds, "retune_cents": cents, "push_ms_retuned": stat(meds["retuned"]),
                         "push_ms_plain": stat(meds["plain"]),
                         "added_ms_median": round(statistics.median(meds["retuned"]) - statistics.median(meds["plain"]), 4),
                         "kernel_us_per_launch": {n: round(1e3 * t / k, 2) for n, (t, k) in prof.items() if k}})
            del s, pieces
    return rows


def refine_rows(est, recordings, pushes, rounds=3):
    """A push of a stream opened with refine=True beside a push of the same stream without it: `rounds` rounds of `pushes` pushes each,
    the two taking turns in one process; and the launches refine adds, under the library's kernel timer."""
    free = ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)
    rows = []
    for R in recordings:
        for method, owner in (("net", est), ("profile", free)):
            for m in (HOP, SR):
                pieces = [torch.randn((R, m), device=DEV) * 0.3 for _ in range(8)]
                warm = 60 * SR // m + 1                                              # (30 s of lag behind the first window: boundaries are being emitted)
                meds = {"refined": [], "plain": []}
                for _ in range(rounds):
                    for kind, kw in (("refined", dict(refine=True)), ("plain", {})):
                        meds[kind].append(statistics.median(timed_pushes(owner.stream(R, method=method, **kw), pieces, pushes, warm)))
                s = owner.stream(R, method=method, refine=True)
                for i in range(warm):
                    s.push(pieces[i % 8])
                torch.cuda.synchronize()
                _lib.prof_enable("", True)
                ups = [s.push(pieces[i % 8]) for i in range(pushes)]
                prof = _lib.prof_results()
                _lib.prof_enable("", False)
                cells = torch.cat([u.change_frame for u in ups], dim=1)
                stat = lambda xs: {"median_of_rounds": round(statistics.median(xs), 4), "spread": round(max(xs) - min(xs), 4),   # noqa: E731
                                   "rounds": [round(x, 4) for x in xs]}
                rows.append({"recordings": R, "method": method, "chunk_s": round(m / SR, 3), "push_ms_refined": stat(meds["refined"]),
                             "push_ms_plain": stat(meds["plain"]),
                             "added_ms_median": round(statistics.median(meds["refined"]) - statistics.median(meds["plain"]), 4),
                             "kernel_us_per_launch": {n: round(1e3 * t / k, 2) for n, (t, k) in prof.items()
                                                      if k and n in ("stream_key_changes_kernel", "stream_frame_stats_kernel")},
                             "launches_per_push": {n: round(k / pushes, 3) for n, (t, k) in prof.items()
                                                   if k and n in ("stream_key_changes_kernel", "stream_frame_stats_kernel")},
                             "boundaries_emitted": int(cells.shape[1]), "of_them_key_changes": int((cells >= 0).sum()) // R if R else 0})
                del s, pieces
    return rows


def change_kernel_rows(recordings, reps=20):
    """key_changes_kernel and stream_key_changes_kernel per boundary on the same spans, under the library's kernel timer."""
    from ake_amd import keyprofile
    L = _lib.lib()
    wf, sf, slack, W, P = 76, 25, 25, 40, 288
    T = wf + (W - 1) * sf
    stream = torch.cuda.current_stream().cuda_stream
    prof = keyprofile.device_profiles("krumhansl", torch.device(DEV))
    rows = []
    for R in recordings:
        mel = torch.rand((R, P, T), device=DEV) * 3.0
        labels = ((torch.arange(W, device=DEV)[None, :] + torch.arange(R, device=DEV)[:, None]) % 24).to(torch.int32).contiguous()
        outs = [torch.empty((R, W - 1), dtype=torch.int32, device=DEV), torch.empty((R, W - 1), device=DEV), torch.empty((R, W - 1), device=DEV)]
        ring, label_ring = T, W + 3
        chroma = torch.empty(L.ake_stream_profile_state_bytes(R, ring), dtype=torch.uint8, device=DEV)
        state = torch.empty(L.ake_stream_key_changes_state_bytes(R, label_ring), dtype=torch.uint8, device=DEV)
        _lib.check(L.ake_stream_frame_stats_f32(mel.data_ptr(), 0, R, P, T, 0, T, 0, ring, 1, 0, 0.0, chroma.data_ptr(), chroma.numel(), None, None, stream),
                   "ake_stream_frame_stats_f32")

        def offline():
            _lib.check(L.ake_key_changes_f32(mel.data_ptr(), 0, R, P, T, None, labels.data_ptr(), W, None, wf, sf, slack, prof.data_ptr(), 0,
                                             *[o.data_ptr() for o in outs], stream), "ake_key_changes_f32")

        def streamed(first, n, k, before, flush):
            new = labels[:, before:before + k].contiguous()
            _lib.check(L.ake_stream_key_changes_f32(chroma.data_ptr(), chroma.numel(), R, ring, T, new.data_ptr() if k else None, k, before, flush, wf, sf,
                                                    slack, prof.data_ptr(), state.data_ptr(), state.numel(), label_ring, first, n,
                                                    *[o.data_ptr() for o in outs], stream), "ake_stream_key_changes_f32")

        offline()
        want = [o.clone() for o in outs]
        streamed(0, W - 1, W, 0, 1)
        same = all(torch.equal(a, b) for a, b in zip(outs, want))
        torch.cuda.synchronize()
        _lib.prof_enable("key_changes_kernel", True)
        for _ in range(reps):
            offline()
            streamed(0, W - 1, W, 0, 1)
        whole = _lib.prof_results()
        for _ in range(reps):                                                        # one boundary a call: window 21 arrives, boundary 18 is final
            streamed(18, 1, 1, 21, 0)
        one = _lib.prof_results()
        _lib.prof_enable("", False)
        per = lambda res, name, n: round(1e3 * res[name][0] / res[name][1] / n, 3)   # noqa: E731
        rows.append({"recordings": R, "windows": W, "span_frames": sf + 2 * slack, "bits_equal": same,
                     "all_in_one_call_us_per_boundary": {n: per(whole, n, (W - 1) * R) for n in whole},
                     "all_in_one_call_us_per_launch": {n: per(whole, n, 1) for n in whole},
                     "one_boundary_a_call_us_per_launch": {n: per(one, n, 1) for n in one}})
    return rows


def agreement_rows():
    """A profile stream's key labels against track(method="profile") on the whole audio: 24 synthesised modulating recordings of 5 min."""
    from ake_amd import synthetic
    free = ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)
    audio, _ = synthetic.make_modulating_batch_device(range(24), 300.0, DEV)
    rows = []
    for stride in (5.0, 1.0):
        tr = free.track(audio, stride_seconds=stride, method="profile")
        s = free.stream(24, stride_seconds=stride, method="profile", smooth=False)
        ups = [s.push(audio[:, a:a + SR // 2]) for a in range(0, audio.shape[1], SR // 2)] + [s.finish()]
        key_id = torch.cat([u.key_id for u in ups], dim=1)
        chroma = torch.cat([u.key for u in ups], dim=1)
        assert key_id.shape == tr.key_id.shape
        rows.append({"stride_s": stride, "windows": int(key_id.numel()), "labels_equal": int((key_id == tr.key_id).sum()),
                     "share": round(float((key_id == tr.key_id).float().mean()), 5), "largest_chroma_difference": float((chroma - tr.key).abs().max())})
    return rows


def frame_rows(est):
    plan = est.plan
    H = int(_lib.lib().ake_cqt_plan_half_support(plan.handle))
    x = torch.randn((2, 100 * HOP), device=DEV) * 0.3
    offline = plan.logmag(x)
    rows = []
    for name, hops in (("off the grid", 7), ("off the grid", 33), ("on the grid (64 hops)", 64)):
        s0 = hops * HOP
        part = plan.logmag(x[:, s0:].contiguous())
        skip = -(-H // HOP)                                                          # frames whose support reaches in front of s0
        a, b = part[:, :, skip:], offline[:, :, hops + skip:]
        rows.append({"s0_hops": hops, "s0_mod_128": s0 % 128, "grid": name, "max_abs_diff": float((a - b).abs().max()),
                     "rel_to_peak": float((a - b).abs().max() / b.abs().max()), "equal": bool(torch.equal(a, b))})
    return H, rows


def accuracy_rows():
    spec = importlib.util.spec_from_file_location("track_accuracy", os.path.join(REPO, "tools", "track_accuracy.py"))
    ta = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ta)
    from ake_amd import synthetic
    net, training = ta.train_net(10, 604)
    est = ake_amd.KeyEstimator(net, SR, 5)
    R = 24
    audio, ann = synthetic.make_modulating_batch_device(range(R), 300.0, DEV)
    tr = est.track(audio, stride_seconds=5.0, smooth=True)
    rows = [("raw key_id (track)", ta.row_of(tr.score(ann, smoothed=False))), ("offline Viterbi (track)", ta.row_of(tr.score(ann)))]
    for lag in (0, 3, 6, 12):
        s = est.stream(R, stride_seconds=5.0, lag_windows=lag)
        ups = [s.push(audio[:, a:a + 10 * SR]) for a in range(0, audio.shape[1], 10 * SR)] + [s.finish()]
        cat = lambda n: torch.cat([getattr(u, n) for u in ups], dim=1)              # noqa: E731
        W = cat("key_id").shape[1]
        assert W == tr.key.shape[1]
        st = KeyTrack(cat("key"), cat("tonic"), None, cat("key_id"), cat("signature_id"), cat("tonic_id"), cat("confidence"),
                      torch.full((R,), W, dtype=torch.int32, device=DEV), torch.cat([u.times for u in ups]), tr.window_seconds, tr.stride_seconds,
                      cat("emissions"), cat("smooth_key_id"), hop=tr.hop, window_frames=tr.window_frames, stride_frames=tr.stride_frames,
                      sample_rate=SR)
        rows.append((f"fixed lag {lag} ({lag * 5} s)", ta.row_of(st.score(ann))))
        if lag == 0:
            rows.append(("raw key_id (stream)", ta.row_of(st.score(ann, smoothed=False))))
    return {"training": training, "recordings": R, "minutes": 5, "stride_s": 5, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--baseline-reps", type=int, default=10)
    ap.add_argument("--recordings", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--posteriors", action="store_true")
    ap.add_argument("--source-rate", type=int, default=None)
    ap.add_argument("--source-channels", type=int, default=1)
    ap.add_argument("--method", choices=("net", "profile"), default=None)
    ap.add_argument("--tuning-meter", action="store_true")
    ap.add_argument("--retune-cents", type=float, default=None)
    ap.add_argument("--refine", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    gold = np.load(os.path.join(REPO, "tests", "golden", "pcnet_default.npz"))
    sd = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd/")}
    net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True))
    net.load_state_dict(sd, strict=True)
    est = ake_amd.KeyEstimator(net.to(DEV).eval(), SR, 5)
    if args.posteriors:
        print(json.dumps({"device": torch.cuda.get_device_name(0), "pushes": args.pushes, "chunk_s": 1.0,
                          "posteriors": posteriors_rows(est, args.recordings, args.pushes)}))
        return
    if args.source_rate is not None:
        print(json.dumps({"device": torch.cuda.get_device_name(0), "pushes": args.pushes,
                          "source": source_rows(est, args.recordings, args.pushes, args.source_rate, args.source_channels)}))
        return
    if args.retune_cents is not None:
        print(json.dumps({"device": torch.cuda.get_device_name(0), "pushes": args.pushes,
                          "retune": retune_rows(est, args.recordings, args.pushes, args.retune_cents)}))
        return
    if args.refine:
        print(json.dumps({"device": torch.cuda.get_device_name(0), "pushes": args.pushes,
                          "refine": refine_rows(est, args.recordings, args.pushes), "change_kernels": change_kernel_rows(args.recordings)}))
        return
    if args.method is not None or args.tuning_meter:
        method = args.method or "net"
        out = {"device": torch.cuda.get_device_name(0), "pushes": args.pushes, "method": method_rows(est, args.recordings, args.pushes, method, args.tuning_meter)}
        if method == "profile":
            out["streamed_against_offline_labels"] = agreement_rows()
        print(json.dumps(out))
        return
    rows = [push_row(est, R, chunk, dtype, args.pushes, args.baseline_reps)
            for R in args.recordings for chunk in (HOP, SR) for dtype in (torch.float32, torch.int16)]
    H, frames = frame_rows(est)
    result = {"device": torch.cuda.get_device_name(0), "pushes": args.pushes, "stride_s": 5, "lag_windows": 6, "push": rows,
              "smoother": smoother_rows(),
              "support": {"H_samples": H, "H_hops": round(H / HOP, 3), "H_seconds": round(H / SR, 4),
                          "raw_label_latency_s": "H + at most one hop + the chunk: %.2f .. %.2f s behind the window's last frame centre (plus the chunk)"
                                                 % (H / SR, (H + HOP) / SR),
                          "smoothed_label_latency_s": "that + lag_windows x stride (6 x 5 s = 30 s at the defaults)"},
              "frames": frames}
    if args.accuracy:
        result["accuracy"] = accuracy_rows()
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
