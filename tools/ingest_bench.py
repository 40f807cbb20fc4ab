"""Audio that starts in host memory: what the estimator delivers end to end, as float32 and as 16-bit PCM -> one JSON line.

256 clips of 15 s at 22.05 kHz in pinned host memory, fed `--batches` times per measurement; medians of `--reps` wall-clock runs
(perf_counter around the loop, device synchronised before and after).

  a  float32, serial: est(batch.to(dev)) -- upload, then compute, then the next upload
  b  float32 through HostFeeder (uploads on a copy stream under the previous batch's compute); b_pageable: the same from pageable memory,
     which adds the staging copy on the host
  c  int16 mono through HostFeeder; c_pageable likewise
  d  int16 interleaved stereo (B, n, 2) storage, channel=-1, through HostFeeder (the PCM resampler mixes it down in place)
  e  device-resident int16 against device-resident float32 (hipEvent-timed), with the cascade's time from the library's own timers
  f  the box's pinned host-to-device rate on the float32 batch; a-d are also stated as a share of it
  g  eight 5-minute recordings through track(), float32 and int16, serial and through HostFeeder

`--trace-only`: nothing but a few device-resident float32 and int16 CQTs, for a `rocprofv3 --kernel-trace --stats` run of its own (the two
cascade instantiations appear under their own names).

Usage: python tools/ingest_bench.py [--reps 5] [--batches 4] [--trace-only]
"""
import argparse
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
from ake_amd import synthetic  # noqa: E402

SR, DEV = 22050, "cuda:0"


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return statistics.median(s), min(s), max(s)


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def cascade_ms(fn, reps):
    """The cascade kernel's own time per call, from the library's hipEvent timers."""
    ake_amd._lib.prof_enable("cqt_cascade_kernel", True)
    ake_amd._lib.prof_results()
    for _ in range(reps):
        fn()
    ms, n = ake_amd._lib.prof_results()["cqt_cascade_kernel"]
    ake_amd._lib.prof_enable("", False)
    return ms / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()

    B, K = args.clips, args.batches
    f32_dev, _ = synthetic.make_batch_device(range(B), torch.device(DEV))
    pcm_dev = torch.round(f32_dev * 32767.0).to(torch.int16)
    f32_dev = ake_amd.pcm16_to_float(pcm_dev)                          # the same audio in both forms
    n = f32_dev.shape[1]

    if args.trace_only:
        plan = ake_amd.get_plan(SR, 4410, 288, 36, DEV)
        for _ in range(10):
            plan.logmag(f32_dev)
            plan.logmag(pcm_dev)
        torch.cuda.synchronize()
        return

    gold = np.load(os.path.join(REPO, "tests", "golden", "pcnet_default.npz"))
    net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True))
    net.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd/")}, strict=True)
    net = net.to(DEV).eval()
    est = ake_amd.KeyEstimator(net, SR, 5)

    f32_pin, pcm_pin = f32_dev.cpu().pin_memory(), pcm_dev.cpu().pin_memory()
    f32_page, pcm_page = f32_pin.clone(), pcm_pin.clone()
    stereo_pin = torch.stack([pcm_pin, torch.roll(pcm_pin, 1, dims=1)], dim=2).pin_memory().transpose(1, 2)   # (B, n, 2) storage, (B, 2, n) view

    def serial(x):
        def run():
            outs = [est(x.to(DEV)) for _ in range(K)]
            return outs
        return run

    def fed(x, **kw):
        feeder = ake_amd.HostFeeder(est, depth=2, **kw)
        return lambda: list(feeder([x] * K))

    routes = {
        "a_f32_serial": (serial(f32_pin), f32_pin),
        "b_f32_feeder": (fed(f32_pin), f32_pin),
        "b_f32_feeder_pageable": (fed(f32_page), f32_page),
        "c_pcm_feeder": (fed(pcm_pin), pcm_pin),
        "c_pcm_feeder_pageable": (fed(pcm_page), pcm_page),
        "d_pcm_stereo_interleaved_feeder": (fed(stereo_pin, channel=-1), stereo_pin),
    }

    # f: the link, on the float32 batch
    dst = torch.empty_like(f32_dev)
    h2d_ms, _, _ = event_ms(lambda: dst.copy_(f32_pin, non_blocking=True), args.reps)
    link = f32_pin.numel() * 4 / (h2d_ms * 1e-3)                       # bytes per second

    res = {"device": torch.cuda.get_device_name(0), "clips": B, "seconds": n / SR, "batches": K, "reps": args.reps,
           "f_h2d_pinned_GBps": round(link / 1e9, 2)}
    for name, (fn, x) in routes.items():
        med, lo, hi = wall(fn, args.reps)
        nbytes = x.numel() * x.element_size() * K
        res[name] = {"clips_per_s": round(B * K / med), "spread_clips_per_s": [round(B * K / hi), round(B * K / lo)],
                     "ms_per_batch": round(med / K * 1e3, 3), "link_share": round(nbytes / med / link, 3)}
    base = res["a_f32_serial"]["clips_per_s"]
    for name in routes:
        res[name]["vs_a"] = round(res[name]["clips_per_s"] / base, 3)

    # e: device-resident
    plan = est.plan
    e = {}
    for name, x in (("f32", f32_dev), ("pcm", pcm_dev)):
        med, lo, hi = event_ms(lambda: est(x), 20)
        e[name] = {"estimator_ms": round(med, 4), "spread_ms": [round(lo, 4), round(hi, 4)],
                   "cascade_ms": round(cascade_ms(lambda: plan.logmag(x), 20), 4)}
    e["bit_identical"] = all(torch.equal(p, q) for p, q in zip(est(f32_dev), est(pcm_dev)))
    res["e_resident"] = e

    # g: tracking
    R, per = 8, 20                                                     # 20 clips of 15 s end to end = one 5-minute recording
    rec_pcm = pcm_dev.repeat((R * per + B - 1) // B, 1)[:R * per].reshape(R, per * n)
    n_rec = rec_pcm.shape[1]
    rec_pcm_pin = rec_pcm.cpu().pin_memory()
    rec_f32_pin = ake_amd.pcm16_to_float(rec_pcm_pin).pin_memory()
    g = {"recordings": R, "seconds": n_rec / SR, "batches": K}
    for name, x in (("f32", rec_f32_pin), ("pcm", rec_pcm_pin)):
        feeder = ake_amd.HostFeeder(est, depth=2, track=True)
        s_med, s_lo, s_hi = wall(lambda: [est.track(x.to(DEV)) for _ in range(K)], args.reps)
        f_med, f_lo, f_hi = wall(lambda: list(feeder([x] * K)), args.reps)
        nbytes = x.numel() * x.element_size()
        g[name] = {"serial_ms_per_batch": round(s_med / K * 1e3, 3), "feeder_ms_per_batch": round(f_med / K * 1e3, 3),
                   "feeder_spread_ms": [round(f_lo / K * 1e3, 3), round(f_hi / K * 1e3, 3)], "MB_per_batch": round(nbytes / 1e6, 1),
                   "feeder_link_share": round(nbytes * K / f_med / link, 3)}
    dev_ms = {name: round(event_ms(lambda: est.track(x), 10)[0], 4) for name, x in (("f32", rec_f32_pin.to(DEV)), ("pcm", rec_pcm_pin.to(DEV)))}
    g["resident_ms"] = dev_ms
    res["g_track"] = g
    print(json.dumps(res))


if __name__ == "__main__":
    main()
