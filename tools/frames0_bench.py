"""Whole-song mode (--frames 0) timings -> one JSON line.

  per_clip_cqt   : ake_cqt_logmag_hops_f32 on 64 songs of 3 min at 22.05 kHz, lengths ragged +-30 % (each clip its own hop), 592 frames
  key_estimator  : the same batch through KeyEstimator(frames=0): per-clip-hop CQT + the default net at T = 592, seq_length None
  uniform_ab     : the bench batch (256 x 15 s, hop 4410 for every clip): logmag_hops on the hop-1 plan vs the fixed-hop engine-3 logmag

hipEvent-timed (torch.cuda.Event), warm, median of --reps launches each.  Usage: python tools/frames0_bench.py [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ake_amd  # noqa: E402
from ake_amd import synthetic  # noqa: E402
from ake_amd.cqt import get_any_hop_plan, hop_for_window  # noqa: E402

SR, DEV = 22050, "cuda:0"


def timed(fn, reps, warmup=3):
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
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--songs", type=int, default=64)
    args = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)

    # 64 whole songs: 3 min +-30 %, white noise (the CQT's cost does not depend on the content)
    B = args.songs
    lens = (SR * 180 * rng.uniform(0.7, 1.3, B)).astype(np.int64)
    n_max = int(lens.max())
    audio = torch.randn((B, n_max), device=DEV) * 0.3
    lengths = torch.from_numpy(lens).to(DEV)
    hops = hop_for_window(lengths, 592).to(torch.int32)
    plan = get_any_hop_plan(SR, 288, device=DEV)
    out = torch.empty((B, 288, 592), device=DEV)
    ws = torch.empty(plan.workspace_bytes_hops(B, n_max, 592), dtype=torch.uint8, device=DEV)
    cqt_ms = timed(lambda: plan.logmag_hops(audio, hops, lengths, out_frames=592, out=out, workspace=ws), args.reps)
    ake_amd._lib.prof_enable("", True)
    plan.logmag_hops(audio, hops, lengths, out_frames=592, out=out, workspace=ws)
    per_kernel_songs = {k: round(v[0], 4) for k, v in ake_amd._lib.prof_results().items()}
    ake_amd._lib.prof_enable("", False)

    gold = np.load(os.path.join(REPO, "tests", "golden", "pcnet_default.npz"))
    sd = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd/")}
    from argparse import Namespace
    net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True))
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    est = ake_amd.KeyEstimator(net, SR, frames=0, window_size=592)
    est_ms = timed(lambda: est(audio, lengths), args.reps)

    # uniform-hop A/B on the bench batch
    a256, _ = synthetic.make_batch_device(range(256), torch.device(DEV))
    fixed = ake_amd.CQTPlan(SR, 4410, 288, 36, device=DEV)
    T = fixed.num_frames(a256.shape[1])
    o1 = torch.empty((256, 288, T), device=DEV)
    o2 = torch.empty((256, 288, T), device=DEV)
    h256 = torch.full((256,), 4410, dtype=torch.int32, device=DEV)
    ws2 = torch.empty(plan.workspace_bytes_hops(256, a256.shape[1], T), dtype=torch.uint8, device=DEV)
    fixed_ms = timed(lambda: fixed.logmag(a256, out=o1), args.reps)
    hops_ms = timed(lambda: plan.logmag_hops(a256, h256, out_frames=T, out=o2, workspace=ws2), args.reps)
    ake_amd._lib.prof_enable("", True)
    plan.logmag_hops(a256, h256, out_frames=T, out=o2, workspace=ws2)
    per_kernel = {k: round(v[0], 4) for k, v in ake_amd._lib.prof_results().items()}
    fixed.logmag(a256, out=o1)
    per_kernel_fixed = {k: round(v[0], 4) for k, v in ake_amd._lib.prof_results().items()}
    ake_amd._lib.prof_enable("", False)
    torch.cuda.synchronize()
    print(json.dumps({
        "device": torch.cuda.get_device_name(0), "reps": args.reps,
        "per_clip_cqt": {"songs": B, "seconds_min": round(float(lens.min()) / SR, 1), "seconds_max": round(float(lens.max()) / SR, 1),
                         "ms": round(cqt_ms, 4), "clips_per_s": round(B / cqt_ms * 1e3, 1), "kernels_ms": per_kernel_songs},
        "key_estimator": {"songs": B, "frames": 592, "ms": round(est_ms, 4), "clips_per_s": round(B / est_ms * 1e3, 1)},
        "uniform_ab": {"batch": 256, "seconds": 15, "hop": 4410, "fixed_hop_ms": round(fixed_ms, 4), "logmag_hops_ms": round(hops_ms, 4),
                       "ratio": round(hops_ms / fixed_ms, 3), "bit_identical": bool(torch.equal(o1, o2)),
                       "kernels_logmag_hops_ms": per_kernel, "kernels_fixed_ms": per_kernel_fixed},
    }))


if __name__ == "__main__":
    main()
