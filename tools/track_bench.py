"""Key tracking over long recordings: KeyEstimator.track against the clip-wise route -> one JSON line.

  workload : 8 recordings x 5 min at 22.05 kHz (white noise: neither side's cost depends on the content), 15 s windows,
             strides of 15 s, 5 s and 1 s
  A        : est.track(audio, stride_seconds=s) -- one CQT per recording, the net on gathered windows of its frames, the decode kernel
  B        : the clip-wise route: the overlapping windows cut with unfold(...).contiguous() on the device (timed), KeyEstimator.__call__
             on them in batches of 256 clips (the benchmarked shape, which takes the frames-major path), metrics.decode_keys

Both sides run in this process, hipEvent-timed (torch.cuda.Event), warm, median of --reps runs each; per-kernel times from one run of each
under the library's kernel timer.  max_abs_diff is for information: A and B differ at window edges by design (A's edge frames see the
recording's neighbouring audio, B's see zero padding).  Usage: python tools/track_bench.py [--reps 30] [--smooth] [--posteriors]

  --smooth : also, at every stride, what a smooth track costs ("smooth" in each row):
             track_smooth_ms      est.track(audio, stride_seconds=s, smooth=True), timed as A is
             smooth_adds_ms       that minus A
             kernels_ms           key_emissions_kernel and viterbi_keys_kernel under the library's kernel timer
             viterbi_us_per_window  the Viterbi kernel's time over the W windows of a recording (one wave per recording walks them in turn)
             host_route_ms        what a user writes without the kernels: key / tonic / counts of a finished track copied to the CPU, then
                                  metrics.key_emissions and metrics.viterbi_keys there (float32); wall clock from a synchronised device,
                                  copies included, median of min(--reps, 10) runs
             path_agreement       share of windows where the device path equals the host route's (the host route takes its logarithms
                                  with torch on the CPU, so its emissions differ from the kernel's in the last bits; white noise through
                                  seeded weights scores the keys that close)
             viterbi_exact        the device path equals metrics.viterbi_keys on the device's own emissions (what the tests assert)

  --posteriors : also, at every stride, what the posteriors of a smooth track cost ("posteriors" in each row):
             track_posteriors_ms / track_smooth_ms   est.track(..., smooth=True, posteriors=True) and est.track(..., smooth=True), timed in
                                  turn (one of each per repetition), medians
             posteriors_add_ms    their difference
             kernels_ms           key_forward_backward_kernel, key_posteriors_kernel and viterbi_keys_kernel under the library's kernel timer
             chain_us_per_window / viterbi_us_per_window   the chain kernel's and the Viterbi kernel's time over the W windows of a recording
             host_route_ms        emissions and counts of a finished smooth track copied to the CPU, metrics.key_posteriors there (float32);
                                  wall clock from a synchronised device, copies included, median of min(--reps, 10) runs
             fit_device_ms / fit_host_ms   one ake_amd.fit_key_transition of 10 iterations on the track (E-step on the device, the three
                                  launches, M-step on the host) against metrics.fit_key_transition on the copied emissions (float32, copies
                                  included); wall clock, median of 3 runs of each
             max_abs_diff         device posteriors against the host route's, fitted probabilities device against host (for information)
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
from ake_amd import metrics  # noqa: E402

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


def kernels(fn):
    ake_amd._lib.prof_enable("", True)
    fn()
    res = {k: round(v[0], 4) for k, v in ake_amd._lib.prof_results().items()}
    ake_amd._lib.prof_enable("", False)
    return res


def timed_in_turn(f, g, reps, warmup=3):
    """Medians of f and of g, one of each per repetition."""
    for _ in range(warmup):
        f()
        g()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for fn, out in ((f, ms[0]), (g, ms[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
    return statistics.median(ms[0]), statistics.median(ms[1])


def wall(fn, runs):
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), out


def posteriors_row(est, audio, stride, reps):
    smooth = lambda: est.track(audio, stride_seconds=stride, smooth=True)                      # noqa: E731
    both = lambda: est.track(audio, stride_seconds=stride, smooth=True, posteriors=True)      # noqa: E731
    p_ms, s_ms = timed_in_turn(both, smooth, reps)
    k = kernels(both)
    tr = both()
    W = tr.key.shape[1]
    trans = metrics.key_transition_log(stay=float(np.exp(-tr.stride_seconds / 60.0))).float()
    torch.cuda.synchronize()
    h_ms, (post, _) = wall(lambda: metrics.key_posteriors(tr.emissions.cpu(), trans, counts=tr.counts.cpu()), max(1, min(reps, 10)))
    fd_ms, (A_dev, _) = wall(lambda: ake_amd.fit_key_transition(tr, iterations=10), 3)
    fh_ms, (A_host, _) = wall(lambda: metrics.fit_key_transition(tr.emissions.cpu(), counts=tr.counts.cpu(), iterations=10), 3)
    names = ("key_forward_backward_kernel", "key_posteriors_kernel", "viterbi_keys_kernel")
    return {"windows_per_recording": W, "track_posteriors_ms": round(p_ms, 4), "track_smooth_ms": round(s_ms, 4),
            "posteriors_add_ms": round(p_ms - s_ms, 4), "kernels_ms": {n: k.get(n) for n in names},
            "chain_us_per_window": round(1e3 * k.get(names[0], float("nan")) / W, 4),
            "viterbi_us_per_window": round(1e3 * k.get(names[2], float("nan")) / W, 4),
            "host_route_ms": round(h_ms, 4), "host_over_posteriors_add": round(h_ms / max(p_ms - s_ms, 1e-6), 1),
            "fit_device_ms": round(fd_ms, 3), "fit_host_ms": round(fh_ms, 3), "fit_host_over_device": round(fh_ms / fd_ms, 1),
            "max_abs_diff": {"posteriors": float((tr.posteriors.cpu() - post).abs().max()),
                             "fitted_probabilities": float((torch.exp(A_dev) - torch.exp(A_host)).abs().max())}}


def smooth_row(est, audio, stride, track_ms, reps):
    smooth = lambda: est.track(audio, stride_seconds=stride, smooth=True)     # noqa: E731
    s_ms = timed(smooth, reps)
    k = kernels(smooth)
    tr = smooth()
    W = tr.key.shape[1]
    trans = metrics.key_transition_log(stay=float(np.exp(-tr.stride_seconds / 60.0))).float()
    torch.cuda.synchronize()

    def host():
        key, tonic, counts = tr.key.cpu(), tr.tonic.cpu(), tr.counts.cpu()
        return metrics.viterbi_keys(metrics.key_emissions(key, tonic, counts=counts), trans, counts=counts)

    ms = []
    for _ in range(max(1, min(reps, 10))):
        t0 = time.perf_counter()
        path = host()
        ms.append((time.perf_counter() - t0) * 1e3)
    h_ms = statistics.median(ms)
    vit = k.get("viterbi_keys_kernel", float("nan"))
    return {"windows_per_recording": W, "track_smooth_ms": round(s_ms, 4), "smooth_adds_ms": round(s_ms - track_ms, 4),
            "kernels_ms": {n: k.get(n) for n in ("key_emissions_kernel", "viterbi_keys_kernel")},
            "viterbi_us_per_window": round(1e3 * vit / W, 4), "host_route_ms": round(h_ms, 4),
            "host_over_smooth_adds": round(h_ms / max(s_ms - track_ms, 1e-6), 1),
            "path_agreement": round(float((path == tr.smooth_key_id.cpu()).float().mean()), 4),
            "viterbi_exact": bool(torch.equal(metrics.viterbi_keys(tr.emissions.cpu(), trans, counts=tr.counts.cpu()), tr.smooth_key_id.cpu()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--strides", type=float, nargs="+", default=[15.0, 5.0, 1.0])
    ap.add_argument("--smooth", action="store_true", help="also measure track(smooth=True) and the host route it replaces")
    ap.add_argument("--posteriors", action="store_true", help="also measure track(smooth=True, posteriors=True), the host route and the EM fit")
    args = ap.parse_args()
    torch.manual_seed(0)
    gold = np.load(os.path.join(REPO, "tests", "golden", "pcnet_default.npz"))
    sd = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd/")}
    net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True))
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    est = ake_amd.KeyEstimator(net, SR, 5)
    R, n = args.recordings, int(SR * 60 * args.minutes)
    audio = torch.randn((R, n), device=DEV) * 0.3
    win = 15 * SR
    rows = []
    for stride in args.strides:
        step = int(round(stride * 5)) * est.plan.hop_length          # the stride track() uses, in samples

        def clipwise():
            clips = audio.unfold(1, win, step).reshape(-1, win).contiguous()
            outs = [est(clips[c:c + 256]) for c in range(0, clips.shape[0], 256)]
            key, tonic = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
            return key, tonic, metrics.decode_keys(key, tonic)

        track = lambda: est.track(audio, stride_seconds=stride)     # noqa: E731
        a_ms, b_ms = timed(track, args.reps), timed(clipwise, args.reps)
        a_k, b_k = kernels(track), kernels(clipwise)
        tr = track()
        key_b, tonic_b, (key_id_b, _, _, _) = clipwise()
        W = tr.key.shape[1]
        assert key_b.shape[0] == R * W, (key_b.shape, R, W)
        agree = float((tr.key_id.reshape(-1) == key_id_b).float().mean())
        rows.append({"stride_s": stride, "windows": R * W, "track_ms": round(a_ms, 4), "clipwise_ms": round(b_ms, 4),
                     "track_over_clipwise": round(a_ms / b_ms, 3),
                     "max_abs_diff": {"key": float((tr.key.reshape(-1, 12) - key_b).abs().max()),
                                      "tonic": float((tr.tonic.reshape(-1, 12) - tonic_b).abs().max())},
                     "key_id_agreement": round(agree, 4), "track_kernels_ms": a_k, "clipwise_kernels_ms": b_k})
        if args.smooth:
            rows[-1]["smooth"] = smooth_row(est, audio, stride, a_ms, args.reps)
        if args.posteriors:
            rows[-1]["posteriors"] = posteriors_row(est, audio, stride, args.reps)
        del tr, key_b, tonic_b
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "recordings": R, "minutes": args.minutes,
                      "window_s": 15, "strides": rows}))


if __name__ == "__main__":
    main()
