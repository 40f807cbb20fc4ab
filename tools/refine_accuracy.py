#!/usr/bin/env python3
"""How far a key track's boundaries lie from the annotated key changes, with and without the change-point refinement, and what the
refinement's launch costs -> markdown tables (profiles/track_refine.md).

  recordings : synthetic.make_modulating_batch_device, indices 0..23 of 5 min (the scored set of tools/track_accuracy.py)
  net        : the default PitchClassNet trained as tools/track_accuracy.py trains its own (--epochs 0: leave the net's rows out)
  rows       : per method, KeyTrack.boundary_score of the raw key_id on the grid, of the Viterbi path on the grid, and of both after
               track(refine=True); and, for the refinement alone, the annotated key of every window centre as the labels
               (metrics.window_truth), where every deviation is the placement's own
  columns    : annotated key changes, median distance to the nearest predicted boundary in seconds, share within 1 s
  --time     : ake_key_changes_f32 on a 10-minute recording (3001 frames of 288 bins, 118 windows of 76 frames, 25 apart, slack 25; every
               pair of windows a boundary, random log-CQT), R = 1 and R = 256: the launch under the library's kernel timer and the
               package call between device events, warm, medians of --reps

Sine mixes say nothing about real music: the table compares placements on audio whose key changes are known, and no more.
    python3 tools/refine_accuracy.py [--epochs 10] [--time] [--reps 50]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import ake_amd  # noqa: E402
from ake_amd import metrics, synthetic  # noqa: E402
from track_accuracy import train_net  # noqa: E402

SR, DEV = 22050, "cuda:0"


def fmt(score):
    return f"{score['count']} | {score['median_abs_seconds']:.2f} | {score['within_tolerance']:.3f}"


def accuracy(est, method, audio, ann):
    rows = []
    for smooth in (False, True):
        track = est.track(audio, method=method, smooth=smooth, refine=True)
        name = "Viterbi path" if smooth else "raw `key_id`"
        rows.append((f"{method}: {name}, grid", track.boundary_score(ann, refined=False)))
        rows.append((f"{method}: {name}, refined", track.boundary_score(ann, refined=True)))
    return rows


def truth_rows(est, audio, ann):
    """The annotated key at every window centre as the labels: a KeyTrack whose key_id is the truth, refined by hand."""
    track = est.track(audio, method="profile")
    W = track.key_id.shape[1]
    track.key_id, _ = metrics.window_truth(ann.seg_start, ann.seg_key, ann.seg_count, W, track.hop, track.window_frames, track.stride_frames,
                                           track.counts)
    grid = track.boundary_score(ann)
    track.change_frame, track.change_gain, track.change_contrast = ake_amd.key_changes(est.plan.logmag(audio), track.key_id, track.window_frames,
                                                                                       track.stride_frames, window_counts=track.counts)
    track.refined_source = "key_id"
    return [("annotated labels, grid", grid), ("annotated labels, refined", track.boundary_score(ann, refined=True))]


def timing(reps):
    wf, sf, T, P = 76, 25, 3001, 288
    W = (T - wf) // sf + 1
    lines = ["| R | boundaries | `key_changes_kernel` (us) | `ake_amd.key_changes` call (us) |", "|---|---|---|---|"]
    for R in (1, 256):
        mel = torch.rand((R, P, T), device=DEV) * 3.0
        labels = ((torch.arange(W, device=DEV)[None, :] * 7 + torch.arange(R, device=DEV)[:, None]) % 24).to(torch.int32)
        call = lambda: ake_amd.key_changes(mel, labels, wf, sf)      # noqa: E731
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        kernel = []
        ake_amd._lib.prof_enable("key_changes_kernel", True)
        for _ in range(reps):
            call()
            kernel.append(ake_amd._lib.prof_results()["key_changes_kernel"][0])
        ake_amd._lib.prof_enable("", False)
        lines.append(f"| {R} | {R * (W - 1)} | {1e3 * statistics.median(kernel):.1f} | {1e3 * statistics.median(ms):.1f} |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--clips", type=int, default=604)
    ap.add_argument("--recordings", type=int, default=24)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--time", action="store_true", help="also time the launch at R = 1 and R = 256")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    audio, ann = synthetic.make_modulating_batch_device(range(args.recordings), 60.0 * args.minutes, DEV)
    bare = ake_amd.KeyEstimator(None, SR, 5, device=DEV, pitches=288)
    rows = truth_rows(bare, audio, ann) + accuracy(bare, "profile", audio, ann)
    print(f"Device: {torch.cuda.get_device_name(0)}.  {args.recordings} recordings of {args.minutes:g} min, 15 s windows 5 s apart, slack 5 s.")
    if args.epochs > 0:
        net, info = train_net(args.epochs, args.clips)
        print(f"Net: default PitchClassNet, {info['epochs']} epochs on {info['clips']} stationary synthetic clips (validation MIREX "
              f"{info['val_mirex']}, accuracy {info['val_accuracy']}).")
        rows += accuracy(ake_amd.KeyEstimator(net, SR, 5), "net", audio, ann)
    print("\n| labels and placement | annotated changes | median distance (s) | within 1 s |\n|---|---|---|---|")
    for name, score in rows:
        print(f"| {name} | {fmt(score)} |")
    if args.time:
        print()
        print("\n".join(timing(args.reps)))


if __name__ == "__main__":
    main()
