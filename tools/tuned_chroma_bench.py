#!/usr/bin/env python3
"""Tuned chroma: the profile method on detuned recordings with and without retuning the audio -> profiles/tuned_chroma.md.

Modulating recordings (synthetic.make_modulating_batch_device) are played off pitch with ake_amd.retune, one detuning per recording,
and their annotations moved onto the detuned recordings' clock.  Three routes of KeyEstimator.track(method="profile", smooth=True):
  tuning=None                         : the uniform chroma of the detuned audio
  tuning="auto"                       : estimate, retune the audio, transform again (the route there was before tuned_chroma)
  tuning="auto", tuned_chroma=True    : estimate, then cut the chroma of the one transform by the cents

  timing    : device events on the stream around warm calls (median [min, max] ms), and every route's launch set with the mean time
              per kernel from the library's kernel timer
  accuracy  : KeyTrack.score (MIREX-weighted, smoothed and raw) of the three routes, and how many windows the two tuned routes label alike

    python3 tools/tuned_chroma_bench.py [--recordings 8] [--seconds 300] [--reps 20] [--markdown profiles/tuned_chroma.md]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SR, DEV = 22050, "cuda:0"
ROUTES = (("tuning=None", dict()), ('tuning="auto"', dict(tuning="auto")), ('tuning="auto", tuned_chroma=True', dict(tuning="auto", tuned_chroma=True)))


def timed(fn, reps, warmup=3):
    import torch
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
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def kernel_set(fn, reps):
    """{kernel: [launches per call, mean ms per launch]} from the library's kernel timer."""
    import ake_amd
    ake_amd._lib.prof_enable("", True)
    try:
        for _ in range(reps):
            fn()
        return {k: [v[1] // reps, round(v[0] / v[1], 4)] for k, v in sorted(ake_amd._lib.prof_results().items())}
    finally:
        ake_amd._lib.prof_enable("", False)


def row_of(score):
    return {"weighted": round(score.weighted()[1], 4), "weighted_pure": round(score.weighted(pure=True)[1], 4),
            "changes_ratio": round(score.flicker()[1], 3)}


def model_errors():
    """ake_profile_emissions_tuned_f32 against metrics.profile_emissions(cents=...) on the shapes of tests/test_gpu_tuned_chroma.py:
    uniform [0, 3] log-CQTs of 36 and 288 bins, 1 .. 129 frames, both layouts, four window geometries over the three compressions,
    a grid of cents that holds 0, +-50, NaN and 80 -> the worst |difference| of emissions / sharpness, confidence and chroma, and the
    number of cells whose key differs."""
    import torch
    import ake_amd
    from ake_amd import metrics
    cents_of = (0.0, 50.0, -50.0, 16.6, -33.4, float("nan"), 80.0)
    worst, cells, other = {"emissions": 0.0, "confidence": 0.0, "chroma": 0.0}, 0, 0
    for P in (36, 288):
        for T in (1, 63, 64, 65, 129):
            mel = torch.rand((8, P, T), generator=torch.Generator().manual_seed(5000 + 7 * T + P)) * 3.0
            for wf, sf, profiles, compression, sharpness in ((1, 1, "krumhansl", "log", 10.0), (5, 2, "temperley", "power", 30.0),
                                                             (76, 1, "temperley", "magnitude", 3.0), (0, 1, "krumhansl", "magnitude", 10.0)):
                if wf > T:
                    continue
                W = 1 if wf == 0 else (T - wf) // sf + 1
                grid = torch.tensor([[cents_of[(r + 3 * w) % len(cents_of)] for w in range(W)] for r in range(8)])
                table = metrics.key_profile_table(profiles).to(torch.float32).to(torch.float64)
                want = metrics.profile_emissions(mel, wf, sf, None, table, compression, sharpness, cents=grid)
                for fm in (False, True):
                    x = (mel.transpose(1, 2) if fm else mel).contiguous().to(DEV)
                    got = ake_amd.profile_emissions(x, wf, sf, frames_major=fm, profiles=profiles, compression=compression, sharpness=sharpness,
                                                    cents=grid)
                    for name, i, scale in (("chroma", 0, 1.0), ("emissions", 1, sharpness), ("confidence", 3, 1.0)):
                        worst[name] = max(worst[name], float((got[i].cpu().double() - want[i]).abs().max()) / scale)
                    cells += want[2].numel()
                    other += int((got[2].cpu() != want[2]).sum())
    return {"worst": worst, "cells": cells, "other_key": other}


def run(args):
    import torch
    import ake_amd
    from ake_amd import metrics, synthetic
    est = ake_amd.KeyEstimator(None, SR, 5, device=DEV)
    R = args.recordings
    clean, ann = synthetic.make_modulating_batch_device(range(R), float(args.seconds), DEV)
    detune = torch.linspace(-45.0, 45.0, R, device=DEV) if R > 1 else torch.tensor([30.0], device=DEV)
    audio, lengths = ake_amd.retune(clean.contiguous(), -detune)                         # undoing -c plays the recording c cents off
    audio = audio.contiguous()
    own = dataclasses.replace(ann, seg_start=metrics.scale_boundaries(ann.seg_start, -detune))    # boundaries on the detuned clock
    kw = dict(method="profile", smooth=True)
    out = {"device": torch.cuda.get_device_name(0), "recordings": R, "seconds": args.seconds, "samples": int(audio.shape[1]),
           "detune": [round(float(c), 1) for c in detune.cpu()], "routes": {}}
    tracks = {}
    for name, extra in ROUTES:
        call = lambda: est.track(audio, lengths, **kw, **extra)
        tracks[name] = call()
        out["routes"][name] = {"ms": timed(call, args.reps), "kernels": kernel_set(call, args.reps),
                               "smoothed": row_of(tracks[name].score(own, smoothed=True)), "raw": row_of(tracks[name].score(own, smoothed=False))}
    a, b = tracks[ROUTES[1][0]], tracks[ROUTES[2][0]]
    out["estimate_error"] = [round(float(v), 3) for v in (b.tuning_cents - detune).abs().cpu()]
    # the retuned route's windows lie on the retuned clock and differ in number; compare the two in the middle of every tuned window
    t_retuned = b.times.to(DEV)[None, :] * metrics.tuning_ratio(a.tuning_cents).reshape(-1, 1)       # seconds on the retuned clock
    idx = ((t_retuned - a.times[0].item()) / (a.times[1].item() - a.times[0].item())).round().long().clamp(0, a.key_id.shape[1] - 1)
    live = (torch.arange(b.key_id.shape[1], device=DEV)[None, :] < b.counts[:, None]) & (idx < a.counts[:, None])
    same = (torch.gather(a.smooth_key_id, 1, idx) == b.smooth_key_id) & live
    out["same_label_share"] = round(float(same.sum()) / max(int(live.sum()), 1), 4)
    out["model_errors"] = model_errors()
    return out


def report(res):
    r = res["routes"]
    f = lambda v: f"{v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]"
    old, new = r[ROUTES[1][0]], r[ROUTES[2][0]]
    md = ["# Tuned chroma: the profile method on detuned recordings without retuning them", "",
          "What was built: `profile_fold_kernel` / `profile_tuned_score_kernel` (`ake_profile_emissions_tuned_f32`), `ake_amd.profile_emissions(cents=...)`,",
          "`tuned_chroma=True` on `KeyEstimator.track(method=\"profile\")` and `profile_key`.  Tool: `tools/tuned_chroma_bench.py`; host model:",
          "`metrics.profile_emissions(cents=...)`.", "",
          f"## Timing and accuracy ({res['device']})", "",
          f"{res['recordings']} modulating recordings of {res['seconds']} s, played {res['detune']} cents off with `ake_amd.retune` ({res['samples']} samples per row);",
          "`track(method=\"profile\", smooth=True)`, 15 s windows 5 s apart; device events around warm calls, median [min, max] ms; MIREX-weighted",
          "`KeyTrack.score` against the annotations on the detuned recordings' clock.  Sine mixes say nothing about real music: the table compares",
          "code paths, no more.", "",
          "| route | call (ms) | smoothed score | raw score | changes per true change |", "|---|---|---|---|---|"]
    for name, _ in ROUTES:
        md.append(f"| `{name}` | {f(r[name]['ms'])} | {r[name]['smoothed']['weighted']:.4f} | {r[name]['raw']['weighted']:.4f} | {r[name]['smoothed']['changes_ratio']:.3f} |")
    md += ["", f"The tuned chroma takes {new['ms'][0] / old['ms'][0]:.3f} of the retuning route's time ({old['ms'][0] / new['ms'][0]:.2f} times as fast).  "
           f"Estimate error of the one transform: {res['estimate_error']} cents.  The two tuned routes give the same smoothed label in "
           f"{res['same_label_share']:.4f} of the windows (each tuned-chroma window against the retuned route's window nearest its centre).", "",
           "Launch sets (launches per call, mean ms per launch, the library's kernel timer):", ""]
    for name, _ in ROUTES:
        md += [f"- `{name}`: " + ", ".join(f"{k} x{v[0]} ({v[1]:.4f})" for k, v in r[name]["kernels"].items())]
    e = res["model_errors"]
    md += ["", "## Errors against the float64 model", "",
           f"`ake_profile_emissions_tuned_f32` against `metrics.profile_emissions(cents=...)`, {e['cells']} cells (36 and 288 bins; 1, 63, 64, 65 and 129",
           "frames; both layouts; windows (1, 1), (5, 2), (76, 1) and the whole clip; the three compressions; a grid of cents that holds 0, +-50, 16.6,",
           f"-33.4, NaN and 80): worst |emissions| / sharpness {e['worst']['emissions']:.2e}, |confidence| {e['worst']['confidence']:.2e}, |chroma| "
           f"{e['worst']['chroma']:.2e}; {e['other_key']} cells with another key.  `tests/test_gpu_tuned_chroma.py` holds all three to 2^-22 = 2.4e-07, the bound",
           "of the uniform chroma's tests: both sides are double chains rounded once to float32.", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tuned_chroma_bench needs the GPU"
    res = run(args)
    torch.cuda.synchronize()
    if args.json:
        json.dump(res, open(args.json, "w"), indent=1)
    md = report(res)
    print(md)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(md)


if __name__ == "__main__":
    main()
