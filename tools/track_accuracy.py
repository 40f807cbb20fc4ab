#!/usr/bin/env python3
"""Key tracks scored against ground truth on synthesised modulating recordings -> a markdown report (profiles/track_accuracy.md).

  net        : the default PitchClassNet trained on the stationary synthetic clips with the config-3 settings (tools/config3_train.py's route:
               604 + 96 clips of 15 s, batch 8, accumulate 8, Adam 3e-4, ExponentialLR 0.96, --genre), --epochs epochs
  recordings : synthetic.make_modulating_batch_device -- indices 0..23 of 5 min are scored, indices 24..47 are what transitions are fitted on
  tracks     : 15 s windows at strides of 15 / 5 / 1 s; per stride one row for the raw key_id, for the Viterbi path at mean_key_seconds of
               15 / 30 / 60 / 120, under the EM-fitted transition (ake_amd.fit_key_transition on the fit set's emissions) and under the
               transition counted from the fit set's labels (metrics.transition_from_labels)
  columns    : MIREX-weighted score over all windows and over pure windows, share of undecoded windows, predicted / true key changes
  timings    : the additive-synthesiser kernel for 8 x 5 min against the same recipe in torch ops on the device (float64 phase, one
               partial at a time, torch.randn noise), and KeyTrack.score against metrics.track_score on the device's tensors; device events
               around warm calls, medians

Sine mixes say nothing about real music: the table compares this library's decoders with each other on audio whose key changes are
known, and no more.     python3 tools/track_accuracy.py [--epochs 10] [--markdown report.md]
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
from ake_amd import metrics, synthetic  # noqa: E402

SR, DEV = 22050, "cuda:0"


def train_net(epochs, clips):
    """tools/config3_train.py's route, without its per-epoch printing."""
    opt = Namespace(conv_layers=3, n_filters=4, head_layers=2, time_pool_size=2, genre=True, max_pool=False, frames=5, octaves=8, lr=3e-4,
                    gamma=0.96, acc_grad=8, reg=0, key_weight=1.0, tonic_weight=1.0, genre_weight=0.1, use_cos=False, no_ckpt=True, local=False,
                    only_semitones=False, multi_scale=False)
    train = ake_amd.KeyDataset(True, opt)
    train.import_data(ake_amd.SyntheticSineMixLoader(clips), shuffle=True)
    val = ake_amd.KeyDataset(True, opt)
    val.import_data(ake_amd.SyntheticSineMixLoader(96, first=10_000), shuffle=False)
    torch.manual_seed(0)
    net = ake_amd.PitchClassNet(288, 12, 2, 7, opt, batch_size=8, train_set=train, val_set=val).cuda()
    trainer = ake_amd.Trainer(max_epochs=epochs, accumulate_grad_batches=opt.acc_grad)
    trainer.fit(net)
    res = trainer.val_results[-1]
    return net.eval(), {"epochs": epochs, "clips": clips, "val_mirex": round(float(res["val_mirex_score"]), 4), "val_accuracy": round(float(res["val_accuracy"]), 4)}


def timed(fn, reps, warmup=2):
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


def synth_torch_ops(arrays, device):
    """The recipe of ake_synth_partials_f32 in torch ops on the device, in the style of synthetic.make_batch_device: float64 phase, one
    partial at a time over the samples it sounds on, torch.randn noise (another stream than the kernel's), peak normalisation."""
    R, n_max = len(arrays["n"]), int(arrays["n"].max())
    out = torch.zeros((R, n_max), device=device, dtype=torch.float32)
    fade = int(arrays["fade"])
    gen = torch.Generator(device=device)
    for r in range(R):
        nr = int(arrays["n"][r])
        y = torch.zeros(nr, device=device, dtype=torch.float32)
        for p in range(int(arrays["offsets"][r]), int(arrays["offsets"][r + 1])):
            s, e = int(arrays["start"][p]), int(arrays["end"][p])
            a, b = max(s, 0), min(e, nr)
            if a >= b:
                continue
            t = torch.arange(a, b, device=device, dtype=torch.float64)
            turns = float(arrays["cps"][p]) * t + float(arrays["phase"][p])
            v = float(arrays["amp"][p]) * torch.sin(2 * np.pi * (turns - torch.floor(turns))).float()
            if fade > 0:
                k, m = t - s, (e - 1) - t
                v = v * torch.where(k < fade, 0.5 - 0.5 * torch.cos(np.pi * (k + 0.5) / fade), torch.ones_like(k)).float()
                v = v * torch.where(m < fade, 0.5 - 0.5 * torch.cos(np.pi * (m + 0.5) / fade), torch.ones_like(m)).float()
            y[a:b] += v
        gen.manual_seed(int(arrays["seed"][r]) & 0x7FFFFFFF)
        y += torch.randn(nr, device=device, generator=gen) * float(arrays["noise_sigma"])
        mx = y.abs().max()
        out[r, :nr] = torch.where(mx > 0, y * (float(arrays["peak"]) / mx), y)
    return out


def row_of(score):
    frac = score.fractions()[1]
    return {"weighted": round(score.weighted()[1], 4), "weighted_pure": round(score.weighted(pure=True)[1], 4),
            "undecoded": round(float(frac[5]), 4), "changes_ratio": round(score.flicker()[1], 3),
            "windows": int(score.tally[:, 0].sum()), "pure_windows": int(score.tally[:, 1].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--clips", type=int, default=604)
    ap.add_argument("--recordings", type=int, default=24)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--strides", type=float, nargs="+", default=[15.0, 5.0, 1.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--markdown", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_accuracy needs the GPU"
    t0 = time.perf_counter()
    net, training = train_net(args.epochs, args.clips)
    training["seconds"] = round(time.perf_counter() - t0, 1)
    est = ake_amd.KeyEstimator(net, SR, 5)
    R, seconds = args.recordings, 60.0 * args.minutes
    audio, ann = synthetic.make_modulating_batch_device(range(R), seconds, DEV)
    fit_audio, fit_ann = synthetic.make_modulating_batch_device(range(R, 2 * R), seconds, DEV)
    segments = int(ann.seg_count.sum())

    tables = []
    for stride in args.strides:
        fit_track = est.track(fit_audio, stride_seconds=stride, smooth=True)
        A_em, lls = ake_amd.fit_key_transition(fit_track, iterations=10)
        fit_score = fit_track.score(fit_ann, smoothed=False)
        A_lab = metrics.transition_from_labels(fit_score.truth, fit_track.counts)
        rows = []
        tr = est.track(audio, stride_seconds=stride, smooth=True)
        rows.append(("raw key_id", row_of(tr.score(ann, smoothed=False))))
        for mks in (15.0, 30.0, 60.0, 120.0):
            tr = est.track(audio, stride_seconds=stride, smooth=True, mean_key_seconds=mks)
            rows.append((f"Viterbi, mean_key_seconds {mks:g}" + (" (default)" if mks == 60.0 else ""), row_of(tr.score(ann))))
        for name, A in (("Viterbi, EM-fitted transition", A_em), ("Viterbi, label-fitted transition", A_lab)):
            tr = est.track(audio, stride_seconds=stride, smooth=True, transition=A)
            rows.append((name, row_of(tr.score(ann))))
        tables.append({"stride_s": stride, "windows_per_recording": int(tr.key.shape[1]),
                       "stay": {"default_60": round(float(np.exp(-tr.stride_seconds / 60.0)), 4), "em": round(float(torch.exp(A_em).diagonal().mean()), 4),
                                "labels": round(float(torch.exp(A_lab).diagonal().mean()), 4)},
                       "rows": rows})

    # ---- timings ----
    arrays, _ = synthetic.modulating_batch_arrays(range(8), seconds)
    dev_arrays = {k: (torch.as_tensor(v, device=DEV) if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}
    k_ms = timed(lambda: ake_amd.synth_partials(device=DEV, **dev_arrays), args.reps)
    t_ms = timed(lambda: synth_torch_ops(arrays, DEV), 3, warmup=1)
    quiet = dict(arrays, noise_sigma=0.0)
    diff = float((ake_amd.synth_partials(device=DEV, **quiet) - synth_torch_ops(quiet, DEV)).abs().max())
    tr1 = est.track(audio, stride_seconds=1.0, smooth=True)
    s_ms = timed(lambda: tr1.score(ann), args.reps * 5, warmup=5)
    args_host = (tr1.smooth_key_id, tr1.counts, ann.seg_start, ann.seg_key, ann.seg_count, tr1.hop, tr1.window_frames, tr1.stride_frames)
    h_ms = timed(lambda: metrics.track_score(*args_host), args.reps, warmup=3)
    same = all(torch.equal(a, b) for a, b in zip(metrics.track_score(*args_host),
                                                 (lambda s: (s.truth, s.category, s.tally, s.changes))(tr1.score(ann))))
    torch.cuda.synchronize()

    timings = {"synth_kernel_ms": [round(x, 3) for x in k_ms], "synth_torch_ops_ms": [round(x, 1) for x in t_ms],
               "synth_samples": int(arrays["n"].sum()), "synth_partials": int(len(arrays["cps"])), "synth_max_abs_diff_without_noise": diff,
               "score_kernel_ms": [round(x, 4) for x in s_ms], "score_torch_ops_ms": [round(x, 3) for x in h_ms],
               "score_windows": int(tr1.key.shape[0] * tr1.key.shape[1]), "score_equal": bool(same)}
    result = {"device": torch.cuda.get_device_name(0), "training": training, "recordings": R, "minutes": args.minutes, "segments": segments,
              "tables": tables, "timings": timings}
    print(json.dumps(result))

    md = [f"Device: {result['device']}.  Net: default PitchClassNet, {training['epochs']} epochs on {training['clips']} stationary synthetic clips "
          f"(validation MIREX {training['val_mirex']}, accuracy {training['val_accuracy']}; {training['seconds']} s with the dataset).",
          f"Scored: {R} modulating recordings of {args.minutes:g} min (indices 0..{R - 1}, {segments} segments in all); transitions fitted on "
          f"indices {R}..{2 * R - 1}.  Windows of 15 s.", ""]
    for t in tables:
        md += [f"### stride {t['stride_s']:g} s ({t['windows_per_recording']} windows per recording; stay probability: default "
               f"{t['stay']['default_60']}, EM-fitted {t['stay']['em']}, label-fitted {t['stay']['labels']})", "",
               "| track | weighted, all windows | weighted, pure windows | undecoded | predicted / true changes |", "|---|---|---|---|---|"]
        md += [f"| {name} | {r['weighted']:.4f} | {r['weighted_pure']:.4f} | {r['undecoded']:.4f} | {r['changes_ratio']:.3f} |" for name, r in t["rows"]]
        md += [f"", f"({t['rows'][0][1]['windows']} scored windows, {t['rows'][0][1]['pure_windows']} of them pure.)", ""]
    md += ["### timings (median [min, max] ms, device events around warm calls)", "",
           f"- synthesiser, 8 x {args.minutes:g} min ({timings['synth_samples']} samples, {timings['synth_partials']} partials): kernel route "
           f"{k_ms[0]:.3f} [{k_ms[1]:.3f}, {k_ms[2]:.3f}] ms over {args.reps} calls; torch ops {t_ms[0]:.1f} [{t_ms[1]:.1f}, {t_ms[2]:.1f}] ms over 3 calls "
           f"({t_ms[0] / k_ms[0]:.0f}x); largest difference of the two without noise {diff:.2e}",
           f"- score, {R} recordings at a 1 s stride ({timings['score_windows']} windows): `KeyTrack.score` {s_ms[0]:.4f} [{s_ms[1]:.4f}, {s_ms[2]:.4f}] ms over "
           f"{args.reps * 5} calls; `metrics.track_score` on the same device tensors {h_ms[0]:.3f} [{h_ms[1]:.3f}, {h_ms[2]:.3f}] ms over {args.reps} calls "
           f"({h_ms[0] / s_ms[0]:.0f}x); outputs equal: {same}", ""]
    print("\n".join(md))
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("\n".join(md))


if __name__ == "__main__":
    main()
