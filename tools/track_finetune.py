#!/usr/bin/env python3
"""Fine-tune the tracker's net on windows of annotated modulating recordings, drawn on the device -> a markdown report
(profiles/track_finetune.md).

  base net   : tools/track_accuracy.py's route (the default PitchClassNet, config-3 settings, --epochs epochs on the stationary
               synthetic clips of 15 s)
  fine-tuning: KeyEstimator.training_windows on modulating recordings 24..95 (synthetic.make_modulating_batch_device, 5 min each;
               indices 0..23 stay held out), random windows of 15 s, --ft-epochs epochs of --ft-batches batches of 8, Adam at --ft-lr;
               once with weighting="purity" and once with weighting="uniform", each from a copy of the base net
  scored     : the 24 held-out recordings, 15 s windows at strides of 15 / 5 / 1 s: KeyTrack.score of the raw key_id and of the
               Viterbi path at mean_key_seconds = 60, before and after; and the validation MIREX on the stationary clips before and
               after, which shows what the fine-tuning forgot
  timing     : one batch assembly on the device (ake_draw_windows_i32 + ake_window_batch_f32, two launches) against the same batch
               built on the host: the starts read back, the windows sliced out of the transform one by one and stacked, the labels from
               KeyDataset.labels_for_signature; device events around warm calls, medians

Sine mixes say nothing about real music: the tables compare this library's nets with each other on audio whose key changes are known,
and no more.     python3 tools/track_finetune.py [--epochs 10] [--markdown report.md]
"""
import argparse
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import ake_amd  # noqa: E402
from ake_amd import metrics  # noqa: E402
from ake_amd.KeyDataset import labels_for_signature  # noqa: E402
from ake_amd import synthetic  # noqa: E402
from track_accuracy import row_of, timed, train_net  # noqa: E402

SR, DEV = 22050, "cuda:0"


def score_rows(net, audio, ann, strides):
    est = ake_amd.KeyEstimator(net.eval(), SR, 5)
    rows = {}
    for stride in strides:
        tr = est.track(audio, stride_seconds=stride, smooth=True, mean_key_seconds=60.0)
        rows[stride] = {"raw": row_of(tr.score(ann, smoothed=False)), "viterbi60": row_of(tr.score(ann))}
    return rows


def val_mirex(net):
    res = ake_amd.Trainer().validate(net)[0]
    return round(float(res["val_mirex_score"]), 4)


def fine_tune(base, audio, ann, weighting, epochs, batches, lr, seed):
    net = copy.deepcopy(base).train()
    net.opt = argparse.Namespace(**{**vars(base.opt), "lr": lr})
    tw = ake_amd.KeyEstimator(net, SR, 5).training_windows(audio, ann, batch_size=8, batches_per_epoch=batches, seed=seed, weighting=weighting)
    trainer = ake_amd.Trainer(max_epochs=epochs, accumulate_grad_batches=1)
    trainer.fit(net, train_dataloaders=tw)
    k = max(1, len(trainer.train_losses) // 10)
    return net, {"first_losses": round(sum(trainer.train_losses[:k]) / k, 4), "last_losses": round(sum(trainer.train_losses[-k:]) / k, 4)}


def host_batch(mel, recording, start, wf, hop, ann_host):
    """The batch of TrackWindows built the host's way: read the list back, slice every window out of the transform, look every label up."""
    rec, st = recording.tolist(), start.tolist()
    mels = torch.stack([mel[r, :, s:s + wf] for r, s in zip(rec, st)])[:, None]
    lab = metrics.window_labels(*ann_host, torch.tensor(rec), torch.tensor(st), hop, wf)
    keys, sigs, tonics = [], [], []
    for t in lab["truth"].tolist():
        k, s, _, tn = labels_for_signature(max(t, 0), None, True)
        z = 0.0 if t < 0 else 1.0
        keys.append(k * z); sigs.append(s * z); tonics.append(tn * z)
    return {"mel": mels, "key_labels": torch.stack(keys).to(DEV), "tonic_labels": torch.stack(tonics).to(DEV),
            "key_signature_id": torch.stack(sigs).to(DEV), "sample_weight": lab["sample_weight"].to(DEV)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--clips", type=int, default=604)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--ft-epochs", type=int, default=4)
    ap.add_argument("--ft-batches", type=int, default=180)
    ap.add_argument("--ft-lr", type=float, default=1e-4)
    ap.add_argument("--strides", type=float, nargs="+", default=[15.0, 5.0, 1.0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--markdown", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_finetune needs the GPU"
    base, training = train_net(args.epochs, args.clips)
    seconds = 60.0 * args.minutes
    held_audio, held_ann = synthetic.make_modulating_batch_device(range(24), seconds, DEV)
    ft_audio, ft_ann = synthetic.make_modulating_batch_device(range(24, 96), seconds, DEV)
    before = {"rows": score_rows(base, held_audio, held_ann, args.strides), "val_mirex": val_mirex(base)}
    after = {}
    for weighting in ("purity", "uniform"):
        net, losses = fine_tune(base, ft_audio, ft_ann, weighting, args.ft_epochs, args.ft_batches, args.ft_lr, seed=0)
        after[weighting] = {"rows": score_rows(net, held_audio, held_ann, args.strides), "val_mirex": val_mirex(net), **losses}

    # ---- one batch: the device route against the host's ----
    tw = ake_amd.KeyEstimator(base, SR, 5).training_windows(ft_audio, ft_ann, batch_size=8, batches_per_epoch=1, seed=0)
    ann_host = (ft_ann.seg_start.cpu(), ft_ann.seg_key.cpu(), ft_ann.seg_count.cpu())

    prefix = torch.tensor(metrics.window_prefix(tw.frames, tw.window_frames), dtype=torch.int64, device=DEV)

    def device_route():
        rec, st = ake_amd.draw_windows(prefix, 0, 0, 0, 8)
        return ake_amd.window_batch(tw.mel, rec, st, tw.window_frames, tw.hop, tw.annotations)

    def host_route():
        rec, st = ake_amd.draw_windows(prefix, 0, 0, 0, 8)
        return host_batch(tw.mel, rec, st, tw.window_frames, tw.hop, ann_host)

    a, b = device_route(), host_route()
    same = all(torch.equal(a[k], b[k]) for k in b)
    d_ms, h_ms = timed(device_route, args.reps, warmup=5), timed(host_route, args.reps, warmup=5)
    torch.cuda.synchronize()

    result = {"device": torch.cuda.get_device_name(0), "training": training, "fine_tuning": {"epochs": args.ft_epochs, "batches": args.ft_batches,
              "batch": 8, "lr": args.ft_lr, "recordings": 72, "minutes": args.minutes}, "before": before, "after": after,
              "batch_ms": {"device": [round(x, 4) for x in d_ms], "host": [round(x, 3) for x in h_ms], "equal": bool(same)}}
    print(json.dumps(result))

    md = [f"Device: {result['device']}.  Base net: default PitchClassNet, {training['epochs']} epochs on {training['clips']} stationary synthetic clips "
          f"(validation MIREX {training['val_mirex']}).  Fine-tuned on random 15 s windows of modulating recordings 24..95 ({args.minutes:g} min each): "
          f"{args.ft_epochs} epochs of {args.ft_batches} batches of 8, Adam at {args.ft_lr:g}, from the base net, once per weighting.  "
          f"Scored on recordings 0..23, which no training saw.", "",
          "| net | validation MIREX, stationary clips | mean loss, first tenth of the steps | last tenth |", "|---|---|---|---|",
          f"| base | {before['val_mirex']:.4f} | | |"]
    md += [f"| fine-tuned, weighting=\"{w}\" | {after[w]['val_mirex']:.4f} | {after[w]['first_losses']:.4f} | {after[w]['last_losses']:.4f} |" for w in after]
    md += [""]
    for stride in args.strides:
        md += [f"### stride {stride:g} s ({before['rows'][stride]['raw']['windows']} scored windows, {before['rows'][stride]['raw']['pure_windows']} of them pure)", "",
               "| net | track | weighted, all windows | weighted, pure windows | undecoded | predicted / true changes |", "|---|---|---|---|---|---|"]
        for name, res in [("base", before)] + [(f"fine-tuned, {w}", after[w]) for w in after]:
            for track, label in (("raw", "raw key_id"), ("viterbi60", "Viterbi, mean_key_seconds 60")):
                r = res["rows"][stride][track]
                md += [f"| {name} | {label} | {r['weighted']:.4f} | {r['weighted_pure']:.4f} | {r['undecoded']:.4f} | {r['changes_ratio']:.3f} |"]
        md += [""]
    md += ["### one batch of 8 windows (median [min, max] ms, device events around warm calls)", "",
           f"- on the device (`ake_draw_windows_i32` + `ake_window_batch_f32`, two launches): {d_ms[0]:.4f} [{d_ms[1]:.4f}, {d_ms[2]:.4f}] ms over {args.reps} calls",
           f"- the same list read back, the windows sliced and stacked, the labels from `labels_for_signature`: {h_ms[0]:.3f} [{h_ms[1]:.3f}, {h_ms[2]:.3f}] ms "
           f"over {args.reps} calls ({h_ms[0] / d_ms[0]:.0f}x); batches equal: {same}", ""]
    print("\n".join(md))
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("\n".join(md))


if __name__ == "__main__":
    main()
