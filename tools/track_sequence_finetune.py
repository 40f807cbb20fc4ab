#!/usr/bin/env python3
"""Fine-tune the tracker's net for the smoothed track: sequences of consecutive windows with the sequence loss against random windows
-> a markdown report (profiles/track_sequence.md).

tools/track_finetune.py's protocol: the same base net, the same recordings (24..95 to train on, 0..23 held out), the same strides and
scoring.  From a copy of the base net each:

  windows   : random 15 s windows with purity weights, --ft-epochs epochs of --ft-batches batches of 8 (that tool's "purity" row)
  sequences : KeyEstimator.training_windows(sequence_windows=--sequence, stride_seconds=--sequence-stride): batches of
              8 / --sequence sequences, so a step sees as many windows; general_step adds --sequence-weight times the sequence loss
              (ake_key_sequence_loss_f32) under the transition track(smooth=True) uses at that stride

  timing    : one ake_amd.key_sequence_loss call on a batch's shape and on a track's, against metrics.key_sequence_loss on the same
              float32 device tensors (the same arithmetic as torch ops); device events around warm calls, medians
  launches  : the kernels of one call, counted by the library's own kernel timer

Sine mixes say nothing about real music: the tables compare this library's nets with each other on audio whose key changes are known,
and no more.     python3 tools/track_sequence_finetune.py [--epochs 10] [--markdown report.md]
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
from ake_amd import _lib, metrics, synthetic  # noqa: E402
from track_accuracy import timed, train_net  # noqa: E402
from track_finetune import score_rows, val_mirex  # noqa: E402

SR, DEV = 22050, "cuda:0"


def fine_tune(base, audio, ann, epochs, batches, lr, seed, sequence=None, stride=None, sequence_weight=1.0):
    net = copy.deepcopy(base).train()
    net.opt = argparse.Namespace(**{**vars(base.opt), "lr": lr, "sequence_weight": sequence_weight})
    est = ake_amd.KeyEstimator(net, SR, 5)
    if sequence is None:
        tw = est.training_windows(audio, ann, batch_size=8, batches_per_epoch=batches, seed=seed, weighting="purity")
    else:
        tw = est.training_windows(audio, ann, batch_size=max(1, 8 // sequence), batches_per_epoch=batches, seed=seed, weighting="purity",
                                  sequence_windows=sequence, stride_seconds=stride)
    trainer = ake_amd.Trainer(max_epochs=epochs, accumulate_grad_batches=1)
    trainer.fit(net, train_dataloaders=tw)
    k = max(1, len(trainer.train_losses) // 10)
    return net, {"first_losses": round(sum(trainer.train_losses[:k]) / k, 4), "last_losses": round(sum(trainer.train_losses[-k:]) / k, 4)}


def loss_inputs(R, W, seed):
    g = torch.Generator().manual_seed(seed)
    key = (torch.rand((R, W, 12), generator=g) * 0.98 + 0.01).to(DEV)
    tonic = (torch.randn((R, W, 12), generator=g) * 3.0).to(DEV)
    labels = torch.randint(-4, 24, (R, W), generator=g).to(device=DEV, dtype=torch.int32)
    return key, tonic, labels


def launches(fn):
    _lib.prof_results()
    _lib.prof_enable("", True)
    try:
        fn()
        torch.cuda.synchronize()
        res = _lib.prof_results()
    finally:
        _lib.prof_enable("", False)
    return {k: int(v[1]) for k, v in res.items()}


def stage(what):
    print(f"[track_sequence_finetune] {what}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--clips", type=int, default=604)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--ft-epochs", type=int, default=4)
    ap.add_argument("--ft-batches", type=int, default=180)
    ap.add_argument("--ft-lr", type=float, default=1e-4)
    ap.add_argument("--sequence", type=int, default=4)
    ap.add_argument("--sequence-stride", type=float, default=5.0)
    ap.add_argument("--sequence-weight", type=float, default=1.0)
    ap.add_argument("--strides", type=float, nargs="+", default=[15.0, 5.0, 1.0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--markdown", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_sequence_finetune needs the GPU"
    stage("training the base net")
    base, training = train_net(args.epochs, args.clips)
    seconds = 60.0 * args.minutes
    stage("synthesising the recordings and scoring the base net")
    held_audio, held_ann = synthetic.make_modulating_batch_device(range(24), seconds, DEV)
    ft_audio, ft_ann = synthetic.make_modulating_batch_device(range(24, 96), seconds, DEV)
    before = {"rows": score_rows(base, held_audio, held_ann, args.strides), "val_mirex": val_mirex(base)}
    after = {}
    for name, kw in (("windows", {}), ("sequences", {"sequence": args.sequence, "stride": args.sequence_stride, "sequence_weight": args.sequence_weight})):
        stage(f"fine-tuning on {name}")
        net, losses = fine_tune(base, ft_audio, ft_ann, args.ft_epochs, args.ft_batches, args.ft_lr, seed=0, **kw)
        after[name] = {"rows": score_rows(net, held_audio, held_ann, args.strides), "val_mirex": val_mirex(net), **losses}

    # ---- one loss call: the entry against the same arithmetic as float32 torch ops on the device ----
    stage("timing the loss call")
    A = metrics.key_transition_log(stay=0.92).float().to(DEV)
    timing, counted = {}, {}
    for R, W in ((max(1, 8 // args.sequence), args.sequence), (8, 57)):
        key, tonic, labels = loss_inputs(R, W, 10 * R + W)
        leaf = A.clone().requires_grad_()
        entry = lambda: ake_amd.key_sequence_loss(key, tonic, labels, leaf)                                   # noqa: E731
        torch_ops = lambda: metrics.key_sequence_loss(key, tonic, labels, A)                                  # noqa: E731
        a, b = float(entry().detach()), float(torch_ops()["loss"])
        timing[f"{R}x{W}"] = {"entry_ms": [round(x, 4) for x in timed(entry, args.reps, warmup=5)],
                              "torch_ms": [round(x, 3) for x in timed(torch_ops, max(5, args.reps // 5), warmup=2)], "loss": [a, b]}
        counted[f"{R}x{W}"] = {"with d_trans": launches(entry), "without": launches(lambda: ake_amd.key_sequence_loss(key, tonic, labels, A))}
    torch.cuda.synchronize()

    result = {"device": torch.cuda.get_device_name(0), "training": training,
              "fine_tuning": {"epochs": args.ft_epochs, "batches": args.ft_batches, "windows_per_batch": 8, "lr": args.ft_lr, "recordings": 72,
                              "minutes": args.minutes, "sequence_windows": args.sequence, "sequence_stride": args.sequence_stride,
                              "sequence_weight": args.sequence_weight},
              "before": before, "after": after, "loss_call": timing, "launches": counted}
    print(json.dumps(result))

    md = [f"Device: {result['device']}.  Base net: default PitchClassNet, {training['epochs']} epochs on {training['clips']} stationary synthetic clips "
          f"(validation MIREX {training['val_mirex']}).  Fine-tuned on modulating recordings 24..95 ({args.minutes:g} min each), {args.ft_epochs} epochs of "
          f"{args.ft_batches} batches of 8 windows, Adam at {args.ft_lr:g}, from the base net: once on random windows, once on sequences of "
          f"{args.sequence} windows {args.sequence_stride:g} s apart with {args.sequence_weight:g} x the sequence loss added.  Scored on recordings 0..23, "
          f"which no training saw.", "",
          "| net | validation MIREX, stationary clips | mean loss, first tenth of the steps | last tenth |", "|---|---|---|---|",
          f"| base | {before['val_mirex']:.4f} | | |"]
    md += [f"| fine-tuned, {w} | {after[w]['val_mirex']:.4f} | {after[w]['first_losses']:.4f} | {after[w]['last_losses']:.4f} |" for w in after]
    md += ["", "(the sequences' loss includes the sequence term, so the two rows' losses are not comparable with each other)", ""]
    for stride in args.strides:
        md += [f"### stride {stride:g} s ({before['rows'][stride]['raw']['windows']} scored windows, {before['rows'][stride]['raw']['pure_windows']} of them pure)", "",
               "| net | track | weighted, all windows | weighted, pure windows | undecoded | predicted / true changes |", "|---|---|---|---|---|---|"]
        for name, res in [("base", before)] + [(f"fine-tuned, {w}", after[w]) for w in after]:
            for track, label in (("raw", "raw key_id"), ("viterbi60", "Viterbi, mean_key_seconds 60")):
                r = res["rows"][stride][track]
                md += [f"| {name} | {label} | {r['weighted']:.4f} | {r['weighted_pure']:.4f} | {r['undecoded']:.4f} | {r['changes_ratio']:.3f} |"]
        md += [""]
    md += ["### one loss call (median [min, max] ms, device events around warm calls)", "",
           "| recordings x windows | `ake_amd.key_sequence_loss`, transition gradient included | the same formulas as float32 torch ops on the device | ratio |",
           "|---|---|---|---|"]
    for shape, t in timing.items():
        e, h = t["entry_ms"], t["torch_ms"]
        md += [f"| {shape} | {e[0]:.4f} [{e[1]:.4f}, {e[2]:.4f}] | {h[0]:.3f} [{h[1]:.3f}, {h[2]:.3f}] | {h[0] / e[0]:.0f}x |"]
    md += ["", "### launches of one call", ""]
    for shape, c in counted.items():
        for what, k in c.items():
            md += [f"- {shape}, {what}: {sum(k.values())} ({', '.join(f'{n} x {v}' for n, v in k.items())})"]
    md += [""]
    print("\n".join(md))
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("\n".join(md))


if __name__ == "__main__":
    main()
