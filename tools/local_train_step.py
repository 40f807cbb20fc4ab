"""One --local training step (forward, general_step, backward, Adam) at B = 8 clips of T = 300 and of T = 1500 CQT frames, with
general_step's fused --local loss (ake_general_step_local_f32) and with its torch-op loop (fused_loss = False).  GPU box only.

  python tools/local_train_step.py --steps 50 --warmup 10
      host clock around each step ending in a device synchronise; median per shape and path -> one JSON line
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/local_train_step.py --markers --steps 5
      the same steps, each timed window between two torch.cuda._sleep marker launches (spin_kernel)
  python tools/local_train_step.py --count DIR
      kernel launches per step of each shape and path, counted between the markers of DIR's kernel trace -> one JSON line
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((8, 300), (8, 1500))
PATHS = ("fused", "loop")
SPAN = 50                      # loc_window_size * frames


def make_step(B, T, fused, seed=0):
    import torch
    import torch.nn.functional as F
    from argparse import Namespace
    import ake_amd
    dev = torch.device("cuda", 0)
    opt = Namespace(local=True, genre=False, frames=5, loc_window_size=10, lr=3e-4, gamma=0.96, acc_grad=1)
    torch.manual_seed(seed)
    net = ake_amd.PitchClassNet(288, 12, 2, 7, opt).to(dev).train()
    net.fused_loss = fused
    net.trainer = ake_amd.Trainer()
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(T - T // 4, T + 1, (B,), generator=g)
    seq[0] = T
    kid = torch.randint(0, 24, (B,), generator=g)
    rows = lambda t: t[:, None].expand(B, T, t.shape[1]).clone()
    batch = {"mel": (torch.rand((B, 1, 288, T), generator=g) * 2.5).to(dev), "seq_length": seq,      # seq_length on the host, as a DataLoader gives it
             "key_labels": rows(ake_amd.KEY_SIGNATURE_MAP[kid % 21]), "tonic_labels": rows(F.one_hot(kid % 12, 12).float()),
             "key_signature_id": rows(F.one_hot(kid, 24).float())}
    for i, s in enumerate(seq.tolist()):
        for k in ("key_labels", "tonic_labels", "key_signature_id"):
            batch[k][i, s - SPAN + 1:] = 0
    batch = {k: (v.to(dev) if k not in ("seq_length", "mel") else v) for k, v in batch.items()}
    optim = net.configure_optimizers()[0][0]

    def step(i):
        optim.zero_grad()
        out = net.training_step(batch, i)
        out["loss"].backward()
        optim.step()
        return out["loss"]
    return step


def timed(args):
    import torch
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "ms": {}}
    for B, T in SHAPES:
        for path in PATHS:
            step = make_step(B, T, path == "fused")
            for i in range(args.warmup):
                step(i)
            torch.cuda.synchronize()
            ms = []
            for i in range(args.steps):
                t0 = time.perf_counter()
                step(i)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0))
            res["ms"][f"{B}x{T}_{path}"] = round(statistics.median(ms), 4)
        res["ms"][f"{B}x{T}_loop_over_fused"] = round(res["ms"][f"{B}x{T}_loop"] / res["ms"][f"{B}x{T}_fused"], 3)
    print(json.dumps(res))


def markers(args):
    import torch
    for B, T in SHAPES:
        for path in PATHS:
            step = make_step(B, T, path == "fused")
            for i in range(args.warmup):
                step(i)
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)                  # marker: one spin_kernel launch before and after the timed steps
            for i in range(args.steps):
                step(i)
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
    print(json.dumps({"markers": [f"{B}x{T}_{p}" for B, T in SHAPES for p in PATHS], "steps": args.steps}))


def count(args):
    files = sorted(glob.glob(os.path.join(args.count, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {args.count}"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    is_marker = ["spin_kernel" in r["Kernel_Name"] for r in rows]
    idx = [i for i, m in enumerate(is_marker) if m]
    names = [f"{B}x{T}_{p}" for B, T in SHAPES for p in PATHS]
    assert len(idx) == 2 * len(names), f"{len(idx)} marker launches, expected {2 * len(names)}"
    out = {"steps": args.steps, "launches_per_step": {}, "loss_kernels_per_step": {}}
    for k, name in enumerate(names):
        window = rows[idx[2 * k] + 1:idx[2 * k + 1]]
        out["launches_per_step"][name] = round(len(window) / args.steps, 2)
        out["loss_kernels_per_step"][name] = {
            "general_step_local": sum("general_step_local" in r["Kernel_Name"] for r in window) / args.steps}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--markers", action="store_true")
    ap.add_argument("--count", metavar="DIR")
    a = ap.parse_args()
    if a.count:
        count(a)
    elif a.markers:
        markers(a)
    else:
        timed(a)
