#!/usr/bin/env python3
"""Key tracks without a net: the key-profile method scored beside the net's tracker, its errors against the float64 model, and its
timings -> profiles/key_profiles.md.

  errors   : ake_profile_emissions_f32 against metrics.profile_emissions on the shapes of tests/test_gpu_profiles.py (36 and 288 bins;
             1, 63, 64, 65 and 129 frames; both layouts; windows of 1 / 5 / 76 frames and the whole clip; the three compressions; full
             and ragged counts), largest |emissions| / sharpness, |confidence| and |chroma| differences beside the tests' bound of 2^-22
  scores   : track_accuracy.py's modulating recordings, 24 x 5 min (indices 0..23) at 15 / 5 / 1 s strides, KeyTrack.score of the raw
             key_id and of the Viterbi path at mean_key_seconds 60: Krumhansl, Temperley, profiles fitted on recordings 24..95
             (KeyEstimator.fit_key_profiles), sharpness 3 / 10 / 30, the three compressions; the net's rows are copied from
             profiles/track_accuracy.md
  timings  : tuning_bench.py's protocol (device events around warm calls, medians) on 8 x 5 min: the two launches against the same
             arithmetic in float64 torch ops on the device, and the whole track(method="profile") against track() with the net

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time ends the run, and
the report says "Not measured" for every step without a result (--json keeps results between runs).
     python3 tools/profile_baseline.py [--markdown profiles/key_profiles.md]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SR, DEV, HOP = 22050, "cuda:0", 4410
STEPS = (("errors", 300), ("scores", 420), ("timings", 300))               # name, time limit in seconds
STRIDES = (15.0, 5.0, 1.0)
# profiles/track_accuracy.md: the net's raw key_id and Viterbi (mean_key_seconds 60) rows, (weighted over all windows, predicted / true changes)
NET_ROWS = {15.0: {"raw": (0.5919, 1.082), "viterbi": (0.6815, 0.705)}, 5.0: {"raw": (0.5959, 1.438), "viterbi": (0.7061, 0.801)},
            1.0: {"raw": (0.5972, 1.986), "viterbi": (0.6792, 0.925)}}
# the figures of the issue that asked for this method: exact keys on the stationary clips 0..47, float64 model on the oracle CQT
HOST_TABLE = {"krumhansl": {"log": 0.5208, "magnitude": 0.4792, "power": 0.4583}, "fitted": {"log": 0.6667, "magnitude": 0.5833, "power": 0.3750}}


# ---- step: errors ----

def step_errors(args):
    import torch
    import ake_amd
    from ake_amd import metrics
    user = torch.rand((2, 12), generator=torch.Generator().manual_seed(41), dtype=torch.float64) + 0.2
    configs = [(1, 1, "krumhansl", "log", 10.0), (5, 5, "temperley", "magnitude", 3.0), (5, 1, user, "power", 30.0),
               (76, 5, "krumhansl", "log", 10.0), (76, 1, "temperley", "power", 10.0), (0, 1, "krumhansl", "magnitude", 10.0)]
    worst = {"emissions": 0.0, "confidence": 0.0, "chroma": 0.0}
    cases = windows = keys_differ = 0
    for P in (36, 288):
        for T in (1, 63, 64, 65, 129):
            g = torch.Generator().manual_seed(1000 + 7 * T + P)
            mel = torch.rand((3, P, T), generator=g) * 3.0
            for wf, sf, profiles, compression, sharpness in configs:
                if wf > T:
                    continue
                table = metrics.key_profile_table(profiles).float()              # the model reads what the kernel reads
                for counts in (None, [T, max(wf - 1, 0), 0] if wf else [T, T // 2, 0]):
                    want = metrics.profile_emissions(mel, wf, sf, counts, table.double(), compression, sharpness)
                    for fm in (False, True):
                        x = (mel.transpose(1, 2) if fm else mel).contiguous().to(DEV)
                        c, e, k, f = ake_amd.profile_emissions(x, wf, sf, counts, frames_major=fm, profiles=table, compression=compression,
                                                               sharpness=sharpness)
                        worst["chroma"] = max(worst["chroma"], float((c.cpu().double() - want[0]).abs().max()))
                        worst["emissions"] = max(worst["emissions"], float((e.cpu().double() - want[1]).abs().max()) / sharpness)
                        worst["confidence"] = max(worst["confidence"], float((f.cpu().double() - want[3]).abs().max()))
                        keys_differ += int((k.cpu() != want[2]).sum())
                        cases, windows = cases + 1, windows + k.numel()
    return {"worst": worst, "cases": cases, "windows": windows, "keys_differ": keys_differ, "bound": 2.0 ** -22}


# ---- step: scores ----

def row_of(score):
    return {"weighted": round(score.weighted()[1], 4), "weighted_pure": round(score.weighted(pure=True)[1], 4),
            "undecoded": round(float(score.fractions()[1][5]), 4), "changes_ratio": round(score.flicker()[1], 3)}


def step_scores(args):
    import torch
    import ake_amd
    from ake_amd import synthetic
    est = ake_amd.KeyEstimator(None, SR, 5, device=DEV)
    R = args.recordings
    audio, ann = synthetic.make_modulating_batch_device(range(R), 300.0, DEV)
    fit_audio, fit_ann = synthetic.make_modulating_batch_device(range(R, 4 * R), 300.0, DEV)
    fitted = {c: est.fit_key_profiles(fit_audio, fit_ann, compression=c) for c in ("log", "magnitude")}
    del fit_audio
    variants = [("Krumhansl", dict(profiles="krumhansl")), ("Temperley", dict(profiles="temperley")),
                (f"fitted on recordings {R}..{4 * R - 1}", dict(profiles=fitted["log"])),
                ("Krumhansl, sharpness 3", dict(profile_sharpness=3.0)), ("Krumhansl, sharpness 30", dict(profile_sharpness=30.0)),
                ("Krumhansl, magnitude", dict(compression="magnitude")), ("Krumhansl, power", dict(compression="power")),
                ("fitted, magnitude", dict(profiles=fitted["magnitude"], compression="magnitude"))]
    tables = []
    for stride in STRIDES:
        rows = []
        for name, kw in variants:
            tr = est.track(audio, stride_seconds=stride, smooth=True, method="profile", **kw)
            rows.append((name, row_of(tr.score(ann, smoothed=False)), row_of(tr.score(ann, smoothed=True))))
        tables.append({"stride_s": stride, "windows_per_recording": int(tr.key.shape[1]), "rows": rows})
    torch.cuda.synchronize()
    return {"recordings": R, "fit_recordings": 3 * R, "tables": tables, "fitted_log": [[round(v, 4) for v in row] for row in fitted["log"].cpu().tolist()]}


# ---- step: timings ----

def profile_torch_ops(mel, wf, sf, table, sharpness):
    """metrics.profile_emissions' arithmetic ("log") in float64 torch ops on the device: index_add over the bins, unfold over the
    frames, one matrix product with the 24 centred rotations."""
    import torch
    R, P, T = mel.shape
    dev = mel.device
    pc = ((torch.arange(P, device=dev) + 1) // 3) % 12
    c = torch.zeros((R, 12, T), dtype=torch.float64, device=dev).index_add_(1, pc, mel.double())
    x = c.unfold(2, wf, sf).sum(dim=3).transpose(1, 2)                                        # (R, W, 12)
    d = x - x.mean(dim=2, keepdim=True)
    e = table - table.mean(dim=1, keepdim=True)
    j = torch.arange(12, device=dev)
    q = torch.stack([e[k // 12][(j - k % 12) % 12] for k in range(24)])                        # (24, 12)
    r = (d @ q.T) / torch.sqrt((d * d).sum(dim=2, keepdim=True) * (q * q).sum(dim=1)[None, None, :])
    return (x / x.sum(dim=2, keepdim=True)).float(), (sharpness * r).float(), r.argmax(dim=2).int(), r.max(dim=2).values.float()


def step_timings(args):
    import torch
    import ake_amd
    from ake_amd import metrics, synthetic
    from tuning_bench import default_net, timed
    est = ake_amd.KeyEstimator(default_net(), SR, 5)
    recs = synthetic.make_batch_device(range(160), torch.device(DEV))[0].reshape(8, -1).contiguous()      # 8 x 5 min
    mel = est.plan.logmag(recs)
    table = metrics.key_profile_table("krumhansl").to(DEV)
    out = {"device": torch.cuda.get_device_name(0), "frames": int(mel.shape[2]), "samples": int(recs.shape[1]), "strides": {}}
    for stride, sf in ((5.0, 25), (1.0, 5)):
        got = ake_amd.profile_emissions(mel, 76, sf)
        ops = profile_torch_ops(mel, 76, sf, table, 10.0)
        out["strides"][str(stride)] = {
            "windows": int(got[2].shape[1]),
            "launches_ms": timed(lambda: ake_amd.profile_emissions(mel, 76, sf), args.reps),
            "torch_ops_ms": timed(lambda: profile_torch_ops(mel, 76, sf, table, 10.0), args.reps),
            "emissions_max_abs_diff": float((got[1] - ops[1]).abs().max()), "keys_equal": bool(torch.equal(got[2], ops[2])),
            "cqt_ms": timed(lambda: est.plan.logmag(recs), args.reps),
            "track_profile_ms": timed(lambda: est.track(recs, stride_seconds=stride, method="profile"), args.reps),
            "track_net_ms": timed(lambda: est.track(recs, stride_seconds=stride), args.reps),
            "track_profile_smooth_ms": timed(lambda: est.track(recs, stride_seconds=stride, method="profile", smooth=True), args.reps),
            "track_net_smooth_ms": timed(lambda: est.track(recs, stride_seconds=stride, smooth=True), args.reps),
        }
    out["whole_clip_ms"] = timed(lambda: ake_amd.profile_emissions(mel, 0, 1), args.reps)
    return out


# ---- report ----

def report(res):
    md = ["# Key tracks without a net: key-profile emissions", "",
          "What was built: `profile_chroma_kernel` / `profile_score_kernel` (`ake_profile_emissions_f32`), `ake_amd.profile_emissions`,",
          "`ake_amd.fit_key_profiles`, and `KeyEstimator.track(method=\"profile\")`, `profile_key`, `fit_key_profiles`,",
          "`KeyEstimator(None, ...)`.  Tool: `tools/profile_baseline.py`; host model: `metrics.profile_emissions`.", "",
          "**Sine mixes say nothing about real music** (see `profiles/track_accuracy.md`): the tables compare this library's trackers with",
          "each other on audio whose key changes are known.  `sharpness = 10` and `compression = \"log\"` are starting values; no default is",
          "changed on the strength of these tables.", "",
          "## The float64 model on the stationary clips (no GPU)", "",
          "Share of clips whose key comes out exactly: `metrics.profile_emissions` on the oracle CQT (22 050 Hz, hop 4410) of",
          "`synthetic.make_batch` clips 0..47, one window of 76 frames each; \"fitted\" is `metrics.fit_key_profiles` on clips 48..143.",
          "Measured with `metrics.profile_emissions` itself; the figures of the scratch model that the method was proposed with (0.52 / 0.48 /",
          "0.46 and 0.67 / 0.58) are the same to two digits.  `tests/test_profiles_host.py` asserts fitted >= Krumhansl + 0.05 for `log`.", "",
          "| profiles | `log` | `magnitude` | `power` |", "|---|---|---|---|",
          "| Krumhansl-Kessler | {log:.4f} | {magnitude:.4f} | {power:.4f} |".format(**HOST_TABLE["krumhansl"]),
          "| fitted on clips 48..143 | {log:.4f} | {magnitude:.4f} | {power:.4f} |".format(**HOST_TABLE["fitted"]), ""]
    md += ["## Errors against the float64 model", ""]
    if "errors" in res:
        e = res["errors"]
        w = e["worst"]
        md += [f"{e['cases']} calls over the shapes of `tests/test_gpu_profiles.py` ({e['windows']} windows; the model reads the float32 log-CQT and the",
               "float32 profile table the kernel reads).  Both sides are double chains rounded once to float32.", "",
               "| output | largest difference | bound of the tests |", "|---|---|---|",
               f"| emissions / sharpness | {w['emissions']:.2e} | 2^-22 = {e['bound']:.2e} |", f"| confidence | {w['confidence']:.2e} | 2^-22 = {e['bound']:.2e} |",
               f"| chroma | {w['chroma']:.2e} | 2^-22 = {e['bound']:.2e} |", "", f"`key_id` differs from the model's in {e['keys_differ']} windows.", ""]
    else:
        md += ["Not measured.", ""]
    md += ["## Scores on the modulating recordings", ""]
    if "scores" in res:
        s = res["scores"]
        md += [f"{s['recordings']} modulating recordings of 5 min (indices 0..{s['recordings'] - 1}), 15 s windows, `KeyTrack.score`: the MIREX-weighted score over all",
               "windows and the track's key changes per key change of the truth, for the raw `key_id` and for the Viterbi path at",
               f"`mean_key_seconds = 60`.  Fitted profiles: `KeyEstimator.fit_key_profiles` on recordings {s['recordings']}..{s['recordings'] + s['fit_recordings'] - 1} (15 s windows, 5 s stride).",
               "The net's rows are copied from `profiles/track_accuracy.md` (a net trained on stationary clips of the same kind).", ""]
        for t in s["tables"]:
            net = NET_ROWS.get(float(t["stride_s"]))
            md += [f"### stride {t['stride_s']:g} s ({t['windows_per_recording']} windows per recording)", "",
                   "| emissions | raw: weighted | raw: changes | Viterbi 60: weighted | Viterbi 60: changes | raw: silent or undecoded |", "|---|---|---|---|---|---|"]
            if net:
                md += [f"| the net (`profiles/track_accuracy.md`) | {net['raw'][0]:.4f} | {net['raw'][1]:.3f} | {net['viterbi'][0]:.4f} | {net['viterbi'][1]:.3f} | |"]
            md += [f"| {name} | {raw['weighted']:.4f} | {raw['changes_ratio']:.3f} | {vit['weighted']:.4f} | {vit['changes_ratio']:.3f} | {raw['undecoded']:.4f} |"
                   for name, raw, vit in t["rows"]]
            md += [""]
        md += ["The fitted `log` profiles (rows minor, major; tonic first): `" + json.dumps(s["fitted_log"]) + "`", ""]
    else:
        md += ["Not measured.", ""]
    if "timings" in res:
        t = res["timings"]
        f = lambda v: f"{v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]"
        md += [f"## Timings (median [min, max] ms, device events around warm calls; {t['device']})", "",
               f"8 recordings of 5 min ({t['frames']} frames, {t['samples']} samples per row), 15 s windows.", ""]
        for stride, r in t["strides"].items():
            md += [f"### stride {float(stride):g} s ({r['windows']} windows per recording)", "",
                   f"- the two launches on the log-CQT: {f(r['launches_ms'])}; the same arithmetic in float64 torch ops on the device: {f(r['torch_ops_ms'])} "
                   f"(largest emission difference of the two {r['emissions_max_abs_diff']:.2e}, keys equal: {r['keys_equal']})",
                   f"- the transform alone: {f(r['cqt_ms'])}",
                   f"- the whole call: `track(method=\"profile\")` {f(r['track_profile_ms'])}, `track()` with the net {f(r['track_net_ms'])}; with `smooth=True`: "
                   f"{f(r['track_profile_smooth_ms'])} and {f(r['track_net_smooth_ms'])}", ""]
        md += [f"The whole-clip mode on the same log-CQT (one window of {t['frames']} frames per recording): {f(t['whole_clip_ms'])}.", ""]
    else:
        md += ["## Timings", "", "Not measured.", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--steps", nargs="+", default=[s for s, _ in STEPS])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--recordings", type=int, default=24)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--json", default=None, help="keep the steps' results here, and start from what it already holds")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "profile_baseline needs the GPU"
        res = {"errors": step_errors, "scores": step_scores, "timings": step_timings}[args.step](args)
        torch.cuda.synchronize()
        print("RESULT " + json.dumps(res))
        return
    res = {}
    if args.json and os.path.exists(args.json):
        res = json.load(open(args.json))
    for name, limit in STEPS:
        if name not in args.steps:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--recordings", str(args.recordings)]
        try:
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {limit} s; stopping here", file=sys.stderr)
            break
        lines = [l for l in child.stdout.splitlines() if l.startswith("RESULT ")]
        if child.returncode != 0 or not lines:
            print(f"step {name} failed ({child.returncode}); stopping here\n{child.stderr[-3000:]}", file=sys.stderr)
            break
        res[name] = json.loads(lines[-1][7:])
        print(f"step {name}: done", file=sys.stderr)
        if args.json:
            json.dump(res, open(args.json, "w"))
    md = report(res)
    print(md)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write(md)
    sys.exit(0 if all(s in res for s in args.steps) else 1)


if __name__ == "__main__":
    main()
