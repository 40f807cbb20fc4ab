#!/usr/bin/env python3
"""Tuning estimate and retuner: errors against the float64 models, timings, and what retuning does to key tracks of detuned
recordings -> profiles/tuning.md.

  errors    : ake_tuning_estimate_f32 and ake_retune_f32 against metrics.estimate_tuning / metrics.retune_reference on the shapes of
              tests/test_gpu_tuning.py (worst figures: the tests' tolerances are four times these), the retuner's design error, and the
              end-to-end distances of three detuned 15 s clips to their in-tune originals with and without tuning="auto"
  timings   : the two launches (estimate on the batch's log-CQT, retune on its audio) at 256 x 15 s and at 8 x 5 min, device events
              around warm calls, medians; the same arithmetic in torch ops on the device; KeyEstimator.__call__ / track with
              tuning=None, a given tensor of cents, and "auto"; the data-sheet floor of the retuner (bytes moved / 6.29 TB/s)
  accuracy  : KeyTrack.score (smoothed path) on 24 modulating recordings of 5 min whose partials are scaled by 2^(c / 1200),
              c = -45 .. 45, with tuning=None and tuning="auto", on a net trained as tools/track_accuracy.py trains its own

  follow    : the tuning track and the curve retuner (tuning="follow") -> profiles/tuning_follow.md holds its figures: the drift table
              (ramp, sine, constant) on the device, and the new launches' times at 256 x 15 s and 8 x 10 min beside retune_kernel's

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time ends the run,
and the report says "Not measured" for every step without a result (--json keeps results between runs).     python3 tools/tuning_bench.py [--markdown profiles/tuning.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SR, DEV, HOP = 22050, "cuda:0", 4410
STEPS = (("errors", 300), ("timings", 420), ("accuracy", 900), ("follow", 420))             # name, time limit in seconds
DETUNINGS = (-45.0, -30.0, -15.0, 0.0, 15.0, 30.0, 45.0)


def timed(fn, reps, warmup=2):
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


def default_net():
    import numpy as np
    import torch
    from argparse import Namespace
    import ake_amd
    gold = np.load(os.path.join(REPO, "tests", "golden", "pcnet_default.npz"))
    net = ake_amd.PitchClassNet(288, 12, 2, 7, Namespace(genre=True))
    net.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd/")}, strict=True)
    return net.to(DEV).eval()


# ---- step: errors ----

def harmonic_clip(seed, cents, n, sr=SR):
    """tests/test_tuning_host.py's clip: 8 to 10 sustained notes of 5 partials, every frequency scaled by 2 ** (cents / 1200)."""
    import numpy as np
    rng = np.random.default_rng(9000 + seed)
    notes = int(rng.integers(8, 11))
    midi = rng.integers(40, 85, size=notes)
    phase = rng.uniform(0.0, 2 * np.pi, size=(notes, 5))
    t = np.arange(n, dtype=np.float64) / sr
    y, total = np.zeros(n), 0.0
    for i in range(notes):
        f0 = 440.0 * 2.0 ** ((midi[i] - 69) / 12.0) * 2.0 ** (cents / 1200.0)
        for h in range(1, 6):
            y += np.sin(2 * np.pi * f0 * h * t + phase[i, h - 1]) / h
            total += 1.0 / h
    return y / (0.5 * total)


def end_to_end_distances():
    """tests/test_gpu_tuning.py's three ragged detuned clips on the seeded weights: largest output difference to the in-tune originals
    (the same notes at rho times the length), every arm in a buffer of the retuned batch's width."""
    import numpy as np
    import torch
    import ake_amd
    est = ake_amd.KeyEstimator(default_net(), SR, 5)
    N15 = 15 * SR
    truth, lens = (-38.0, 22.0, 47.0), (N15, N15 - 30011, N15 - 77777)
    width = ake_amd.retune_out_len(N15)
    wide = np.zeros((3, width), dtype=np.float32)
    for i, (c, n) in enumerate(zip(truth, lens)):
        wide[i, :n] = harmonic_clip(20 + i, c, n)
    lengths = torch.tensor(lens, device=DEV)
    audio = torch.from_numpy(wide).to(DEV)
    cents, strength = est.estimate_tuning(audio[:, :N15], lengths)
    n_out = ake_amd.retune(audio[:, :N15], cents, lengths)[1].cpu().tolist()
    original = np.zeros((3, width), dtype=np.float32)
    for i, n in enumerate(n_out):
        original[i, :n] = harmonic_clip(20 + i, 0.0, n)
    got, plain = est(audio[:, :N15], lengths, tuning="auto"), est(audio, lengths)
    ref = est(torch.from_numpy(original).to(DEV), torch.tensor(n_out, device=DEV))
    return {"truth": list(truth), "estimates": [round(float(c), 3) for c in cents.cpu()], "strength": [round(float(v), 3) for v in strength.cpu()],
            "heads": {name: {"compensated": float((a - r).abs().max()), "uncompensated": float((p - r).abs().max())}
                      for name, a, p, r in zip(("key", "tonic", "genre"), got, plain, ref)}}


def step_errors(args):
    import numpy as np
    import torch
    import ake_amd
    from ake_amd import metrics
    out = {"estimate": [], "retune": [], "design": []}
    for P, T in ((288, 1), (288, 7), (288, 76), (288, 65), (288, 1501), (36, 76)):
        g = torch.Generator().manual_seed(100 + T + P)
        mel = torch.rand((3, P, T), generator=g) * 3.0
        for counts in (None, [T, (T + 1) // 2, 0]):
            wc, wst = metrics.estimate_tuning(mel, counts)
            for fm in (False, True):
                x = (mel.transpose(1, 2) if fm else mel).contiguous().to(DEV)
                c, s = ake_amd.estimate_tuning(x, counts, frames_major=fm)
                out["estimate"].append({"bins": P, "frames": T, "ragged": counts is not None, "frames_major": fm,
                                        "cents": float((c.cpu().double() - wc).abs().max()), "strength": float((s.cpu().double() - wst).abs().max())})
    plan = ake_amd.get_plan(SR, HOP, 288, 36, DEV)                                        # a real log-CQT: three detuned harmonic clips
    real = plan.logmag(torch.from_numpy(np.stack([harmonic_clip(10 + i, c, 15 * SR) for i, c in enumerate((-38.0, 22.0, 47.0))]).astype(np.float32)).to(DEV))
    wc, wst = metrics.estimate_tuning(real.cpu())
    for fm in (False, True):
        c, s = ake_amd.estimate_tuning((real.transpose(1, 2) if fm else real).contiguous(), frames_major=fm)
        out["estimate"].append({"bins": 288, "frames": int(real.shape[2]), "ragged": False, "frames_major": fm, "real": True,
                                "cents": float((c.cpu().double() - wc).abs().max()), "strength": float((s.cpu().double() - wst).abs().max())})
    G = np.abs(metrics.retune_table().astype(np.float64))
    Z, R = metrics.RETUNE_ZEROS, metrics.RETUNE_RESOLUTION
    sum_h = float(max(sum(G[r + m * R] for m in range(Z)) + sum(G[m * R - r] for m in range(1, Z + 1)) for r in range(R + 1)))
    cases = [((0, 1, 63), (33.3, 50.0, -50.0)), ((64, 65, 1), (-17.3, 50.0, -50.0)), ((2047, 2049, 2048), (50.0, -50.0, 33.3)),
             ((16383, 16385, 16384), (-17.3, 33.3, 0.0)), ((49211, 30011, 16385), (50.0, -50.0, 0.0)), ((777, 20000, 4099), (0.0, -17.3, 33.3))]
    for i, (lengths, cents) in enumerate(cases):
        g = torch.Generator().manual_seed(700 + i)
        x = torch.rand((3, max(lengths)), generator=g) * 2.0 - 1.0
        want, want_n = metrics.retune_reference(x.double().numpy(), np.array(cents, dtype=np.float32), lengths)
        y, n_out = ake_amd.retune(x.to(DEV), torch.tensor(cents), torch.tensor(lengths))
        got = y.cpu().double().numpy()
        err = max(float(np.abs(got[b, :int(want_n[b])] - want[b, :int(want_n[b])]).max(initial=0.0)) for b in range(3)) / sum_h
        out["retune"].append({"lengths": list(lengths), "cents": list(cents), "lengths_equal": n_out.cpu().tolist() == want_n.tolist(), "e": err})
    for f in (100.0, 3000.0, 8200.0):
        for c in (-49.0, 37.0):
            rho = 2.0 ** (c / 1200.0)
            x = np.sin(2 * np.pi * f * rho * np.arange(20000) / SR + 0.3)
            ideal = lambda n: np.sin(2 * np.pi * f * np.arange(n) / SR + 0.3)
            ym, nm = metrics.retune_reference(x, c)
            yd, nd = ake_amd.retune(torch.from_numpy(x.astype(np.float32))[None].to(DEV), c)
            nd = int(nd[0])
            out["design"].append({"hz": f, "cents": c, "model": float(np.abs(ym[:nm] - ideal(nm))[200:nm - 200].max()),
                                  "device": float(np.abs(yd[0, :nd].cpu().double().numpy() - ideal(nd))[200:nd - 200].max())})
    out["sum_abs_h"] = sum_h
    out["end_to_end"] = end_to_end_distances()
    return out


# ---- step: timings ----

def estimate_torch_ops(mel):
    import torch
    p = torch.expm1(mel.double()) ** 2
    P0, P1, P2 = (p[:, j::3].sum(dim=(1, 2)) for j in range(3))
    re, im = P0 - 0.5 * (P1 + P2), (3.0 ** 0.5 / 2.0) * (P1 - P2)
    return (100.0 * torch.atan2(im, re) / (2.0 * torch.pi)).float(), (torch.sqrt(re * re + im * im) / (P0 + P1 + P2)).float()


def retune_torch_ops(x, cents, table, rows=8):
    """metrics.retune_reference's arithmetic in float32 torch ops on the device, `rows` rows at a time (the index tensors are large)."""
    import torch
    from ake_amd import metrics
    Z, R = metrics.RETUNE_ZEROS, metrics.RETUNE_RESOLUTION
    B, n = x.shape
    width = metrics.retune_out_len(n)
    out = torch.zeros((B, width), device=x.device)
    xp = torch.nn.functional.pad(x, (Z, Z + 1))
    for b0 in range(0, B, rows):
        c = cents[b0:b0 + rows].double()
        rho = torch.exp2(c / 1200.0)[:, None]
        k = torch.arange(width, device=x.device, dtype=torch.float64)[None, :]
        pos = k / rho
        j0 = torch.floor(pos)
        fr = (pos - j0).float() * R
        r = fr.long().clamp(max=R - 1)
        t = fr - r.float()
        j0 = j0.long().clamp(max=n - 1)
        acc = torch.zeros_like(t)
        for m in range(-Z + 1, Z + 1):
            q = r - m * R if m <= 0 else m * R - r - 1
            lo, hi = table[q], table[q + 1]
            w = lo + t * (hi - lo) if m <= 0 else hi + t * (lo - hi)
            acc += xp[b0:b0 + rows].gather(1, j0 + (m + Z)) * w
        out[b0:b0 + rows] = torch.where(k < torch.floor(n * rho), acc, torch.zeros_like(acc))
    return out


def step_timings(args):
    import torch
    import ake_amd
    from ake_amd import metrics, synthetic
    est = ake_amd.KeyEstimator(default_net(), SR, 5)
    table = torch.from_numpy(metrics.retune_table()).to(DEV)
    clips = synthetic.make_batch_device(range(256), torch.device(DEV))[0]
    recs = clips[:160].reshape(8, -1).contiguous()                                       # 8 x 5 min
    out = {"device": torch.cuda.get_device_name(0)}
    for name, audio, run in (("256 x 15 s", clips, lambda a, **kw: est(a, **kw)), ("8 x 5 min", recs, lambda a, **kw: est.track(a, **kw))):
        B, n = audio.shape
        g = torch.Generator(device=DEV).manual_seed(1)
        cents = (torch.rand(B, device=DEV, generator=g) * 90.0 - 45.0)
        mel = est.plan.logmag(audio)
        width = ake_amd.retune_out_len(n)
        moved = B * (n + width) * 4
        y_dev = ake_amd.retune(audio, cents)[0]
        y_ops = retune_torch_ops(audio, cents, table)
        out[name] = {
            "frames": int(mel.shape[2]), "samples": int(n),
            "estimate_ms": timed(lambda: ake_amd.estimate_tuning(mel), args.reps),
            "estimate_torch_ops_ms": timed(lambda: estimate_torch_ops(mel), 5),
            "retune_ms": timed(lambda: ake_amd.retune(audio, cents), args.reps),
            "retune_pcm16_ms": timed(lambda a=(audio * 32767).round().to(torch.int16): ake_amd.retune(a, cents), args.reps),
            "retune_torch_ops_ms": timed(lambda: retune_torch_ops(audio, cents, table), 3, warmup=1),
            "retune_vs_torch_ops_max_abs": float((y_dev - y_ops).abs().max()),
            "retune_bytes": moved, "retune_floor_ms": round(moved / 6.29e12 * 1e3, 4),
            "cqt_ms": timed(lambda: est.plan.logmag(audio), args.reps),
            "call_plain_ms": timed(lambda: run(audio), args.reps),
            "call_given_ms": timed(lambda: run(audio, tuning=cents), args.reps),
            "call_auto_ms": timed(lambda: run(audio, tuning="auto"), args.reps),
        }
    return out


# ---- step: accuracy ----

def step_accuracy(args):
    import numpy as np
    import torch
    import ake_amd
    from ake_amd import synthetic
    from track_accuracy import row_of, train_net
    net, training = train_net(args.epochs, 604)
    est = ake_amd.KeyEstimator(net, SR, 5)
    R = args.recordings
    arrays, segments = synthetic.modulating_batch_arrays(range(R), 300.0)
    ann = ake_amd.KeyAnnotations.from_segments([[(s / SR, k) for s, k in segs] for segs in segments], SR, DEV)
    rows = []
    for c in DETUNINGS:
        audio = ake_amd.synth_partials(device=DEV, **dict(arrays, cps=arrays["cps"] * 2.0 ** (c / 1200.0)))
        plain = est.track(audio, stride_seconds=5.0, smooth=True)
        auto = est.track(audio, stride_seconds=5.0, smooth=True, tuning="auto")
        e = auto.tuning_cents.cpu().double() - c
        rows.append({"cents": c, "none": row_of(plain.score(ann)), "auto": row_of(auto.score(ann)),
                     "estimate_error": [round(float(e.abs().mean()), 3), round(float(e.abs().max()), 3)],
                     "strength_mean": round(float(auto.tuning_strength.mean()), 3)})
    return {"training": training, "recordings": R, "rows": rows}


# ---- step: follow ----

def drifting_clip(seed, cents_fn, seconds):
    """tests/test_tuning_follow_host.py's clip: harmonic_clip's notes, every frequency times 2 ** (c(t) / 1200), the phase the running sum."""
    import numpy as np
    n = seconds * SR
    rng = np.random.default_rng(9000 + seed)
    notes = int(rng.integers(8, 11))
    midi = rng.integers(40, 85, size=notes)
    phase = rng.uniform(0.0, 2 * np.pi, size=(notes, 5))
    scale = 2.0 ** (cents_fn(np.arange(n, dtype=np.float64) / SR) / 1200.0)
    warped = (np.cumsum(scale) - scale[0]) / SR
    y, total = np.zeros(n), 0.0
    for i in range(notes):
        f0 = 440.0 * 2.0 ** ((midi[i] - 69) / 12.0)
        for h in range(1, 6):
            y += np.sin(2 * np.pi * f0 * h * warped + phase[i, h - 1]) / h
            total += 1.0 / h
    return y / (0.5 * total)


def step_follow(args):
    import numpy as np
    import torch
    import ake_amd
    from ake_amd import synthetic
    est = ake_amd.KeyEstimator(None, SR, 5, device=DEV)
    wf, sf = 25, 5
    first, step = (wf - 1) // 2 * HOP, sf * HOP
    drifts = (("ramp -35 .. +35", lambda t: -35.0 + 70.0 * t / 40.0), ("25 sin(2 pi t / 30 s) + 5", lambda t: 25.0 * np.sin(2 * np.pi * t / 30.0) + 5.0),
              ("constant +20", lambda t: np.full_like(t, 20.0)))
    audio = torch.from_numpy(np.stack([drifting_clip(i, fn, 40) for i, (_, fn) in enumerate(drifts)]).astype(np.float32)).to(DEV)
    whole_c, whole_s = est.estimate_tuning(audio)
    raw, strength, curve, n_win = est.tuning_track(audio)
    centres = (np.arange(raw.shape[1]) * sf + (wf - 1) / 2) * HOP / SR
    followed, len_f = ake_amd.retune_curve(audio, curve, first, step)
    one, len_o = ake_amd.retune(audio, whole_c)
    left_f = est.tuning_track(followed, len_f)
    left_o = est.tuning_track(one, len_o)
    after_c, after_s = est.estimate_tuning(followed, len_f)
    table = []
    for i, (name, fn) in enumerate(drifts):
        live = lambda t, i=i: t[0][i, :int(t[3][i])].abs().max()
        table.append({"drift": name, "whole": [round(float(whole_c[i]), 2), round(float(whole_s[i]), 2)],
                      "window_error": round(float(np.abs(raw[i].cpu().double().numpy() - fn(centres)).max()), 2),
                      "left_one_number": round(float(live(left_o)), 2), "left_follow": round(float(live(left_f)), 2),
                      "strength_after": round(float(after_s[i]), 2)})
    out = {"device": torch.cuda.get_device_name(0), "table": table}
    clips = synthetic.make_batch_device(range(256), torch.device(DEV))[0]
    recs = torch.cat([clips[:160].reshape(8, -1)] * 2, dim=1).contiguous()                # 8 x 10 min
    for name, x in (("256 x 15 s", clips), ("8 x 10 min", recs)):
        B, n = x.shape
        mel = est.plan.logmag(x)
        cv = ake_amd.tuning_track(mel, wf, sf)[2]
        g = torch.Generator(device=DEV).manual_seed(1)
        cv = (torch.rand(cv.shape, device=DEV, generator=g) * 90.0 - 45.0)
        cents = cv[:, 0].contiguous()
        idx = torch.arange(0, n, 1000, device=DEV)[None].expand(B, -1).contiguous()
        ake_amd._lib.prof_enable("", True)
        for _ in range(args.reps):
            ake_amd.tuning_track(mel, wf, sf); ake_amd.retune_curve(x, cv, first, step); ake_amd.retune(x, cents)
            ake_amd.retune_curve_positions(idx, cv, first, step)
        kernels = {k: round(v[0] / v[1], 4) for k, v in ake_amd._lib.prof_results().items()}
        ake_amd._lib.prof_enable("", False)
        out[name] = {"frames": int(mel.shape[2]), "samples": int(n), "knots": int(cv.shape[1]), "kernel_mean_ms": kernels,
                     "tuning_track_ms": timed(lambda: ake_amd.tuning_track(mel, wf, sf), args.reps),
                     "estimate_ms": timed(lambda: ake_amd.estimate_tuning(mel), args.reps),
                     "retune_curve_ms": timed(lambda: ake_amd.retune_curve(x, cv, first, step), args.reps),
                     "retune_ms": timed(lambda: ake_amd.retune(x, cents), args.reps),
                     "positions_ms": timed(lambda: ake_amd.retune_curve_positions(idx, cv, first, step), args.reps)}
    return out


# ---- report ----

def report(res):
    md = ["# Tuning estimate and retuner", "",
          "What was built: `tuning_sums_kernel` / `tuning_finish_kernel` (`ake_tuning_estimate_f32`), `retune_kernel<float>` / `<short>`",
          "(`ake_retune_f32`, `ake_retune_pcm16_f32`), `ake_amd.estimate_tuning` / `ake_amd.retune`, and `tuning=` on `KeyEstimator.__call__`",
          "and `track`.  Tool: `tools/tuning_bench.py`; host models: `metrics.estimate_tuning`, `metrics.retune_reference`.", ""]
    if "errors" in res:
        e = res["errors"]
        wc, wst = max(r["cents"] for r in e["estimate"]), max(r["strength"] for r in e["estimate"])
        we = max(r["e"] for r in e["retune"])
        md += ["## Errors against the float64 models", "",
               f"- estimate, {len(e['estimate'])} cases (288 and 36 bins; 1, 7, 76, 65 and 1501 frames; both layouts; full and ragged counts; uniform [0, 3], and the device log-CQT of three detuned 15 s harmonic clips): "
               f"worst |cents| {wc:.2e}, worst |strength| {wst:.2e}.  The sums run in double: this is the float32 rounding of the two outputs.",
               f"- retune, {len(e['retune'])} ragged batches of 3 rows (lengths 0 .. 49211, cents -50 .. 50): worst e = {we:.2e} of sum|h| max|x| "
               f"(sum|h| = {e['sum_abs_h']:.4f}, so {we * e['sum_abs_h']:.2e} of max|x|); lengths equal to the model's in "
               f"{sum(r['lengths_equal'] for r in e['retune'])} of {len(e['retune'])}.",
               "- `tests/test_gpu_tuning.py` uses four times these figures.", "",
               "Design error, a sine at f rho against the ideal sine at f (200 samples from the ends; limit 1e-4):", "",
               "| f | cents | float64 model | device |", "|---|---|---|---|"]
        md += [f"| {r['hz']:.0f} Hz | {r['cents']:+.0f} | {r['model']:.2e} | {r['device']:.2e} |" for r in e["design"]]
        ee = e["end_to_end"]
        md += ["", f"End to end, three ragged 15 s harmonic clips detuned by {ee['truth']} cents on the seeded weights (estimates {ee['estimates']}, strength "
               f"{ee['strength']}): largest output difference to the in-tune originals (the same notes at rho times the length), every arm in a "
               "buffer of the retuned batch's width (78 frames):", "", "| head | tuning=\"auto\" | tuning=None |", "|---|---|---|"]
        md += [f"| {name} | {h['compensated']:.3e} | {h['uncompensated']:.3e} |" for name, h in ee["heads"].items()]
        md += [""]
    else:
        md += ["## Errors against the float64 models", "", "Not measured.", ""]
    if "timings" in res:
        t = res["timings"]
        md += [f"## Timings (median [min, max] ms, device events around warm calls; {t['device']})", ""]
        for name in ("256 x 15 s", "8 x 5 min"):
            r = t[name]
            f = lambda k: f"{r[k][0]:.4f} [{r[k][1]:.4f}, {r[k][2]:.4f}]"
            md += [f"### {name} ({r['frames']} frames, {r['samples']} samples per row)", "",
                   f"- estimate (two launches): {f('estimate_ms')}; the same sums in torch ops (float64): {f('estimate_torch_ops_ms')}",
                   f"- retune (one launch): float32 {f('retune_ms')}, int16 {f('retune_pcm16_ms')}; the same taps in float32 torch ops: {f('retune_torch_ops_ms')} "
                   f"(largest difference of the two {r['retune_vs_torch_ops_max_abs']:.2e}); data-sheet floor {r['retune_floor_ms']:.4f} ms for "
                   f"{r['retune_bytes'] / 1e9:.3f} GB at 6.29 TB/s",
                   f"- the transform alone: {f('cqt_ms')}",
                   f"- the whole call: tuning=None {f('call_plain_ms')}, a given tensor of cents {f('call_given_ms')}, \"auto\" {f('call_auto_ms')}", ""]
    else:
        md += ["## Timings", "", "Not measured.", ""]
    if "accuracy" in res:
        a = res["accuracy"]
        tr = a["training"]
        md += ["## Key tracks of detuned recordings", "",
               f"Net: default PitchClassNet, {tr['epochs']} epochs on {tr['clips']} stationary synthetic clips (validation MIREX {tr['val_mirex']}).  "
               f"{a['recordings']} modulating recordings of 5 min, every partial scaled by 2^(c / 1200); 15 s windows, 5 s stride, the smoothed path; "
               "MIREX-weighted score over all windows.  Sine mixes say nothing about real music: the table compares the two code paths, no more.", "",
               "| c (cents) | tuning=None | tuning=\"auto\" | estimate error, mean / max (cents) | mean strength |", "|---|---|---|---|---|"]
        md += [f"| {r['cents']:+.0f} | {r['none']['weighted']:.4f} | {r['auto']['weighted']:.4f} | {r['estimate_error'][0]:.3f} / {r['estimate_error'][1]:.3f} | "
               f"{r['strength_mean']:.3f} |" for r in a["rows"]]
        md += [""]
    else:
        md += ["## Key tracks of detuned recordings", "", "Not measured.", ""]
    if "follow" in res:
        md += ["## A tuning that drifts (profiles/tuning_follow.md)", "", "```json", json.dumps(res["follow"], indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--steps", nargs="+", default=[s for s, _ in STEPS])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--recordings", type=int, default=24)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--json", default=None, help="keep the steps' results here, and start from what it already holds")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "tuning_bench needs the GPU"
        res = {"errors": step_errors, "timings": step_timings, "accuracy": step_accuracy, "follow": step_follow}[args.step](args)
        torch.cuda.synchronize()
        print("RESULT " + json.dumps(res))
        return
    res = {}
    if args.json and os.path.exists(args.json):
        res = json.load(open(args.json))
    for name, limit in STEPS:
        if name not in args.steps:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--epochs", str(args.epochs),
               "--recordings", str(args.recordings)]
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
