"""Seeded synthetic "sine-mix" clips with key labels.

Stands in for the audio files + annotation files the reference's dataset loaders
read (KeyDataset.py:514-1233, out of scope): there is no dataset on the GPU box.
Labels follow the reference's encoding (KeyDataset.py:443-454): ``key_labels`` is
the 12-vector pitch-class set of the key signature, ``tonic_labels`` one-hot 12,
``key_signature_id`` one-hot 24 with 0..11 = C..B minor and 12..23 = C..B major
(``signature`` ordering, KeyDataset.py:524-527), ``genre`` one-hot 11.
"""
from __future__ import annotations

import numpy as np

SR = 22050
CLIP_SECONDS = 15
N_SAMPLES = SR * CLIP_SECONDS          # 330 750
_MAJOR = (0, 2, 4, 5, 7, 9, 11)
N_GENRES = 11
N_PARTIALS = 12


def key_pitch_classes(sig_id: int) -> np.ndarray:
    """Pitch-class set (12,) of key ``sig_id`` (natural minor shares its relative major's set)."""
    tonic = sig_id % 12
    major_tonic = tonic if sig_id >= 12 else (tonic + 3) % 12
    v = np.zeros(12, dtype=np.float32)
    for s in _MAJOR:
        v[(major_tonic + s) % 12] = 1.0
    return v


def clip_recipe(i: int):
    """Partials (freq, amp, phase) and labels of clip ``i``; seed = 1234 + i."""
    rng = np.random.default_rng(1234 + i)
    sig = i % 24
    tonic = sig % 12
    scale = np.flatnonzero(key_pitch_classes(sig))
    weights = np.where(scale == tonic, 3.0, 1.0)
    weights /= weights.sum()
    pcs = rng.choice(scale, size=N_PARTIALS, p=weights)
    octaves = rng.integers(2, 7, size=N_PARTIALS)
    midi = 12 * (octaves + 1) + pcs
    freq = 440.0 * 2.0 ** ((midi - 69) / 12.0)
    amp = rng.uniform(0.05, 0.25, size=N_PARTIALS)
    phase = rng.uniform(0.0, 2 * np.pi, size=N_PARTIALS)
    noise_seed = int(rng.integers(0, 2 ** 31 - 1))
    labels = {
        "key_labels": key_pitch_classes(sig),
        "tonic_labels": np.eye(12, dtype=np.float32)[tonic],
        "key_signature_id": np.eye(24, dtype=np.float32)[sig],
        "genre": np.eye(N_GENRES, dtype=np.float32)[i % N_GENRES],
    }
    return freq, amp, phase, noise_seed, labels


def make_clip(i: int, n_samples: int = N_SAMPLES, sr: int = SR):
    """float32 waveform (n_samples,) in [-0.9, 0.9] and the label dict of clip ``i``."""
    freq, amp, phase, noise_seed, labels = clip_recipe(i)
    n = np.arange(n_samples, dtype=np.float64)
    y = np.zeros(n_samples, dtype=np.float64)
    for f, a, p in zip(freq, amp, phase):
        y += a * np.sin(2 * np.pi * f * n / sr + p)
    y += np.random.default_rng(noise_seed).normal(0.0, 0.003, size=n_samples)
    y *= 0.9 / np.max(np.abs(y))
    return y.astype(np.float32), labels


def make_batch(indices, n_samples: int = N_SAMPLES, sr: int = SR):
    """Stack clips: waveforms (B, n) float32 + dict of stacked label arrays."""
    ys, labs = zip(*(make_clip(int(i), n_samples, sr) for i in indices))
    labels = {k: np.stack([l[k] for l in labs]) for k in labs[0]}
    return np.stack(ys), labels


def make_batch_device(indices, device, n_samples: int = N_SAMPLES, sr: int = SR):
    """Same recipe synthesised with torch on ``device`` (fast path for large benches).

    Partials are identical to :func:`make_clip`; the noise stream is torch's, so the
    waveforms agree with the numpy version only up to the noise floor (sigma 0.003).
    """
    import torch
    recipes = [clip_recipe(int(i)) for i in indices]
    f = torch.tensor(np.stack([r[0] for r in recipes]), device=device, dtype=torch.float64)
    a = torch.tensor(np.stack([r[1] for r in recipes]), device=device, dtype=torch.float32)
    p = torch.tensor(np.stack([r[2] for r in recipes]), device=device, dtype=torch.float64)
    out = torch.empty((len(recipes), n_samples), device=device, dtype=torch.float32)
    n = torch.arange(n_samples, device=device, dtype=torch.float64)
    gen = torch.Generator(device=device)
    for b in range(len(recipes)):
        arg = (2 * np.pi / sr) * f[b][:, None] * n[None, :] + p[b][:, None]
        y = (a[b][:, None] * torch.sin(arg).float()).sum(0)
        gen.manual_seed(recipes[b][3])
        y += torch.randn(n_samples, device=device, generator=gen) * 0.003
        out[b] = y * (0.9 / y.abs().max())
    labels = {k: np.stack([r[4][k] for r in recipes]) for k in recipes[0][4]}
    return out, labels


# ---- long recordings that modulate, with their ground truth: lists of enveloped partials for the additive synthesiser (ake_synth_partials_f32) ----

_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)
MODULATION_NOISE_SIGMA = 0.003
MODULATION_PEAK = 0.9
# P(next key | current key) of modulating_recipe: fifth up, fifth down, relative, parallel, any of the 19 other keys
MODULATION_MOVES = (0.3, 0.3, 0.2, 0.1, 0.1)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC 2011) in uint64 arithmetic: ``counter`` (..., 4) and ``key`` (..., 2) words -> (..., 4) uint32."""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(counter)[..., k].astype(np.uint64) & mask for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) & mask for k in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M[0]) * c[0], np.uint64(_PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(_PHILOX_W[0])) & mask, (k1 + np.uint64(_PHILOX_W[1])) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_uniform(x):
    """uint32 words -> float64 ``((x >> 9) + 0.5) * 2**-23``: odd multiples of 2**-24 strictly inside (0, 1), exact in float32 too."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def philox_normal(n, seed, recording):
    """(n,) float64 standard normals of row ``recording`` under ``seed``: block b = t >> 2 has counter (b low, b high, recording, 0) and
    key (seed low, seed high); Box-Muller on its four words gives the samples 4b .. 4b+3."""
    blocks = (int(n) + 3) // 4
    b = np.arange(blocks, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    counter = np.stack([b & np.uint64(0xFFFFFFFF), b >> np.uint64(32), np.full(blocks, recording, np.uint64), np.zeros(blocks, np.uint64)], axis=-1)
    u = philox_uniform(philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)))
    z = np.empty((blocks, 4), dtype=np.float64)
    for h in (0, 1):
        rad = np.sqrt(-2.0 * np.log(u[:, 2 * h]))
        z[:, 2 * h] = rad * np.cos(2 * np.pi * u[:, 2 * h + 1])
        z[:, 2 * h + 1] = rad * np.sin(2 * np.pi * u[:, 2 * h + 1])
    return z.reshape(-1)[:int(n)]


def fade_envelope(t, start, end, fade):
    """g_in * g_out of a partial sounding on [start, end) at the integer samples ``t`` (all inside it), float64: raised-cosine ramps of
    ``fade`` samples at both ends; a partial that ends at E and one that starts at E - fade sum to 1."""
    g = np.ones(len(t), dtype=np.float64)
    if fade > 0:
        k, m = t - start, end - 1 - t
        g = np.where(k < fade, 0.5 - 0.5 * np.cos(np.pi * (k + 0.5) / fade), g)
        g = g * np.where(m < fade, 0.5 - 0.5 * np.cos(np.pi * (m + 0.5) / fade), 1.0)
    return g


def synth_partials_reference(offsets, cps, phase, amp, start, end, fade, n, noise_sigma=0.0, seed=None, peak=0.0, n_max=None):
    """The float64 model of ``ake_synth_partials_f32`` (``ake_amd.synth_partials``), formula for formula -> (R, n_max) float64, zeros behind
    every row's ``n[r]``::

        y[t] = sum_p amp_p * g_in * g_out * sin(2 pi frac(cps_p * t + phase_p)) + noise_sigma * z_r[t]       start_p <= t < end_p

    with the envelopes of ``fade_envelope`` and the noise of ``philox_normal``; ``peak`` > 0 scales every row to max |y| = peak (an
    all-zero row stays zero)."""
    offsets, n = np.asarray(offsets, dtype=np.int64), np.asarray(n, dtype=np.int64).reshape(-1)
    R = len(n)
    n_max = int(n.max(initial=0)) if n_max is None else int(n_max)
    out = np.zeros((R, n_max), dtype=np.float64)
    for r in range(R):
        nr = int(n[r])
        y = out[r, :nr]
        for p in range(int(offsets[r]), int(offsets[r + 1])):
            a, b = max(int(start[p]), 0), min(int(end[p]), nr)
            if a >= b:
                continue
            t = np.arange(a, b, dtype=np.int64)
            turns = float(cps[p]) * t.astype(np.float64) + float(phase[p])          # (a product of a double and an integer below 2^53, then
            turns -= np.floor(turns)                                                # one rounding more than the kernel's fma: below 1e-9 turn)
            y[a:b] += float(amp[p]) * fade_envelope(t, int(start[p]), int(end[p]), int(fade)) * np.sin(2 * np.pi * turns)
        if noise_sigma != 0.0 and nr > 0:
            y += float(noise_sigma) * philox_normal(nr, int(seed[r]), r)
        if peak > 0.0 and nr > 0:
            mx = float(np.max(np.abs(y)))
            if mx > 0.0:
                y *= float(peak) / mx
    return out


def _related_keys(key):
    """(fifth up, fifth down, relative, parallel) of key ``key`` in the 24-way order (0-11 minor, 12-23 major, tonic = id mod 12)."""
    major, t = divmod(int(key), 12)
    relative = (t + 9) % 12 if major else 12 + (t + 3) % 12
    return 12 * major + (t + 7) % 12, 12 * major + (t + 5) % 12, relative, 12 * (1 - major) + t


def modulating_recipe(i, seconds, sr=SR, mean_seconds=45.0, min_seconds=20.0, fade_seconds=0.5):
    """Recording ``i`` of ``seconds`` seconds that changes key: -> ``(partials, segments)``; seed = 4321 + i.

    The first key is ``i % 24``.  Segment lengths are ``min_seconds + Exponential(mean_seconds - min_seconds)``, drawn until ``seconds``
    is covered; the last piece is cut at the end, and joins the piece before it when that leaves it shorter than ``min_seconds``.  Every
    following key is a move from the current one, drawn with ``MODULATION_MOVES``: a fifth up, a fifth down, the relative, the parallel,
    or one of the 19 other keys.  Every segment draws ``N_PARTIALS`` partials the way ``clip_recipe`` does (the key's scale with the
    tonic weighted x3, octaves 2-6, amplitude U(0.05, 0.25), phase uniform) and sounds from ``fade / 2`` before its boundary to
    ``fade / 2`` behind the next, so neighbours cross-fade centred on the boundary with envelopes that sum to 1.

    ``partials``: dict of ``cps`` (float64, cycles per sample), ``phase`` (float64, turns), ``amp`` (float32), ``start`` / ``end``
    (int64 samples) -- the arrays ``synth_partials`` takes -- and the scalars ``fade``, ``n``, ``seed``, ``noise_sigma`` (0.003) and
    ``peak`` (0.9).  ``segments``: list of ``(start_sample, key_id)``, the first at 0."""
    rng = np.random.default_rng(4321 + int(i))
    n = int(round(float(seconds) * sr))
    lengths, total = [], 0.0
    while total < seconds:
        lengths.append(float(min_seconds) + float(rng.exponential(float(mean_seconds) - float(min_seconds))))
        total += lengths[-1]
    lengths[-1] -= total - float(seconds)
    if len(lengths) > 1 and lengths[-1] < min_seconds:
        last = lengths.pop()
        lengths[-1] += last
    bounds = [0] + [int(round(s * sr)) for s in np.cumsum(lengths)[:-1]] + [n]
    keys = [int(i) % 24]
    for _ in lengths[1:]:
        move = int(rng.choice(5, p=MODULATION_MOVES))
        named = _related_keys(keys[-1])
        if move < 4:
            keys.append(named[move])
        else:
            others = [k for k in range(24) if k != keys[-1] and k not in named]
            keys.append(int(others[int(rng.integers(0, len(others)))]))
    fade = int(round(float(fade_seconds) * sr))
    half = fade // 2
    cps, phase, amp, start, end = [], [], [], [], []
    for s, sig in enumerate(keys):
        tonic = sig % 12
        scale = np.flatnonzero(key_pitch_classes(sig))
        weights = np.where(scale == tonic, 3.0, 1.0)
        weights /= weights.sum()
        pcs = rng.choice(scale, size=N_PARTIALS, p=weights)
        octaves = rng.integers(2, 7, size=N_PARTIALS)
        midi = 12 * (octaves + 1) + pcs
        cps.append(440.0 * 2.0 ** ((midi - 69) / 12.0) / sr)
        amp.append(rng.uniform(0.05, 0.25, size=N_PARTIALS))
        phase.append(rng.uniform(0.0, 1.0, size=N_PARTIALS))
        start.append(np.full(N_PARTIALS, bounds[s] - half, dtype=np.int64))
        end.append(np.full(N_PARTIALS, bounds[s + 1] - half + fade, dtype=np.int64))          # = the next segment's start + fade
    partials = {
        "cps": np.concatenate(cps).astype(np.float64), "phase": np.concatenate(phase).astype(np.float64),
        "amp": np.concatenate(amp).astype(np.float32), "start": np.concatenate(start), "end": np.concatenate(end),
        "fade": fade, "n": n, "seed": int(rng.integers(0, 2 ** 63 - 1)), "noise_sigma": MODULATION_NOISE_SIGMA, "peak": MODULATION_PEAK,
    }
    return partials, list(zip(bounds[:-1], keys))


def modulating_batch_arrays(indices, seconds, sr=SR, **recipe):
    """The recipes of ``indices`` joined into the arrays ``synth_partials`` / ``synth_partials_reference`` take -> ``(arrays, segments)``:
    ``arrays`` a dict of ``offsets``, ``cps``, ``phase``, ``amp``, ``start``, ``end``, ``fade``, ``n``, ``noise_sigma``, ``seed``, ``peak``;
    ``segments`` one list of ``(start_sample, key_id)`` per recording.  ``seconds``: one value or one per recording."""
    indices = [int(i) for i in indices]
    secs = [float(seconds)] * len(indices) if np.ndim(seconds) == 0 else [float(s) for s in seconds]
    if len(secs) != len(indices):
        raise ValueError(f"modulating_batch_arrays: {len(indices)} recordings but {len(secs)} durations")
    made = [modulating_recipe(i, s, sr, **recipe) for i, s in zip(indices, secs)]
    parts = [m[0] for m in made]
    arrays = {k: np.concatenate([p[k] for p in parts]) for k in ("cps", "phase", "amp", "start", "end")}
    arrays["offsets"] = np.concatenate([[0], np.cumsum([len(p["cps"]) for p in parts])]).astype(np.int32)
    arrays["n"] = np.array([p["n"] for p in parts], dtype=np.int64)
    arrays["seed"] = np.array([p["seed"] for p in parts], dtype=np.int64)
    arrays["fade"], arrays["noise_sigma"], arrays["peak"] = parts[0]["fade"], parts[0]["noise_sigma"], parts[0]["peak"]
    return arrays, [m[1] for m in made]


def make_modulating_batch_device(indices, seconds, device, sr=SR, **recipe):
    """Modulating recordings synthesised on ``device`` by the additive-synthesiser kernel -> ``(audio, annotations)``, or
    ``(audio, annotations, lengths)`` when ``seconds`` holds one duration per recording.

    ``audio`` (R, n) float32 (rows may be strided; samples behind a shorter recording's end are zeros), ``annotations`` the
    ``ake_amd.KeyAnnotations`` of the recipes' segments, ``lengths`` int64 (R,) on the device.  ``recipe``: ``mean_seconds``,
    ``min_seconds``, ``fade_seconds`` of ``modulating_recipe``."""
    import torch
    from .pipeline import KeyAnnotations
    from .synth import synth_partials
    arrays, segments = modulating_batch_arrays(indices, seconds, sr, **recipe)
    audio = synth_partials(device=device, **arrays)
    ann = KeyAnnotations.from_segments([[(s / sr, k) for s, k in segs] for segs in segments], sr, device)
    # (from_segments rounds start_s * sr: put the recipes' own integer starts back, a float round trip must not move a boundary)
    for r, segs in enumerate(segments):
        ann.seg_start[r, :len(segs)] = torch.tensor([s for s, _ in segs], dtype=torch.int64, device=device)
    if np.ndim(seconds) == 0:
        return audio, ann
    return audio, ann, torch.as_tensor(arrays["n"], device=device)
