"""GPU: the additive synthesiser (ake_synth_partials_f32) against its float64 model, synthetic.synth_partials_reference.

Before normalisation the bound is |dev - f64| <= 1e-6 * A_r + 8e-6 * sigma, A_r the sum of the recording's amplitudes: the fraction's
float32 rounding (2^-25 turn), sine and cosine at a couple of ulp, the envelope product and the accumulation; a float32 emulation of the
same arithmetic gives 2.3e-7 * A and 1.6e-6 * sigma, the bounds leave 4-5 times that for another libm.  With a peak the bound scales by
peak / max64 and adds 2^-23 * peak.  Every output buffer starts as NaN."""
import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import synthetic
from ake_amd.synth import synth_batch_partials, synth_partials

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def arrays_of(recordings, fade=0):
    """[(n, [(cps, phase, amp, start, end), ...]), ...] -> the keyword arrays of synth_partials / synth_partials_reference."""
    parts = [p for _, ps in recordings for p in ps]
    col = lambda k, dt: np.array([p[k] for p in parts], dtype=dt)
    return dict(offsets=np.concatenate([[0], np.cumsum([len(ps) for _, ps in recordings])]).astype(np.int32),
                cps=col(0, np.float64), phase=col(1, np.float64), amp=col(2, np.float32), start=col(3, np.int64), end=col(4, np.int64),
                fade=fade, n=np.array([n for n, _ in recordings], dtype=np.int64))


def run(arrays, sigma=0.0, seed=None, peak=0.0, pad=0):
    """The kernel on a NaN-filled (R, stride) buffer -> the whole buffer as float64 numpy (stride = n_max rounded up to 4, + pad)."""
    R, n_max = len(arrays["n"]), int(arrays["n"].max())
    stride = max(4, (n_max + 3) // 4 * 4) + pad
    out = torch.full((R, stride), float("nan"), dtype=torch.float32, device=DEV)
    got = synth_partials(noise_sigma=sigma, seed=seed, peak=peak, device=DEV, out=out, **arrays)
    torch.cuda.synchronize()
    assert got.shape == (R, n_max) and got.data_ptr() == out.data_ptr()
    return out.cpu().numpy().astype(np.float64)


def check(arrays, sigma=0.0, seed=None, peak=0.0, pad=0, label=""):
    """Device within the bound of the float64 model, zeros behind every row's end up to the stride -> (device buffer, model)."""
    full = run(arrays, sigma, seed, peak, pad)
    n, n_max = arrays["n"], int(arrays["n"].max())
    raw = synthetic.synth_partials_reference(noise_sigma=sigma, seed=seed, peak=0.0, **arrays)
    want = synthetic.synth_partials_reference(noise_sigma=sigma, seed=seed, peak=peak, **arrays) if peak else raw
    assert np.all(np.isfinite(full))
    for r in range(len(n)):
        nr = int(n[r])
        assert np.all(full[r, nr:] == 0.0), f"{label} row {r}: samples behind its end must be zeros"
        A = float(np.sum(arrays["amp"][arrays["offsets"][r]:arrays["offsets"][r + 1]].astype(np.float64)))
        bound = 1e-6 * A + 8e-6 * sigma
        if peak:
            mx = float(np.max(np.abs(raw[r, :nr]))) if nr else 0.0
            bound = bound * peak / mx + 2.0 ** -23 * peak if mx > 0 else 0.0
        err = float(np.max(np.abs(full[r, :nr] - want[r, :nr]))) if nr else 0.0
        print(f"{label} row {r}: n {nr}, A {A:.3f}, sigma {sigma}, peak {peak}: max error {err:.3e}, bound {bound:.3e}"
              + (f" ({err / A:.2e} * A)" if A > 0 and not sigma and not peak else ""))
        assert err <= bound, (label, r, err, bound)
        if peak and bound > 0:
            assert abs(float(np.max(np.abs(full[r, :nr]))) - peak) <= bound, (label, r)        # max |y| = peak within the bound
    return full[:, :n_max], want


@pytest.mark.parametrize("cps", [0.45, 32.7 / 22050])
def test_phase_stays_exact_over_a_million_samples(cps):
    """One partial, no fade, n = 2^20 + 3: a float32 phase would be wrong by 0.03 turns at the end."""
    n = 2 ** 20 + 3
    got, want = check(arrays_of([(n, [(cps, 0.3125, 0.8, 0, n)])]), label=f"cps {cps:.5f}")
    assert np.max(np.abs(want[0, -4096:])) > 0.7                       # (the end of the row still sounds)


def test_ragged_rows_end_in_zeros():
    """R = 4 with n = 4099, 1, 0 and 1024 (n_max = 4099: two tiles and a rest; a row of one sample; an empty row; exactly one tile),
    with noise, in a buffer whose stride is longer than n_max."""
    rng = np.random.default_rng(3)
    recs = []
    for n in (4099, 1, 0, 1024):
        recs.append((n, [(rng.uniform(0.001, 0.49), rng.uniform(0, 1), rng.uniform(0.05, 0.25), int(rng.integers(-50, 50)), int(rng.integers(900, 5000)))
                         for _ in range(5)]))
    arrays = arrays_of(recs, fade=16)
    seed = np.array([11, 12, 13, 14], dtype=np.int64)
    check(arrays, sigma=0.01, seed=seed, pad=8, label="ragged")
    check(arrays, sigma=0.01, seed=seed, peak=0.9, pad=8, label="ragged+peak")


def test_a_recording_without_partials():
    arrays = arrays_of([(3000, []), (3000, [(0.01, 0.0, 0.2, 0, 3000)]), (3000, [])])
    got, _ = check(arrays, label="no partials")
    assert np.all(got[0] == 0.0) and np.all(got[2] == 0.0) and np.max(np.abs(got[1])) > 0.19
    got, _ = check(arrays, sigma=0.5, seed=np.array([1, 2, 3], dtype=np.int64), label="no partials, noise")
    assert np.std(got[0]) > 0.4 and not np.array_equal(got[0], got[2])
    # no partial at all in the call: the partial arrays are empty
    got, _ = check(arrays_of([(100, []), (7, [])]), sigma=1.0, seed=np.array([5, 6], dtype=np.int64), label="empty call")
    assert np.std(got[0]) > 0.5


def test_fades():
    n, fade = 5000, 300
    recs = [(n, [(0.0130, 0.10, 0.20, 1000, 1400),          # shorter than 2 * fade: both ramps at once
                 (0.0270, 0.55, 0.15, -120, 2500),           # start < 0: the recording begins inside the fade-in
                 (0.0410, 0.80, 0.10, 3000, n + 170),        # end > n: it ends inside the fade-out
                 (0.0090, 0.00, 0.25, 2000, 2001)]),         # one sample long
            (n, [(0.0200, 0.25, 0.30, -fade, 2600),          # a cross-fading pair of one tone: a steady sine
                 (0.0200, 0.25, 0.30, 2600 - fade, n + fade)])]
    got, want = check(arrays_of(recs, fade=fade), label="fades")
    t = np.arange(n)
    assert np.max(np.abs(got[1] - 0.30 * np.sin(2 * np.pi * (0.02 * t + 0.25)))) < 1e-6 * 0.6
    got0, want0 = check(arrays_of(recs, fade=0), label="fade 0")
    assert np.max(np.abs(want0[0] - want[0])) > 0.05                   # (the envelopes do something)
    check(arrays_of(recs, fade=1), label="fade 1")


def test_more_partials_than_the_lds_list_holds():
    """2 * capacity + 1 partials that all overlap tile 0, between others that do not: three rounds of compaction, in order."""
    cap = synth_batch_partials()
    assert cap >= 64
    rng = np.random.default_rng(9)
    n, parts = 1500, []
    for k in range(2 * cap + 1):
        parts.append((rng.uniform(0.001, 0.49), rng.uniform(0, 1), rng.uniform(0.001, 0.004), int(rng.integers(-20, 600)), int(rng.integers(700, 1600))))
        if k % 3 == 0:
            parts.append((rng.uniform(0.001, 0.49), rng.uniform(0, 1), 0.004, int(rng.integers(1030, 1200)), int(rng.integers(1300, 1600))))   # tile 1 only
        if k % 50 == 0:
            parts.append((0.1, 0.0, 0.004, 400, 400))                   # empty
            parts.append((0.1, 0.0, 0.004, 2000, 3000))                 # behind the end
    assert sum(1 for p in parts if p[3] < 1024 and p[4] > 0 and p[3] < p[4]) == 2 * cap + 1
    check(arrays_of([(n, parts), (n, parts[:cap + 1])], fade=32), label="many partials")


def test_noise_alone():
    n = 2 ** 20
    arrays = arrays_of([(n, [])])
    got, want = check(arrays, sigma=1.0, seed=np.array([2024], dtype=np.int64), label="noise")
    z = got[0]
    mean, var = float(z.mean()), float(z.var())
    print(f"noise: mean {mean:.3e} (se {n ** -0.5:.3e}), variance {var:.5f} (se {(2 / n) ** 0.5:.3e}), max |z| {np.max(np.abs(z)):.3f}")
    assert abs(mean) < 4 * n ** -0.5 and abs(var - 1.0) < 4 * (2 / n) ** 0.5
    other = run(arrays_of([(4096, [])]), sigma=1.0, seed=np.array([2025], dtype=np.int64))
    assert not np.array_equal(other[0], z[:4096]) and abs(np.corrcoef(other[0], z[:4096])[0, 1]) < 0.1
    high = run(arrays_of([(4096, [])]), sigma=1.0, seed=np.array([2024 + (1 << 32)], dtype=np.int64))      # the seed's high word counts
    assert not np.array_equal(high[0], z[:4096])


def test_peak_normalisation():
    rng = np.random.default_rng(4)
    recs = [(6000, [(rng.uniform(0.001, 0.2), rng.uniform(0, 1), rng.uniform(0.05, 0.25), 0, 6000) for _ in range(12)]),
            (2500, []),                                                # all zero: stays zero, nothing divides by zero
            (4100, [(0.25, 0.0, 1e-3, 10, 4000)])]
    arrays = arrays_of(recs, fade=100)
    got, _ = check(arrays, peak=0.9, label="peak")
    assert np.all(got[1] == 0.0) and abs(np.max(np.abs(got[0])) - 0.9) < 1e-6 and abs(np.max(np.abs(got[2])) - 0.9) < 1e-6
    check(arrays, sigma=0.003, seed=np.array([7, 8, 9], dtype=np.int64), peak=0.9, label="peak+noise")


def test_reruns_are_bit_identical():
    rng = np.random.default_rng(6)
    recs = [(n, [(rng.uniform(0.001, 0.49), rng.uniform(0, 1), rng.uniform(0.05, 0.25), int(rng.integers(-500, 3000)), int(rng.integers(3000, 9000)))
                 for _ in range(40)]) for n in (8191, 5000)]
    arrays = arrays_of(recs, fade=200)
    seed = np.array([31, 32], dtype=np.int64)
    first = run(arrays, sigma=0.003, seed=seed, peak=0.9)
    for _ in range(3):
        assert np.array_equal(run(arrays, sigma=0.003, seed=seed, peak=0.9), first)


def test_modulating_batch_on_the_device():
    """3 recordings of 25 s whose key changes every 5 s + Exp(3 s): the device batch against the host model of the same recipes."""
    recipe = dict(min_seconds=5.0, mean_seconds=8.0)
    audio, ann = synthetic.make_modulating_batch_device([0, 1, 2], 25.0, DEV, **recipe)
    torch.cuda.synchronize()
    arrays, segments = synthetic.modulating_batch_arrays([0, 1, 2], 25.0, **recipe)
    n = 25 * synthetic.SR
    assert audio.shape == (3, n) and audio.dtype == torch.float32 and audio.stride(0) % 4 == 0
    assert isinstance(ann, ake_amd.KeyAnnotations) and ann.seg_start.device.type == "cuda" and ann.sample_rate == synthetic.SR
    assert ann.seg_count.tolist() == [len(s) for s in segments] and min(len(s) for s in segments) >= 2
    for r, segs in enumerate(segments):
        assert ann.seg_start[r, :len(segs)].tolist() == [s for s, _ in segs] and ann.seg_key[r, :len(segs)].tolist() == [k for _, k in segs]
    raw = synthetic.synth_partials_reference(**dict(arrays, peak=0.0))
    want = synthetic.synth_partials_reference(**arrays)
    got = audio.cpu().numpy().astype(np.float64)
    for r in range(3):
        # at most two segments (24 partials) sound at once; A_r sums the amplitudes of all of the recording's partials all the same
        A = float(arrays["amp"][arrays["offsets"][r]:arrays["offsets"][r + 1]].astype(np.float64).sum())
        bound = (1e-6 * A + 8e-6 * arrays["noise_sigma"]) * 0.9 / np.max(np.abs(raw[r])) + 2.0 ** -23 * 0.9
        err = float(np.max(np.abs(got[r] - want[r])))
        print(f"modulating {r}: {len(segments[r])} segments, A {A:.2f}, max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound and abs(np.max(np.abs(got[r])) - 0.9) <= bound
    # one duration per recording: ragged rows and their lengths
    audio2, ann2, lengths = synthetic.make_modulating_batch_device([0, 1], [25.0, 12.5], DEV, **recipe)
    assert lengths.tolist() == [n, n // 2] and audio2.shape == (2, n) and bool((audio2[1, n // 2:] == 0).all())
    assert torch.equal(audio2[0], audio[0])
