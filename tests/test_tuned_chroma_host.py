"""The float64 model of the tuned chroma (metrics.profile_emissions(cents=...), metrics.folded_chroma): the class boundaries of the
key-profile method moved by a detuning instead of the audio being retuned.  No GPU."""
import types

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd import metrics, synthetic
from oracle import cqt_oracle

# cents -> (n, g) by hand: delta = 3 c / 100, n = floor(delta - 1), g = delta - 1 - n
CUTS = {0.0: (-1, 0.0), 10.0: (-1, 0.3), -10.0: (-2, 0.7), 16.6: (-1, 0.498), -16.6: (-2, 0.502), 33.4: (0, 0.002), -33.4: (-3, 0.998),
        50.0: (0, 0.5), -50.0: (-3, 0.5)}
F32 = 1e-6                       # the cents are rounded to float32 first: g moves by less than 3 * 2^-24 * 50 / 100


def random_logmag(R, P, T, seed):
    return torch.rand((R, P, T), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 3.0


def window_chroma_by_hand(FW, cents):
    """The definition, one scalar at a time: FW (36,) and one float -> x (12,)."""
    c = float(np.float32(cents))
    c = 0.0 if c != c else min(max(c, -50.0), 50.0)
    u = 3.0 * c / 100.0 - 1.0
    n = int(np.floor(u))
    g = u - n
    x = []
    for j in range(12):
        b = [(3 * j + n + i) % 36 for i in range(4)]
        s = ((1.0 - g) * float(FW[b[0]]) + float(FW[b[1]])) + float(FW[b[2]])
        if g != 0.0:
            s = s + g * float(FW[b[3]])
        x.append(s)
    return torch.tensor(x, dtype=torch.float64)


@pytest.mark.parametrize("cents", sorted(CUTS))
def test_one_lit_folded_bin_is_split_as_computed_by_hand(cents):
    n, g = CUTS[cents]
    cut_n, cut_g = metrics.tuned_cut(torch.tensor(float(np.float32(cents)), dtype=torch.float64))
    assert int(cut_n) == n and abs(float(cut_g) - g) <= F32
    for P in (36, 288):
        for p in range(36):
            L = torch.zeros((1, P, 3), dtype=torch.float64)
            L[0, p + (P - 36), :] = 2.0                              # (the top octave: the fold brings it to p)
            F = metrics.folded_chroma(L)
            assert F.shape == (1, 3, 36) and bool((F[0, :, p] == 2.0).all()) and float(F.sum()) == 6.0
            x = metrics.tuned_class_sums(F.sum(dim=1), torch.tensor([float(np.float32(cents))], dtype=torch.float64))[0]
            assert abs(float(x.sum()) - 6.0) <= 1e-12                # the twelve class sums add up to the bin's value
            q = (p - n) % 36                                         # bin p is the i-th of class j's four: 3 j + n + i = p (mod 36)
            want = torch.zeros(12, dtype=torch.float64)
            if q % 3 == 0:                                           # on a boundary: 1 - g to the class above it, g to the one below
                want[q // 3] += 6.0 * (1.0 - g)
                want[(q // 3 - 1) % 12] += 6.0 * g
            else:
                want[q // 3] = 6.0
            assert float((x - want).abs().max()) <= 6.0 * F32, (cents, P, p, x, want)
            assert torch.equal(x, window_chroma_by_hand(F.sum(dim=1)[0], cents))
            chroma = metrics.profile_emissions(L, 3, 1, cents=cents)[0][0, 0]
            assert float((chroma - want / 6.0).abs().max()) <= F32


@pytest.mark.parametrize("P", [36, 288])
def test_zero_cents_is_the_chroma_as_it_is(P):
    L = random_logmag(3, P, 21, 100 + P)
    for compression in metrics.PROFILE_COMPRESSIONS:
        for wf, sf in ((1, 1), (5, 2), (0, 1)):
            plain = metrics.profile_emissions(L, wf, sf, compression=compression)
            tuned = metrics.profile_emissions(L, wf, sf, compression=compression, cents=0.0)
            for a, b in zip(plain, tuned):
                assert float((a.double() - b.double()).abs().max()) <= 1e-12, (compression, wf, sf)
            assert torch.equal(plain[2], tuned[2])


def test_plus_fifty_is_minus_fifty_one_class_on():
    L = random_logmag(2, 72, 9, 7)
    up, down = metrics.profile_emissions(L, 4, 1, cents=50.0), metrics.profile_emissions(L, 4, 1, cents=-50.0)
    FW = metrics.folded_chroma(L)[:, :4].sum(dim=1)
    x_up, x_down = (metrics.tuned_class_sums(FW, torch.full((2,), c, dtype=torch.float64)) for c in (50.0, -50.0))
    assert torch.equal(x_up, torch.roll(x_down, -1, dims=1))         # class j at +50 holds what class j + 1 holds at -50, to the bit
    assert float((up[0] - torch.roll(down[0], -1, dims=2)).abs().max()) <= 1e-15     # (their total is added in another order)
    assert torch.equal(up[2] % 12, (down[2] - 1) % 12) and torch.equal(up[2] // 12, down[2] // 12)
    assert float((up[3] - down[3]).abs().max()) <= 1e-12


def test_a_shift_of_one_whole_bin_is_the_rolled_spectrum():
    """delta = 1 exactly: n = 0 and g = 0, so class j holds the folded bins 3 j, 3 j + 1, 3 j + 2, the uniform classes of the spectrum
    moved down by one bin.  No float32 has 3 c / 100 == 1, so the cents go in as the double 100 / 3 (tuned_class_sums takes them as
    they are); the spectrum holds small integers, whose sums are exact in any order."""
    c = torch.tensor([100.0 / 3.0], dtype=torch.float64)
    n, g = metrics.tuned_cut(c)
    assert int(n) == 0 and float(g) == 0.0
    L = torch.randint(0, 9, (1, 36, 6), generator=torch.Generator().manual_seed(3)).to(torch.float64)
    x = metrics.tuned_class_sums(metrics.folded_chroma(L).sum(dim=1), c)
    rolled = metrics.profile_emissions(torch.roll(L, -1, dims=1), 6, 1)[0][0, 0]
    assert torch.equal(x[0] / x[0].sum(), rolled)
    # the nearest float32 below it sits a hair in front of the floor step: the weights are continuous across it
    near = metrics.profile_emissions(L, 6, 1, cents=float(np.float32(100.0 / 3.0)))[0][0, 0]
    assert int(metrics.tuned_cut(torch.tensor(float(np.float32(100.0 / 3.0)), dtype=torch.float64))[0]) == -1
    assert float((near - rolled).abs().max()) <= F32


def test_cents_are_read_as_the_kernel_reads_them():
    L = random_logmag(2, 36, 12, 11)
    at = lambda c: metrics.profile_emissions(L, 4, 4, cents=c)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    assert same(at(float("nan")), at(0.0))
    assert same(at(80.0), at(50.0)) and same(at(-1e9), at(-50.0))
    assert same(at(16.6), at(float(np.float32(16.6))))               # rounded to float32 first
    per_rec = at(torch.tensor([16.6, -33.4]))                        # (R,)
    for r, c in enumerate((16.6, -33.4)):
        assert all(torch.equal(x[r], y[r]) for x, y in zip(per_rec, at(c)))
    grid = torch.tensor([[0.0, 50.0, float("nan")], [-50.0, 16.6, 80.0]])     # (R, W)
    per_win = at(grid)
    for r in range(2):
        for w in range(3):
            assert all(torch.equal(x[r, w], y[r, w]) for x, y in zip(per_win, at(float(grid[r, w]))))
    for bad in (torch.zeros(3), torch.zeros((2, 2)), torch.zeros((3, 2))):
        with pytest.raises(ValueError):
            at(bad)


def test_window_geometry_is_that_of_the_uniform_chroma():
    L = random_logmag(4, 36, 20, 13)
    counts = [20, 9, 4, 0]                                           # 4: one below a window of 5
    plain = metrics.profile_emissions(L, 5, 5, counts)
    zero = metrics.profile_emissions(L, 5, 5, counts, cents=0.0)
    tuned = metrics.profile_emissions(L, 5, 5, counts, cents=torch.tensor([22.0, -38.0, 47.0, 5.0]))
    live = torch.tensor([[True] * 4, [True] + [False] * 3, [False] * 4, [False] * 4])
    for out in (plain, zero, tuned):
        assert torch.equal(out[2] >= 0, live)
        assert not bool(out[0][~live].any()) and not bool(out[1][~live].any()) and not bool(out[3][~live].any())
    F = metrics.folded_chroma(L, counts)
    assert not bool(F[1, 9:].any()) and not bool(F[3].any()) and bool(F[1, :9].all())
    want = window_chroma_by_hand(F[1, :5].sum(dim=0), -38.0)
    assert float((tuned[0][1, 0] - want / want.sum()).abs().max()) <= 1e-12
    whole = metrics.profile_emissions(L, 0, 1, counts, cents=torch.tensor([22.0, -38.0, 47.0, 5.0]))    # the whole clip: own frames
    assert whole[2].shape == (4, 1) and (whole[2][:, 0] >= 0).tolist() == [True, True, True, False]
    want = window_chroma_by_hand(F[2, :4].sum(dim=0), 47.0)
    assert float((whole[0][2, 0] - want / want.sum()).abs().max()) <= 1e-12
    alone = metrics.profile_emissions(L[2:3, :, :4], 0, 1, cents=47.0)
    assert all(torch.equal(a[0], b[2]) for a, b in zip(alone, whole))


def _stand_in(n_bins=288, frames=5):
    """A KeyEstimator as far as its refusals read it (they come before any device work, and building a real one needs a device)."""
    e = object.__new__(ake_amd.KeyEstimator)
    e.frames, e.net, e.sample_rate = frames, None, 22050
    e.plan = types.SimpleNamespace(n_bins=n_bins, hop_length=4410, bins_per_octave=36)
    return e


def test_refusals():
    L = random_logmag(1, 39, 4, 1)                                   # a multiple of 3, not of 36
    metrics.profile_emissions(L, 2, 1)
    with pytest.raises(ValueError, match="36"):
        metrics.profile_emissions(L, 2, 1, cents=0.0)
    with pytest.raises(ValueError, match="36"):
        metrics.folded_chroma(L)
    with pytest.raises(ValueError):
        metrics.folded_chroma(random_logmag(1, 36, 4, 1), compression="sqrt")
    audio = torch.zeros((1, 22050 * 20))
    est = _stand_in()
    with pytest.raises(ValueError, match="net"):
        est.track(audio, tuning="auto", tuned_chroma=True)           # method="net"
    with pytest.raises(ValueError, match="net"):
        est.track(audio, method="net", tuning="auto", tuned_chroma=True)
    with pytest.raises(ValueError, match="needs a tuning"):
        est.track(audio, method="profile", tuned_chroma=True)
    with pytest.raises(ValueError, match="refine"):
        est.track(audio, method="profile", tuning="auto", refine=True, tuned_chroma=True)
    with pytest.raises(ValueError, match="needs a tuning"):
        est.profile_key(audio, tuned_chroma=True)
    odd = _stand_in(n_bins=39)
    with pytest.raises(ValueError, match="multiple of 36"):
        odd.track(audio, method="profile", tuning="auto", tuned_chroma=True)
    with pytest.raises(ValueError, match="multiple of 36"):
        odd.profile_key(audio, tuning=10.0, tuned_chroma=True)


def test_tuned_chroma_keeps_the_in_tune_accuracy_on_detuned_clips():
    """The oracle CQT of synthetic.make_batch clips 0..47, in tune and detuned by -45 and by +49 cents (metrics.retune_reference(x, -c)
    plays an in-tune clip c cents off), "log", Krumhansl-Kessler, one window over every clip's own frames, the cents from
    metrics.estimate_tuning on the same transform: the share of clips whose key comes out exactly.  Measured with this model:
    in tune 0.5208 (uniform and tuned); -45 cents: uniform 0.3333, tuned 0.5208; +49 cents: uniform 0.1250, tuned 0.5208."""
    hop = 4410
    cqt = cqt_oracle.FastDirectCQT(synthetic.SR, hop, dtype=torch.float64)
    x = np.concatenate([synthetic.make_batch(range(lo, lo + 24))[0] for lo in (0, 24)]).astype(np.float64)
    truth = torch.arange(48) % 24                                    # clip i is in key i % 24 (synthetic.clip_recipe)

    def shares(audio, n):
        mel = torch.cat([cqt(audio[lo:lo + 24]) for lo in (0, 24)])
        counts = torch.as_tensor(1 + n // hop).clamp(max=mel.shape[2])
        cents, _ = metrics.estimate_tuning(mel, counts)
        uniform = metrics.profile_emissions(mel, 0, 1, counts)[2][:, 0]
        tuned = metrics.profile_emissions(mel, 0, 1, counts, cents=cents)[2][:, 0]
        return float(cents.mean()), float((uniform == truth).double().mean()), float((tuned == truth).double().mean())

    est0, uniform0, tuned0 = shares(x, np.full(48, x.shape[1]))
    print(f"exact keys on clips 0..47, in tune (estimate {est0:+.2f}): uniform {uniform0:.4f}, tuned {tuned0:.4f}")
    assert tuned0 >= uniform0 - 0.05
    for c in (-45.0, 49.0):
        y, n = metrics.retune_reference(x, -c)
        est, uniform, tuned = shares(y, n)
        print(f"exact keys on clips 0..47, {c:+.0f} cents (estimate {est:+.2f}): uniform {uniform:.4f}, tuned {tuned:.4f}")
        assert tuned >= uniform0 - 0.05, (c, tuned, uniform0)
        assert tuned >= uniform + 0.05, (c, tuned, uniform)
