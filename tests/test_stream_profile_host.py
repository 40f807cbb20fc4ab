"""Host: the float64 models of a net-free key stream -- metrics.stream_profile against metrics.profile_emissions on the joined frames,
metrics.stream_tuning against metrics.estimate_tuning on the prefixes -- and the chroma ring's capacity rule over the stream's geometry.
No GPU."""
import math
import random

import numpy as np
import pytest
import torch

from ake_amd import metrics, stream

NAMES = ("chroma", "emissions", "key_id", "confidence")


def frames(R, P, T, seed, silent=None):
    """Random log-magnitudes in [0, 3]; `silent` = (recording, first, last): a stretch of exact zeros."""
    L = torch.rand((R, P, T), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 3.0
    if silent is not None:
        r, a, b = silent
        L[r, :, a:b] = 0.0
    return L


def random_cut(T, rng, longest):
    """Piece lengths that sum to T: pieces of 0 and 1 frame in every cut, the rest up to `longest`."""
    cut, left = [0, 1, 0], T - 1
    while left > 0:
        cut.append(min(left, rng.choice((0, 1, 1, min(2, longest), rng.randint(1, longest)))))
        left -= cut[-1]
    rng.shuffle(cut)
    return cut


def pieces_of(L, cut):
    out, at = [], 0
    for m in cut:
        out.append(L[:, :, at:at + m])
        at += m
    assert at == L.shape[2]
    return out


def join(outs):
    return [torch.cat([o[i] for o in outs], dim=1) for i in range(4)]


def user_profile():
    return torch.rand((2, 12), generator=torch.Generator().manual_seed(41), dtype=torch.float64) + 0.2


# (wf, sf, T, compression, profiles, the ring (None: the default), the longest piece): sf below, equal to and above wf; rings that wrap often
CONFIGS = [(1, 1, 40, "log", "krumhansl", 3, 2), (1, 3, 40, "power", "temperley", 1, 1), (5, 2, 90, "log", "krumhansl", 7, 2),
           (5, 2, 90, "magnitude", "user", None, 9), (5, 5, 90, "power", "krumhansl", 8, 3), (5, 9, 90, "log", "temperley", 6, 1),
           (5, 9, 90, "magnitude", "krumhansl", None, 30), (76, 5, 200, "log", "krumhansl", 79, 3), (76, 76, 200, "power", "user", None, 40),
           (76, 1, 190, "magnitude", "temperley", 88, 12)]


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"wf{c[0]}-sf{c[1]}-{c[3]}-{c[4]}-ring{c[5]}")
def test_joined_stream_equals_the_offline_model(config):
    """20 random cuts per configuration, 200 in all: to the bit, the silent windows included."""
    wf, sf, T, compression, profiles, ring, longest = config
    prof = user_profile() if profiles == "user" else profiles
    L = frames(2, 36, T, 100 + wf + sf, silent=(1, T // 3, T // 3 + 2 * wf + 3))
    want = metrics.profile_emissions(L, wf, sf, None, prof, compression, 7.5)
    assert int((want[2] < 0).sum()) >= 1 and int((want[2] >= 0).sum()) >= 1     # a silent window and a sounding one
    rng = random.Random(wf * 1000 + sf)
    for _ in range(20):
        cut = random_cut(T, rng, longest)
        outs = metrics.stream_profile(pieces_of(L, cut), wf, sf, prof, compression, 7.5, ring_frames=ring, return_state=True)
        state = outs.pop()
        assert len(outs) == len(cut) and state["frames"] == T and state["windows"] == want[2].shape[1]
        if ring is not None:
            assert state["ring"].shape[1] == ring and T > 2 * ring                # it wrapped several times
        at = 0
        for m, o in zip(cut, outs):                                               # each piece emits the windows it completed
            at += m
            k = stream.windows_ready(at, wf, sf) - stream.windows_ready(at - m, wf, sf)
            assert o[0].shape == (2, k, 12) and o[1].shape == (2, k, 24) and o[2].shape == (2, k) and o[3].shape == (2, k)
        for name, a, b in zip(NAMES, join(outs), want):
            assert a.dtype == b.dtype and torch.equal(a, b), (name, cut)


def test_state_carries_between_calls_and_does_not_depend_on_the_cut():
    L = frames(3, 36, 60, 7)
    whole = metrics.stream_profile([L], 5, 2, ring_frames=5 + 60, return_state=True)
    first = metrics.stream_profile(pieces_of(L[:, :, :23], [4, 0, 19]), 5, 2, ring_frames=41, return_state=True)
    second = metrics.stream_profile(pieces_of(L[:, :, 23:], [1, 36]), 5, 2, state=first[-1], return_state=True)
    for a, b in zip(join(first[:-1] + second[:-1]), join(whole[:-1])):
        assert torch.equal(a, b)
    other = metrics.stream_profile(pieces_of(L, [7] * 8 + [4]), 5, 2, ring_frames=41, return_state=True)[-1]
    assert torch.equal(other["ring"], second[-1]["ring"]) and other["frames"] == second[-1]["frames"] == 60
    # every frame is in the ring, also those a stride longer than the window skips
    skipping = metrics.stream_profile(pieces_of(L, [60]), 2, 7, ring_frames=60, return_state=True)[-1]["ring"]
    assert torch.equal(skipping, metrics._profile_frame_chroma(L, 0))


def test_stream_profile_refusals():
    L = frames(1, 36, 20, 3)
    for kw in (dict(window_frames=0, stride_frames=1), dict(window_frames=5, stride_frames=0), dict(window_frames=5, stride_frames=1, ring_frames=4),
               dict(window_frames=5, stride_frames=1, sharpness=0.0), dict(window_frames=5, stride_frames=1, sharpness=float("nan")),
               dict(window_frames=5, stride_frames=1, compression="sqrt"), dict(window_frames=5, stride_frames=1, profiles="nobody")):
        with pytest.raises(ValueError):
            metrics.stream_profile([L], **kw)
    with pytest.raises(ValueError):
        metrics.stream_profile([frames(1, 37, 20, 3)], 5, 1)
    with pytest.raises(ValueError):
        metrics.stream_profile([L, frames(2, 36, 4, 3)], 5, 1)
    with pytest.raises(ValueError, match="ring"):                                # 20 frames at once into a ring of 8: window 0 is gone
        metrics.stream_profile([L], 5, 1, ring_frames=8)
    with pytest.raises(ValueError):
        metrics.stream_profile_ring_frames(0, 4)
    assert metrics.stream_profile([], 5, 1) == []


# ---- the tuning meter ----

def placed(R, T, seed, P=36):
    """A log-CQT from hand-placed bin positions: per bin and frame the power on position 0 drawn from [1, 2], on 1 from [0, 0.5], on 2
    from [0, 0.3], so the estimate is strong (strength >= 0.05 by far) and differs from frame to frame."""
    g = torch.Generator().manual_seed(seed)
    power = torch.rand((R, P, T), generator=g, dtype=torch.float64)
    power[:, 0::3] = 1.0 + power[:, 0::3]
    power[:, 1::3] = 0.5 * power[:, 1::3]
    power[:, 2::3] = 0.3 * power[:, 2::3]
    return torch.log1p(torch.sqrt(power))


@pytest.mark.parametrize("P", [36, 288])
def test_running_tuning_equals_the_estimate_on_every_prefix(P):
    L = placed(3, 50, 11, P)
    rng = random.Random(P)
    for _ in range(5):
        cut = random_cut(50, rng, 12)
        outs = metrics.stream_tuning(pieces_of(L, cut))
        assert len(outs) == len(cut)
        at = 0
        for m, (cents, strength) in zip(cut, outs):
            at += m
            assert cents.dtype == torch.float64 and cents.shape == (3,) and strength.shape == (3,)
            if at == 0:
                assert not bool(cents.any()) and not bool(strength.any())
                continue
            want_c, want_s = metrics.estimate_tuning(L[:, :, :at])
            assert float(want_s.min()) >= 0.05
            assert float((cents - want_c).abs().max()) <= 1e-9 and float((strength - want_s).abs().max()) <= 1e-12, (cut, at)
    # the state carries, and is the three sums
    a = metrics.stream_tuning(pieces_of(L[:, :, :20], [20]), return_state=True)
    b = metrics.stream_tuning(pieces_of(L[:, :, 20:], [1, 29]), state=a[-1], return_state=True)
    c = metrics.stream_tuning([L], return_state=True)
    assert a[-1].shape == (3, 3) and torch.equal(b[-1], c[-1]) and torch.equal(b[-2][0], c[0][0]) and torch.equal(b[-2][1], c[0][1])


def test_tuning_without_power_and_min_strength_at_equality():
    zero = torch.zeros((2, 36, 4), dtype=torch.float64)
    for cents, strength in metrics.stream_tuning([zero, zero[:, :, :0], zero]):
        assert torch.equal(cents, torch.zeros(2, dtype=torch.float64)) and torch.equal(strength, torch.zeros(2, dtype=torch.float64))
    L = placed(1, 9, 5)
    L[:, 1::3] += 0.4                                                            # off centre: cents far from 0
    (cents, strength), = metrics.stream_tuning([L])
    s = float(strength)
    assert abs(float(cents)) > 1.0 and 0.05 <= s < 1.0
    (kept, s1), = metrics.stream_tuning([L], min_strength=s)                     # strength < min_strength decides: equality keeps the estimate
    (dropped, s2), = metrics.stream_tuning([L], min_strength=math.nextafter(s, 1.0))
    assert torch.equal(kept, cents) and float(dropped) == 0.0 and float(s1) == float(s2) == s
    with pytest.raises(ValueError):
        metrics.stream_tuning([L], min_strength=float("nan"))
    with pytest.raises(ValueError):
        metrics.stream_tuning([torch.zeros((1, 37, 4))])


# ---- the ring's capacity over the stream's geometry ----

def test_ring_capacity_holds_over_random_schedules():
    """KeyStream's counts (final_frames, windows_ready) on random plans and schedules: with no piece above max_new frames, a ring of
    stream_profile_ring_frames(wf, max_new) rows holds every frame the new windows read, at every piece."""
    rng = random.Random(2024)
    checked = 0
    for _ in range(400):
        hop = rng.choice((1, 7, 441, 4410))
        H = rng.randint(0, 6 * hop)
        wf, sf = rng.choice((1, 2, 5, 76)), rng.choice((1, 2, 5, 25, 100))
        max_chunk = rng.randint(1, 12 * hop)
        max_new = 1 + (2 * H + hop + max_chunk + 3) // 4 * 4 // hop              # KeyStream.max_mel: frames of the longest re-transform
        ring = metrics.stream_profile_ring_frames(wf, max_new)
        assert ring == wf + max_new
        N = F = W = 0
        for piece in range(rng.randint(1, 60)):
            finishing = piece > 0 and rng.random() < 0.05
            N += 0 if finishing else rng.choice((0, 1, hop, rng.randint(0, max_chunk)))
            F_new = max(F, stream.final_frames(N, hop, H, finishing))
            W_new = stream.windows_ready(F_new, wf, sf)
            assert F_new - F <= max_new
            if W_new > W:
                assert W * sf >= F_new - ring and W * sf > F - wf and (W_new - 1) * sf + wf <= F_new
                checked += 1
            F, W = F_new, W_new
            if finishing:
                break
    assert checked > 500
