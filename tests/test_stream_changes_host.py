"""CPU: which boundaries a push of a key stream makes final, how long the two carried rings must be, and the float64 model of the
streamed change-point kernel (metrics.stream_changes_ready / stream_changes_ring_frames / stream_changes_labels_carried /
stream_key_changes) against metrics.key_changes on the joined frames and labels."""
import random

import pytest
import torch

from ake_amd import metrics
from ake_amd.stream import final_frames, windows_ready


def brute_ready(L, F, wf, sf, slack, finishing):
    """The rule as it is stated, boundary by boundary."""
    n = 0
    for w in range(max(L, 0) + 2):
        m1 = (w + 1) * sf + wf // 2
        n += bool((w + 2 < L and F >= m1 + slack) or (finishing and w + 1 < L))
    return n


@pytest.mark.parametrize("wf", [1, 5, 76])
def test_ready_equals_the_rule_counted_by_hand_and_is_monotone(wf):
    for sf in sorted({max(1, wf // 2), wf, wf + 3}):                  # below, at and above the window
        for slack in (0, sf, 3 * sf):
            edges = {(w + 1) * sf + wf // 2 + slack + d for w in range(62) for d in (-1, 0, 1)}
            top = 62 * sf + wf + slack
            frames = sorted(f for f in (set(range(0, min(top, 400))) | edges | {top}) if f >= 0)
            for L in range(61):
                last = [None, None]
                for F in frames:
                    for fin in (False, True):
                        got = metrics.stream_changes_ready(L, F, wf, sf, slack, fin)
                        assert got == brute_ready(L, F, wf, sf, slack, fin), (L, F, wf, sf, slack, fin)
                        assert last[fin] is None or got >= last[fin]                                  # in F
                        last[fin] = got
                        assert got <= metrics.stream_changes_ready(L + 1, F, wf, sf, slack, fin)       # in L
                    assert last[0] <= last[1]                                                          # in finishing
    with pytest.raises(ValueError):
        metrics.stream_changes_ready(-1, 0, wf, 1, 0)
    with pytest.raises(ValueError):
        metrics.stream_changes_ready(3, 10, wf, 0, 0)


def test_ring_rules_hold_and_are_tight_over_random_schedules():
    """200 schedules of chunk lengths, driven through the stream's own geometry: no boundary a push makes final reaches behind a chroma
    ring of stream_changes_ring_frames rows, no window behind one of stream_profile_ring_frames, no label is needed that is older than
    stream_changes_labels_carried, and each of the bounds is attained (both branches of the boundaries' rule), so none can be lowered."""
    rng = random.Random(20240)
    # how far below each bound the worst case stayed
    spare = {"profile": 10 ** 9, "frames": 10 ** 9, "labels": 10 ** 9, "carried": 10 ** 9}
    for trial in range(200):
        hop, H = rng.choice([(4, 6), (3, 1), (5, 11)])
        wf, sf = rng.choice([(5, 2), (5, 5), (4, 7), (1, 1), (7, 3)])
        slack = rng.choice([0, sf, 3 * sf, 7])
        lag = rng.choice([0, 2, 6])
        smooth = lag > 0 or rng.random() < 0.5
        chunks = [rng.choice([0, 1, hop - 1, hop, hop + 1, 3 * hop, rng.randrange(0, 8 * hop)]) for _ in range(rng.randrange(10, 60))]
        counts, N = [], 0
        for i, m in enumerate(chunks + [0]):
            N += m
            fin = i == len(chunks)
            F = final_frames(N, hop, H, fin)
            W = windows_ready(F, wf, sf)
            L = sum(metrics.key_stream_count(0, W, lag, fin)) if smooth else W
            counts.append((F, W, L, fin))
        max_new = max(b[0] - a[0] for a, b in zip([(0, 0, 0, False)] + counts[:-1], counts))
        ring_c = metrics.stream_changes_ring_frames(wf, sf, slack, lag, max_new)
        ring_p = metrics.stream_profile_ring_frames(wf, max_new)
        by_frames, by_labels = max_new + sf + 2 * slack - 1, max_new + wf - wf // 2 + (lag + 2) * sf + slack - 1
        assert ring_c == max(by_frames, by_labels, 1)
        carried = metrics.stream_changes_labels_carried(wf, sf, slack)
        F0 = W0 = L0 = B0 = 0
        for F, W, L, fin in counts:
            assert L >= L0 and F >= F0 and L <= W
            B = metrics.stream_changes_ready(L, F, wf, sf, slack, fin)
            if W > W0:                                                # the new windows read the frames W0 * sf .. F - 1
                assert F - W0 * sf <= ring_p
                spare["profile"] = min(spare["profile"], ring_p - 1 - (F - W0 * sf))   # (its docstring: the span is shorter than the ring)
            if B > B0:                                                # the new boundaries read from max(m_B0 - slack, 0) on
                reach = F - max(B0 * sf + wf // 2 - slack, 0)
                assert reach <= ring_c, (trial, reach, ring_c)
                waited_for_labels = B0 + 2 >= L0
                waited_for_frames = F0 < (B0 + 1) * sf + wf // 2 + slack
                assert waited_for_labels or waited_for_frames
                if waited_for_frames:
                    assert reach <= by_frames
                    spare["frames"] = min(spare["frames"], by_frames - reach)
                if waited_for_labels and not waited_for_frames:
                    assert reach <= by_labels
                    spare["labels"] = min(spare["labels"], by_labels - reach)
            if not fin:
                kept = L - max(B - 1, 0)
                assert kept <= carried, (trial, kept, carried)
                if slack >= 3 * sf:                                   # (where the bound exceeds the three labels every boundary needs)
                    spare["carried"] = min(spare["carried"], carried - kept)
            F0, W0, L0, B0 = F, W, L, B
        assert B0 == max(L0 - 1, 0)                                   # the flush emitted the rest
    assert spare == {"profile": 0, "frames": 0, "labels": 0, "carried": 0}, spare
    for bad in (dict(window_frames=0), dict(stride_frames=0), dict(slack_frames=-1), dict(lag_windows=-1), dict(max_new_frames=-1)):
        with pytest.raises(ValueError):
            metrics.stream_changes_ring_frames(**{**dict(window_frames=5, stride_frames=2, slack_frames=2, lag_windows=0, max_new_frames=3), **bad})
    with pytest.raises(ValueError):
        metrics.stream_changes_labels_carried(5, 2, -1)
    assert metrics.stream_changes_labels_carried(76, 25, 25) == 3 and metrics.stream_changes_ring_frames(1, 1, 0, 0, 0) == 2


def seeded_labels(rng, W):
    """Runs of one, two and more windows, with -1 and 24 (no key) among the keys."""
    row = []
    while len(row) < W:
        key = rng.choice([-1, 24] + list(range(24)) * 2)
        row += [key] * rng.choice([1, 1, 1, 2, 2, 3, 5])
    return row[:W]


def random_case(rng, trial):
    R = rng.choice([1, 2])
    wf, sf = rng.choice([(5, 2), (5, 2), (4, 5), (1, 1), (6, 3)])
    slack = rng.choice([0, sf, 3 * sf, 7])
    lag = rng.choice([0, 2, 6])
    T = rng.choice([wf - 1, wf, wf + sf, wf + sf + 1]) if trial % 10 == 0 else rng.randrange(wf + 2 * sf, wf + 24 * sf)   # (few windows: a flush below 3 labels)
    W = windows_ready(T, wf, sf)
    frames = torch.rand((R, 36, T), generator=torch.Generator().manual_seed(1000 + trial), dtype=torch.float64).to(torch.float32) * 3.0
    if trial % 7 == 0 and T > 6:
        frames[R - 1, :, T // 2:T // 2 + 3] = 0.0                     # silent frames score 0 for every key
    labels = torch.tensor([seeded_labels(rng, W) for _ in range(R)], dtype=torch.int64).reshape(R, W)
    cuts, left = [], T
    while left > 0:
        m = min(left, rng.choice([0, 0, 1, 1, 2, 3, 5, 9]))
        cuts.append(m)
        left -= m
    flush_alone = rng.random() < 0.5 or not cuts                      # the end arrives with a piece of its own, or with the last frames
    if flush_alone:
        cuts.append(0)
    pieces, F, L = [], 0, 0
    for i, m in enumerate(cuts):
        fin = i == len(cuts) - 1
        Wn = windows_ready(F + m, wf, sf)
        Ln = Wn if fin else max(Wn - lag, 0)
        pieces.append((frames[:, :, F:F + m], labels[:, L:Ln], fin))
        F, L = F + m, Ln
    assert F == T and L == W
    ring = metrics.stream_changes_ring_frames(wf, sf, slack, lag, max(cuts)) if trial % 2 else None
    return frames, labels, wf, sf, slack, pieces, ring, rng.choice(metrics.PROFILE_COMPRESSIONS)


def test_joined_model_equals_key_changes_on_the_whole():
    rng = random.Random(4711)
    seen = {"boundaries": 0, "short_flush": 0, "empty": 0, "one": 0, "wrapped": 0}
    for trial in range(200):
        frames, labels, wf, sf, slack, pieces, ring, compression = random_case(rng, trial)
        R, _, T = frames.shape
        W = labels.shape[1]
        want = metrics.key_changes(frames, labels, wf, sf, torch.full((R,), T), torch.full((R,), W), slack, compression=compression)
        outs = metrics.stream_key_changes(pieces, wf, sf, slack, compression=compression, ring_frames=ring)
        assert len(outs) == len(pieces)
        at = 0
        for first, frame, gain, contrast in outs:                     # every boundary once, in order
            assert first == at and frame.dtype == torch.int32 and gain.dtype == contrast.dtype == torch.float64
            at += frame.shape[1]
        assert at == max(W - 1, 0)
        for i, name in ((1, "change_frame"), (2, "gain"), (3, "contrast")):
            assert torch.equal(torch.cat([o[i] for o in outs], dim=1), want[i - 1]), (trial, name)
        seen["boundaries"] += int((want[0] >= 0).sum())
        seen["short_flush"] += W < 3
        seen["empty"] += any(p[0].shape[2] == 0 for p in pieces)
        seen["one"] += any(p[0].shape[2] == 1 for p in pieces)
        seen["wrapped"] += ring is not None and ring < T
        # the same again in two calls with the state handed on
        if trial % 20 == 1 and len(pieces) > 2:
            cut = len(pieces) // 2
            head = metrics.stream_key_changes(pieces[:cut], wf, sf, slack, compression=compression, ring_frames=ring or T, return_state=True)
            tail = metrics.stream_key_changes(pieces[cut:], wf, sf, slack, compression=compression, state=head[-1])
            for a, b in zip(head[:-1] + tail, outs):
                assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert seen["boundaries"] > 1000 and min(seen.values()) >= 10, seen


def test_model_refusals():
    frames = torch.rand((1, 36, 20))
    labels = torch.tensor([[1, 1, 2, 2, 3, 3, 4, 4]])
    with pytest.raises(ValueError):                                  # windows the frames do not hold yet
        metrics.stream_key_changes([(frames[:, :, :6], labels, False)], 5, 2)
    with pytest.raises(ValueError):                                  # a ring too short for the piece
        metrics.stream_key_changes([(frames, labels, True)], 5, 2, ring_frames=6)
    for bad in (dict(window_frames=0), dict(stride_frames=0), dict(slack_frames=-1), dict(compression="sqrt")):
        with pytest.raises(ValueError):
            metrics.stream_key_changes([(frames, labels, True)], **{**dict(window_frames=5, stride_frames=2), **bad})
    with pytest.raises(ValueError):
        metrics.stream_key_changes([(torch.rand((1, 37, 20)), labels, True)], 5, 2)
    out, = metrics.stream_key_changes([(frames, labels, True)], 5, 2)
    assert out[0] == 0 and out[1].shape == (1, 7)
