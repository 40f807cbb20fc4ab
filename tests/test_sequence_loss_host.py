"""Host: metrics.key_sequence_loss (the float64 model of ake_key_sequence_loss_f32) against autograd through a plain forward algorithm, its
identities, and the host model of TrackWindows' sequence mode.  No GPU."""
import math

import pytest
import torch

import ake_amd
from ake_amd import metrics
from ake_amd.pipeline import KeyAnnotations

F64 = torch.float64


def default_trans(stride=5.0):
    return metrics.key_transition_log(stay=math.exp(-stride / 60.0))


def heads(R, W, seed, tonic_scale=3.0):
    g = torch.Generator().manual_seed(seed)
    key = torch.rand((R, W, 12), generator=g, dtype=F64) * 0.96 + 0.02
    tonic = torch.randn((R, W, 12), generator=g, dtype=F64) * tonic_scale
    labels = torch.randint(0, 24, (R, W), generator=g)
    return key, tonic, labels, g


def forward_loglik(e, A, prior):
    """log Z of one recording's (n, 24) scores: the forward algorithm, out of place."""
    alpha = prior + e[0]
    for w in range(1, e.shape[0]):
        alpha = e[w] + torch.logsumexp(alpha[:, None] + A, dim=0)
    return torch.logsumexp(alpha, dim=0)


def autograd_loss(key, tonic, labels, A, counts, weight, prior):
    e = metrics.key_emissions(key, tonic, weight)
    k = torch.arange(24)
    total, N = torch.zeros((), dtype=F64), 0
    for r in range(key.shape[0]):
        n = min(max(int(counts[r]), 0), key.shape[1])
        if n == 0:
            continue
        lab = labels[r, :n]
        labelled = (lab >= 0) & (lab < 24)
        N += int(labelled.sum())
        ec = torch.where(labelled[:, None] & (k[None, :] != lab[:, None]), torch.full_like(e[r, :n], -1e4), e[r, :n])
        total = total + forward_loglik(e[r, :n], A, prior) - forward_loglik(ec, A, prior)
    return total / N, N


CASES = {
    "issue": dict(R=3, W=9, counts=[9, 5, 1], unlabelled=[(0, 2), (0, 3), (1, 0), (0, 8)], prior=False, forbid=False, weight=1.0),
    "ragged": dict(R=4, W=7, counts=[7, 0, 1, 4], unlabelled=[(0, 0), (3, 3), (3, 1)], prior=True, forbid=True, weight=0.5),
}


def make_case(c, seed=5):
    key, tonic, labels, g = heads(c["R"], c["W"], seed)
    for r, w in c["unlabelled"]:
        labels[r, w] = -1 if (r + w) % 2 else 24
    prior = torch.randn(24, generator=g, dtype=F64) if c["prior"] else None
    A = default_trans()
    if c["forbid"]:                                                                      # a user transition with forbidden moves
        A = A.clone()
        A[3, 17] = A[17, 3] = A[0, 5] = -1e4
    return key, tonic, labels, A, prior


@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_equals_autograd(name):
    c = CASES[name]
    key, tonic, labels, A, prior = make_case(c)
    out = metrics.key_sequence_loss(key, tonic, labels, A, counts=c["counts"], signature_weight=c["weight"], log_prior=prior)
    k, t, a = key.clone().requires_grad_(), tonic.clone().requires_grad_(), A.clone().requires_grad_()
    loss, N = autograd_loss(k, t, labels, a, c["counts"], c["weight"], torch.zeros(24, dtype=F64) if prior is None else prior)
    loss.backward()
    assert float(out["labelled"]) == N
    for what, got, want in (("loss", out["loss"], loss.detach()), ("d_key", out["d_key"], k.grad), ("d_tonic", out["d_tonic"], t.grad),
                            ("d_trans", out["d_trans"], a.grad)):
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"{name} {what}: error {err:.2e} at magnitude {scale:.2e}")
        assert err <= 1e-12 * scale, what
    live = torch.arange(c["W"])[None, :] < torch.tensor(c["counts"])[:, None]
    for what in ("d_key", "d_tonic", "d_emis"):
        assert bool((out[what][~live] == 0).all())
    # identities
    assert float(out["loss"]) >= 0.0
    assert float(out["loss"]) == pytest.approx(float(out["loglik"] - out["loglik_clamped"]), abs=1e-12)
    assert abs(float(out["d_trans"].sum())) <= 1e-12
    assert float(out["d_emis"].sum(dim=-1).abs().max()) <= 1e-15
    assert out["d_trans"].shape == (24, 24) and out["d_emis"].shape == (c["R"], c["W"], 24)


def test_off_label_clamped_posteriors_are_exactly_zero_and_the_rows_are_accepted():
    c = CASES["issue"]
    key, tonic, labels, A, _ = make_case(c)
    for dtype in (F64, torch.float32):
        e = metrics.key_emissions(key.to(dtype), tonic.to(dtype))
        labelled = (labels >= 0) & (labels < 24)
        off = labelled[..., None] & (torch.arange(24)[None, None, :] != labels[..., None])
        ec = torch.where(off, torch.full_like(e, metrics.SEQUENCE_CLAMP), e)
        post, ll = metrics.key_posteriors(ec, A.to(dtype), counts=c["counts"])
        live = (torch.arange(c["W"])[None, :] < torch.tensor(c["counts"])[:, None])[..., None]
        assert bool(torch.isfinite(post).all()) and bool(torch.isfinite(ll).all())
        assert bool((post[off & live] == 0).all())
        assert math.exp(metrics.SEQUENCE_CLAMP) == 0.0 and float(torch.exp(torch.tensor(metrics.SEQUENCE_CLAMP, dtype=dtype))) == 0.0


@pytest.mark.parametrize("labels_of", ["unlabelled", "behind the counts"])
def test_nothing_labelled_gives_exact_zeros(labels_of):
    key, tonic, labels, _ = heads(2, 6, 8)
    counts = [6, 4]
    if labels_of == "unlabelled":
        labels = torch.full_like(labels, -1)
        labels[1, 2] = 99
    else:
        counts = [0, 0]
    out = metrics.key_sequence_loss(key, tonic, labels, default_trans(), counts=counts)
    assert float(out["labelled"]) == 0 and float(out["loss"]) == 0.0
    for what in ("d_key", "d_tonic", "d_trans", "d_emis"):
        assert bool((out[what] == 0).all()), what


def test_all_labelled_is_log_z_minus_the_score_of_the_path():
    key, tonic, labels, g = heads(2, 8, 11)
    A, prior = default_trans(), torch.randn(24, generator=g, dtype=F64)
    out = metrics.key_sequence_loss(key, tonic, labels, A, signature_weight=0.7, log_prior=prior)
    e = metrics.key_emissions(key, tonic, 0.7)
    want = 0.0
    for r in range(2):
        path = labels[r]
        score = prior[path[0]] + e[r, torch.arange(8), path].sum() + A[path[:-1], path[1:]].sum()
        want += float(forward_loglik(e[r], A, prior) - score)
    assert float(out["labelled"]) == 16
    assert float(out["loss"]) * 16 == pytest.approx(want, rel=1e-12)


def test_one_window_is_the_cross_entropy_of_the_softmax():
    key, tonic, labels, g = heads(3, 1, 12)
    prior = torch.randn(24, generator=g, dtype=F64)
    out = metrics.key_sequence_loss(key, tonic, labels, default_trans(), log_prior=prior)
    e = metrics.key_emissions(key, tonic)
    ce = torch.nn.functional.cross_entropy(e[:, 0] + prior, labels[:, 0], reduction="mean")
    assert float(out["loss"]) == pytest.approx(float(ce), rel=1e-12)
    assert bool((out["d_trans"] == 0).all())


def test_a_constant_added_to_one_windows_emissions_changes_nothing():
    """The tonic logits of one window shifted by a constant leave its emissions as they are (log-softmax), and an emission row shifted
    by a constant moves both log-likelihoods alike: g sums to 0 per row, so the loss does not see it."""
    key, tonic, labels, _ = heads(2, 5, 13)
    A = default_trans()
    base = metrics.key_sequence_loss(key, tonic, labels, A)
    shifted = tonic.clone()
    shifted[1, 2] += 7.0
    out = metrics.key_sequence_loss(key, shifted, labels, A)
    assert float(out["loss"]) == pytest.approx(float(base["loss"]), abs=1e-13)
    assert float((out["d_key"] - base["d_key"]).abs().max()) <= 1e-13
    # the same through the chains: a constant on a whole emission row
    e = metrics.key_emissions(key, tonic)
    e2 = e.clone()
    e2[0, 3] += 5.0
    off = torch.arange(24)[None, None, :] != labels[..., None]
    diff = lambda x: float((metrics.key_posteriors(x, A)[1] - metrics.key_posteriors(torch.where(off, torch.full_like(x, -1e4), x), A)[1]).sum())  # noqa: E731
    assert diff(e2) == pytest.approx(diff(e), abs=1e-12)


def test_saturated_rows_give_finite_gradients_with_zero_derivative_at_the_clamps():
    key, tonic, labels, _ = heads(1, 4, 14)
    p32 = torch.tensor([0.0, 1.0, 1e-45, 1e-30], dtype=torch.float32)
    assert float(p32[2]) > 0 and float(p32[2]) < 1.2e-38                                 # subnormal in float32
    key[0, 1, :4] = p32.double()
    key[0, 2, 4:8] = p32.double()
    tonic[0, 1, 0], tonic[0, 1, 5], tonic[0, 3, 2] = 40.0, -40.0, -40.0
    for dtype in (F64, torch.float32):
        out = metrics.key_sequence_loss(key.to(dtype), tonic.to(dtype), labels, default_trans().to(dtype))
        for what in ("loss", "d_key", "d_tonic", "d_trans", "d_emis"):
            assert bool(torch.isfinite(out[what]).all()), (dtype, what)
        for w, j0 in ((1, 0), (2, 4)):
            row = out["d_key"][0, w]
            g = out["d_emis"][0, w].double()
            S = metrics.KEY_SCALES
            inside, outside = (g @ S), (g @ (1 - S))
            tol = 1e-5 * float(g.abs().max())                                            # (sums of 24 terms of either sign, in float32 too)
            # p = 0: log p is clamped (u = 0), 1 - p = 1 (v = 1);  p = 1: u = 1, log1p(-p) is clamped (v = 0)
            assert float(row[j0]) == pytest.approx(-float(outside[j0]) / 12, abs=tol)
            assert float(row[j0 + 1]) == pytest.approx(float(inside[j0 + 1]) / 12, abs=tol)
            # p = 1e-45: subnormal and below exp(-100), u = 0;  p = 1e-30: u = 1e30, v = 1
            assert float(row[j0 + 2]) == pytest.approx(-float(outside[j0 + 2]) / 12, abs=tol)
            assert float(row[j0 + 3]) == pytest.approx(float(inside[j0 + 3]) * 1e30 / 12 - float(outside[j0 + 3]) / 12, abs=tol * 1e30)
            assert abs(float(row[j0 + 3])) > 1e20                                        # (the large derivative is really there)


def test_refusals_of_the_model():
    key, tonic, labels, _ = heads(2, 3, 15)
    with pytest.raises(ValueError, match="labels"):
        metrics.key_sequence_loss(key, tonic, labels[:, :2], default_trans())
    with pytest.raises(ValueError, match=r"\(R, W, 12\)"):
        metrics.key_sequence_loss(key[0], tonic[0], labels[0], default_trans())
    bad = default_trans().clone()
    bad[0, 1] = -math.inf
    with pytest.raises(ValueError, match="finite"):
        metrics.key_sequence_loss(key, tonic, labels, bad)


def test_the_cpu_function_is_differentiable_by_its_closed_form():
    """Off the device ake_amd.key_sequence_loss runs the model; its backward hands out the stored gradients times the upstream scalar."""
    c = CASES["issue"]
    key, tonic, labels, A, _ = make_case(c)
    out = metrics.key_sequence_loss(key, tonic, labels, A, counts=c["counts"])
    k, t, a = key.clone().requires_grad_(), tonic.clone().requires_grad_(), A.clone().requires_grad_()
    loss = ake_amd.key_sequence_loss(k, t, labels, a, counts=c["counts"])
    assert loss.shape == () and float(loss) == float(out["loss"])
    (3.0 * loss).backward()
    assert torch.equal(k.grad, 3.0 * out["d_key"]) and torch.equal(t.grad, 3.0 * out["d_tonic"]) and torch.equal(a.grad, 3.0 * out["d_trans"])
    k2 = key.clone().requires_grad_()
    ake_amd.key_sequence_loss(k2, tonic, labels, A, counts=c["counts"]).backward()          # a transition that asks for no gradient
    assert torch.equal(k2.grad, out["d_key"])


# ---- sequence-mode batches: the host model of the positions, the labels, and the refusals ----

HOP, WF, SF, K = 4410, 76, 25, 4


def annotations(R):
    start = torch.tensor([[0, 200000, 500000], [0, 300000, 0], [0, 0, 0]][:R], dtype=torch.int64)
    key = torch.tensor([[3, -1, 17], [20, 8, 0], [5, 0, 0]][:R], dtype=torch.int32)
    count = torch.tensor([3, 2, 1][:R], dtype=torch.int32)
    return KeyAnnotations(start, key, count, 22050)


def test_sequence_positions_follow_the_draw_over_whole_sequences():
    frames = [301, 226, 100]                                                              # the last holds one window, not one sequence
    span = WF + (K - 1) * SF
    prefix = metrics.window_prefix(frames, span)
    assert prefix == [0, 301 - span + 1, 301 - span + 1 + 226 - span + 1, 301 - span + 1 + 226 - span + 1]
    rec0, start0, _ = metrics.draw_windows(prefix, 7, 2, 6, 3)
    rec, start = metrics.sequence_windows(prefix, 7, 2, 6, 3, K, SF)
    assert len(rec) == len(start) == 3 * K
    for s in range(3):
        assert rec[s * K:(s + 1) * K] == [rec0[s]] * K
        assert start[s * K:(s + 1) * K] == [start0[s] + k * SF for k in range(K)]
        assert rec0[s] in (0, 1) and start[(s + 1) * K - 1] + WF <= frames[rec0[s]]
    # slot i * batch_size + s is sequence s of batch i, however the slots are split into calls
    both = metrics.sequence_windows(prefix, 7, 2, 6, 2, K, SF), metrics.sequence_windows(prefix, 7, 2, 8, 1, K, SF)
    assert both[0][0] + both[1][0] == rec and both[0][1] + both[1][1] == start
    # key_id as the batches carry it: the window's key where its weight is positive, else -1
    ann = annotations(3)
    lab = metrics.window_labels(ann.seg_start, ann.seg_key, ann.seg_count, rec, start, HOP, WF)
    key_id = torch.where(lab["sample_weight"] > 0, lab["truth"], torch.full_like(lab["truth"], -1))
    assert bool(((key_id >= 0) == (lab["truth"] >= 0)).all())
    strict = metrics.window_labels(ann.seg_start, ann.seg_key, ann.seg_count, rec, start, HOP, WF, min_purity=1.0)
    impure = (strict["sample_weight"] == 0) & (strict["truth"] >= 0)
    assert bool((torch.where(strict["sample_weight"] > 0, strict["truth"], torch.full_like(strict["truth"], -1))[impure] == -1).all())


def test_track_windows_sequence_mode_and_its_refusals():
    mel = torch.zeros((3, 288, 301))
    ann = annotations(3)
    tw = ake_amd.TrackWindows(mel, [301, 226, 100], ann, HOP, WF, batch_size=2, stride_frames=SF, sequence_windows=K, log_trans=default_trans().float())
    assert tw.sequence_windows == K and tw._prefix.tolist() == metrics.window_prefix([301, 226, 100], WF + (K - 1) * SF)
    assert len(tw) == -(-(10 + 7 + 1) // (2 * K))                                         # the track's windows at this stride, once
    assert len(ake_amd.TrackWindows(mel, [301, 226, 100], ann, HOP, WF, batch_size=2, stride_frames=SF, sequence_windows=K,
                                    log_trans=default_trans().float(), batches_per_epoch=5)) == 5
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match="sequence_windows"):
            ake_amd.TrackWindows(mel, [301, 226, 100], ann, HOP, WF, stride_frames=SF, sequence_windows=bad, log_trans=default_trans())
    with pytest.raises(ValueError, match="stride"):
        ake_amd.TrackWindows(mel, [301, 226, 100], ann, HOP, WF, sequence_windows=K, log_trans=default_trans())
    with pytest.raises(ValueError, match="sequence"):
        ake_amd.TrackWindows(mel, [150, 100, 100], ann, HOP, WF, stride_frames=SF, sequence_windows=K, log_trans=default_trans())
    with pytest.raises(ValueError, match="log_trans"):
        ake_amd.TrackWindows(mel, [301, 226, 100], ann, HOP, WF, stride_frames=SF, sequence_windows=K)
    # without sequence_windows nothing changes: grid mode
    grid = ake_amd.TrackWindows(mel, [301, 226, 100], ann, HOP, WF, batch_size=4, stride_frames=SF)
    assert grid.sequence_windows is None and len(grid) == -(-(10 + 7 + 1) // 4)
