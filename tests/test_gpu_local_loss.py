"""PARITY (GPU): ake_general_step_local_f32 -- general_step's --local loss, its gradient with respect to the per-frame outputs and the
nine metrics (models.py:861-876, 898-909) over a ragged batch -- against the per-clip loop in float64 (autograd for the gradients),
and pinned on the reference-generated MIREX fixture (tests/golden/mirex_loss_cases.npz)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ake_amd
from ake_amd import _lib, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AKE_ERR_INVALID, AKE_ERR_WORKSPACE = -1, -4


def run(key, tonic, key_labels, tonic_labels, sig, valid, weights=(1.0, 1.0), grads=True):
    """-> (scalars[10], d_key, d_tonic) numpy straight through the C ABI; the gradient buffers start as NaN."""
    L = _lib.lib()
    dev = lambda t: (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))).to(DEV).contiguous()
    key, tonic, key_labels = dev(key).float(), dev(tonic).float(), dev(key_labels).float()
    tl, sl = dev(tonic_labels), dev(sig)
    n_dev = torch.tensor(valid, dtype=torch.int32, device=DEV)
    B, T, R = key.shape[0], key.shape[1], key_labels.shape[1]
    ws = torch.empty(L.ake_general_step_local_workspace_bytes(B, T), dtype=torch.uint8, device=DEV)
    scal = torch.full((10,), float("nan"), device=DEV)
    dk, dt = (torch.full((B, T, 12), float("nan"), device=DEV) for _ in range(2)) if grads else (None, None)
    p = lambda t: t.data_ptr() if t is not None else None
    i64 = lambda t: int(t.dtype == torch.int64)
    _lib.check(L.ake_general_step_local_f32(p(key), p(tonic), p(key_labels), p(tl), i64(tl), p(sl), i64(sl), p(n_dev), B, T, R,
                                            weights[0], weights[1], p(scal), p(dk), p(dt), p(ws), ws.numel(), None),
               "ake_general_step_local_f32")
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return n(scal), n(dk), n(dt)


def loop_f64(key, tonic, key_labels, tonic_labels, sig, valid, weights):
    """general_step's --local loop (models.py:861-876, 898-909) in float64 on the host: -> (10 values, d_key, d_tonic)."""
    key, tonic = key.double().requires_grad_(True), tonic.double().requires_grad_(True)
    kl, tl, sl = key_labels.double(), tonic_labels.long(), sig.double()
    t_idx = tl.argmax(2)
    B = key.shape[0]
    bce = ce = 0
    sums = [0.0] * 7
    acc_tonic = 0.0
    for i, n in enumerate(valid):
        bce = bce + F.binary_cross_entropy(key[i, :n], kl[i, :n])
        ce = ce + F.cross_entropy(tonic[i, :n], t_idx[i, :n])
        with torch.no_grad():
            sub = metrics.mirex_score(kl[i, :n], key[i, :n], tl[i, :n], tonic[i, :n], sl[i, :n])
            sums = [a + float(b) for a, b in zip(sums, sub)]
            acc_tonic += float((tonic[i, :n - 2].argmax(1) == t_idx[i, :n - 2]).double().mean())
    loss = weights[0] * bce / B + weights[1] * ce / B
    loss.backward()
    mirex, correct, fifths, relative, parallel, other, accuracy = (v / B for v in sums)
    vals = [float(loss.detach()), accuracy, mirex, correct, fifths, relative, parallel, other, acc_tonic / B, 0.0]
    return np.array(vals), key.grad.numpy(), tonic.grad.numpy()


def ragged_batch(seed, B, T, R, valid, i64):
    g = torch.Generator().manual_seed(seed)
    key = torch.rand((B, T, 12), generator=g) * 0.98 + 0.01
    tonic = torch.randn((B, T, 12), generator=g) * 2
    kid = torch.randint(0, 24, (B, R), generator=g)
    key_labels = ake_amd.KEY_SIGNATURE_MAP[torch.randint(0, 21, (B, R), generator=g)].clone()
    tonic_labels = F.one_hot(torch.randint(0, 12, (B, R), generator=g), 12)
    sig = F.one_hot(kid, 24)
    key[:, ::3] = key_labels[:, :T:3] * 0.9 + 0.05               # a third of the frames predict their label's scale
    tonic[:, ::2] += 6 * tonic_labels[:, :T:2]
    cast = (lambda t: t.long()) if i64 else (lambda t: t.float())
    tonic_labels, sig = cast(tonic_labels), cast(sig)
    # behind each clip's n frames: values that poison any read (the kernel must not look at them)
    for i, n in enumerate(valid):
        key[i, n:] = float("nan")
        tonic[i, n:] = float("nan")
        key_labels[i, n:] = float("nan")
        tonic_labels[i, n:] = 7
        sig[i, n:] = 5
    return key, tonic, key_labels, tonic_labels, sig


@pytest.mark.parametrize("i64", [False, True])
def test_ragged_batch_against_the_loop(i64):
    B, T = 5, 200
    R = T + 49
    valid = [T, T - 1, 3, 57, 120]
    weights = (1.0, 0.7)
    key, tonic, key_labels, tonic_labels, sig = ragged_batch(7 + i64, B, T, R, valid, i64)
    scal, dk, dt = run(key, tonic, key_labels, tonic_labels, sig, valid, weights)
    want, gk, gt = loop_f64(key, tonic, key_labels, tonic_labels, sig, valid, weights)
    assert abs(scal[0] - want[0]) < 3e-7 * abs(want[0]), (scal[0], want[0])
    assert np.abs(scal[1:] - want[1:]).max() < 1e-6, (scal[1:], want[1:])
    assert 0 < want[2] < 1 and want[4] > 0 and want[5] > 0                         # categories do occur
    for got, ref in ((dk, gk), (dt, gt)):
        for i, n in enumerate(valid):
            assert np.abs(got[i, :n] - ref[i, :n]).max() < 1e-6 * np.abs(ref[i, :n]).max(), i
            assert (got[i, n:] == 0).all() and not np.signbit(got[i, n:]).any()      # exact (+) zeros behind the clip
    again = run(key, tonic, key_labels, tonic_labels, sig, valid, weights)
    for a, b in zip((scal, dk, dt), again):
        assert a.tobytes() == b.tobytes()                                          # bit-reproducible


def test_without_gradient_buffers():
    B, T = 3, 130
    valid = [130, 64, 65]
    key, tonic, key_labels, tonic_labels, sig = ragged_batch(3, B, T, T, valid, True)
    scal, dk, dt = run(key, tonic, key_labels, tonic_labels, sig, valid, grads=False)
    assert dk is None and np.array_equal(scal, run(key, tonic, key_labels, tonic_labels, sig, valid)[0])


def test_reference_mirex_fixture_as_one_clip(gold_mirex):
    """The fixture's 96 labelled predictions as the 96 frames of one clip: the reference's batch MIREX scores, and the loss that
    ake_general_step_f32 gives on the same 96 rows."""
    g = gold_mirex
    kp, tp = g["key_preds"].astype(np.float32), g["tonic_preds"].astype(np.float32)
    scal, *_ = run(kp[None], tp[None], g["key_labels"][None], g["tonic_labels"][None], g["key_signature_id"][None], [96], grads=False)
    order = [2, 3, 4, 5, 6, 7, 1]          # fixture: mirex, correct, fifths, relative, parallel, other, accuracy
    assert np.allclose(scal[order], g["mirex"], atol=1e-7), (scal[order], g["mirex"])
    L = _lib.lib()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    key, tonic, kl, tl, sl = d(kp), d(tp), d(g["key_labels"]), d(g["tonic_labels"]), d(g["key_signature_id"])
    glob = torch.empty(10, device=DEV)
    _lib.check(L.ake_general_step_f32(key.data_ptr(), tonic.data_ptr(), None, kl.data_ptr(), tl.data_ptr(), 0, None, 0, sl.data_ptr(), 0,
                                      96, 1.0, 1.0, 0.1, 0, glob.data_ptr(), None, None, None, None), "ake_general_step_f32")
    glob = glob.cpu().numpy()
    assert abs(scal[0] - glob[0]) <= 3e-7 * abs(glob[0]), (scal[0], glob[0])
    assert np.allclose(scal[1:8], glob[1:8], atol=1e-7), (scal[1:8], glob[1:8])


def test_bad_arguments_are_refused():
    L = _lib.lib()
    B, T, R = 2, 70, 80
    key, tonic, kl, tl = (torch.zeros((B, T if i < 2 else R, 12), device=DEV) for i in range(4))
    sl = torch.zeros((B, R, 24), device=DEV)
    n_dev = torch.tensor([70, 21], dtype=torch.int32, device=DEV)
    need = L.ake_general_step_local_workspace_bytes(B, T)
    assert need >= B * 2 * 8 * 8 and L.ake_general_step_local_workspace_bytes(0, T) == 0 and L.ake_general_step_local_workspace_bytes(B, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    scal, dk, dt = torch.empty(10, device=DEV), torch.empty((B, T, 12), device=DEV), torch.empty((B, T, 12), device=DEV)
    ok = dict(key=key.data_ptr(), tonic=tonic.data_ptr(), kl=kl.data_ptr(), tl=tl.data_ptr(), tl64=0, sl=sl.data_ptr(), sl64=0,
              n=n_dev.data_ptr(), B=B, T=T, R=R, kw=1.0, tw=1.0, scal=scal.data_ptr(), dk=dk.data_ptr(), dt=dt.data_ptr(),
              ws=ws.data_ptr(), wsb=ws.numel())

    def call(**kw):
        a = dict(ok, **kw)
        return L.ake_general_step_local_f32(*a.values(), None)

    assert call() == 0
    torch.cuda.synchronize()
    for name in ("key", "tonic", "kl", "tl", "sl", "n", "scal", "ws"):
        assert call(**{name: None}) == AKE_ERR_INVALID, name
    for bad in (dict(B=0), dict(T=0), dict(R=0), dict(B=-3), dict(dk=None), dict(dt=None)):
        assert call(**bad) == AKE_ERR_INVALID, bad
    assert call(wsb=need - 1) == AKE_ERR_WORKSPACE
    assert b"general_step_local" in L.ake_last_error()
    assert call(dk=None, dt=None) == 0
    torch.cuda.synchronize()
