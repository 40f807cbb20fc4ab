"""Key-signature table and the MIREX key score, batched.

Same results as the reference's per-sample Python loop (``PitchClassNet.mirex_score``,
models.py:1065-1116, table utils/key_signatures.py:19-42) but evaluated for the whole batch
at once on whatever device the predictions live on (no per-sample table upload, models.py:1077).
"""
from __future__ import annotations

import math

import torch


def _build_table() -> torch.Tensor:
    # circle of fifths Cb .. C# (15 rows) + six enharmonic "theoretical" keys
    rows = []
    for i in range(15):
        tonic = (7 * (i - 7)) % 12
        rows.append([1.0 if ((pc - tonic) % 12) in (0, 2, 4, 5, 7, 9, 11) else 0.0 for pc in range(12)])
    rows += [rows[j] for j in (9, 11, 10, 4, 3, 5)]
    return torch.tensor(rows, dtype=torch.float32)


KEY_SIGNATURE_MAP = _build_table()      # (21, 12)


_tables = {}


def _device_table(dev, dtype):
    """The table on `dev`, uploaded once (the reference re-uploads it per sample, models.py:1077; a host-to-device copy per call
    also stalls the launch queue and cannot be captured into a graph)."""
    key = (str(dev), dtype)
    if key not in _tables:
        _tables[key] = KEY_SIGNATURE_MAP.to(device=dev, dtype=dtype)
    return _tables[key]


# major tonic (pitch class) of every table row: the circle of fifths, then the duplicates' own rows
MAJOR_TONIC = torch.tensor([(7 * (i - 7)) % 12 for i in list(range(15)) + [9, 11, 10, 4, 3, 5]], dtype=torch.int64)

_PITCH_NAMES = ("C", "Db", "D", "Eb", "E", "F", "Gb", "G", "Ab", "A", "Bb", "B")
# the project's 24-way key labels: 0-11 minor, 12-23 major, tonic = id mod 12 (KeyDataset.py:524-527; the same list as KeyDataset.SIGNATURE)
KEY_NAMES = tuple(f"{n} minor" for n in _PITCH_NAMES) + tuple(f"{n} major" for n in _PITCH_NAMES)


def _fma(x, y, z):
    """x * y + z rounded once, as a fused multiply-add rounds it.  float32: the product is exact in float64, the sum's rounding error is
    recovered (TwoSum), and where the float64 sum sits exactly halfway between two float32 values that error decides the direction,
    not the tie rule.  Other dtypes: x * y + z (float64 is the model's own precision)."""
    if x.dtype != torch.float32:
        return x * y + z
    a, q = x.double() * y.double(), z.double()
    s = a + q
    bb = s - a
    err = (a - (s - bb)) + (q - bb)
    r = s.float()
    other = torch.nextafter(r, torch.where(s > r.double(), torch.full_like(r, float("inf")), torch.full_like(r, float("-inf"))))
    halfway = (s - r.double()) == (other.double() - s)
    up, down = torch.nextafter(s, torch.full_like(s, float("inf"))), torch.nextafter(s, torch.full_like(s, float("-inf")))
    s = torch.where(halfway & (err > 0), up, torch.where(halfway & (err < 0), down, s))
    return s.float()


def decode_keys(key, tonic):
    """(..., 12) key outputs (sigmoid) and (..., 12) tonic logits -> (key_id, sig, tonic_id, confidence), shaped like the leading dims.

    The decode of ``ake_decode_keys_f32`` in torch ops, on whatever device the tensors live on: ``sig`` (0..20) is the first-maximum
    cosine match over ``KEY_SIGNATURE_MAP`` with ``mirex_score``'s arithmetic and tie rule, ``confidence`` that cosine, ``tonic_id``
    (0..11) the first maximum of the tonic logits, and ``key_id`` the 24-way label (``KEY_NAMES``): ``12 + tonic_id`` if the tonic is the
    major tonic of row ``sig``, ``tonic_id`` if it is that tonic + 9 mod 12 (the relative minor), -1 if signature and tonic disagree.
    ``key_id``, ``sig`` and ``tonic_id`` are int32.  On float32 inputs the sums run in the kernel's own order and every root and quotient is
    rounded once, so ``confidence`` equals the kernel's to the bit, on the CPU and on the device alike; float64 inputs give the model."""
    lead = key.shape[:-1]
    k2, t2 = key.reshape(-1, 12), tonic.reshape(-1, 12)
    # the cosines as sums over the 12 pitch classes in one order for every table row, so that the duplicate rows (0/12, 1/13, ...) get
    # bit-identical values and the first of them wins (a matmul may block the 21 columns differently and break such ties either way)
    # -- and in the kernel's own order, so that float32 inputs give the kernel's confidence to the bit.  Additions and products round alike
    # everywhere; the square roots and the quotient are taken in float64 and rounded once, which is the correctly rounded float32 result
    # (53 >= 2 * 24 + 2 bits).  |p|^2 as decode_keys_kernel's build takes it: the first two squares meet in one fused multiply-add,
    # fma(p_0, p_0, p_1 * p_1), the other ten are rounded and added in turn; a dot product is the sum of its row's members in turn.
    table = _device_table(k2.device, k2.dtype)
    eps = 1e-8
    wide = torch.float64 if k2.dtype == torch.float32 else k2.dtype
    col = lambda j: k2[:, j:j + 1]
    pp = _fma(col(0), col(0), col(1) * col(1))
    dot = k2.new_zeros((k2.shape[0], table.shape[0]))
    for j in range(12):
        if j >= 2:
            pp = pp + col(j) * col(j)
        dot = dot + col(j) * table[None, :, j]
    pn = pp.to(wide).sqrt().to(k2.dtype).clamp_min(eps)
    tn = table.to(wide).square().sum(dim=1, keepdim=True).sqrt().to(k2.dtype).clamp_min(eps)      # (sqrt(7): the sum is exact)
    sims = (dot.to(wide) / (pn * tn.T).to(wide)).to(k2.dtype)                  # (B, 21)
    conf = sims.max(dim=1).values
    idx21 = torch.arange(table.shape[0], device=k2.device)[None, :].expand_as(sims)
    sig = torch.where(sims == conf[:, None], idx21, torch.full_like(idx21, table.shape[0])).min(dim=1).values
    # first maximum of the logits (torch.argmax does not promise which of equal maxima it returns)
    is_max = t2 == t2.max(dim=1, keepdim=True).values
    idx = torch.arange(12, device=t2.device)[None, :].expand_as(t2)
    tonic_id = torch.where(is_max, idx, torch.full_like(idx, 12)).min(dim=1).values
    maj = MAJOR_TONIC.to(sig.device)[sig]
    key_id = torch.where(tonic_id == maj, 12 + tonic_id, torch.where(tonic_id == (maj + 9) % 12, tonic_id, torch.full_like(tonic_id, -1)))
    return (key_id.to(torch.int32).reshape(lead), sig.to(torch.int32).reshape(lead), tonic_id.to(torch.int32).reshape(lead),
            conf.reshape(lead))


def mirex_categories(key_labels, key_preds, tonic_labels, tonic_preds, key_signature_id):
    """-> (correct, fifths, relative, parallel, other, full): bool (B,) each, every prediction's MIREX category (at most one of the first
    five) and whether all 12 key bits are right.

    Category logic and its quirks follow models.py:1084-1114 exactly: the predicted key is the
    first-maximum cosine match over the 21-row table, ``diff`` compares that row index with the
    24-way label index, and the if-chain gives 'fifths' precedence.
    """
    dev = key_preds.device
    table = _device_table(dev, key_preds.dtype)
    eps = 1e-8
    pn = key_preds.norm(dim=1, keepdim=True).clamp_min(eps)
    tn = table.norm(dim=1, keepdim=True).clamp_min(eps)
    sims = (key_preds @ table.T) / (pn * tn.T)                               # (B, 21)
    # torch.argmax returns the first maximum on CPU and CUDA alike for exact ties only when
    # computed on identical values; duplicates rows (0/12, 1/13, ...) give bit-identical sims.
    pred_id = torch.argmax(sims, dim=1)
    first = torch.full_like(pred_id, table.shape[0])
    is_max = sims == sims.gather(1, pred_id[:, None])
    idx = torch.arange(table.shape[0], device=dev)[None, :].expand_as(sims)
    pred_id = torch.where(is_max, idx, first[:, None].expand_as(sims)).min(dim=1).values
    key_pred = table[pred_id]
    label_id = torch.argmax(key_signature_id, dim=1)
    correct_keys = (key_pred == key_labels.to(key_pred.dtype)).sum(dim=1)
    full = correct_keys == 12
    diff = (pred_id - label_id).abs()
    tonic_ok = torch.argmax(tonic_labels, dim=1) == torch.argmax(tonic_preds, dim=1)
    fifths = (diff == 1) & ~(tonic_ok & full)
    correct = tonic_ok & full & ~fifths
    relative = full & ~tonic_ok & ~fifths
    parallel = tonic_ok & ~full & ~fifths
    other = ~(fifths | correct | relative | parallel)
    return correct, fifths, relative, parallel, other, full


def mirex_score(key_labels, key_preds, tonic_labels, tonic_preds, key_signature_id):
    """-> (mirex, correct, fifths, relative, parallel, other, accuracy), float32 scalars: the shares of ``mirex_categories`` over the
    batch and their MIREX-weighted sum."""
    correct, fifths, relative, parallel, other, full = mirex_categories(key_labels, key_preds, tonic_labels, tonic_preds, key_signature_id)
    n = float(key_preds.shape[0])
    f = lambda m: (m.sum().float() / n).float()
    mirex = (1.0 * correct.sum() + 0.5 * fifths.sum() + 0.3 * relative.sum() + 0.2 * parallel.sum()).float() / n
    return mirex.float(), f(correct), f(fifths), f(relative), f(parallel), f(other), f(full)


# ---- a smooth key track: per-window log-scores of the 24 keys and a first-order Viterbi decode (ake_key_emissions_f32 / ake_viterbi_keys_f32) ----

_MAJOR_SCALE = (0, 2, 4, 5, 7, 9, 11)
# the major tonic whose scale key k uses (k in KEY_NAMES order): its own for a major key, tonic + 3 for a minor one
KEY_MAJOR_TONIC = tuple(k - 12 if k >= 12 else (k + 3) % 12 for k in range(24))
# S_k: (24, 12), 1 where pitch class j belongs to key k's scale
KEY_SCALES = torch.tensor([[1.0 if (j - m) % 12 in _MAJOR_SCALE else 0.0 for j in range(12)] for m in KEY_MAJOR_TONIC], dtype=torch.float64)


def _behind_count(counts, R, W, device):
    """(R, W) bool: window w of recording r lies at or behind counts[r]."""
    counts = torch.as_tensor(counts, device=device).to(torch.int64).reshape(R)
    return torch.arange(W, device=device)[None, :] >= counts[:, None]


def key_emissions(key, tonic, signature_weight=1.0, counts=None):
    """(..., 12) key outputs (sigmoid memberships) and (..., 12) tonic logits -> (..., 24) log-scores of the 24 keys (``KEY_NAMES`` order).

    The arithmetic of ``ake_key_emissions_f32`` in torch ops, in the tensors' dtype (float64 inputs give the test model).  The key head is
    trained with BCE and the tonic head with cross-entropy, so with p = key and S_k the scale of key k (``KEY_SCALES``)::

        e[k] = log_softmax(tonic)[k mod 12] + signature_weight / 12 * sum_j (S_k[j] * max(log p_j, -100) + (1 - S_k[j]) * max(log1p(-p_j), -100))

    (-100 is ``nn.BCELoss``'s clamp).  ``counts`` (R,) with inputs shaped (R, W, 12): windows at index >= ``counts[r]`` get zeros."""
    inside = torch.log(key).clamp_min(-100.0)
    outside = torch.log1p(-key).clamp_min(-100.0)
    S = KEY_SCALES.to(device=key.device, dtype=key.dtype)
    sig = (S * inside[..., None, :] + (1.0 - S) * outside[..., None, :]).sum(dim=-1)          # (..., 24)
    ls = torch.log_softmax(tonic, dim=-1)
    e = torch.cat([ls, ls], dim=-1) + (float(signature_weight) / 12.0) * sig
    if counts is not None:
        if key.dim() != 3:
            raise ValueError("key_emissions: counts needs inputs shaped (R, W, 12)")
        e = torch.where(_behind_count(counts, key.shape[0], key.shape[1], key.device)[..., None], torch.zeros_like(e), e)
    return e


def _check_finite(name, t):
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} must be finite: write a forbidden transition as a large negative number (say -1e4), not as -inf "
                         "(the recurrence subtracts each step's maximum, and max - max of infinities is NaN)")


def viterbi_keys(emissions, log_trans, log_prior=None, counts=None):
    """The most likely key path through (R, W, 24) or (W, 24) ``emissions`` -> int32 (R, W) or (W,).

    ``log_trans`` (24, 24): log-probability of moving from key i (row) to key j; ``log_prior`` (24,), default zeros; ``counts`` (R,):
    recording r has ``counts[r]`` windows (clamped to 0..W), the path holds -1 behind them.  The recurrence of ``ake_viterbi_keys_f32``,
    operation for operation, in the emissions' dtype -- additions, subtractions and comparisons only, so the float32 run on the host is
    bit-identical to the kernel's::

        d_0[j] = prior[j] + e[0][j]
        m[j]   = max_i (d_{w-1}[i] + A[i][j]),  bp_w[j] = the smallest i that attains it,  d_w[j] = m[j] + e[w][j]
        d_w[j] -= max_j d_w[j]                  (every step, w = 0 included)

    The last state is the smallest j attaining max d; the path follows bp backwards."""
    single = emissions.dim() == 2
    e = emissions[None] if single else emissions
    if e.dim() != 3 or e.shape[2] != 24:
        raise ValueError(f"viterbi_keys: emissions must be (R, W, 24) or (W, 24), got {tuple(emissions.shape)}")
    R, W, K = e.shape
    dev = e.device
    A = torch.as_tensor(log_trans).to(device=dev, dtype=e.dtype)
    if A.shape != (K, K):
        raise ValueError(f"viterbi_keys: log_trans must be (24, 24), got {tuple(A.shape)}")
    prior = torch.zeros(K, device=dev, dtype=e.dtype) if log_prior is None else torch.as_tensor(log_prior).to(device=dev, dtype=e.dtype).reshape(K)
    _check_finite("log_trans", A)
    _check_finite("log_prior", prior)
    n = torch.full((R,), W, device=dev, dtype=torch.int64) if counts is None else \
        torch.as_tensor(counts, device=dev).to(torch.int64).reshape(R).clamp(0, W)
    path = torch.full((R, W), -1, device=dev, dtype=torch.int64)
    idx = torch.arange(K, device=dev)
    none = torch.full((), K, device=dev, dtype=torch.int64)
    d = torch.zeros((R, K), device=dev, dtype=e.dtype)
    last = torch.zeros((R,), device=dev, dtype=torch.int64)
    bps = torch.zeros((W, R, K), device=dev, dtype=torch.int64)
    for w in range(W):
        if w == 0:
            raw = prior[None, :] + e[:, 0]
        else:
            cand = d[:, :, None] + A[None, :, :]                                    # (R, from i, to j)
            m = cand.max(dim=1).values
            bps[w] = torch.where(cand == m[:, None, :], idx[None, :, None], none).min(dim=1).values
            raw = m + e[:, w]
        mx = raw.max(dim=1, keepdim=True).values
        dn = raw - mx
        d = torch.where((w < n)[:, None], dn, d)
        first = torch.where(dn == dn.max(dim=1, keepdim=True).values, idx[None, :], none).min(dim=1).values
        last = torch.where(n == w + 1, first, last)
    cur = last
    for w in range(W - 1, -1, -1):
        live = w < n
        path[:, w] = torch.where(live, cur, torch.full_like(cur, -1))
        if w > 0:
            cur = torch.where(live, bps[w].gather(1, cur[:, None])[:, 0], cur)
    path = path.to(torch.int32)
    return path[0] if single else path


def key_transition_log(stay, fifth=0.5, relative=0.3, parallel=0.2, other=0.02):
    """(24, 24) float64 log transition matrix between the 24 keys (``KEY_NAMES`` order), from key i (row) to key j.

    The diagonal is ``stay``.  The off-diagonal weights of a row are the MIREX weights ``mirex_score`` uses -- ``fifth``: same mode, tonic
    +-7; ``relative``: major t <-> minor t + 9; ``parallel``: same tonic, other mode; ``other``: every other key -- normalised to
    ``1 - stay``, so every row sums to 1 before the logarithm.  The matrix is symmetric."""
    stay = float(stay)
    if not 0.0 < stay < 1.0:
        raise ValueError(f"key_transition_log: stay must lie strictly between 0 and 1, got {stay}")
    if min(fifth, relative, parallel, other) <= 0.0:
        raise ValueError("key_transition_log: the weights must be positive (a zero weight is a forbidden transition, whose logarithm is "
                         "-inf: use a small positive weight instead)")
    Wt = torch.full((24, 24), float(other), dtype=torch.float64)
    for i in range(24):
        major, t = divmod(i, 12)
        Wt[i, 12 * major + (t + 7) % 12] = Wt[i, 12 * major + (t + 5) % 12] = float(fifth)
        Wt[i, (t + 9) % 12 if major else 12 + (t + 3) % 12] = float(relative)
        Wt[i, 12 * (1 - major) + t] = float(parallel)
        Wt[i, i] = 0.0
    # every row holds the same weights (2 fifths, 1 relative, 1 parallel, 19 others): one scale for all, so P is symmetric to the bit
    P = Wt * ((1.0 - stay) / (2.0 * float(fifth) + float(relative) + float(parallel) + 19.0 * float(other)))
    P[torch.arange(24), torch.arange(24)] = stay
    return torch.log(P)


# ---- posterior key probabilities and a fitted transition: forward-backward over the emissions (ake_key_posteriors_f32) and EM on top ----

def key_posteriors(emissions, log_trans, log_prior=None, counts=None, transitions=False):
    """Posterior marginals of the 24 keys at every window of (R, W, 24) or (W, 24) ``emissions`` -> ``(post, loglik)``, or
    ``(post, loglik, xi_sum)`` with ``transitions=True``.

    ``log_trans``, ``log_prior`` and ``counts`` as in ``viterbi_keys``, all finite.  The recurrence of ``ake_key_posteriors_f32`` in torch
    ops, in the emissions' dtype (float64 inputs give the test model), for a recording of n = count windows, LSE = log-sum-exp::

        a_0[j] = prior[j] + e[0][j]
        a_w[j] = e[w][j] + LSE_i (a_{w-1}[i] + A[i][j])
        c_w = LSE_j a_w[j];  a_w[j] -= c_w                                  (every step, w = 0 included)
        b_{n-1}[i] = 0
        b_w[i] = LSE_j (A[i][j] + e[w+1][j] + b_{w+1}[j]);  b_w[i] -= LSE_i b_w[i]
        post_w[j]  = softmax_j (a_w[j] + b_w[j])
        xi_w[i][j] = softmax over all 576 (i, j) of (a_{w-1}[i] + A[i][j] + e[w][j] + b_w[j])      w = 1..n-1

    ``post`` (R, W, 24): every row below the count sums to 1, rows at or behind it are zeros.  ``loglik`` (R,) = sum_w c_w, 0 for a count
    of 0.  The emissions are log-scores, not normalised likelihoods, so ``loglik`` is a log-score of the recording under ``log_trans``:
    the quantity ``fit_key_transition`` raises, and no more than that.  ``xi_sum`` (R, 24, 24) = sum_w xi_w: the expected number of
    moves from key i to key j, n - 1 in all, zeros for counts 0 and 1."""
    single = emissions.dim() == 2
    e = emissions[None] if single else emissions
    if e.dim() != 3 or e.shape[2] != 24:
        raise ValueError(f"key_posteriors: emissions must be (R, W, 24) or (W, 24), got {tuple(emissions.shape)}")
    R, W, K = e.shape
    dev = e.device
    A = torch.as_tensor(log_trans).to(device=dev, dtype=e.dtype)
    if A.shape != (K, K):
        raise ValueError(f"key_posteriors: log_trans must be (24, 24), got {tuple(A.shape)}")
    prior = torch.zeros(K, device=dev, dtype=e.dtype) if log_prior is None else torch.as_tensor(log_prior).to(device=dev, dtype=e.dtype).reshape(K)
    _check_finite("log_trans", A)
    _check_finite("log_prior", prior)
    _check_finite("emissions", e)
    n = torch.full((R,), W, device=dev, dtype=torch.int64) if counts is None else \
        torch.as_tensor(counts, device=dev).to(torch.int64).reshape(R).clamp(0, W)
    a, b, c = e.new_zeros((R, W, K)), e.new_zeros((R, W, K)), e.new_zeros((R, W))
    for w in range(W):
        raw = prior[None, :] + e[:, 0] if w == 0 else e[:, w] + torch.logsumexp(a[:, w - 1, :, None] + A[None, :, :], dim=1)
        c[:, w] = torch.logsumexp(raw, dim=1)
        a[:, w] = raw - c[:, w, None]
    for w in range(W - 2, -1, -1):                                                  # (b stays 0 at w >= n - 1)
        raw = torch.logsumexp(A[None, :, :] + (e[:, w + 1] + b[:, w + 1])[:, None, :], dim=2)
        raw = raw - torch.logsumexp(raw, dim=1, keepdim=True)
        b[:, w] = torch.where((w < n - 1)[:, None], raw, torch.zeros_like(raw))
    live = torch.arange(W, device=dev)[None, :] < n[:, None]                        # (R, W)
    post = torch.where(live[..., None], torch.softmax(a + b, dim=2), torch.zeros_like(a))
    loglik = torch.where(live, c, torch.zeros_like(c)).sum(dim=1)
    if single:
        post, loglik = post[0], loglik[0]
    if not transitions:
        return post, loglik
    xi_sum = e.new_zeros((R, K, K))
    for w0 in range(1, W, 256):                                                     # (a chunk of windows at a time bounds the memory)
        w1 = min(w0 + 256, W)
        x = a[:, w0 - 1:w1 - 1, :, None] + A[None, None, :, :] + e[:, w0:w1, None, :] + b[:, w0:w1, None, :]
        xi = torch.softmax(x.reshape(R, w1 - w0, K * K), dim=2).reshape(R, w1 - w0, K, K)
        xi_sum += torch.where(live[:, w0:w1, None, None], xi, torch.zeros_like(xi)).sum(dim=1)
    return post, loglik, (xi_sum[0] if single else xi_sum)


# ---- a smoother that carries its state: the filtered scores and a fixed-lag path, window by window (ake_key_stream_step_f32) ----

def key_stream_count(windows_before, k, lag, flush):
    """Windows whose fixed-lag label a step over ``k`` new windows writes, after ``windows_before`` earlier ones -> ``(first, k_out)``:
    window v leaves the lag once window v + lag has been stepped, and a flush writes every window that is left."""
    windows_before, k, lag = int(windows_before), int(k), int(lag)
    first = max(0, windows_before - lag)
    total = windows_before + k
    return first, (total if flush else max(0, total - lag)) - first


def key_stream(emissions, log_trans, log_prior=None, lag=6, state=None, flush=True, return_state=False):
    """Filtered key scores and the fixed-lag Viterbi path of (R, W, 24) or (W, 24) ``emissions`` -> ``(filtered, path)``.

    The host model of ``ake_key_stream_step_f32``, in torch ops, in the emissions' dtype.  ``log_trans`` and ``log_prior`` as in
    ``viterbi_keys``, all finite; ``lag`` 0..255.

    ``filtered[w]`` is ``key_posteriors``' normalised forward row a_w (the same recurrence, c_w subtracted at every step, w = 0 included):
    ``exp`` of it is the probability of each key given the windows up to w.  ``path[v]`` is ``viterbi_keys(e[:v + lag + 1])[v]``: the
    label window v gets once ``lag`` more windows have been seen -- the Viterbi step of ``viterbi_keys``, operation for operation, then
    ``lag`` back-pointers followed from the first maximum of d_{v + lag}.  With ``flush`` (the recording ends here) the last ``lag``
    windows get ``viterbi_keys(e)[v]``.  One forward sweep; the back-pointers of the last ``lag`` windows live in a ring.

    In pieces: ``state`` is what an earlier call returned with ``return_state=True`` (the call then returns ``(filtered, path, state)``),
    and ``flush=False`` leaves the last ``lag`` windows to a later call.  ``path`` then holds the ``key_stream_count`` windows this call
    decides, in order, int32 (R, k_out); the results do not depend on how the windows are cut into calls, to the bit."""
    single = emissions.dim() == 2
    e = emissions[None] if single else emissions
    if e.dim() != 3 or e.shape[2] != 24:
        raise ValueError(f"key_stream: emissions must be (R, W, 24) or (W, 24), got {tuple(emissions.shape)}")
    lag = int(lag)
    if not 0 <= lag <= 255:
        raise ValueError(f"key_stream: lag must lie in 0..255, got {lag}")
    R, W, K = e.shape
    dev = e.device
    A = torch.as_tensor(log_trans).to(device=dev, dtype=e.dtype)
    if A.shape != (K, K):
        raise ValueError(f"key_stream: log_trans must be (24, 24), got {tuple(A.shape)}")
    prior = torch.zeros(K, device=dev, dtype=e.dtype) if log_prior is None else torch.as_tensor(log_prior).to(device=dev, dtype=e.dtype).reshape(K)
    _check_finite("log_trans", A)
    _check_finite("log_prior", prior)
    _check_finite("emissions", e)
    idx = torch.arange(K, device=dev)
    none = torch.full((), K, device=dev, dtype=torch.int64)
    if state is None:
        before = 0
        d, a = e.new_zeros((R, K)), e.new_zeros((R, K))
        ring = torch.zeros((max(lag, 1), R, K), device=dev, dtype=torch.int64)       # row w % lag: bp_w
    else:
        before, d, a, ring = state["windows"], state["d"].clone(), state["a"].clone(), state["ring"].clone()
    first_out, k_out = key_stream_count(before, W, lag, flush)
    filtered = e.new_zeros((R, W, K))
    path = torch.full((R, k_out), -1, device=dev, dtype=torch.int64)

    def first_max(x):
        return torch.where(x == x.max(dim=1, keepdim=True).values, idx[None, :], none).min(dim=1).values

    for i in range(W):
        w = before + i
        if w == 0:
            raw = prior[None, :] + e[:, 0]
            fraw = prior[None, :] + e[:, 0]
        else:
            cand = d[:, :, None] + A[None, :, :]                                    # (R, from i, to j)
            m = cand.max(dim=1).values
            if lag:
                ring[w % lag] = torch.where(cand == m[:, None, :], idx[None, :, None], none).min(dim=1).values
            raw = m + e[:, i]
            fraw = e[:, i] + torch.logsumexp(a[:, :, None] + A[None, :, :], dim=1)
        d = raw - raw.max(dim=1, keepdim=True).values
        a = fraw - torch.logsumexp(fraw, dim=1, keepdim=True)
        filtered[:, i] = a
        if w >= lag:
            cur = first_max(d)
            for back in range(lag):
                cur = ring[(w - back) % lag].gather(1, cur[:, None])[:, 0]
            path[:, w - lag - first_out] = cur
    total = before + W
    if flush and total > 0:
        cur = first_max(d)
        for v in range(total - 1, max(0, total - lag) - 1, -1):
            path[:, v - first_out] = cur
            if v > max(0, total - lag):
                cur = ring[v % lag].gather(1, cur[:, None])[:, 0]
    path = path.to(torch.int32)
    if single:
        filtered, path = filtered[0], path[0]
    if return_state:
        return filtered, path, {"windows": total, "d": d, "a": a, "ring": ring}
    return filtered, path


def key_stream_posteriors(emissions, log_trans, log_prior=None, lag=6, state=None, flush=True, return_state=False, path=None):
    """Fixed-lag posteriors and the running log-likelihood of (R, W, 24) or (W, 24) ``emissions`` -> ``(post, loglik)``, or
    ``(post, loglik, path_post)`` with ``path``.

    The host model of ``ake_key_stream_posteriors_f32``, in torch ops, in the emissions' dtype.  ``log_trans``, ``log_prior`` and ``lag``
    as in ``key_stream``.  With a_u ``key_stream``'s ``filtered`` rows and c_u what their steps subtract, window v's row is the posterior
    given everything up to its end window s = v + lag (with ``flush``, for the windows still inside the lag: the last window)::

        b_s[i] = 0
        b_u[i] = LSE_j (A[i][j] + e[u+1][j] + b_{u+1}[j]);  b_u[i] -= LSE_i b_u[i]        u = s-1 .. v
        post[v][j] = softmax_j (a_v[j] + b_v[j])

    which is ``key_posteriors(e[:s + 1])[0][v]``: the evidence ``key_stream``'s label of window v was decided on.  ``post`` (R, k_out, 24)
    holds the ``key_stream_count`` windows this call decides, as ``key_stream``'s path does; with ``lag`` 0 it is ``softmax(filtered)``.
    ``loglik`` (R, W): ``loglik[w]`` = sum of c_u up to window w = ``key_posteriors(e[:w + 1])[1]``, added in a float64 and rounded to
    the emissions' dtype on the way out.  ``path`` (R, k_out) or (k_out,), ``key_stream``'s path of the same call: ``path_post[v]`` =
    ``post[v][path[v]]``, 0 where the path holds -1.

    In pieces: ``state`` and ``return_state`` as in ``key_stream`` (the state: the last ``lag`` rows of e and of a, row w % lag for
    window w -- one row for lag 0 --, and the float64 sum); the results do not depend on how the windows are cut into calls, to the
    bit."""
    single = emissions.dim() == 2
    e = emissions[None] if single else emissions
    if e.dim() != 3 or e.shape[2] != 24:
        raise ValueError(f"key_stream_posteriors: emissions must be (R, W, 24) or (W, 24), got {tuple(emissions.shape)}")
    lag = int(lag)
    if not 0 <= lag <= 255:
        raise ValueError(f"key_stream_posteriors: lag must lie in 0..255, got {lag}")
    R, W, K = e.shape
    dev = e.device
    A = torch.as_tensor(log_trans).to(device=dev, dtype=e.dtype)
    if A.shape != (K, K):
        raise ValueError(f"key_stream_posteriors: log_trans must be (24, 24), got {tuple(A.shape)}")
    prior = torch.zeros(K, device=dev, dtype=e.dtype) if log_prior is None else torch.as_tensor(log_prior).to(device=dev, dtype=e.dtype).reshape(K)
    _check_finite("log_trans", A)
    _check_finite("log_prior", prior)
    _check_finite("emissions", e)
    rows = max(lag, 1)
    if state is None:
        before = 0
        e_ring, a_ring = e.new_zeros((rows, R, K)), e.new_zeros((rows, R, K))       # row w % rows: e_w, a_w
        ll = torch.zeros((R,), device=dev, dtype=torch.float64)
    else:
        before, e_ring, a_ring, ll = state["windows"], state["e"].clone(), state["a"].clone(), state["loglik"].clone()
    first_out, k_out = key_stream_count(before, W, lag, flush)
    if path is not None:
        path = torch.as_tensor(path, device=dev).to(torch.int64)
        path = path[None] if single and path.dim() == 1 else path
        if tuple(path.shape) != (R, k_out):
            raise ValueError(f"key_stream_posteriors: path must hold the {k_out} windows this call decides, got {tuple(path.shape)}")
    total = before + W
    e_at = {u: e_ring[u % rows] for u in range(max(0, before - lag), before)}       # the rows a sweep may read, by window
    a_at = {u: a_ring[u % rows] for u in range(max(0, before - lag), before)}
    a = a_ring[(before - 1) % rows] if before > 0 else None
    loglik = e.new_zeros((R, W))
    for i in range(W):
        w = before + i
        fraw = prior[None, :] + e[:, 0] if w == 0 else e[:, i] + torch.logsumexp(a[:, :, None] + A[None, :, :], dim=1)
        c = torch.logsumexp(fraw, dim=1)
        a = fraw - c[:, None]
        ll = ll + c.double()
        loglik[:, i] = ll.to(e.dtype)
        e_at[w], a_at[w] = e[:, i], a
    post = e.new_zeros((R, k_out, K))
    for v in range(first_out, first_out + k_out):                                  # one sweep per written window, each on its own
        b = e.new_zeros((R, K))
        for u in range(min(v + lag, total - 1) - 1, v - 1, -1):
            raw = torch.logsumexp(A[None, :, :] + (e_at[u + 1] + b)[:, None, :], dim=2)
            b = raw - torch.logsumexp(raw, dim=1, keepdim=True)
        post[:, v - first_out] = torch.softmax(a_at[v] + b, dim=1)
    for w in range(max(before, total - rows), total):
        e_ring[w % rows], a_ring[w % rows] = e_at[w], a_at[w]
    out = [post, loglik]
    if path is not None:
        out.append(torch.where(path >= 0, post.gather(2, path.clamp(min=0)[..., None])[..., 0], torch.zeros_like(post[..., 0])))
    if single:
        out = [t[0] for t in out]
    if return_state:
        out.append({"windows": total, "e": e_ring, "a": a_ring, "loglik": ll})
    return tuple(out)


def _transposition_classes():
    """(24, 24) int64: the class 0..47 of cell (i, j) under transposition -- (mode of i, mode of j, (t_j - t_i) mod 12); 12 cells each."""
    k = torch.arange(24)
    mode, t = k // 12, k % 12
    return (mode[:, None] * 2 + mode[None, :]) * 12 + (t[None, :] - t[:, None]) % 12


def transition_m_step(xi_sum, init_log, tied=True, pseudo_count=1.0):
    """The M-step of the transition fit: expected transition counts -> float64 (24, 24) log matrix, from key i (row) to key j.

    ``C`` = ``xi_sum`` ((24, 24), or (R, 24, 24) summed over the recordings) + ``pseudo_count * exp(init_log)``: ``pseudo_count``
    pseudo-transitions per row, spread as ``init``, so ``C`` stays positive and the result finite.  ``tied``: every cell of ``C`` is
    replaced by the mean over its transposition class -- the cells (i', j') with the modes of i and j and the same tonic interval
    ``(t_j - t_i) mod 12``: 48 classes of 12 cells -- so the matrix depends on the interval moved, not on the key left.  The result is
    ``log(C / rowsum(C))``."""
    xi = torch.as_tensor(xi_sum).detach().to(device="cpu", dtype=torch.float64)
    if xi.dim() == 3:
        xi = xi.sum(dim=0)
    init = torch.as_tensor(init_log).detach().to(device="cpu", dtype=torch.float64)
    if xi.shape != (24, 24) or init.shape != (24, 24):
        raise ValueError(f"transition_m_step: xi_sum must be (24, 24) or (R, 24, 24) and init_log (24, 24), got {tuple(xi.shape)} and {tuple(init.shape)}")
    _check_finite("xi_sum", xi)
    _check_finite("init_log", init)
    if float(pseudo_count) < 0.0:
        raise ValueError("transition_m_step: pseudo_count must not be negative")
    C = xi + float(pseudo_count) * torch.exp(init)
    if tied:
        cls = _transposition_classes().reshape(-1)
        mean = torch.zeros(48, dtype=torch.float64).index_add_(0, cls, C.reshape(-1)) / 12.0
        C = mean[cls].reshape(24, 24)
    return torch.log(C / C.sum(dim=1, keepdim=True))


def fit_key_transition(emissions, counts=None, init=None, iterations=10, tied=True, pseudo_count=1.0, log_prior=None, e_step=None):
    """Fit the transition matrix to recordings' own emissions by EM (Baum-Welch with the emissions held fixed) ->
    ``(log_trans, log_likelihoods)``.

    ``emissions``: one (R, W, 24) or (W, 24) tensor or a list of them, ``counts`` matching (one per tensor, or None).  ``init``: the
    (24, 24) log matrix to start from, default ``key_transition_log(stay=0.9)``; it also spreads the M-step's pseudo-counts
    (``transition_m_step``).  Every iteration runs ``e_step(emissions_k, log_trans, log_prior, counts_k)`` -> ``(loglik, xi_sum)`` on
    every tensor -- default: ``key_posteriors`` -- and then one M-step.  ``log_trans`` is float64 (24, 24); ``log_likelihoods`` holds one
    float per iteration: the summed score of all recordings under the matrix that ENTERED that iteration, which EM does not lower.
    No accuracy claim goes with the fitted matrix: it is the matrix under which these emissions score highest, and no more."""
    batches = list(emissions) if isinstance(emissions, (list, tuple)) else [emissions]
    if not batches:
        raise ValueError("fit_key_transition: no emissions")
    if counts is None:
        cnts = [None] * len(batches)
    elif isinstance(emissions, (list, tuple)):
        cnts = list(counts)
        if len(cnts) != len(batches):
            raise ValueError(f"fit_key_transition: {len(batches)} emission tensors but {len(cnts)} counts")
    else:
        cnts = [counts]
    if int(iterations) < 1:
        raise ValueError("fit_key_transition: iterations must be at least 1")
    init = key_transition_log(stay=0.9) if init is None else torch.as_tensor(init).detach().to(device="cpu", dtype=torch.float64)
    if init.shape != (24, 24):
        raise ValueError(f"fit_key_transition: init must be (24, 24), got {tuple(init.shape)}")
    _check_finite("init", init)
    if e_step is None:
        def e_step(e, log_trans, prior, cnt):
            _, ll, xi = key_posteriors(e, log_trans, log_prior=prior, counts=cnt, transitions=True)
            return ll, xi
    log_trans, scores = init.clone(), []
    for _ in range(int(iterations)):
        xi_total, score = torch.zeros((24, 24), dtype=torch.float64), 0.0
        for e, cnt in zip(batches, cnts):
            ll, xi = e_step(e, log_trans, log_prior, cnt)
            xi = xi.detach().to(device="cpu", dtype=torch.float64)
            xi_total += xi.sum(dim=0) if xi.dim() == 3 else xi
            score += float(ll.detach().to(device="cpu", dtype=torch.float64).sum())
        scores.append(score)
        log_trans = transition_m_step(xi_total, init, tied=tied, pseudo_count=pseudo_count)
    return log_trans, scores


# ---- a key track against key annotations (ake_track_score_i32) and a transition counted from labels ----

# category codes of track_score: the relations key_transition_log uses, and their MIREX weights
SCORE_CATEGORIES = ("correct", "fifth", "relative", "parallel", "other", "undecoded")
SCORE_WEIGHTS = (1.0, 0.5, 0.3, 0.2, 0.0, 0.0)
_I64_MAX = 2 ** 63 - 1


def _window_spans(W, hop, window_frames, stride_frames, device):
    """(lo, hi, centre) int64 (W,): the first, last and centre sample of every window (frame f is centred on sample f * hop)."""
    f0 = torch.arange(W, device=device, dtype=torch.int64) * int(stride_frames)
    hop, wf = int(hop), int(window_frames)
    return f0 * hop, (f0 + wf - 1) * hop, torch.div((2 * f0 + wf - 1) * hop, 2, rounding_mode="floor")


def window_truth(seg_start, seg_key, seg_count, windows, hop, window_frames, stride_frames, counts=None):
    """The annotated key of every window -> ``(truth, pure)``: int32 (R, W) and bool (R, W), on the annotations' device.

    ``seg_start`` int64 (R, S) in samples, ``seg_key`` int32 (R, S) (-1 = unlabelled), ``seg_count`` (R,): the arrays of
    ``KeyAnnotations``.  Window w covers the samples ``w * stride_frames * hop .. (w * stride_frames + window_frames - 1) * hop``
    inclusive; its centre sample is ``(2 * w * stride_frames + window_frames - 1) * hop // 2`` (``KeyTrack.times`` in samples).
    ``truth`` is the key of the last segment that starts at or before the centre sample: -1 for windows at or behind ``counts[r]``, in an
    unlabelled segment, or in a recording without segments.  ``pure``: the truth is a key and every segment that overlaps the window's
    samples carries it.  Integer torch ops, exact: the restatement of ``ake_track_score_i32``'s geometry."""
    dev = seg_start.device
    R, S = seg_start.shape
    W = int(windows)
    start = seg_start.to(torch.int64)
    key = seg_key.to(device=dev, dtype=torch.int64)
    ns = torch.as_tensor(seg_count, device=dev).to(torch.int64).reshape(R).clamp(0, S)
    lo, hi, centre = _window_spans(W, hop, window_frames, stride_frames, dev)
    s_idx = torch.arange(S, device=dev)
    valid = s_idx[None, :] < ns[:, None]                                                            # (R, S)
    holds = valid[:, None, :] & (start[:, None, :] <= centre[None, :, None])                        # (R, W, S)
    last = (holds * (s_idx + 1)[None, None, :]).amax(dim=2) - 1 if S > 0 else torch.full((R, W), -1, device=dev, dtype=torch.int64)
    truth = torch.where(last >= 0, key.gather(1, last.clamp_min(0)), torch.full_like(last, -1))
    n = torch.full((R,), W, device=dev, dtype=torch.int64) if counts is None else \
        torch.as_tensor(counts, device=dev).to(torch.int64).reshape(R).clamp(0, W)
    truth = torch.where(torch.arange(W, device=dev)[None, :] < n[:, None], truth, torch.full_like(truth, -1))
    nxt = torch.cat([start[:, 1:], torch.full((R, 1), _I64_MAX, device=dev, dtype=torch.int64)], dim=1)
    nxt = torch.where(s_idx[None, :] + 1 < ns[:, None], nxt, torch.full_like(nxt, _I64_MAX))         # the last segment has no end
    overlaps = valid[:, None, :] & (start[:, None, :] <= hi[None, :, None]) & (nxt[:, None, :] > lo[None, :, None])
    pure = (truth >= 0) & (~overlaps | (key[:, None, :] == truth[:, :, None])).all(dim=2)
    return truth.to(torch.int32), pure


def key_category(pred, truth):
    """Category 0..5 (``SCORE_CATEGORIES``) of decoded keys ``pred`` (-1..23) against true keys ``truth`` (0..23), -1 where ``truth``
    is -1; integer tensors of one shape -> int32."""
    p, t = pred.to(torch.int64), truth.to(torch.int64)
    tc = t.clamp(0, 23)
    pc = p.clamp(0, 23)
    maj = torch.tensor(KEY_MAJOR_TONIC, device=p.device, dtype=torch.int64)
    same_mode = (pc >= 12) == (tc >= 12)
    d = (pc % 12 - tc % 12) % 12
    cat = torch.full_like(p, 4)
    cat = torch.where(~same_mode & (pc % 12 == tc % 12), torch.full_like(p, 3), cat)
    cat = torch.where(~same_mode & (maj[pc] == maj[tc]), torch.full_like(p, 2), cat)
    cat = torch.where(same_mode & ((d == 5) | (d == 7)), torch.full_like(p, 1), cat)
    cat = torch.where(p > 23, torch.full_like(p, 4), cat)
    cat = torch.where(p == t, torch.zeros_like(p), cat)
    cat = torch.where(p < 0, torch.full_like(p, 5), cat)
    return torch.where(t < 0, torch.full_like(p, -1), cat).to(torch.int32)


def tuning_ratio(cents):
    """``rho = 2 ** (cents / 1200)`` in float64, on the device of ``cents``: what retuning by ``cents`` stretches the time axis by."""
    return torch.exp2(torch.as_tensor(cents).to(torch.float64) / 1200.0)


def scale_boundaries(seg_start, tuning_cents):
    """Annotation boundaries int64 (R, S) in samples of the recording -> in samples of the recording retuned by ``tuning_cents`` (R,):
    ``floor(float64(start) * rho_i)`` as float64 torch ops on the boundaries' device; INT64_MAX (no segment) stays."""
    start = seg_start.to(torch.int64)
    rho = tuning_ratio(torch.as_tensor(tuning_cents, device=start.device)).reshape(-1, 1)
    if rho.shape[0] != start.shape[0]:
        raise ValueError(f"scale_boundaries: {start.shape[0]} recordings but {rho.shape[0]} tunings")
    return torch.where(start == _I64_MAX, start, torch.floor(start.to(torch.float64) * rho).to(torch.int64))


def track_score(pred, counts, seg_start, seg_key, seg_count, hop, window_frames, stride_frames, tuning_cents=None):
    """Score decoded keys against annotations -> ``(truth, category, tally, changes)``: ``ake_track_score_i32`` in integer torch ops,
    exact, on the device of ``pred``.

    ``pred`` int32 (R, W), -1..23 (``KeyTrack.key_id`` or ``smooth_key_id``); ``counts`` (R,) or None.  ``truth`` as ``window_truth``;
    ``category`` int32 (R, W): -1 where the truth is -1, else 0 correct, 1 fifth, 2 relative, 3 parallel, 4 other, 5 undecoded
    (``SCORE_CATEGORIES``, weighted by ``SCORE_WEIGHTS``).  ``tally`` int32 (R, 2, 6): the category counts over all scored windows and
    over the pure ones.  ``changes`` int32 (R, 2): the number of w in 1..count-1 with ``pred[w] != pred[w-1]``, and the same for
    ``truth``.  A recording with count 0 or no segments gets zeros in both.

    ``tuning_cents`` (R,): the track was made from retuned audio (``KeyTrack.tuning_cents``), whose time axis is stretched by
    ``rho_i = 2 ** (cents_i / 1200)``: the boundaries are moved with it first (``scale_boundaries``), as ``KeyTrack.score`` does."""
    dev = pred.device
    R, W = pred.shape
    seg_start, seg_key = seg_start.to(dev), seg_key.to(dev)
    if tuning_cents is not None:
        seg_start = scale_boundaries(seg_start, tuning_cents)
    ns = torch.as_tensor(seg_count, device=dev).to(torch.int64).reshape(R).clamp(0, seg_start.shape[1])
    n = torch.full((R,), W, device=dev, dtype=torch.int64) if counts is None else \
        torch.as_tensor(counts, device=dev).to(torch.int64).reshape(R).clamp(0, W)
    truth, pure = window_truth(seg_start, seg_key, ns, W, hop, window_frames, stride_frames, counts=n)
    category = key_category(pred, truth)
    onehot = category[:, :, None] == torch.arange(6, device=dev, dtype=torch.int32)[None, None, :]     # (R, W, 6); -1 matches none
    tally = torch.stack([onehot.sum(dim=1), (onehot & pure[:, :, None]).sum(dim=1)], dim=1).to(torch.int32)
    live = (torch.arange(1, W, device=dev)[None, :] < n[:, None]) & (ns > 0)[:, None]                  # (R, W - 1): w = 1..count-1
    changes = torch.stack([((pred[:, 1:] != pred[:, :-1]) & live).sum(dim=1), ((truth[:, 1:] != truth[:, :-1]) & live).sum(dim=1)],
                          dim=1).to(torch.int32)
    return truth, category, tally, changes


def transition_from_labels(truth, counts=None, tied=True, pseudo_count=1.0, init=None):
    """A transition matrix counted from key labels -> float64 (24, 24) log matrix that ``track(transition=...)`` accepts.

    ``truth`` integer (R, W) or (W,) labels per window (``window_truth`` / ``TrackScore.truth``; -1 = none), ``counts`` (R,) or None.
    Every pair of consecutive windows below the count with both labels >= 0 is one move (i -> j); the (24, 24) count matrix goes through
    ``transition_m_step`` as expected counts would: ``pseudo_count`` pseudo-moves per row spread as ``init`` (default
    ``key_transition_log(stay=0.9)``), and ``tied`` averages over the transposition classes."""
    t = torch.as_tensor(truth).detach().to(device="cpu", dtype=torch.int64)
    if t.dim() == 1:
        t = t[None]
    R, W = t.shape
    n = torch.full((R,), W, dtype=torch.int64) if counts is None else torch.as_tensor(counts).detach().to(device="cpu", dtype=torch.int64).reshape(R).clamp(0, W)
    a, b = t[:, :-1], t[:, 1:]
    ok = (torch.arange(1, W)[None, :] < n[:, None]) & (a >= 0) & (b >= 0)
    C = torch.zeros(576, dtype=torch.float64).index_add_(0, (a * 24 + b)[ok], torch.ones(int(ok.sum()), dtype=torch.float64)).reshape(24, 24)
    init = key_transition_log(stay=0.9) if init is None else init
    return transition_m_step(C, init, tied=tied, pseudo_count=pseudo_count)


# ---- training windows of annotated recordings: host models of ake_draw_windows_i32, ake_window_batch_f32's labels and the weighted loss ----

DRAW_DOMAIN = 0x57494E44             # "WIND": the fourth counter word of the window draw (the synthesiser's noise uses 0 there)


def window_prefix(frames, window_frames):
    """``[0, c_0, c_0 + c_1, ...]`` (Python ints, R + 1 entries) with ``c_i = max(0, T_i - window_frames + 1)``: the number of window
    starts of every recording, summed exclusively -- the population ``draw_windows`` draws from."""
    prefix = [0]
    for t in frames:
        prefix.append(prefix[-1] + max(0, int(t) - int(window_frames) + 1))
    return prefix


def draw_windows(prefix, seed, epoch, first_slot, batch):
    """``batch`` window positions -> ``(recording, start, index)``, lists of Python ints: ``ake_draw_windows_i32`` restated in
    Python-int arithmetic on ``synthetic.philox4x32_10``.

    ``prefix`` (R + 1 ints, ``window_prefix``; a prefix alone describes the population, no recording needs to exist), ``N = prefix[R]``.
    Slot ``j = first_slot + b`` takes one Philox block with counter ``(j low 32, j high 32, epoch, DRAW_DOMAIN)`` and key
    ``(seed low 32, seed high 32)``; ``x = word0 | word1 << 32``, ``index = (x * N) >> 64``, ``recording`` = the last i < R with
    ``prefix[i] <= index``, ``start = index - prefix[recording]``.  ``ValueError`` for N <= 0."""
    import bisect
    import numpy as np
    from .synthetic import philox4x32_10
    prefix = [int(v) for v in prefix]
    R, N = len(prefix) - 1, prefix[-1]
    if R < 1 or N <= 0:
        raise ValueError("draw_windows: no recording is as long as one window (N = 0)")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    j = [int(first_slot) + b for b in range(int(batch))]
    counter = np.array([[v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, DRAW_DOMAIN] for v in j], dtype=np.uint64).reshape(-1, 4)
    words = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    recording, start, index = [], [], []
    for w in words:
        x = int(w[0]) | int(w[1]) << 32
        idx = (x * N) >> 64
        r = bisect.bisect_right(prefix, idx, 0, R) - 1
        recording.append(r); start.append(idx - prefix[r]); index.append(idx)
    return recording, start, index


def window_labels(seg_start, seg_key, seg_count, recording, start, hop, window_frames, min_purity=0.0, uniform=False):
    """Labels and weights of the windows ``(recording[b], start[b])`` -> dict of ``truth`` int32 (B,), ``purity`` float32 (B,),
    ``key_labels`` (B, 12), ``tonic_labels`` (B, 12), ``key_signature_id`` (B, 24), ``sample_weight`` (B,) float32 and ``seq_length``
    int64 (B,): ``ake_window_batch_f32``'s labels in integer torch ops, on the annotations' device.

    The geometry is ``window_truth``'s at the window's own start frame: ``lo = start * hop``, ``hi = (start + window_frames - 1) * hop``,
    ``centre = (2 * start + window_frames - 1) * hop // 2``; ``truth`` = the key of the last segment that starts at or before ``centre``;
    ``purity = float32(float64(c) / float64(hi - lo + 1))`` with ``c`` the samples of ``lo..hi`` inside segments that carry ``truth``
    (``window_truth``'s ``pure`` is ``purity == 1``); the weight is 0 where ``truth < 0`` or ``purity < min_purity``, else 1
    (``uniform``) or ``purity``.  The labels of key k are ``synthetic.key_pitch_classes(k)``, one-hot ``k % 12`` and one-hot ``k``; zeros
    for ``truth < 0``."""
    dev = seg_start.device
    R, S = seg_start.shape
    rec = torch.as_tensor(recording, device=dev).to(torch.int64).reshape(-1)
    st = torch.as_tensor(start, device=dev).to(torch.int64).reshape(-1)
    hop, wf = int(hop), int(window_frames)
    begin = seg_start.to(torch.int64)[rec]                                                          # (B, S)
    key = seg_key.to(device=dev, dtype=torch.int64)[rec]
    ns = torch.as_tensor(seg_count, device=dev).to(torch.int64).reshape(R).clamp(0, S)[rec]
    lo, hi, centre = st * hop, (st + wf - 1) * hop, torch.div((2 * st + wf - 1) * hop, 2, rounding_mode="floor")
    s_idx = torch.arange(S, device=dev)
    valid = s_idx[None, :] < ns[:, None]
    holds = valid & (begin <= centre[:, None])
    last = (holds * (s_idx + 1)[None, :]).amax(dim=1) - 1
    truth = torch.where(last >= 0, key.gather(1, last.clamp_min(0)[:, None])[:, 0], torch.full_like(last, -1))
    nxt = torch.cat([begin[:, 1:], torch.full((len(rec), 1), _I64_MAX, device=dev, dtype=torch.int64)], dim=1)
    end = torch.where(s_idx[None, :] + 1 < ns[:, None], nxt - 1, torch.full_like(nxt, _I64_MAX))      # a segment's last sample
    a, b = torch.maximum(begin, lo[:, None]), torch.minimum(end, hi[:, None])
    c = torch.where(valid & (key == truth[:, None]) & (truth >= 0)[:, None] & (b >= a), b - a + 1, torch.zeros_like(a)).sum(dim=1)
    purity = (c.to(torch.float64) / (hi - lo + 1).to(torch.float64)).to(torch.float32)
    keep = (truth >= 0) & ~(purity < torch.tensor(float(min_purity), dtype=torch.float32, device=dev))
    weight = torch.where(keep, torch.ones_like(purity) if uniform else purity, torch.zeros_like(purity))
    k = truth.clamp_min(0)
    labelled = (truth >= 0)[:, None]
    scales = KEY_SCALES.to(device=dev, dtype=torch.float32)
    eye = lambda n, i: (torch.arange(n, device=dev)[None, :] == i[:, None]) & labelled
    return {"truth": truth.to(torch.int32), "purity": purity,
            "key_labels": torch.where(labelled, scales[k], torch.zeros((), device=dev)),
            "tonic_labels": eye(12, k % 12).to(torch.float32), "key_signature_id": eye(24, k).to(torch.float32),
            "sample_weight": weight, "seq_length": torch.full((len(rec),), wf, dtype=torch.int64, device=dev)}


def weighted_general_step(key_out, tonic_out, genre_out, key_labels, tonic_labels, genre_labels, key_signature_id, sample_weight,
                          weights=(1.0, 1.0, 0.1), use_cos=False, grads=False):
    """``general_step``'s loss and nine metrics with a weight per row -> the 10 scalars in ``general_step``'s order, and with
    ``grads=True`` also ``(d_key, d_tonic, d_genre)``, the loss's derivatives written out: the formulas of
    ``ake_general_step_weighted_f32`` in torch ops, in the outputs' dtype (float64 inputs give the test model; the loss is
    differentiable, which is what ``PitchClassNet.general_step`` uses off the fused path).

    With ``w_i >= 0`` the weights, ``Wsum`` their sum and ``m_i`` the genre mask (the row's one-hot label sums to 1)::

        loss = key_w * sum_i w_i sum_j BCE_ij / (12 Wsum) + tonic_w * sum_i w_i CE_i / Wsum
               + genre_w * sum_i w_i m_i CE_i / sum_i w_i m_i        (0 when that denominator is 0)
               [+ 1 - sum_i w_i cos_i / Wsum]                        (use_cos)

    The metrics are the same weighted means; ``other`` is 1 minus the four categories.  Rows with ``w_i = 0`` contribute exact zeros
    whatever they hold (NaN included); ``Wsum = 0`` gives zeros everywhere.  ``genre_out`` None: no genre term, accuracy_genre 0."""
    import torch.nn.functional as F
    dt, dev = key_out.dtype, key_out.device
    w = torch.as_tensor(sample_weight, device=dev).to(dt).reshape(-1)
    live = w > 0
    w = torch.where(live, w, torch.zeros_like(w))
    row = live[:, None]
    # rows that do not count are replaced by harmless values before anything is computed: whatever they hold stays out of every sum
    key = torch.where(row, key_out, torch.full_like(key_out, 0.5))
    tonic = torch.where(row, tonic_out, torch.zeros_like(tonic_out))
    y = torch.where(row, key_labels.to(device=dev, dtype=dt), torch.zeros((), dtype=dt, device=dev))
    tl = torch.where(row, tonic_labels.to(dev).long(), torch.zeros((), dtype=torch.int64, device=dev))
    sig = torch.where(row, key_signature_id.to(dev), torch.zeros((), dtype=key_signature_id.dtype, device=dev))
    t_idx = torch.argmax(tl, dim=1)
    wsum = w.sum()
    inv = torch.where(wsum > 0, 1.0 / wsum.clamp_min(torch.finfo(dt).tiny), torch.zeros_like(wsum))
    bce = F.binary_cross_entropy(key, y, reduction="none").sum(dim=1)
    ce = F.cross_entropy(tonic, t_idx, reduction="none")
    kw, tw, gw = (float(v) for v in weights)
    loss = kw * (w * bce).sum() * inv / 12.0 + tw * (w * ce).sum() * inv
    acc_genre = torch.zeros((), dtype=dt, device=dev)
    if genre_out is not None:
        genre = torch.where(row, genre_out, torch.zeros_like(genre_out))
        gl = torch.where(row, genre_labels.to(dev).long(), torch.zeros((), dtype=torch.int64, device=dev))
        g_idx = torch.argmax(gl, dim=1)
        wm = w * (gl.sum(dim=1) == 1).to(dt)
        cnt = wm.sum()
        inv_g = torch.where(cnt > 0, 1.0 / cnt.clamp_min(torch.finfo(dt).tiny), torch.zeros_like(cnt))
        ce_g = F.cross_entropy(genre, g_idx, reduction="none")
        loss = loss + gw * (wm * ce_g).sum() * inv_g
        acc_genre = (wm * (torch.argmax(genre, dim=1) == g_idx).to(dt)).sum() * inv_g
    if use_cos:
        cos = F.cosine_similarity(key, y, dim=1)
        loss = loss + torch.where(wsum > 0, 1.0 - (w * cos).sum() * inv, torch.zeros_like(wsum))
    with torch.no_grad():
        correct, fifths, relative, parallel, _, full = mirex_categories(y, key, tl, tonic, sig)
        mean = lambda m: (w * m.to(dt)).sum() * inv
        c, f, r, p = mean(correct), mean(fifths), mean(relative), mean(parallel)
        other = torch.where(wsum > 0, 1.0 - c - f - r - p, torch.zeros_like(wsum))
        tonic_ok = mean(torch.argmax(tonic, dim=1) == t_idx)
        scalars = (loss, mean(full), 1.0 * c + 0.5 * f + 0.3 * r + 0.2 * p, c, f, r, p, other, tonic_ok, acc_genre)
        if not grads:
            return scalars
        d_key = kw * (w * inv)[:, None] * (key - y) / ((1.0 - key) * key).clamp_min(1e-12) / 12.0       # torch's binary_cross_entropy_backward
        if use_cos:
            pn, yn = key.norm(dim=1, keepdim=True).clamp_min(1e-8), y.norm(dim=1, keepdim=True).clamp_min(1e-8)
            py = (key * y).sum(dim=1, keepdim=True)
            d_key = d_key - (w * inv)[:, None] * (y / (pn * yn) - py * key / (pn ** 3 * yn))
        d_tonic = tw * (w * inv)[:, None] * (torch.softmax(tonic, dim=1) - F.one_hot(t_idx, 12).to(dt))
        d_genre = None
        if genre_out is not None:
            d_genre = gw * (wm * inv_g)[:, None] * (torch.softmax(genre, dim=1) - F.one_hot(g_idx, genre.shape[1]).to(dt))
        return scalars, (d_key, d_tonic, d_genre)


# ---- a sequence loss for training: the labelled windows' conditional log-likelihood under the tracker's own chain (ake_key_sequence_loss_f32) ----

SEQUENCE_CLAMP = -1e4                   # AKE_SEQUENCE_CLAMP: the score of an off-label key of a labelled window (finite; exp() of it is 0)
_FLT_MIN = 1.1754943508222875e-38       # the smallest normal float32


def key_sequence_loss(key, tonic, labels, log_trans, counts=None, signature_weight=1.0, log_prior=None):
    """The sequence loss of (R, W, 12) ``key`` (sigmoid memberships) and ``tonic`` (logits) against ``labels`` (R, W) -> dict:
    ``ake_key_sequence_loss_f32`` in torch ops, in ``key``'s dtype (float64 inputs give the test model), backward written out.

    A linear-chain CRF whose unary scores are the tracker's own emissions ``e = key_emissions(key, tonic, signature_weight)`` under
    ``log_trans``, ``log_prior`` and ``counts`` (as ``key_posteriors`` takes them).  A label outside 0..23 is an unlabelled window and is
    marginalised; a labelled window's other keys are clamped to ``SEQUENCE_CLAMP`` in ``e~``.  With N the labelled windows below their
    recording's count, over the whole call::

        loss    = (sum_r loglik(e[r]) - sum_r loglik(e~[r])) / N                 (0, with zero gradients, when N == 0)
        g       = (post - post~) / N                                              (d loss / d e: ``d_emis``)
        d_trans = sum_r (xi_sum[r] - xi~_sum[r]) / N
        d_tonic[j] = g[j] + g[j + 12] - softmax(tonic)[j] * sum_k g[k]
        d_key[j]   = signature_weight / 12 * (sum_k S_k[j] g[k] * u(p_j) - sum_k (1 - S_k[j]) g[k] * v(p_j))
        u(p) = 1 / p where p >= FLT_MIN and log p > -100, else 0;  v(p) = 1 / (1 - p) where 1 - p >= FLT_MIN and log1p(-p) > -100, else 0

    (``key_posteriors``'s loglik, post and xi_sum; the derivative is 0 where ``nn.BCELoss``'s clamp is active and for subnormal
    arguments, where autograd would give NaN).  Keys of the dict: ``loss``, ``loglik`` (sum_r loglik / N), ``loglik_clamped``,
    ``labelled`` (N), ``d_key``, ``d_tonic`` (R, W, 12), ``d_trans`` (24, 24), ``d_emis`` (R, W, 24); the gradients are zeros at and
    behind the counts.  ``log_prior`` gets no gradient."""
    if key.dim() != 3 or key.shape[2] != 12 or tonic.shape != key.shape:
        raise ValueError(f"key_sequence_loss: key and tonic must be (R, W, 12), got {tuple(key.shape)} and {tuple(tonic.shape)}")
    with torch.no_grad():
        R, W, _ = key.shape
        dt, dev = key.dtype, key.device
        tonic = tonic.to(dt)
        lab = torch.as_tensor(labels, device=dev).to(torch.int64)
        if lab.shape != (R, W):
            raise ValueError(f"key_sequence_loss: labels must be ({R}, {W}), got {tuple(lab.shape)}")
        live = torch.ones((R, W), dtype=torch.bool, device=dev) if counts is None else ~_behind_count(counts, R, W, dev)
        labelled = live & (lab >= 0) & (lab < 24)
        A = torch.as_tensor(log_trans).detach().to(device=dev, dtype=dt)
        prior = None if log_prior is None else torch.as_tensor(log_prior).detach().to(device=dev, dtype=dt)
        e = key_emissions(key, tonic, signature_weight, counts)
        off_label = labelled[..., None] & (torch.arange(24, device=dev)[None, None, :] != lab[..., None])
        ec = torch.where(off_label, torch.full_like(e, SEQUENCE_CLAMP), e)
        post, ll, xi = key_posteriors(e, A, prior, counts, transitions=True)
        postc, llc, xic = key_posteriors(ec, A, prior, counts, transitions=True)
        n = labelled.sum().to(dt)
        inv = torch.where(n > 0, 1.0 / n.clamp_min(1.0), torch.zeros_like(n))
        g = (post - postc) * inv
        sm = torch.softmax(tonic, dim=-1)
        d_tonic = g[..., :12] + g[..., 12:] - sm * g.sum(dim=-1, keepdim=True)
        S = KEY_SCALES.to(device=dev, dtype=dt)
        zero = torch.zeros((), dtype=dt, device=dev)
        q = 1.0 - key
        u = torch.where((key >= _FLT_MIN) & (torch.log(key) > -100.0), 1.0 / key, zero)
        v = torch.where((q >= _FLT_MIN) & (torch.log1p(-key) > -100.0), 1.0 / q, zero)
        d_key = (float(signature_weight) / 12.0) * ((g @ S) * u - (g @ (1.0 - S)) * v)
        d_key = torch.where(live[..., None], d_key, zero)
        d_tonic = torch.where(live[..., None], d_tonic, zero)
        return {"loss": (ll - llc).sum() * inv, "loglik": ll.sum() * inv, "loglik_clamped": llc.sum() * inv, "labelled": n,
                "d_key": d_key, "d_tonic": d_tonic, "d_trans": (xi - xic).sum(dim=0) * inv, "d_emis": g}


def sequence_windows(prefix, seed, epoch, first_slot, batch, sequence_windows, stride_frames):
    """``batch`` sequences of ``sequence_windows`` consecutive windows -> ``(recording, start)``, lists of ``batch * sequence_windows``
    Python ints ordered ``[sequence][window]``: the host model of ``TrackWindows``' sequence mode.  ``prefix`` is ``window_prefix`` over
    the span of a whole sequence, ``window_frames + (sequence_windows - 1) * stride_frames``; slot ``first_slot + s`` of ``draw_windows``
    is the first window of sequence ``s``, and window ``k`` starts ``k * stride_frames`` frames behind it."""
    K, sf = int(sequence_windows), int(stride_frames)
    rec, start, _ = draw_windows(prefix, seed, epoch, first_slot, batch)
    return [r for r in rec for _ in range(K)], [s + k * sf for s in start for k in range(K)]


# ---- tuning: how far a recording sits from A4 = 440 Hz, and the varispeed resampler that puts it back (ake_tuning_estimate_f32 / ake_retune_f32) ----

TUNING_BINS_PER_SEMITONE = 3
RETUNE_MAX_CENTS = 50.0
RETUNE_MAX_RATIO = 1.029302236643492  # 2 ** (50 / 1200) as one double: the same literal in csrc/audio.hip, so every floor agrees
RETUNE_ZEROS = 32                    # Z: zero crossings of the windowed sinc on either side
RETUNE_BETA = 9.0                    # Kaiser beta of its window
RETUNE_CUTOFF = 0.94                 # c: its cutoff as a share of Nyquist, below 2 ** (-50 / 1200) = 0.9715
RETUNE_RESOLUTION = 256              # table entries per sample; the kernel interpolates linearly between them


def estimate_tuning(logmag, counts=None, min_strength=0.0):
    """The detuning of B recordings from their log-CQT (B, n_bins, T) -> ``(cents, strength)``, float64 (B,): the float64 model of
    ``ake_tuning_estimate_f32``.

    The transform has 3 bins per semitone with in-tune notes on bins ``k = 0 (mod 3)`` (``n_bins`` a multiple of 3, else
    ``ValueError``).  With ``m = expm1(L)`` the magnitudes and ``P_j`` the sum of ``m ** 2`` over the bins ``k = j (mod 3)`` and the frames
    ``t < counts[i]`` (default: all)::

        z = P_0 + P_1 e^{2 pi i / 3} + P_2 e^{4 pi i / 3},    cents = 100 arg(z) / (2 pi),    strength = |z| / (P_0 + P_1 + P_2)

    ``cents`` lies in (-50, 50], positive = sharp; ``strength`` in [0, 1] is 1 when all power sits on one bin position and 0 when the
    three carry the same.  A row without power gives (0, 0).  A row with ``strength < min_strength`` reports ``cents = 0``."""
    L = torch.as_tensor(logmag).detach().to(torch.float64)
    if L.dim() != 3 or L.shape[1] % TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"estimate_tuning: logmag must be (B, n_bins, T) with n_bins a multiple of 3, got {tuple(L.shape)}")
    B, P, T = L.shape
    power = torch.expm1(L) ** 2
    if counts is not None:
        power = torch.where(_behind_count(counts, B, T, L.device)[:, None, :], torch.zeros_like(power), power)
    P0, P1, P2 = (power[:, j::3].sum(dim=(1, 2)) for j in range(3))
    return _tuning_finish(P0, P1, P2, min_strength)


def _tuning_finish(P0, P1, P2, min_strength):
    """The three sums over bin positions, float64 (B,) -> ``estimate_tuning``'s ``(cents, strength)``."""
    re, im = P0 - 0.5 * (P1 + P2), (3.0 ** 0.5 / 2.0) * (P1 - P2)
    total = P0 + P1 + P2
    live = total > 0
    cents = torch.where(live, 100.0 * torch.atan2(im, re) / (2.0 * torch.pi), torch.zeros_like(total))
    strength = torch.where(live, torch.sqrt(re * re + im * im) / torch.where(live, total, torch.ones_like(total)), torch.zeros_like(total))
    strength = strength.clamp(max=1.0)
    return torch.where(strength < float(min_strength), torch.zeros_like(cents), cents), strength


def retune_out_len(n):
    """Width of a retuned buffer for rows of ``n`` samples: ``floor(n * 2 ** (50 / 1200)) + 1``, the longest output plus one
    (``ake_retune_out_len``)."""
    import math
    return int(math.floor(int(n) * RETUNE_MAX_RATIO)) + 1


def retune_table():
    """The retuner's filter as the kernel holds it: float32 ``h(q / RETUNE_RESOLUTION)``, ``q = 0 .. Z * RETUNE_RESOLUTION``, of
    ``h(d) = c sinc(c d) I0(beta sqrt(1 - (d / Z) ** 2)) / I0(beta)``; the last entry (``d = Z``) is 0."""
    import numpy as np
    Z, R, c = RETUNE_ZEROS, RETUNE_RESOLUTION, RETUNE_CUTOFF
    d = np.arange(Z * R + 1, dtype=np.float64) / R
    h = c * np.sinc(c * d) * np.i0(RETUNE_BETA * np.sqrt(np.maximum(0.0, 1.0 - (d / Z) ** 2))) / np.i0(RETUNE_BETA)
    h[-1] = 0.0
    return h.astype(np.float32)


def retune_reference(x, cents, lengths=None):
    """Varispeed resampling that undoes a detuning of ``cents``: the float64 model of ``ake_retune_f32`` -> ``(y, n_out)``, numpy.

    ``x`` (B, n) or (n,); ``cents`` one value or (B,), rounded to float32 as the kernel receives it, NaN read as 0 and clamped to
    +-50; ``lengths`` (B,): row i holds ``lengths[i] <= n`` samples.  With ``rho = 2 ** (cents / 1200)``: ``n_out = floor(n_i * rho)`` and::

        y[k] = sum_j x[j] h(k / rho - j)      over |k / rho - j| < Z,    x = 0 outside [0, n_i)

    so a recording that is sharp (``cents > 0``) comes out longer and lower.  ``h`` is read from ``retune_table`` the way the kernel
    reads it: ``k / rho`` in float64, its fraction rounded to float32, the two neighbouring table entries blended linearly; the 2 Z taps
    are added in ascending j.  ``y`` is (B, ``retune_out_len(n)``), zeros behind ``n_out[i]``.  A row with ``cents == 0`` is copied."""
    import numpy as np
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 1
    if single:
        x = x[None]
    B, n = x.shape
    c32 = np.broadcast_to(np.asarray(cents, dtype=np.float32), (B,)).astype(np.float64)
    c32 = np.clip(np.where(np.isnan(c32), 0.0, c32), -RETUNE_MAX_CENTS, RETUNE_MAX_CENTS)
    n_in = np.full(B, n, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64).reshape(B), 0, n)
    Z, R = RETUNE_ZEROS, RETUNE_RESOLUTION
    G = retune_table().astype(np.float64)
    y = np.zeros((B, retune_out_len(n)), dtype=np.float64)
    n_out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        nb = int(n_in[b])
        if c32[b] == 0.0:
            y[b, :nb], n_out[b] = x[b, :nb], nb
            continue
        # (at the clamp the ratio is the literal, not a power: no rounding of exp2 can push n_out past the buffer's width)
        rho = RETUNE_MAX_RATIO if c32[b] >= RETUNE_MAX_CENTS else 1.0 / RETUNE_MAX_RATIO if c32[b] <= -RETUNE_MAX_CENTS else 2.0 ** (c32[b] / 1200.0)
        inv = 1.0 / rho
        no = int(np.floor(nb * rho))
        n_out[b] = no
        pos = np.arange(no, dtype=np.float64) * inv
        j0 = np.floor(pos)
        fr = (pos - j0).astype(np.float32) * np.float32(R)                                   # exact: R is a power of two
        r = np.minimum(fr.astype(np.int64), R - 1)
        t = (fr - r.astype(np.float32)).astype(np.float64)
        xp = np.concatenate([np.zeros(Z), x[b, :nb], np.zeros(Z + 1)])                      # sample j at index j + Z
        j0 = j0.astype(np.int64)
        acc = np.zeros(no, dtype=np.float64)
        for m in range(-Z + 1, Z + 1):                                                      # tap j = j0 + m, at d = fraction - m
            if m <= 0:
                q = r - m * R
                w = G[q] + t * (G[q + 1] - G[q])
            else:
                q = m * R - r - 1
                w = G[q + 1] + t * (G[q] - G[q + 1])
            acc += xp[j0 + m + Z] * w
        y[b, :no] = acc
    return (y[0], int(n_out[0])) if single else (y, n_out)


# ---- a tuning that drifts: the estimate over sliding windows and a retuner that follows a curve (ake_tuning_track_f32 / ake_retune_curve_f32) ----

def tuning_track_windows(frames, window_frames, stride_frames):
    """Windows of a recording of ``frames`` frames: ``1 + (frames - wf) // sf`` from ``wf`` frames on, one window over all of a shorter
    recording, none of an empty one (``ake_tuning_track_windows``)."""
    T, wf, sf = int(frames), int(window_frames), int(stride_frames)
    if wf < 1 or sf < 1:
        raise ValueError(f"tuning_track: windows of {wf} frames, {sf} apart; both must be at least 1")
    return 0 if T <= 0 else 1 if T < wf else 1 + (T - wf) // sf


def tuning_track(logmag, window_frames, stride_frames, counts=None, min_strength=0.0):
    """The detuning of B recordings over time from their log-CQT (B, n_bins, T) -> ``(cents_raw, strength, curve, window_counts)``:
    float64 (B, W) three times and int32 (B,), the float64 model of ``ake_tuning_track_f32``.

    Recording i has ``T_i = counts[i]`` frames (default T) and ``W_i = tuning_track_windows(T_i, ...)`` windows; window w covers the frames
    ``[w * sf, min(w * sf + wf, T_i))``; ``W = tuning_track_windows(T, ...)``.  ``cents_raw`` and ``strength`` are ``estimate_tuning`` on
    each window's frames (``min_strength`` not applied), 0 in the columns ``>= W_i``.  ``curve`` is what a retuner follows
    (``retune_curve_reference``), made per recording in window order: a window with ``strength < min_strength`` takes the value of the
    nearest earlier window that is strong (the leading ones the first strong window's; 0 everywhere if none is); then each value ``v``
    becomes ``v + 100 * floor((before - v) / 100 + 0.5)``, within 50 of the unwrapped value ``before`` it; then it is clamped to +-50, so a
    drift that leaves the semitone saturates instead of jumping; columns ``>= W_i`` repeat the last valid value."""
    L = torch.as_tensor(logmag).detach().to(torch.float64)
    if L.dim() != 3 or L.shape[1] % TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"tuning_track: logmag must be (B, n_bins, T) with n_bins a multiple of 3, got {tuple(L.shape)}")
    B, P, T = L.shape
    wf, sf = int(window_frames), int(stride_frames)
    W = tuning_track_windows(T, wf, sf)
    power = torch.expm1(L) ** 2
    if counts is None:
        frames = [T] * B
    else:
        power = torch.where(_behind_count(counts, B, T, L.device)[:, None, :], torch.zeros_like(power), power)
        frames = torch.as_tensor(counts).reshape(B).clamp(0, T).tolist()
    n_win = [tuning_track_windows(t, wf, sf) for t in frames]
    cents = torch.zeros((B, W), dtype=torch.float64)
    strength = torch.zeros((B, W), dtype=torch.float64)
    for w in range(W):
        f0, f1 = w * sf, min(w * sf + wf, T)
        c, s = _tuning_finish(*(power[:, j::3, f0:f1].sum(dim=(1, 2)) for j in range(3)), 0.0)
        cents[:, w], strength[:, w] = c.cpu(), s.cpu()
    live = torch.arange(W)[None, :] < torch.tensor(n_win)[:, None]
    cents, strength = torch.where(live, cents, torch.zeros_like(cents)), torch.where(live, strength, torch.zeros_like(strength))
    curve = torch.zeros((B, W), dtype=torch.float64)
    for b in range(B):
        raw, strong = cents[b].tolist(), (strength[b, :n_win[b]] >= float(min_strength)).tolist()
        if True not in strong:
            continue
        held = before = raw[strong.index(True)]
        last = 0.0
        for w in range(W):
            if w < n_win[b]:
                if strong[w]:
                    held = raw[w]
                before = held + 100.0 * math.floor((before - held) / 100.0 + 0.5)
                last = min(max(before, -RETUNE_MAX_CENTS), RETUNE_MAX_CENTS)
            curve[b, w] = last
    return cents, strength, curve, torch.tensor(n_win, dtype=torch.int32)


def _retune_curve_knots(cents, knot_first, knot_step):
    """``cents`` (K,) or (B, K), read as the kernel reads them -> ``(rho, kpos)`` float64 (B, K) on the device of ``cents``: the ratio
    at every knot and the output index ``K_i`` of every knot's input sample."""
    c = torch.as_tensor(cents).detach().to(torch.float32)
    c = c[None] if c.dim() == 1 else c
    if c.dim() != 2 or c.shape[1] < 1:
        raise ValueError(f"a tuning curve is (K,) or (B, K) with K >= 1, got {tuple(c.shape)}")
    if int(knot_first) < 0 or int(knot_step) < 1:
        raise ValueError(f"a tuning curve's knots start at a sample >= 0 and lie >= 1 apart, got {knot_first}, {knot_step}")
    c = torch.where(torch.isnan(c), torch.zeros_like(c), c).clamp(-RETUNE_MAX_CENTS, RETUNE_MAX_CENTS).to(torch.float64)
    rho = torch.exp2(c / 1200.0)
    # (at the clamp the ratio is the literal, as in retune_reference)
    rho = torch.where(c >= RETUNE_MAX_CENTS, torch.full_like(rho, RETUNE_MAX_RATIO), rho)
    rho = torch.where(c <= -RETUNE_MAX_CENTS, torch.full_like(rho, 1.0 / RETUNE_MAX_RATIO), rho)
    inc = float(knot_step) * (rho[:, :-1] + rho[:, 1:]) / 2.0
    kpos = torch.cumsum(torch.cat([rho[:, :1] * float(knot_first), inc], dim=1), dim=1)
    return rho, kpos


def _curve_rows(v, rows, dtype=torch.float64):
    v = torch.as_tensor(v).to(dtype)
    single = v.dim() <= 1
    v = v.reshape(1, -1) if single else v
    return (v.expand(rows, -1) if v.shape[0] == 1 else v), single and rows == 1


def retune_curve_forward(p, cents, knot_first, knot_step):
    """``K(p)``: where input position ``p`` (samples; (m,) or (B, m), float64) of a recording lands in its copy retuned along a curve ->
    float64 of ``p``'s shape ((B, m) for a (B, K) curve), torch ops on the device of ``cents``.

    ``cents`` (K,) or (B, K): knot i sits at ``p_i = knot_first + i * knot_step`` with ``rho_i = 2 ** (cents_i / 1200)`` (rounded to
    float32, NaN read as 0, clamped to +-50, as the kernel reads them); ``rho`` is ``rho_0`` in front of the first knot, ``rho_{K-1}``
    behind the last, linear in between, and ``K`` is its integral: ``rho_0 p`` in front; ``K_0 = rho_0 p_0``,
    ``K_{i+1} = K_i + knot_step (rho_i + rho_{i+1}) / 2``; ``K_i + rho_i u + (rho_{i+1} - rho_i) u ** 2 / (2 knot_step)`` with
    ``u = p - p_i`` inside segment i."""
    rho, kpos = _retune_curve_knots(cents, knot_first, knot_step)
    B, K = rho.shape
    p, single = _curve_rows(torch.as_tensor(p).to(rho.device), B)
    first, step = float(knot_first), float(knot_step)
    i = torch.floor((p - first) / step).clamp(0, K - 1).to(torch.int64)
    u = p - (first + i.to(torch.float64) * step)
    r0, r1, k0 = rho.gather(1, i), rho.gather(1, (i + 1).clamp(max=K - 1)), kpos.gather(1, i)
    out = torch.where(p < first, rho[:, :1] * p, k0 + r0 * u + (r1 - r0) * u * u / (2.0 * step))
    return out[0] if single else out


def curve_boundaries(seg_start, cents, knot_first, knot_step):
    """Annotation boundaries int64 (R, S) in samples of the recording -> in samples of the recording retuned along the curve ``cents``
    (R, K): ``floor(K(start))`` (``retune_curve_forward``) as float64 torch ops on the boundaries' device; INT64_MAX (no segment) stays.
    ``scale_boundaries`` for a followed track."""
    start = seg_start.to(torch.int64)
    cents = torch.as_tensor(cents).to(start.device)
    if cents.dim() != 2 or cents.shape[0] != start.shape[0]:
        raise ValueError(f"curve_boundaries: {start.shape[0]} recordings but curves of shape {tuple(cents.shape)}")
    none = start == _I64_MAX
    moved = retune_curve_forward(torch.where(none, torch.zeros_like(start), start).to(torch.float64), cents, knot_first, knot_step)
    return torch.where(none, start, torch.floor(moved).to(torch.int64))


def _retune_curve_read(k, rho, kpos, knot_first, knot_step):
    """Output indices ``k`` (B, m) float64 -> ``(j0 int64, fraction float64)``: the read position ``K^{-1}(k)`` as the kernel keeps it."""
    K = rho.shape[1]
    s = torch.searchsorted(kpos, k.contiguous(), right=True) - 1                     # the last segment with K_s <= k
    front = s < 0
    s = s.clamp_min(0)
    r0, r1 = rho.gather(1, s), rho.gather(1, (s + 1).clamp(max=K - 1))                # (behind the last knot a = 0: u = c / rho)
    c = k - kpos.gather(1, s)
    a = (r1 - r0) / (2.0 * float(knot_step))
    u = torch.where(front, k / rho[:, :1], 2.0 * c / (r0 + torch.sqrt(r0 * r0 + 4.0 * a * c)))
    base = torch.where(front, torch.zeros_like(s), int(knot_first) + s * int(knot_step))
    fl = torch.floor(u)
    return base + fl.to(torch.int64), u - fl


def retune_curve_positions(k, cents, knot_first, knot_step):
    """The inverse of ``retune_curve_forward``: the input position that output index ``k`` ((m,) or (B, m)) reads -> float64.  With s
    the last segment with ``K_s <= k``, ``c = k - K_s`` and ``a = (rho_{s+1} - rho_s) / (2 knot_step)``:
    ``p_s + 2 c / (rho_s + sqrt(rho_s ** 2 + 4 a c))``; ``k / rho_0`` in front of the first knot; ``p_{K-1} + c / rho_{K-1}`` behind the
    last (the float64 model of ``ake_retune_curve_positions``)."""
    rho, kpos = _retune_curve_knots(cents, knot_first, knot_step)
    k, single = _curve_rows(torch.as_tensor(k).to(rho.device), rho.shape[0])
    j0, fr = _retune_curve_read(k, rho, kpos, knot_first, knot_step)
    out = j0.to(torch.float64) + fr
    return out[0] if single else out


def retune_curve_reference(x, cents, knot_first, knot_step, lengths=None):
    """Varispeed resampling along a tuning curve: the float64 model of ``ake_retune_curve_f32`` -> ``(y, n_out)``, numpy.

    ``x`` (B, n) or (n,); ``cents`` (B, K) or (K,) (one curve for every row) with its knots as in ``retune_curve_forward``; ``lengths``
    as in ``retune_reference``.  ``n_out = floor(K(n_i))`` and ``y[k] = sum_j x[j] h(K^{-1}(k) - j)`` with ``retune_reference``'s ``h``,
    table, blend and tap order: the read position is kept as an integer sample and a fraction (``retune_curve_positions``), and the
    fraction is rounded to float32.  ``y`` is (B, ``retune_out_len(n)``), zeros behind ``n_out[i]``.  A row whose clamped cents are all
    0 is copied."""
    import numpy as np
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 1
    if single:
        x = x[None]
    B, n = x.shape
    c32 = torch.as_tensor(np.asarray(cents, dtype=np.float32))
    c32 = (c32[None] if c32.dim() == 1 else c32).expand(B, -1)
    rho, kpos = _retune_curve_knots(c32, knot_first, knot_step)
    moved = (torch.where(torch.isnan(c32), torch.zeros_like(c32), c32).clamp(-RETUNE_MAX_CENTS, RETUNE_MAX_CENTS) != 0).any(dim=1).tolist()
    n_in = np.full(B, n, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64).reshape(B), 0, n)
    Z, R = RETUNE_ZEROS, RETUNE_RESOLUTION
    G = retune_table().astype(np.float64)
    width = retune_out_len(n)
    y = np.zeros((B, width), dtype=np.float64)
    n_out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        nb = int(n_in[b])
        if not moved[b]:
            y[b, :nb], n_out[b] = x[b, :nb], nb
            continue
        end = retune_curve_forward(torch.tensor([float(nb)], dtype=torch.float64), c32[b], knot_first, knot_step)
        no = min(int(math.floor(float(end[0]))), width - 1)
        n_out[b] = no
        j0, fr = _retune_curve_read(torch.arange(no, dtype=torch.float64)[None], rho[b:b + 1], kpos[b:b + 1], knot_first, knot_step)
        j0 = j0[0].numpy()
        fr = fr[0].numpy().astype(np.float32) * np.float32(R)
        r = np.minimum(fr.astype(np.int64), R - 1)
        t = (fr - r.astype(np.float32)).astype(np.float64)
        xp = np.concatenate([np.zeros(Z), x[b, :nb], np.zeros(Z + 1)])                      # sample j at index j + Z
        acc = np.zeros(no, dtype=np.float64)
        for m in range(-Z + 1, Z + 1):
            if m <= 0:
                q = r - m * R
                w = G[q] + t * (G[q + 1] - G[q])
            else:
                q = m * R - r - 1
                w = G[q + 1] + t * (G[q] - G[q + 1])
            at = j0 + m + Z                                                                 # (a tap outside the row reads a zero)
            acc += np.where((at >= 0) & (at < len(xp)), xp[np.clip(at, 0, len(xp) - 1)], 0.0) * w
        y[b, :no] = acc
    return (y[0], int(n_out[0])) if single else (y, n_out)


# ---- the polyphase resampler on audio that arrives in chunks (ake_stream_resample_f32) ----

def resample_ratio(rate_in, rate_out):
    """``(up, down, half)`` of the resampler ``rate_in`` -> ``rate_out``: the rates reduced by their gcd, and the filter's half length
    ``10 * max(up, down)`` (``scipy.signal.resample_poly``'s default), as ``ake_resampler_create`` sets them."""
    import math
    g = math.gcd(int(rate_in), int(rate_out))
    up, down = int(rate_out) // g, int(rate_in) // g
    return up, down, 10 * max(up, down)


def resampled_final(n_in, up, down, half, finished=False):
    """Outputs of the resampler that are final after ``n_in`` inputs (``ake_stream_resample_out_count``): output k reads the inputs up to
    ``floor((k*down + half) / up)``, so it is final iff ``k*down + half < n_in*up``; at the end (``finished``) all
    ``ceil(n_in*up / down)`` are.  With ``up == down`` nothing is filtered and every input is an output."""
    n_in, up, down, half = int(n_in), int(up), int(down), int(half)
    if up == down:
        return n_in
    if finished:
        return -((-n_in * up) // down)
    a = n_in * up - half - 1
    return 0 if a < 0 else a // down + 1


def resample_first_input(k, up, down, half):
    """The first input output ``k`` reads: ``max(0, ceil((k*down - half) / up))``."""
    return max(0, -((int(half) - int(k) * int(down)) // int(up)))


def resample_tail(n_in, up, down, half):
    """Inputs a stream must still hold after ``n_in`` of them: from the first input of the first output that is not final yet.  Never
    more than ``2*half // up`` (``k*down + half >= n_in*up`` for that output, so its first input lies at or behind
    ``n_in - 2*half/up``)."""
    if up == down:
        return 0
    return int(n_in) - min(int(n_in), resample_first_input(resampled_final(n_in, up, down, half), up, down, half))


def stream_resample(chunks, rate_in, rate_out, channel=0):
    """Float64 model of ``ake_stream_resample_f32``: ``chunks`` is a sequence of (C, m) or (m,) arrays, the consecutive pieces of one
    recording (m >= 0, any mix of lengths) -> a list of ``len(chunks) + 1`` float64 arrays: the outputs each piece makes final, and last
    what ``finish()`` adds.  Joined they are ``resample_poly`` of the joined pieces, ``ceil(n*up / down)`` samples.

    Between pieces the model keeps what the kernel keeps: the last ``resample_tail`` inputs with their channels summed (``channel`` >= 0
    takes that channel, -1 the mean; the ``1 / C`` scale is applied to the output).  Every output is one sum in ascending input order over
    "tail, then piece", with the offline sum's limits: the first input never below 0, the last never beyond the end once that is known."""
    import numpy as np
    up, down, half = resample_ratio(rate_in, rate_out)
    mr = max(up, down)
    taps = np.arange(2 * half + 1, dtype=np.float64) - half
    h = np.sinc(taps / mr) / mr * np.kaiser(2 * half + 1, 5.0)         # firwin(2 half + 1, 1 / mr, window=("kaiser", 5.0))
    h = h / h.sum() * up
    held, held_first, n, outs, scale = np.zeros(0), 0, 0, [], 1.0      # held[0] is input `held_first`
    for piece in list(chunks) + [None]:
        finished = piece is None
        if finished:
            summed = np.zeros(0)
        else:
            x = np.atleast_2d(np.asarray(piece, dtype=np.float64))
            scale = 1.0 if channel >= 0 else 1.0 / x.shape[0]
            summed = x[channel] if channel >= 0 else x.sum(axis=0)
        if up == down:
            outs.append(summed * scale)
            continue
        held = np.concatenate([held, summed])
        k0 = resampled_final(n, up, down, half)
        n += summed.shape[0]
        k1 = resampled_final(n, up, down, half, finished)
        y = np.zeros(k1 - k0)
        for k in range(k0, k1):
            i = np.arange(resample_first_input(k, up, down, half), min(n - 1, (k * down + half) // up) + 1)
            y[k - k0] = np.dot(held[i - held_first], h[k * down - i * up + half]) * scale
        keep = resample_tail(n, up, down, half)
        held, held_first = held[held.shape[0] - keep:], n - keep
        outs.append(y)
    return outs


# ---- the retuner on audio that arrives in chunks (ake_stream_retune_f32) ----

def retune_ratio(cents):
    """``cents`` as the retuner reads them -> ``(cents, rho)``: rounded to float32, NaN as 0, beyond +-50 as +-50; ``rho = 2 ** (cents /
    1200)``, the literal ``RETUNE_MAX_RATIO`` (or its inverse) at the clamp.  The host's power: the device's own (``ake_retune_ratio``,
    ``StreamRetuner.rho``) may differ from it in the last place."""
    import numpy as np
    c = float(np.float32(cents))
    c = 0.0 if c != c else min(max(c, -RETUNE_MAX_CENTS), RETUNE_MAX_CENTS)
    rho = RETUNE_MAX_RATIO if c >= RETUNE_MAX_CENTS else 1.0 / RETUNE_MAX_RATIO if c <= -RETUNE_MAX_CENTS else 2.0 ** (c / 1200.0)
    return c, rho


def _retune_is_final(k, inv, n_in):
    """Output k reads the inputs up to ``floor(k * inv) + Z``: the double product the kernel's read position is."""
    import math
    return math.floor(float(k) * inv) + RETUNE_ZEROS <= n_in - 1


def retune_final(n_in, rho, finished=False, copy=None):
    """Outputs of the retuner that are final after ``n_in`` inputs (``ake_stream_retune_out_count``).  With ``inv = 1.0 / rho`` output k
    reads the inputs ``floor(k*inv) - Z + 1 .. floor(k*inv) + Z``, so it is final iff ``floor(float(k) * inv) + Z <= n_in - 1``; the final
    outputs are a prefix (the product is monotone in k), whose size is found from the guess ``floor((n_in - Z) * rho)`` by testing that
    very expression, not from a closed form.  At the end (``finished``) all ``floor(n_in * rho)`` are (never above ``retune_out_len(n_in)
    - 1``).  ``copy``: the stream is not retuned (``cents == 0``: output k is input k, all ``n_in`` are final); default ``rho == 1.0``."""
    import math
    n_in, rho = int(n_in), float(rho)
    if (rho == 1.0) if copy is None else copy:
        return n_in
    if finished:
        return min(int(math.floor(float(n_in) * rho)), retune_out_len(n_in) - 1)
    inv = 1.0 / rho
    k = int(math.floor(float(n_in - RETUNE_ZEROS) * rho)) if n_in > RETUNE_ZEROS else 0
    while k > 0 and not _retune_is_final(k - 1, inv, n_in):
        k -= 1
    while _retune_is_final(k, inv, n_in):
        k += 1
    return k


def retune_tail(n_in, rho, copy=None):
    """Inputs a stream must still hold after ``n_in`` of them: from the first input of the first output that is not final yet,
    ``floor(k*inv) - Z + 1``.  Never more than ``2*Z - 1`` = 63 (``floor(k*inv) + Z > n_in - 1`` for that output)."""
    import math
    if (float(rho) == 1.0) if copy is None else copy:
        return 0
    first = math.floor(float(retune_final(n_in, rho, copy=False)) * (1.0 / float(rho))) - RETUNE_ZEROS + 1
    return int(n_in) - min(int(n_in), max(0, first))


def stream_retune(pieces, cents):
    """Float64 model of ``ake_stream_retune_f32``: ``pieces`` is a sequence of (m,) arrays, the consecutive pieces of one recording (m >= 0,
    any mix of lengths) -> a list of ``len(pieces) + 1`` float64 arrays: the outputs each piece makes final, and last what ``finish()``
    adds.  Joined they are ``retune_reference`` on the joined pieces, ``floor(n * rho)`` samples, exactly: the same products added in the
    same order.

    Between pieces the model keeps what the kernel keeps, the last ``retune_tail`` (at most 63) inputs.  Every output is
    ``retune_reference``'s sum over "tail, then piece": the position ``k / rho`` in float64, its fraction rounded to float32, the two table
    blends, the taps added in ascending j, zeros in front of sample 0 and -- for ``finish()`` alone -- behind the end.  ``cents == 0`` (after
    the clamp): every piece is its own output and nothing is kept."""
    import numpy as np
    c, rho = retune_ratio(cents)
    copy = c == 0.0
    Z, R = RETUNE_ZEROS, RETUNE_RESOLUTION
    G = retune_table().astype(np.float64)
    inv = 1.0 / rho
    held, held_first, n, outs = np.zeros(0), 0, 0, []                  # held[0] is input `held_first`
    for piece in list(pieces) + [None]:
        finished = piece is None
        x = np.zeros(0) if finished else np.asarray(piece, dtype=np.float64).reshape(-1)
        if copy:
            outs.append(x.copy())
            continue
        held = np.concatenate([held, x])
        k0 = retune_final(n, rho, copy=False)
        n += x.shape[0]
        k1 = retune_final(n, rho, finished, copy=False)
        pos = np.arange(k0, k1, dtype=np.float64) * inv
        j0 = np.floor(pos)
        fr = (pos - j0).astype(np.float32) * np.float32(R)
        r = np.minimum(fr.astype(np.int64), R - 1)
        t = (fr - r.astype(np.float32)).astype(np.float64)
        j0 = j0.astype(np.int64)
        assert k1 == k0 or (j0[0] - Z + 1 >= held_first or held_first == 0) and (finished or j0[-1] + Z <= n - 1)
        # input j at xp[j - held_first + 2 Z]: what is held, zeros in front of sample 0 and behind the end
        xp = np.concatenate([np.zeros(2 * Z), held, np.zeros(2 * Z + 1)])
        acc = np.zeros(k1 - k0, dtype=np.float64)
        for m in range(-Z + 1, Z + 1):
            if m <= 0:
                q = r - m * R
                w = G[q] + t * (G[q + 1] - G[q])
            else:
                q = m * R - r - 1
                w = G[q + 1] + t * (G[q] - G[q + 1])
            acc += xp[j0 + m - held_first + 2 * Z] * w
        outs.append(acc)
        keep = retune_tail(n, rho, copy=False)
        held, held_first = held[held.shape[0] - keep:], n - keep
    return outs


# ---- key-profile emissions: a key track without a trained net (ake_profile_emissions_f32) ----

# Published tone profiles, rows minor and major (the order of KEY_NAMES' two halves), tonic first.  "krumhansl": Krumhansl & Kessler
# (1982), the probe-tone ratings; "temperley": Temperley (1999), "What's Key for Key?", the revised Krumhansl-Schmuckler profiles.
KEY_PROFILES = {
    "krumhansl": ((6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17),
                  (6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88)),
    "temperley": ((5.0, 2.0, 3.5, 4.5, 2.0, 4.0, 2.0, 4.5, 3.5, 2.0, 1.5, 4.0),
                  (5.0, 2.0, 3.5, 2.0, 4.5, 4.0, 2.0, 4.5, 2.0, 3.5, 1.5, 4.0)),
}
PROFILE_COMPRESSIONS = ("log", "magnitude", "power")
PROFILE_SILENCE = 1e-12                 # a window is silent when sum_j (x_j - mean)^2 <= PROFILE_SILENCE * 12 * mean^2


def key_profile_table(profiles="krumhansl"):
    """``profiles`` of ``profile_emissions`` checked -> (2, 12) float64 on the host, rows minor and major, tonic first.  A name of
    ``KEY_PROFILES`` or a (2, 12) tensor; ``ValueError`` for an unknown name, another shape, a value that is not finite or a row that is
    constant (it correlates with nothing)."""
    if isinstance(profiles, str):
        if profiles not in KEY_PROFILES:
            raise ValueError(f"profiles: unknown name {profiles!r} (KEY_PROFILES has {sorted(KEY_PROFILES)})")
        return torch.tensor(KEY_PROFILES[profiles], dtype=torch.float64)
    p = torch.as_tensor(profiles).detach().to(device="cpu", dtype=torch.float64)
    if tuple(p.shape) != (2, 12):
        raise ValueError(f"profiles must be a name of KEY_PROFILES or a (2, 12) tensor (rows minor and major, tonic first), got {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError("profiles must be finite")
    if bool((p == p[:, :1]).all(dim=1).any()):
        raise ValueError("profiles: a row is constant; it correlates with nothing")
    return p


def _profile_compression(compression):
    if compression not in PROFILE_COMPRESSIONS:
        raise ValueError(f"compression must be one of {PROFILE_COMPRESSIONS}, got {compression!r}")
    return PROFILE_COMPRESSIONS.index(compression)


def profile_window_counts(frame_counts, window_frames, stride_frames):
    """Windows of recordings of ``frame_counts`` frames (integer tensor): ``pipeline.track_counts``, and in the whole-clip mode
    (``window_frames == 0``) 1 for a recording that has frames, else 0."""
    n = torch.as_tensor(frame_counts).to(torch.int64)
    if int(window_frames) == 0:
        return (n > 0).to(torch.int64)
    w = torch.div(n - int(window_frames), int(stride_frames), rounding_mode="floor") + 1
    return torch.where(n < int(window_frames), torch.zeros_like(w), w)


def profile_emissions(logmag, window_frames, stride_frames, counts=None, profiles="krumhansl", compression="log", sharpness=10.0, cents=None):
    """Key emissions without a net (Krumhansl-Schmuckler): every window's chroma correlated with the 24 rotations of a minor and a major
    key profile -> ``(chroma (R, W, 12), emissions (R, W, 24), key_id int32 (R, W), confidence (R, W))``, float64: the float64 model of
    ``ake_profile_emissions_f32``.

    ``logmag`` (R, n_bins, T): a log-CQT with 3 bins per semitone from C, in-tune notes on the bins ``k = 0 (mod 3)`` (``n_bins`` a
    multiple of 3, else ``ValueError``).  Bin k belongs to semitone ``(k + 1) // 3`` and pitch class ``((k + 1) // 3) % 12``; semitone 0
    lacks its flat-side bin and the top bin is the flat side of a semitone above the range: both are kept as they come.  With L the
    log-CQT, ``v = L`` (``compression="log"``), ``expm1(L)`` (``"magnitude"``) or ``expm1(L) ** 2`` (``"power"``)::

        c[r, t, j] = sum of v[r, k, t] over the bins k of pitch class j, in ascending k
        x[r, w, j] = sum of c[r, t, j] over t = w * stride_frames .. w * stride_frames + window_frames - 1, in ascending t

    ``counts`` (R,): frames of every recording, clamped to 0..T (default T); recording r has
    ``track_counts(counts[r], window_frames, stride_frames)`` windows and W is that of T.  ``window_frames = 0`` is the whole-clip mode:
    W = 1, one window over the recording's own ``counts[r]`` frames, none for a recording of 0 frames.

    Key k (``KEY_NAMES`` order) has mode ``k // 12`` (0 minor, 1 major), tonic ``k % 12`` and the profile
    ``q_k[j] = profiles[mode][(j - tonic) % 12]``.  With ``m = (sum_j x_j) / 12``, ``d_j = x_j - m``, ``sxx = sum_j d_j ** 2`` and the same
    ``e``, ``see`` of a profile row (all sums in ascending j), ``r_k = (sum_j d_j * e[(j - tonic) % 12]) / sqrt(sxx * see)``, the Pearson
    correlation, and ``emissions[k] = sharpness * r_k``.  A window with ``sxx <= 1e-12 * 12 * m ** 2`` (all-zero chroma included) is
    silent: ``r = 0``, ``key_id = -1``, zero chroma.  Otherwise ``key_id`` is the smallest k that attains the maximum ``r_k``,
    ``confidence`` that ``r_k`` and ``chroma = x / sum_j x_j``.  Behind a recording's window count: zeros, and -1 in ``key_id``.

    ``profiles``: a name of ``KEY_PROFILES`` or a (2, 12) tensor (``key_profile_table``).  ``sharpness = 10.0`` and
    ``compression = "log"`` are starting values that nobody has measured against annotated music; ``tools/profile_baseline.py`` scores
    them and their neighbours on synthesised recordings (``profiles/key_profiles.md``).

    ``cents`` (default None: all of the above, untouched) is the tuned chroma, the float64 model of ``ake_profile_emissions_tuned_f32``:
    the chroma of a recording that sits ``cents`` off A4 = 440 Hz, from its own transform, without retuning it.  One value, (R,) or
    (R, W), rounded to float32 as the kernel receives it, NaN read as 0 and clamped to +-50 (``retune_reference``'s rule).  ``n_bins``
    must then be a multiple of 36.  With ``F[r, t, p]`` the octave-folded sums (``folded_chroma``) and ``FW[p]`` their sum over a
    window's frames in ascending t::

        delta = 3.0 * c / 100.0,    n = floor(delta - 1.0) in {-3 .. 0},    g = delta - 1.0 - n in [0, 1)
        x[r, w, j] = (((1 - g) * FW[b0] + FW[b1]) + FW[b2]) + g * FW[b3],    b_i = (3 j + n + i) % 36

    with a term of weight 0 left out: the class boundaries move by ``delta`` bins and split the one bin each crosses.  At ``c = 0`` that
    is ``FW[3j-1] + FW[3j] + FW[3j+1]``, the classes above; everything behind ``x`` is the same."""
    L = torch.as_tensor(logmag).detach().to(device="cpu", dtype=torch.float64)
    if L.dim() != 3 or L.shape[1] % TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"profile_emissions: logmag must be (R, n_bins, T) with n_bins a multiple of 3, got {tuple(L.shape)}")
    if cents is not None and L.shape[1] % FOLDED_BINS != 0:
        raise ValueError(f"profile_emissions: the tuned chroma (cents) needs n_bins a multiple of 36 (whole octaves), got {L.shape[1]}")
    mode = _profile_compression(compression)
    prof = key_profile_table(profiles)
    sharpness = float(sharpness)
    if not sharpness > 0.0:
        raise ValueError("profile_emissions: sharpness must be positive")
    wf, sf = int(window_frames), int(stride_frames)
    if wf < 0 or sf < 1:
        raise ValueError("profile_emissions: window_frames must be >= 0 (0: the whole clip) and stride_frames >= 1")
    R, P, T = L.shape
    n = torch.full((R,), T, dtype=torch.int64) if counts is None else torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(R).clamp(0, T)
    W = int(profile_window_counts(torch.tensor(T), wf, sf))
    n_win = profile_window_counts(n, wf, sf)
    c = _profile_frame_chroma(L, mode) if cents is None else _folded_frames(L, mode)
    c = torch.where((torch.arange(T)[None, :] < n[:, None])[:, :, None], c, torch.zeros_like(c))
    x = torch.zeros((R, W, c.shape[2]), dtype=torch.float64)
    if W > 0:
        start = torch.arange(W) * sf
        for i in range(T if wf == 0 else wf):                                                # ascending t (behind counts[r]: zeros)
            x += c[:, start + i, :]
    if cents is not None:
        x = tuned_class_sums(x, _tuned_cents(cents, R, W))
    live = torch.arange(W)[None, :] < n_win[:, None]                                         # (R, W)
    x = torch.where(live[:, :, None], x, torch.zeros_like(x))
    return _profile_score(x, live, prof, sharpness)


FOLDED_BINS = 36                        # folded positions of the tuned chroma: bin k sits at k % 36


def _folded_frames(L, mode):
    """(R, n_bins, T) float64 log-CQT, n_bins a multiple of 36 -> F (R, T, 36): the bins of every folded position added in ascending
    octave."""
    R, P, T = L.shape
    v = L if mode == 0 else torch.expm1(L) if mode == 1 else torch.expm1(L) ** 2
    F = torch.zeros((R, T, FOLDED_BINS), dtype=torch.float64)
    for k in range(P):                                                                       # ascending k: ascending octave at every p
        F[:, :, k % FOLDED_BINS] += v[:, k, :]
    return F


def folded_chroma(logmag, counts=None, compression="log"):
    """The 36 octave-folded sums of every frame -> (R, T, 36) float64: ``F[r, t, p]`` is the sum of ``v[r, p + 36 o, t]`` over the
    octaves o in ascending order, ``v`` as in ``profile_emissions``; zeros in the frames at or behind ``counts[r]`` (default T).  What
    the tuned chroma (``profile_emissions(cents=...)``) is cut from, and what ``profile_fold_kernel`` writes.  ``logmag`` (R, n_bins, T)
    with ``n_bins`` a multiple of 36, else ``ValueError``."""
    L = torch.as_tensor(logmag).detach().to(device="cpu", dtype=torch.float64)
    if L.dim() != 3 or L.shape[1] % FOLDED_BINS != 0:
        raise ValueError(f"folded_chroma: logmag must be (R, n_bins, T) with n_bins a multiple of 36, got {tuple(L.shape)}")
    R, P, T = L.shape
    F = _folded_frames(L, _profile_compression(compression))
    if counts is not None:
        n = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(R).clamp(0, T)
        F = torch.where((torch.arange(T)[None, :] < n[:, None])[:, :, None], F, torch.zeros_like(F))
    return F


def _tuned_cents(cents, R, W):
    """``cents`` of the tuned chroma (one value, (R,) or (R, W)) -> float64 (R, W) as the kernel reads it: rounded to float32, NaN as
    0, clamped to +-50."""
    c = torch.as_tensor(cents).detach().to(device="cpu", dtype=torch.float32).to(torch.float64)
    if c.dim() == 0:
        c = c.expand(R, W)
    elif c.dim() == 1 and c.shape[0] == R:
        c = c[:, None].expand(R, W)
    elif tuple(c.shape) != (R, W):
        raise ValueError(f"profile_emissions: cents must be one value, ({R},) or ({R}, {W}), got {tuple(c.shape)}")
    return torch.nan_to_num(c, nan=0.0).clamp(-RETUNE_MAX_CENTS, RETUNE_MAX_CENTS)


def tuned_cut(cents):
    """Where ``cents`` (float64, within +-50) put the class boundaries -> ``(n, g)``: class j holds the folded bins ``3 j + n ..
    3 j + n + 3`` (mod 36), the first weighted ``1 - g``, the last ``g``."""
    u = 3.0 * cents / 100.0 - 1.0
    n = torch.floor(u)
    return n.to(torch.int64), u - n


def tuned_class_sums(FW, cents):
    """Folded window sums FW (..., 36) float64 and their windows' cents (...) float64, as ``_tuned_cents`` returns them -> the twelve
    class sums (..., 12), in the order of addition the kernel uses."""
    n, g = tuned_cut(cents)
    b = 3 * torch.arange(12) + n[..., None] + FOLDED_BINS                                      # >= 33
    take = lambda i: torch.gather(FW, -1, (b + i) % FOLDED_BINS)
    w0, w3 = (1.0 - g)[..., None], g[..., None]
    x = w0 * take(0) + take(1)                                                               # (a product and a sum: two roundings)
    x = x + take(2)
    return torch.where(w3 != 0.0, x + w3 * take(3), x)


def _profile_frame_chroma(L, mode):
    """(R, n_bins, T) float64 log-CQT -> per-frame chroma c (R, T, 12): the bins of every pitch class added in ascending k."""
    R, P, T = L.shape
    v = L if mode == 0 else torch.expm1(L) if mode == 1 else torch.expm1(L) ** 2
    c = torch.zeros((R, T, 12), dtype=torch.float64)
    for k in range(P):                                                                       # ascending k
        c[:, :, ((k + 1) // 3) % 12] += v[:, k, :]
    return c


def _profile_score(x, live, prof, sharpness):
    """Window chroma x (R, W, 12) float64 (zeros where not ``live`` (R, W)) -> ``profile_emissions``' four outputs."""
    R, W = x.shape[:2]
    seq_sum = _ascending_sum
    m = seq_sum(x) / 12.0
    d = x - m[..., None]
    sxx = seq_sum(d * d)
    silent = ~live | (sxx <= PROFILE_SILENCE * 12.0 * m * m)
    e = prof - (seq_sum(prof) / 12.0)[:, None]                                               # (2, 12)
    see = seq_sum(e * e)                                                                     # (2,)
    j = torch.arange(12)
    r = torch.zeros((R, W, 24), dtype=torch.float64)
    for k in range(24):
        q = e[k // 12][(j - k % 12) % 12]
        r[:, :, k] = seq_sum(d * q) / torch.sqrt(torch.where(silent, torch.ones_like(sxx), sxx) * see[k // 12])
    r = torch.where(silent[..., None], torch.zeros_like(r), r)
    conf = r.max(dim=2).values
    idx = torch.arange(24)[None, None, :].expand_as(r)
    key_id = torch.where(r == conf[..., None], idx, torch.full_like(idx, 24)).min(dim=2).values
    key_id = torch.where(silent, torch.full_like(key_id, -1), key_id).to(torch.int32)
    conf = torch.where(silent, torch.zeros_like(conf), conf)
    total = seq_sum(x)
    chroma = torch.where(silent[..., None], torch.zeros_like(x), x / torch.where(silent, torch.ones_like(total), total)[..., None])
    return chroma, sharpness * r, key_id, conf


def _ascending_sum(t):
    """Sum over the last dimension in ascending index order (``Tensor.sum`` promises no order)."""
    s = t[..., 0].clone()
    for j in range(1, t.shape[-1]):
        s = s + t[..., j]
    return s


def fit_key_profiles(chroma, key_id, weight=None):
    """Key profiles from labelled chroma -> (2, 12) float64, rows minor and major, tonic first, each summing to 1: what
    ``profile_emissions(profiles=...)`` takes.

    ``chroma`` (..., 12) and ``key_id`` (...) in ``KEY_NAMES`` order, ``weight`` (...) or None (all 1).  Every row is divided by its sum
    and rolled so that its labelled tonic sits at index 0; a mode's profile is the weighted mean of its rows, divided by its sum.  Rows
    with ``key_id < 0`` or zero weight count for nothing; a mode without rows is a ``ValueError``.  Ordinary torch ops in float64 on the
    inputs' device (24 numbers: no kernel)."""
    x = torch.as_tensor(chroma).detach().to(torch.float64).reshape(-1, 12)
    k = torch.as_tensor(key_id).detach().to(device=x.device, dtype=torch.int64).reshape(-1)
    w = torch.ones_like(k, dtype=torch.float64) if weight is None else torch.as_tensor(weight).detach().to(device=x.device, dtype=torch.float64).reshape(-1)
    if k.shape[0] != x.shape[0] or w.shape[0] != x.shape[0]:
        raise ValueError("fit_key_profiles: chroma (..., 12), key_id (...) and weight (...) must agree in their leading dimensions")
    w = torch.where((k >= 0) & (k < 24), w, torch.zeros_like(w))
    total = x.sum(dim=1)
    counted = w != 0
    x = torch.where(counted[:, None], x / torch.where(counted, total, torch.ones_like(total))[:, None], torch.zeros_like(x))
    tonic = k.clamp(0, 23) % 12
    rolled = x.gather(1, (torch.arange(12, device=x.device)[None, :] + tonic[:, None]) % 12)  # rolled[i] = x[(i + tonic) % 12]
    out = []
    for mode in (0, 1):
        wm = torch.where(k.clamp(0, 23) // 12 == mode, w, torch.zeros_like(w))
        if not bool((wm != 0).any()):
            raise ValueError(f"fit_key_profiles: no {'major' if mode else 'minor'} row carries weight")
        p = (rolled * wm[:, None]).sum(dim=0) / wm.sum()
        out.append(p / p.sum())
    return torch.stack(out)


# ---- key changes to the frame: a change point between two windows' centres (ake_key_changes_f32) ----

KEY_CHANGES_MAX_SPAN = 1024              # kMaxSpan of csrc/changes.hip: stride_frames + 2 * slack_frames at most, on the device


def key_frame_scores(logmag, counts=None, profiles="krumhansl", compression="log"):
    """Every frame's Pearson correlation with the 24 keys' profiles -> (R, T, 24) float64: ``profile_emissions(window_frames=1,
    stride_frames=1, sharpness=1)``'s emissions, the silence rule included (a silent frame, or one at or behind ``counts[r]``, scores 0
    for every key).  What ``key_changes`` places its boundaries by."""
    L = torch.as_tensor(logmag).detach().to(device="cpu", dtype=torch.float64)
    if L.dim() != 3 or L.shape[1] % TUNING_BINS_PER_SEMITONE != 0:
        raise ValueError(f"key_changes: logmag must be (R, n_bins, T) with n_bins a multiple of 3, got {tuple(L.shape)}")
    R, P, T = L.shape
    n = torch.full((R,), T, dtype=torch.int64) if counts is None else torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(R).clamp(0, T)
    live = torch.arange(T)[None, :] < n[:, None]
    c = _profile_frame_chroma(L, _profile_compression(compression))
    c = torch.where(live[:, :, None], c, torch.zeros_like(c))
    return _profile_score(c, live, key_profile_table(profiles), 1.0)[1]


def _key_change_span(lab, w, n_win, T, wf, sf, slack):
    """Boundary w of one recording (``lab``: its labels, ``n_win`` windows, ``T`` frames; ``w + 1 < n_win``) -> ``(a, b, m_w, lo, hi)``,
    or None where the two windows do not carry two different keys: ``key_changes``' span."""
    a, b = lab[w], lab[w + 1]
    if not (0 <= a < 24 and 0 <= b < 24) or a == b:
        return None
    m0, m1 = w * sf + wf // 2, (w + 1) * sf + wf // 2
    lo, hi = max(m0 - slack, 0), min(m1 + slack, T)
    if w >= 1 and lab[w - 1] != a:
        lo = max(lo, m0)
    if w + 2 < n_win and lab[w + 2] != b:
        hi = min(hi, m1)
    return a, b, m0, lo, hi


def _key_change_scan(d, m0, lo, hi, sf):
    """The span's differences ``d`` (a list of hi - lo floats) -> ``(change_frame, gain, contrast, margin)``: ``key_changes``' sum in
    ascending i and its first maximum."""
    C = [0.0]
    for x in d:                                                                              # ascending i
        C.append(C[-1] + x)
    best = max(C)
    j = C.index(best)                                                                        # the first maximum
    g = min(max(m0 + (sf + 1) // 2, lo), hi)
    return lo + j, best - C[g - lo], (2.0 * best - C[-1]) / (hi - lo), best - max(C[:j] + C[j + 1:])


def key_changes(logmag, labels, window_frames, stride_frames, counts=None, window_counts=None, slack_frames=None, profiles="krumhansl",
                compression="log"):
    """Where the key changes between two windows of a key track, to the frame -> ``(change_frame int32 (R, W-1), gain (R, W-1),
    contrast (R, W-1), margin (R, W-1))``, the last three float64: the float64 model of ``ake_key_changes_f32`` and its definition.

    ``logmag`` (R, n_bins, T), ``profiles`` and ``compression`` as in ``profile_emissions``; ``counts`` (R,): frames of every
    recording, ``T_r``, clamped to 0..T (default T).  ``labels`` integer (R, W): a key 0..23 per window of ``window_frames`` frames,
    ``stride_frames`` apart (``KeyTrack.key_id`` or ``smooth_key_id``; anything else, -1 included, is no key).  ``window_counts`` (R,):
    windows of every recording, clamped to 0..W and to the ``track_counts(T_r, ...)`` windows its frames hold (the default).

    ``s[r, t, k]`` is frame t's correlation with key k (``key_frame_scores``).  ``m_w = w * stride_frames + window_frames // 2`` is
    window w's centre frame.  Boundary w, between the windows w and w + 1, exists iff ``w + 1 < window_counts[r]`` and
    ``a = labels[r, w]``, ``b = labels[r, w + 1]`` are two different keys.  Its span is ``lo = max(m_w - slack, 0)`` ..
    ``hi = min(m_{w+1} + slack, T_r)``, and never crosses the centre of a window that ends another run: if ``w >= 1`` and
    ``labels[r, w - 1] != a`` then ``lo = max(lo, m_w)``; if ``w + 2 < window_counts[r]`` and ``labels[r, w + 2] != b`` then
    ``hi = min(hi, m_{w+1})``.  The spans on either side of a run of one window then share one frame at the most, and those of a run of
    k windows lie apart when ``(k - 1) * stride_frames >= 2 * slack_frames``: there a recording's change frames never decrease.
    (With the default slack a run of two windows still has spans that share a stride.)  ``slack_frames`` defaults to ``stride_frames``.

    ``d_i = s[lo + i, a] - s[lo + i, b]``, ``C_0 = 0``, ``C_{i+1} = C_i + d_i`` added in ascending i; ``j*`` is the smallest j in
    0..hi-lo that attains the maximum of C and ``change_frame = lo + j*``: the frames below it belong to a, the rest to b (the split
    that maximises the summed score of each side's own key; an objective that is additive over the frames).
    ``gain = C_{j*} - C_{g - lo}`` with ``g = clamp(m_w + (stride_frames + 1) // 2, lo, hi)``, where the grid puts the boundary: how
    much the objective gains over it, never negative.  ``contrast = (2 * C_{j*} - C_{hi-lo}) / (hi - lo)``: the mean per-frame
    advantage of each side's own key, in [-2, 2]; near 0 or below, the labels do not fit the frames.  ``margin`` is ``C_{j*}`` minus the
    largest other ``C_j`` (for tests: how far the decision is from a tie).  Where there is no boundary: -1 and zeros."""
    wf, sf = int(window_frames), int(stride_frames)
    if wf < 1 or sf < 1:
        raise ValueError("key_changes: window_frames and stride_frames must be >= 1")
    slack = sf if slack_frames is None else int(slack_frames)
    if slack < 0:
        raise ValueError("key_changes: slack_frames must be >= 0")
    s = key_frame_scores(logmag, counts, profiles, compression)
    R, T = s.shape[:2]
    lab = torch.as_tensor(labels).detach().cpu().to(torch.int64)
    if lab.dim() != 2 or lab.shape[0] != R:
        raise ValueError(f"key_changes: labels must be (R, W) with R = {R}, got {tuple(lab.shape)}")
    W = lab.shape[1]
    n = torch.full((R,), T, dtype=torch.int64) if counts is None else torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(R).clamp(0, T)
    fits = profile_window_counts(n, wf, sf)
    n_win = fits.clamp(max=W) if window_counts is None else \
        torch.minimum(torch.as_tensor(window_counts).detach().cpu().to(torch.int64).reshape(R).clamp(0, W), fits)
    B = max(W - 1, 0)
    frame = torch.full((R, B), -1, dtype=torch.int32)
    gain, contrast, margin = (torch.zeros((R, B), dtype=torch.float64) for _ in range(3))
    lab, s = lab.tolist(), s.tolist()
    for r in range(R):
        for w in range(min(int(n_win[r]), W) - 1):
            span = _key_change_span(lab[r], w, int(n_win[r]), int(n[r]), wf, sf, slack)
            if span is None:
                continue
            a, b, m0, lo, hi = span
            frame[r, w], gain[r, w], contrast[r, w], margin[r, w] = _key_change_scan([s[r][t][a] - s[r][t][b] for t in range(lo, hi)], m0, lo, hi, sf)
    return frame, gain, contrast, margin


# ---- the profile method and the tuning estimate on frames that arrive in pieces (ake_stream_frame_stats_f32 / ake_stream_profile_emissions_f32) ----

def stream_profile_ring_frames(window_frames, max_new_frames):
    """Rows a stream's chroma ring needs when no piece brings more than ``max_new_frames`` frames: ``window_frames + max_new_frames``.

    With ``F_old`` frames before a piece and ``W_old = track_counts(F_old)`` windows emitted, the new windows read the frames
    ``[W_old * sf, F)``.  Window ``W_old`` was not complete, so ``W_old * sf + wf > F_old``, that is ``W_old * sf > F_old - wf``: the span
    is shorter than ``wf + (F - F_old)``, and a ring of that many rows still holds all of it after the piece's frames are written."""
    wf, m = int(window_frames), int(max_new_frames)
    if wf < 1 or m < 0:
        raise ValueError("stream_profile_ring_frames: window_frames must be >= 1 and max_new_frames >= 0")
    return wf + m


def _stream_windows(frames, wf, sf):
    return 0 if frames < wf else (frames - wf) // sf + 1


def stream_profile(pieces, window_frames, stride_frames, profiles="krumhansl", compression="log", sharpness=10.0, ring_frames=None,
                   state=None, return_state=False):
    """Float64 model of a ``method="profile"`` stream (``ake_stream_frame_stats_f32``'s chroma part, then
    ``ake_stream_profile_emissions_f32``): ``pieces`` is a sequence of (R, n_bins, m) log-CQT frames, the consecutive pieces of R
    recordings in lockstep (m >= 0, any mix) -> a list with one ``(chroma (R, k, 12), emissions (R, k, 24), key_id int32 (R, k),
    confidence (R, k))`` per piece: the k windows that piece completed.  Joined along the windows they are ``profile_emissions`` of the
    joined pieces, to the bit: the same additions in the same order.

    Between pieces the model keeps what the kernels keep: a ring of per-frame chroma, float64 (R, ring_frames, 12), frame t in row
    ``t % ring_frames`` -- every frame is written, also one that a stride longer than the window skips -- and two host integers, the
    frames and the windows so far.  A window's chroma is the sum of its rows in ascending t (the row index wraps).  ``ring_frames``
    (default: ``stream_profile_ring_frames`` of the longest piece) must be at least ``window_frames``; a piece so long that a window's
    first frames have been overwritten is a ``ValueError``, as are ``window_frames < 1`` (there is no whole-clip mode on a stream),
    ``stride_frames < 1``, ``n_bins`` no multiple of 3 and a ``sharpness`` that is not positive.  ``state`` / ``return_state``: continue
    from, and return as a last list element, the carried state (``{"ring", "frames", "windows"}``)."""
    pieces = [torch.as_tensor(p).detach().to(device="cpu", dtype=torch.float64) for p in pieces]
    mode = _profile_compression(compression)
    prof = key_profile_table(profiles)
    sharpness = float(sharpness)
    if not sharpness > 0.0:
        raise ValueError("stream_profile: sharpness must be positive")
    wf, sf = int(window_frames), int(stride_frames)
    if wf < 1 or sf < 1:
        raise ValueError("stream_profile: window_frames and stride_frames must be >= 1")
    for p in pieces:
        if p.dim() != 3 or p.shape[1] % TUNING_BINS_PER_SEMITONE != 0 or p.shape[:2] != pieces[0].shape[:2]:
            raise ValueError(f"stream_profile: every piece must be (R, n_bins, m) with n_bins a multiple of 3, got {tuple(p.shape)}")
    if ring_frames is None:
        ring_frames = state["ring"].shape[1] if state is not None else stream_profile_ring_frames(wf, max([p.shape[2] for p in pieces], default=0))
    ring_frames = int(ring_frames)
    if ring_frames < wf:
        raise ValueError(f"stream_profile: a ring of {ring_frames} frames cannot hold a window of {wf}")
    if state is None:
        ring, F, W = None, 0, 0
    else:
        ring, F, W = state["ring"].clone(), int(state["frames"]), int(state["windows"])
        if ring.shape[1] != ring_frames:
            raise ValueError("stream_profile: the state's ring has another length")
    outs = []
    for p in pieces:
        R, m = p.shape[0], p.shape[2]
        if ring is None:
            ring = torch.zeros((R, ring_frames, 12), dtype=torch.float64)
        c = _profile_frame_chroma(p, mode) if m else None
        for i in range(m):
            ring[:, (F + i) % ring_frames, :] = c[:, i, :]
        F += m
        W_new = _stream_windows(F, wf, sf)
        k = W_new - W
        if k > 0 and W * sf < F - ring_frames:
            raise ValueError(f"stream_profile: window {W} begins at frame {W * sf}, and the ring of {ring_frames} holds {F - ring_frames} on")
        x = torch.zeros((R, k, 12), dtype=torch.float64)
        start = (torch.arange(k) + W) * sf
        for i in range(wf if k > 0 else 0):                                                  # ascending t
            x += ring[:, (start + i) % ring_frames, :]
        if k > 0:
            outs.append(_profile_score(x, torch.ones((R, k), dtype=torch.bool), prof, sharpness))
        else:                                                                                # no window: the four outputs, empty
            outs.append((x, torch.zeros((R, 0, 24), dtype=torch.float64), torch.zeros((R, 0), dtype=torch.int32), torch.zeros((R, 0), dtype=torch.float64)))
        W = W_new
    if return_state:
        outs.append({"ring": ring, "frames": F, "windows": W})
    return outs


def stream_tuning(pieces, min_strength=0.0, state=None, return_state=False):
    """Float64 model of ``ake_stream_frame_stats_f32``'s tuning part: ``pieces`` as in ``stream_profile`` -> a list with one
    ``(cents, strength)``, float64 (R,), per piece: ``estimate_tuning`` over every frame up to and including that piece.

    Carried between pieces: the three sums ``P_j`` (R, 3).  Per frame ``p_j(t)`` is the sum of ``expm1(L) ** 2`` over the bins
    ``k = j (mod 3)`` in ascending k, and ``P_j += p_j(t)`` in ascending t; the two numbers then follow from ``P`` by
    ``estimate_tuning``'s formulas.  The doubles are ``estimate_tuning``'s, added in another order.  ``state`` / ``return_state``: the sums
    (R, 3) float64."""
    pieces = [torch.as_tensor(p).detach().to(device="cpu", dtype=torch.float64) for p in pieces]
    if float(min_strength) != float(min_strength):
        raise ValueError("stream_tuning: min_strength is NaN")
    sums = None if state is None else torch.as_tensor(state).detach().to(torch.float64).clone()
    outs = []
    for p in pieces:
        if p.dim() != 3 or p.shape[1] % TUNING_BINS_PER_SEMITONE != 0 or p.shape[:2] != pieces[0].shape[:2]:
            raise ValueError(f"stream_tuning: every piece must be (R, n_bins, m) with n_bins a multiple of 3, got {tuple(p.shape)}")
        R, P, m = p.shape
        if sums is None:
            sums = torch.zeros((R, 3), dtype=torch.float64)
        power = torch.expm1(p) ** 2
        for j in range(3):
            pj = torch.zeros((R, m), dtype=torch.float64)
            for k in range(j, P, 3):                                                         # ascending k
                pj += power[:, k, :]
            for t in range(m):                                                               # ascending t
                sums[:, j] += pj[:, t]
        outs.append(_tuning_finish(sums[:, 0].clone(), sums[:, 1].clone(), sums[:, 2].clone(), min_strength))
    if return_state:
        outs.append(sums if sums is not None else torch.zeros((0, 3), dtype=torch.float64))
    return outs


# ---- key changes to the frame on frames and labels that arrive in pieces (ake_stream_key_changes_f32) ----

def stream_changes_ready(labels, frames, window_frames, stride_frames, slack_frames, finishing=False):
    """``B``: how many boundaries of a stream are final once ``labels`` = L windows have their label (``key_id`` without the smoother,
    ``smooth_key_id`` with it, which trails the windows by the lag until the flush) and ``frames`` = F frames are final.

    Boundary w lies between the windows w and w + 1.  By ``key_changes`` it depends on ``labels[w-1 .. w+2]``, on the frames
    ``lo .. hi - 1`` with ``hi <= m_{w+1} + slack`` (``m_w = w * stride_frames + window_frames // 2``), and at the recording's end on
    ``T_r`` and the window count.  It is final iff ``w + 2 < L`` and ``F >= m_{w+1} + slack_frames`` -- nothing that arrives later can
    then change what ``key_changes`` reads for it -- or the stream is ``finishing`` and ``w + 1 < L``: then ``T_r = F`` and the window
    count is L, as offline.  Both conditions hold for a prefix of the boundaries, so B is a count, monotone in L, F and ``finishing``; a
    push emits the boundaries ``B_before .. B - 1``, each once and for good."""
    L, F, wf, sf, slack = int(labels), int(frames), int(window_frames), int(stride_frames), int(slack_frames)
    if L < 0 or F < 0 or wf < 1 or sf < 1 or slack < 0:
        raise ValueError("stream_changes_ready: labels, frames and slack_frames must be >= 0, window_frames and stride_frames >= 1")
    if finishing:
        return max(L - 1, 0)
    # F >= (w + 1) * sf + wf // 2 + slack  <=>  w + 1 <= (F - wf // 2 - slack) // sf
    by_frames = (F - wf // 2 - slack) // sf if F >= wf // 2 + slack else 0
    return max(min(L - 2, by_frames), 0)


def stream_changes_ring_frames(window_frames, stride_frames, slack_frames, lag_windows, max_new_frames):
    """Rows a stream's chroma ring needs for ``stream_key_changes`` when no piece brings more than ``max_new_frames`` frames and the
    labels trail the windows by ``lag_windows`` (0 without the smoother):
    ``max_new_frames + max(sf + 2 * slack, wf - wf // 2 + (lag + 2) * sf + slack) - 1``, at least 1.

    With ``F_old`` frames, ``W_old = track_counts(F_old)`` windows and ``L_old >= W_old - lag`` labels before a piece,
    ``B = stream_changes_ready(L_old, F_old)`` is the oldest boundary the piece can make final, and its span begins at
    ``max(m_B - slack, 0)``; after the piece's frames are written the ring must still hold that frame, so it needs
    ``F - max(m_B - slack, 0)`` rows with ``F <= F_old + max_new_frames``.  Boundary B was not final, for one of two reasons.  Its frames
    had not arrived: ``F_old <= m_{B+1} + slack - 1 = m_B + sf + slack - 1``, so ``F - (m_B - slack) <= max_new_frames + sf + 2 * slack - 1``.
    Or its labels had not: ``B >= L_old - 2 >= W_old - lag - 2``, and window ``W_old`` was not complete, ``W_old * sf + wf >= F_old + 1``,
    so ``m_B >= F_old + 1 - wf - (lag + 2) * sf + wf // 2`` and ``F - (m_B - slack) <= max_new_frames + wf - wf // 2 + (lag + 2) * sf +
    slack - 1``.  Either bound is attained, so the rule is tight."""
    wf, sf, slack, lag, m = int(window_frames), int(stride_frames), int(slack_frames), int(lag_windows), int(max_new_frames)
    if wf < 1 or sf < 1 or slack < 0 or lag < 0 or m < 0:
        raise ValueError("stream_changes_ring_frames: window_frames and stride_frames must be >= 1, slack_frames, lag_windows and max_new_frames >= 0")
    return max(m + max(sf + 2 * slack, wf - wf // 2 + (lag + 2) * sf + slack) - 1, 1)


def stream_changes_labels_carried(window_frames, stride_frames, slack_frames):
    """How many decided labels a stream must carry between pieces for ``stream_key_changes`` at the most: those from window ``B - 1`` on,
    with ``B = stream_changes_ready(L, F)`` the first boundary that is not final, ``L - B + 1`` of them:
    ``3 + max(0, (slack - 1 - (wf - wf // 2)) // sf)``.

    Either B waits for a label, ``B >= L - 2``: 3 labels.  Or it waits for its frames, ``F <= m_{B+1} + slack - 1``; the L windows lie
    inside the F frames, ``(L - 1) * sf + wf <= F``, so ``(L - B - 2) * sf <= slack - 1 - (wf - wf // 2)``.  A label ring of that many
    slots and a piece's new labels (``ake_stream_key_changes_f32``'s ``label_ring``) keeps the slots a piece reads apart from the ones
    it writes."""
    wf, sf, slack = int(window_frames), int(stride_frames), int(slack_frames)
    if wf < 1 or sf < 1 or slack < 0:
        raise ValueError("stream_changes_labels_carried: window_frames and stride_frames must be >= 1 and slack_frames >= 0")
    return 3 + max(0, (slack - 1 - (wf - wf // 2)) // sf)


def stream_key_changes(pieces, window_frames, stride_frames, slack_frames=None, profiles="krumhansl", compression="log", ring_frames=None,
                       state=None, return_state=False):
    """Float64 model of ``ake_stream_frame_stats_f32``'s chroma part followed by ``ake_stream_key_changes_f32``: ``pieces`` is a sequence
    of ``(frames, labels, finishing)`` -- the next (R, n_bins, m) log-CQT frames of R recordings in lockstep, the next (R, k) integer
    labels of their windows (the windows ``L .. L + k - 1``, any k >= 0 whose windows lie inside the frames so far) and whether the
    recordings end with this piece -> a list with one ``(first_boundary, change_frame int32 (R, b), gain (R, b), contrast (R, b))`` per
    piece, the last two float64: the b boundaries that piece made final (``stream_changes_ready``).  Joined over the pieces they are
    ``key_changes`` on the joined frames and labels, with ``counts`` = the frames and ``window_counts`` = the labels at the end, to the
    bit: the same additions in the same order.

    Between pieces the model keeps what the kernels keep: the ring of per-frame chroma of ``stream_profile`` (``ring_frames`` rows,
    default: every frame of all pieces; a boundary whose first frame has been overwritten is a ``ValueError``), the labels from window
    ``B - 1`` on, and the host's integers: the frames F, the labels L and the boundaries B so far.  ``slack_frames`` defaults to
    ``stride_frames``.  ``state`` / ``return_state``: continue from, and return as a last list element, the carried state
    (``{"ring", "labels", "frames", "windows", "boundaries"}``, ``labels`` a list per recording that begins at window
    ``max(boundaries - 1, 0)``)."""
    wf, sf = int(window_frames), int(stride_frames)
    if wf < 1 or sf < 1:
        raise ValueError("stream_key_changes: window_frames and stride_frames must be >= 1")
    slack = sf if slack_frames is None else int(slack_frames)
    if slack < 0:
        raise ValueError("stream_key_changes: slack_frames must be >= 0")
    mode = _profile_compression(compression)
    prof = key_profile_table(profiles)
    pieces = [(torch.as_tensor(p).detach().to(device="cpu", dtype=torch.float64), torch.as_tensor(l).detach().cpu().to(torch.int64), bool(f))
              for p, l, f in pieces]
    for p, l, _ in pieces:
        if p.dim() != 3 or p.shape[1] % TUNING_BINS_PER_SEMITONE != 0 or p.shape[:2] != pieces[0][0].shape[:2] or l.dim() != 2 or l.shape[0] != p.shape[0]:
            raise ValueError(f"stream_key_changes: a piece is (R, n_bins, m) frames with n_bins a multiple of 3 and (R, k) labels, got "
                             f"{tuple(p.shape)} and {tuple(l.shape)}")
    if state is None:
        ring, carried, F, L, B = None, None, 0, 0, 0
        if ring_frames is None:
            ring_frames = max(sum(p.shape[2] for p, _, _ in pieces), 1)
    else:
        ring, carried, F, L, B = state["ring"].clone(), [list(row) for row in state["labels"]], int(state["frames"]), int(state["windows"]), int(state["boundaries"])
        ring_frames = ring.shape[1] if ring_frames is None else ring_frames
        if ring.shape[1] != ring_frames:
            raise ValueError("stream_key_changes: the state's ring has another length")
    ring_frames = int(ring_frames)
    outs = []
    for p, l, finishing in pieces:
        R, m, k = p.shape[0], p.shape[2], l.shape[1]
        if ring is None:
            ring, carried = torch.zeros((R, ring_frames, 12), dtype=torch.float64), [[] for _ in range(R)]
        c = _profile_frame_chroma(p, mode) if m else None
        for i in range(max(m - ring_frames, 0), m):
            ring[:, (F + i) % ring_frames, :] = c[:, i, :]
        F += m
        first_label = L - len(carried[0])                                                    # the window carried[r][0] belongs to
        for r in range(R):
            carried[r] += l[r].tolist()
        L += k
        if L > 0 and (L - 1) * sf + wf > F:
            raise ValueError(f"stream_key_changes: window {L - 1} ends at frame {(L - 1) * sf + wf}, and the stream has {F}")
        B_new = stream_changes_ready(L, F, wf, sf, slack, finishing)
        b = B_new - B
        frame = torch.full((R, b), -1, dtype=torch.int32)
        gain, contrast = torch.zeros((R, b), dtype=torch.float64), torch.zeros((R, b), dtype=torch.float64)
        if b > 0 and max(B * sf + wf // 2 - slack, 0) < F - ring_frames:
            raise ValueError(f"stream_key_changes: boundary {B} reads from frame {max(B * sf + wf // 2 - slack, 0)} on, and the ring of "
                             f"{ring_frames} holds {F - ring_frames} on")
        for r in range(R):
            lab = _OffsetList(carried[r], first_label)
            for w in range(B, B_new):
                span = _key_change_span(lab, w, L, F, wf, sf, slack)
                if span is None:
                    continue
                ka, kb, m0, lo, hi = span
                rows = ring[r:r + 1, torch.arange(lo, hi) % ring_frames, :]                  # (1, hi - lo, 12)
                s = _profile_score(rows, torch.ones((1, hi - lo), dtype=torch.bool), prof, 1.0)[1][0]
                d = (s[:, ka] - s[:, kb]).tolist()
                frame[r, w - B], gain[r, w - B], contrast[r, w - B], _ = _key_change_scan(d, m0, lo, hi, sf)
        outs.append((B, frame, gain, contrast))
        B = B_new
        keep_from = max(B - 1, 0)
        carried = [row[keep_from - first_label:] for row in carried]
    if return_state:
        outs.append({"ring": ring, "labels": carried, "frames": F, "windows": L, "boundaries": B})
    return outs


class _OffsetList:
    """``lab[v]`` of a list that begins at window ``first``."""

    def __init__(self, items, first):
        self.items, self.first = items, first

    def __getitem__(self, v):
        if v < self.first:
            raise IndexError(f"the label of window {v} is no longer carried (from {self.first} on)")
        return self.items[v - self.first]
