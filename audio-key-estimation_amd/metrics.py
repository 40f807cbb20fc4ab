"""Key-signature table and the MIREX key score, batched.

Same results as the reference's per-sample Python loop (``PitchClassNet.mirex_score``,
models.py:1065-1116, table utils/key_signatures.py:19-42) but evaluated for the whole batch
at once on whatever device the predictions live on (no per-sample table upload, models.py:1077).
"""
from __future__ import annotations

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


def decode_keys(key, tonic):
    """(..., 12) key outputs (sigmoid) and (..., 12) tonic logits -> (key_id, sig, tonic_id, confidence), shaped like the leading dims.

    The decode of ``ake_decode_keys_f32`` in torch ops, on whatever device the tensors live on: ``sig`` (0..20) is the first-maximum
    cosine match over ``KEY_SIGNATURE_MAP`` with ``mirex_score``'s arithmetic and tie rule, ``confidence`` that cosine, ``tonic_id``
    (0..11) the first maximum of the tonic logits, and ``key_id`` the 24-way label (``KEY_NAMES``): ``12 + tonic_id`` if the tonic is the
    major tonic of row ``sig``, ``tonic_id`` if it is that tonic + 9 mod 12 (the relative minor), -1 if signature and tonic disagree.
    ``key_id``, ``sig`` and ``tonic_id`` are int32."""
    lead = key.shape[:-1]
    k2, t2 = key.reshape(-1, 12), tonic.reshape(-1, 12)
    # the cosines as sums over the 12 pitch classes in one order for every table row, so that the duplicate rows (0/12, 1/13, ...) get
    # bit-identical values and the first of them wins (a matmul may block the 21 columns differently and break such ties either way)
    table = _device_table(k2.device, k2.dtype)
    eps = 1e-8
    pn = k2.norm(dim=1, keepdim=True).clamp_min(eps)
    tn = table.norm(dim=1, keepdim=True).clamp_min(eps)
    sims = (k2[:, None, :] * table[None, :, :]).sum(dim=2) / (pn * tn.T)     # (B, 21)
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


def mirex_score(key_labels, key_preds, tonic_labels, tonic_preds, key_signature_id):
    """-> (mirex, correct, fifths, relative, parallel, other, accuracy), float32 scalars.

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
    n = float(key_preds.shape[0])
    f = lambda m: (m.sum().float() / n).float()
    mirex = (1.0 * correct.sum() + 0.5 * fifths.sum() + 0.3 * relative.sum() + 0.2 * parallel.sum()).float() / n
    return mirex.float(), f(correct), f(fifths), f(relative), f(parallel), f(other), f(full)
