"""Host wrapper of the additive synthesiser (``ake_synth_partials_f32``): lists of enveloped partials + noise -> float32 recordings on
the GPU.  The float64 model of the same formulas is ``synthetic.synth_partials_reference``."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def synth_batch_partials() -> int:
    """Partials the kernel's LDS list holds; a tile that more partials overlap takes them in that many candidates at a time."""
    return int(_lib.lib().ake_synth_batch_partials())


def synth_partials(offsets, cps, phase, amp, start, end, fade, n, noise_sigma=0.0, seed=None, peak=0.0, device="cuda:0", out=None):
    """R recordings from their partials -> (R, n_max) float32 on ``device`` (a view of an (R, stride) buffer, stride = n_max rounded up
    to a multiple of 4; zeros behind every row's ``n[r]``).

    ``offsets`` int32 (R + 1,): recording r owns partials ``offsets[r]:offsets[r + 1]``.  Per partial: ``cps`` float64 cycles per sample,
    ``phase`` float64 turns, ``amp`` float32, ``start`` / ``end`` int64 (it sounds on ``start <= t < end``, clipped to the recording).
    ``fade``: samples of the raised-cosine ramp at both ends of every partial.  ``n`` int64 (R,).  ``noise_sigma`` with ``seed`` int64
    (R,): Philox4x32-10 Gaussian noise.  ``peak`` > 0: every recording is scaled to max |y| = peak.  Arrays may be numpy or tensors.
    ``out``: an (R, stride) float32 buffer on the device to write into (stride a multiple of 4, >= max n)."""
    L, dev = _lib.lib(), torch.device(device)
    as_t = lambda x, dt: torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(device=dev, dtype=dt).contiguous()
    offsets, n = as_t(offsets, torch.int32).reshape(-1), as_t(n, torch.int64).reshape(-1)
    cps, phase, amp = as_t(cps, torch.float64).reshape(-1), as_t(phase, torch.float64).reshape(-1), as_t(amp, torch.float32).reshape(-1)
    start, end = as_t(start, torch.int64).reshape(-1), as_t(end, torch.int64).reshape(-1)
    R = n.numel()
    if R < 1 or offsets.numel() != R + 1:
        raise ValueError(f"synth_partials: {R} recordings need {R + 1} offsets, got {offsets.numel()}")
    host_off = offsets.cpu()
    P = int(host_off[-1])
    if int(host_off[0]) != 0 or bool((host_off[1:] < host_off[:-1]).any()) or any(t.numel() != P for t in (cps, phase, amp, start, end)):
        raise ValueError("synth_partials: offsets must start at 0 and ascend, and every partial array must hold offsets[-1] entries")
    n_host = n.cpu()
    if bool((n_host < 0).any()):
        raise ValueError("synth_partials: negative sample count")
    n_max = int(n_host.max())
    if noise_sigma != 0.0:
        if seed is None:
            raise ValueError("synth_partials: noise needs a seed per recording")
        seed = as_t(seed, torch.int64).reshape(-1)
        if seed.numel() != R:
            raise ValueError(f"synth_partials: {R} recordings but {seed.numel()} seeds")
    else:
        seed = None
    if out is None:
        stride = max(4, (n_max + 3) // 4 * 4)
        out = torch.empty((R, stride), dtype=torch.float32, device=dev)
    else:
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != R or out.device != dev or out.stride(1) != 1:
            raise ValueError("synth_partials: out must be an (R, stride) float32 tensor on the device")
        stride = out.stride(0)
    nbytes = int(L.ake_synth_partials_workspace_bytes(R)) if peak > 0.0 else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(L.ake_synth_partials_f32(offsets.data_ptr(), ptr(cps), ptr(phase), ptr(amp), ptr(start), ptr(end), int(fade), R, n.data_ptr(),
                                            n_max, stride, float(noise_sigma), ptr(seed), float(peak), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream), "ake_synth_partials_f32")
    return out[:, :n_max]
