"""CQT oracle (parity unpinned -- see oracle/cqt_oracle.py): self-consistency and defining properties."""
import math

import numpy as np
import pytest
import torch

from ake_amd import synthetic
from oracle import cqt_multirate_oracle as M
from oracle import cqt_oracle as O

SR, HOP = 22050, 4410


def test_geometry():
    f = O.cqt_frequencies()
    assert abs(f[0] - 32.70319566) < 1e-6 and abs(f[36] / f[0] - 2) < 1e-12 and len(f) == 288
    L = O.cqt_lengths(SR)
    assert abs(L[0] - 35022.66) < 0.01 and abs(L.sum() - 1.829e6) < 5e3      # ~1.81 M taps
    assert O.hop_for(22050, 5) == 4410 and O.hop_for(44100, 5) == 8820
    assert O.n_frames(330750, 4410) == 76                                    # 15 s clip -> T = 76
    n, w = O.filter_taps(101.5)
    assert len(n) == 101 and n[0] == -51 and n[-1] == 49 and abs(w.sum() - 50.5) < 1e-9


def test_sinusoid_peaks_at_its_bin():
    n = SR * 2
    k = 150
    f = O.cqt_frequencies()[k]
    y = 0.5 * np.sin(2 * np.pi * f * np.arange(n) / SR)
    C = np.abs(O.cqt_complex(y, SR, HOP))
    t = 4                                                                     # interior frame
    assert C[:, t].argmax() == k
    # sqrt(N_k) * A/2 for a real sinusoid of amplitude A at the bin centre
    assert abs(C[k, t] - math.sqrt(O.cqt_lengths(SR)[k]) * 0.25) / C[k, t] < 1e-3


def test_linearity_and_zero():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=SR), rng.normal(size=SR)
    Ca, Cb, Cab = (O.cqt_complex(v, SR, HOP, n_bins=72) for v in (a, b, 2 * a - 3 * b))
    assert np.abs(Cab - (2 * Ca - 3 * Cb)).max() < 1e-9
    assert np.abs(O.cqt_logmag(np.zeros(SR), SR, HOP, n_bins=72)).max() == 0


def test_fast_matmul_form_equals_direct_form():
    y, _ = synthetic.make_batch(range(2), SR * 2)
    ref = np.stack([O.cqt_logmag(v, SR, HOP) for v in y])
    fast64 = O.FastDirectCQT(SR, HOP, dtype=torch.float64)(y).numpy()
    assert np.abs(fast64 - ref).max() < 1e-10
    fast32 = O.FastDirectCQT(SR, HOP)(y).numpy()
    assert np.abs(fast32 - ref).max() / ref.max() < 1e-4


# ---- the multirate design (oracle/cqt_multirate_oracle.py), pinned on the CPU ---------------------------------------------------------
# Measure everywhere: e[k, t] = | |C_a| - |C_b| | / F_k, F_k = max|y| sqrt(N_k) / 2 (M.err_full_scale): per element and relative to the
# bin's full-scale response, so a loud component cannot hide a quiet one and a tensor of pure leakage is not blown up by its small peak.

# (half_len, beta) -> max e of the float64 model against the direct form over M.probe_set(2 s), as measured with this model (the worst
# probe in the comment).  The tests assert TWICE these: the probe set is finite, and the bound is there to notice a change of the
# design (taps, window positions, gain correction), not to certify it.  DESIGN.md section 2 carries the same figures.
DESIGN_ERR = {
    (23, 8.0): 2.88e-5,      # transition2_edge (2756.25 Hz); 2.6e-5 .. 2.9e-5 on all six transition-band tones
    (15, 8.0): 7.58e-4,      # chirp; white noise 5.3e-4
    (31, 8.0): 2.88e-5,      # transition2_edge: at 47 taps and up the decimator no longer dominates
}
_direct = {}


def _probes():
    return M.probe_set(2 * SR, SR, HOP)


def _direct_form(name, y):
    if name not in _direct:
        _direct[name] = O.cqt_complex(y, SR, HOP)
    return _direct[name]


@pytest.mark.parametrize("half_len,beta", sorted(DESIGN_ERR))
def test_multirate_design_error_against_direct_form(half_len, beta):
    model = M.MultirateCQT(SR, half_len=half_len, beta=beta)
    worst = {}
    for name, y in _probes().items():
        worst[name] = float(M.err_full_scale(model.cqt_complex(y, HOP), _direct_form(name, y), y, model.lengths).max())
        print(f"half_len {half_len} beta {beta} {name:18s} max e = {worst[name]:.3e}")
    top = max(worst, key=worst.get)
    print(f"half_len {half_len}: worst {top} {worst[top]:.3e}, bound {2 * DESIGN_ERR[(half_len, beta)]:.3e}")
    assert worst[top] < 2 * DESIGN_ERR[(half_len, beta)], (top, worst[top])
    # ... and the bound is a bound of THIS design: a 47-tap decimator is an order of magnitude better than a 31-tap one, a 63-tap one no better
    assert DESIGN_ERR[(23, 8.0)] * 5 < DESIGN_ERR[(15, 8.0)]


def test_vectorised_model_equals_the_per_bin_loop():
    """The same arithmetic twice: one matrix per (octave, phase) here, the prototype's loop over frames and bins there (both with the
    float32-rounded taps) -- equal to 1e-12 of full scale (float64 rounding in another summation order is ~1e-15)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "cqt_multirate_proto", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "cqt_multirate_proto.py"))
    proto = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(proto)
    P = M.probe_set(SR, SR, HOP)
    for name, hop, half_len in (("white", HOP, 23), ("impulse_centre_p1", 4411, 15)):
        y = P[name]
        model = M.MultirateCQT(SR, half_len=half_len, beta=8.0)
        a = model.cqt_complex(y, hop)
        b = proto.multirate_cqt(y, SR, hop, half_len=half_len, beta=8.0)
        assert a.shape == b.shape
        e = np.abs(a - b) / M.full_scale(y, model.lengths)[:, None]
        assert e.max() < 1e-12, (name, e.max())
    # frames= evaluates a subset, in the order asked for
    sub = model.cqt_complex(y, hop, frames=[3, 0])
    assert np.array_equal(sub, a[:, [3, 0]])


# max e of the float64 model (23, 8.0) against the direct form, measured with this model; asserted at twice the value as above
HOPS_QMODE_ERR = {"hop559": 1.52e-5, "hop75": 1.67e-5, "q_mode1": 1.52e-5}


def test_per_clip_hop_and_librosa09_q_against_direct_form():
    """Odd hops visit every phase table of every octave (t * hop mod 2^o); q_mode 1 changes every filter length."""
    rng = np.random.default_rng(5)
    y = rng.normal(0.0, 0.3, SR // 2) + 0.5 * np.sin(2 * np.pi * 5512.5 * np.arange(SR // 2) / SR)
    model = M.MultirateCQT(SR)
    got = {}
    for hop in (559, 75):
        got[f"hop{hop}"] = float(M.err_full_scale(model.cqt_complex(y, hop), O.cqt_complex(y, SR, hop), y, model.lengths).max())
    m1 = M.MultirateCQT(SR, q_mode=1)
    got["q_mode1"] = float(M.err_full_scale(m1.cqt_complex(y, HOP), O.cqt_complex(y, SR, HOP, q_mode="librosa09"), y, m1.lengths).max())
    assert abs(m1.lengths[0] / model.lengths[0] - O.cqt_q(36, "librosa09") / O.cqt_q(36)) < 1e-12
    for k, v in got.items():
        print(f"{k}: max e = {v:.3e}, bound {2 * HOPS_QMODE_ERR[k]:.3e}")
        assert v < 2 * HOPS_QMODE_ERR[k], (k, v)


def test_reduced_precision_modes_of_the_model():
    """The tolerance-deriving modes: float32 is ~1e-7 of full scale from the float64 model, the bf16 split (16 mantissa bits per operand,
    2^-17 relative residual) ~1e-6 -- both far inside the design error, and exactly invariant under a power-of-two gain before the log."""
    y = M.probe_set(SR, SR, HOP)["white"]
    model = M.MultirateCQT(SR)
    c64 = model.cqt_complex(y, HOP)
    c32 = model.cqt_complex(y, HOP, dtype=np.float32)
    cs = model.cqt_complex(y, HOP, dtype=np.float32, split_bf16=True)
    c5 = model.cqt_complex(y, HOP, dtype=np.float32, split_bf16=True, stages=4)
    e32, es, e5 = (float(M.err_full_scale(c, c64, y, model.lengths).max()) for c in (c32, cs, c5))
    # float32: unit roundoff 6e-8 over <= 277-tap sums of noise; split: 3 x 2^-17 = 2.3e-5 per product, averaged over the taps
    assert 0 < e32 < 1e-6 and e32 < es < 1e-5 and es <= e5 * 4 and e5 < 1e-5, (e32, es, e5)
    assert np.array_equal(model.cqt_complex(1024.0 * y, HOP, dtype=np.float32, split_bf16=True, stages=4), 1024.0 * c5)
    lm = M.logmag(c32, np.float32)
    assert lm.dtype == np.float32 and np.abs(lm - M.logmag(c64)).max() < 1e-5
    hi, lo = M.split_bf16_pair(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -3.14159]))
    assert hi[0] == 1.0 and lo[0] == 2.0 ** -8 and hi[1] == 1.0 + 2.0 ** -7 and lo[1] == -2.0 ** -9     # ties to even, residual kept
    assert abs(float(hi[2]) + float(lo[2]) + 3.14159) < 3.2 * 2.0 ** -17
