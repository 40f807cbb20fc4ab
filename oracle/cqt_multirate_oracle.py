"""Float64 model of the multirate CQT the HIP kernels evaluate.  TEST INFRASTRUCTURE ONLY.

``oracle/cqt_oracle.py`` is the *specification* (the direct form); this file restates the *algorithm* that
``ake_cqt_plan_create`` (csrc/cqt.hip, host part) builds, so that against it the kernels have no design error left, only
rounding:

* decimator: Kaiser half-band of ``half_len`` in {15, 23, 31} and ``beta``, normalised to sum 1, then the centre and the odd taps
  rounded to float32 and the even taps dropped (``DecimTaps``); level l + 1 is ``y[m] = h0 x[2m] + sum_q hodd[q] (x[2m-2q-1] +
  x[2m+2q+1])``; the signal is zero outside ``[0, n)`` at level 0 and every level is kept as far as its tail reaches;
* bank of octave o (decimation ``dec = 2^o``; the top octave is o = 0), frame t: ``c = t * hop``, ``c_int, phase = divmod(c, dec)``,
  taps ``u = -uh .. uh`` of level o around ``c_int`` at full-rate offsets ``pos = dec * u - phase``, periodic Hann
  ``0.5 - 0.5 cos(2 pi (pos - lo) / L)`` inside ``[lo, lo + L]`` with ``lo = floor(-N_k / 2)``, ``L = floor(N_k / 2) - lo``, scale
  ``dec * sqrt(N_k) / (L / 2) / cascade_gain(f_k, o)``;
* frames ``t = 0 .. n // hop``.

One matrix per (octave, phase) with the frames as rows, so 15 s clips and 592-frame songs are quick.
``tests/tools/cqt_multirate_proto.py`` keeps the per-bin loop form of the same arithmetic as the slow, obviously-right statement
(``tests/test_oracle_cqt.py`` holds the two together).

Two reduced-precision evaluation modes, still plain numpy, exist only to DERIVE TOLERANCES for the GPU tests
(``tests/test_gpu_cqt_model.py``) from the number formats instead of from what the kernels give:

* ``dtype=np.float32``: every level rounded to float32 after each stage (the stage itself a float32 running sum in tap order), bank
  tables rounded to float32, products and sums in float32 accumulated block by block over 32 taps in tap order (numpy's own float32
  reduction is pairwise, i.e. better than any kernel's order), ``sqrt`` and ``log(1 + x)`` in float32;
* ``split_bf16=True``: level samples and table entries replaced by ``hi + lo`` (both bf16, round to nearest even, ``lo = bf16(v - hi)``)
  and the ``lo * lo`` product dropped -- engine 3's bank (``store_split4``, the ``bf16_rne`` table build); ``stages=4`` applies the
  same split to the inputs and the odd taps of the first four half-band stages (engine 5's Toeplitz stages; the centre tap stays a
  float32 multiply-add there).
"""
from __future__ import annotations

import math

import numpy as np

from . import cqt_oracle as O

Q_MODES = ("librosa010", "librosa09")         # ake_cqt_config::q_mode 0 and 1


# ---- decimator ----------------------------------------------------------------------------------------------------------------

def kaiser_halfband(half_len, beta):
    """Kaiser-windowed half-band sinc, 2 * half_len + 1 taps, normalised to sum 1 (float64, before any rounding)."""
    j = np.arange(-half_len, half_len + 1, dtype=np.float64)
    h = 0.5 * np.sinc(j / 2.0) * np.kaiser(2 * half_len + 1, beta)
    return h / h.sum()


def decim_taps(half_len=23, beta=8.0):
    """``(h0, hodd)`` as ``DecimTaps`` holds them: the centre tap and the odd taps 1, 3, .. rounded to float32 (returned as float64
    values); the even taps, below 1e-17, are dropped."""
    h = kaiser_halfband(half_len, beta)
    h0 = float(np.float32(h[half_len]))
    hodd = h[half_len + 1::2].astype(np.float32).astype(np.float64)
    assert len(hodd) == (half_len + 1) // 2
    return h0, hodd


def cascade_gain(f_hz, o, sr, h0, hodd):
    """|frequency response| of the first ``o`` half-band stages at ``f_hz``, from the float32 taps the kernels keep."""
    gain = 1.0
    q = 2 * np.arange(len(hodd)) + 1
    for s in range(o):
        wn = 2.0 * math.pi * f_hz / (sr / 2.0 ** s)
        gain *= abs(h0 + 2.0 * float(np.sum(hodd * np.cos(wn * q))))
    return gain


def bf16_rne(v):
    """float -> the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split_bf16_pair(v):
    """v ~ hi + lo, both bf16: hi = bf16(v), lo = bf16(v - hi)  (|v - hi - lo| <= 2^-17 |v|)."""
    hi = bf16_rne(v)
    lo = bf16_rne(np.asarray(v, np.float64) - hi.astype(np.float64))
    return hi, lo


def decimate(y, y_lo, h0, hodd, dtype=np.float64, split=False):
    """One half-band stage.  ``y`` holds samples ``y_lo .. y_lo + len - 1`` (zero outside); returns ``(y2, y2_lo)`` on the half-rate grid,
    every output that a non-zero input can reach.  ``dtype=float32``: a float32 running sum in tap order, as the kernels' registers.
    ``split``: the odd-tap products on split-bf16 operands (three products, ``lo * lo`` dropped), the centre tap added last."""
    Hh = 2 * len(hodd) - 1
    hi = y_lo + len(y)
    m_lo = math.floor((y_lo - Hh) / 2)
    m_hi = math.ceil((hi + Hh) / 2)
    M = m_hi - m_lo
    zl = y_lo - (2 * m_lo - Hh)                                   # zeros so that ypad[0] is sample 2 m_lo - Hh ...
    zr = 2 * (m_hi - 1) + Hh + 1 - hi                             # ... and the last one sample 2 (m_hi - 1) + Hh
    ypad = np.concatenate([np.zeros(zl, dtype), np.asarray(y, dtype), np.zeros(zr, dtype)])

    def tap(j):                                                    # sample 2m + j for every output m
        return ypad[Hh + j: Hh + j + 2 * M: 2]

    acc = np.zeros(M, dtype)
    if split:
        for q, g in enumerate(hodd):
            g_hi, g_lo = split_bf16_pair(np.array([g]))
            g_hi, g_lo = dtype(g_hi[0]), dtype(g_lo[0])
            for j in (-(2 * q + 1), 2 * q + 1):
                o_hi, o_lo = split_bf16_pair(tap(j))
                o_hi, o_lo = o_hi.astype(dtype), o_lo.astype(dtype)
                acc = acc + g_hi * o_hi
                acc = acc + g_lo * o_hi
                acc = acc + g_hi * o_lo
    else:
        for q, g in enumerate(hodd):
            acc = acc + dtype(g) * (tap(-(2 * q + 1)) + tap(2 * q + 1))
    return dtype(h0) * tap(0) + acc, m_lo


# ---- the model ----------------------------------------------------------------------------------------------------------------

class MultirateCQT:
    """The plan of ``ake_cqt_plan_create`` in float64: ``cqt_complex(y, hop)`` -> complex128 (n_bins, T)."""

    def __init__(self, sr, n_bins=288, bins_per_octave=36, fmin=None, q_mode=0, half_len=23, beta=8.0):
        assert n_bins % bins_per_octave == 0, "whole octaves"
        self.sr, self.n_bins, self.bpo = int(sr), int(n_bins), int(bins_per_octave)
        self.fmin = float(fmin) if fmin and fmin > 0 else O.C1_HZ
        self.q_mode = Q_MODES[q_mode] if isinstance(q_mode, int) else q_mode
        self.half_len, self.beta = int(half_len), float(beta)
        self.h0, self.hodd = decim_taps(self.half_len, self.beta)
        self.freqs = O.cqt_frequencies(self.n_bins, self.bpo, self.fmin)
        self.lengths = O.cqt_lengths(self.sr, self.n_bins, self.bpo, self.fmin, self.q_mode)
        self.n_oct = self.n_bins // self.bpo
        self._banks = {}

    def k0(self, o):
        return self.n_bins - self.bpo * (o + 1)

    def uh(self, o):
        """Taps u = -uh .. uh of level o: the window of the octave's lowest bin (its longest filter), as ``OctDesc::uh``."""
        return math.ceil(-math.floor(-self.lengths[self.k0(o)] / 2.0) / 2 ** o) + 1

    def bank(self, o, phase):
        """(2 uh + 1, 2 bpo) float64: column 2b = real part, 2b + 1 = imaginary part of bin k0 + b at this phase."""
        key = (o, phase)
        W = self._banks.get(key)
        if W is None:
            dec = 2 ** o
            uh = self.uh(o)
            pos = dec * np.arange(-uh, uh + 1, dtype=np.float64) - phase
            ks = np.arange(self.k0(o), self.k0(o) + self.bpo)
            N = self.lengths[ks]
            lo = np.floor(-N / 2.0)
            L = np.floor(N / 2.0) - lo
            gain = np.array([cascade_gain(self.freqs[k], o, self.sr, self.h0, self.hodd) for k in ks])
            scale = dec * np.sqrt(N) / (L / 2.0) / gain
            inside = (pos[:, None] >= lo[None, :]) & (pos[:, None] <= (lo + L)[None, :])
            win = np.where(inside, 0.5 - 0.5 * np.cos(2.0 * np.pi * (pos[:, None] - lo[None, :]) / L[None, :]), 0.0)
            arg = 2.0 * np.pi * self.freqs[ks][None, :] * pos[:, None] / self.sr
            W = np.empty((2 * uh + 1, 2 * self.bpo), np.float64)
            W[:, 0::2] = scale * win * np.cos(arg)
            W[:, 1::2] = -scale * win * np.sin(arg)
            self._banks[key] = W
        return W

    def levels(self, y, dtype=np.float64, stages=0):
        """[(samples, index of the first)] for levels 0 .. n_oct - 1.  ``stages``: the first that many on split-bf16 operands."""
        lv = [(np.asarray(y, np.float64).astype(dtype), 0)]
        for s in range(self.n_oct - 1):
            lv.append(decimate(lv[-1][0], lv[-1][1], self.h0, self.hodd, dtype, split=s < stages))
        return lv

    def cqt_complex(self, y, hop, frames=None, dtype=np.float64, split_bf16=False, stages=0):
        """Complex CQT of one clip at ``hop`` (any hop >= 1, so a hop per clip is a call per clip), complex128 (n_bins, T) for the
        frames ``t = 0 .. n // hop`` or for the subset ``frames`` (any order)."""
        y = np.asarray(y, np.float64)
        hop = int(hop)
        ts = np.arange(O.n_frames(len(y), hop)) if frames is None else np.asarray(frames, np.int64)
        assert ts.size and ts.min() >= 0 and ts.max() <= len(y) // hop
        out = np.zeros((self.n_bins, len(ts)), np.complex128)
        lv = self.levels(y, dtype, stages if split_bf16 else 0)
        for o in range(self.n_oct):
            dec, uh = 2 ** o, self.uh(o)
            x, x_lo = lv[o]
            c_int, ph = np.divmod(ts * hop, dec)
            left = max(0, uh + x_lo)                                     # zeros in front: the window of the earliest centre, c_int = 0
            right = max(0, int(c_int.max()) + uh + 1 - (x_lo + len(x)))
            xp = np.concatenate([np.zeros(left, dtype), x, np.zeros(right, dtype)])
            start = c_int - uh - x_lo + left                             # index in xp of tap u = -uh
            res = np.zeros((len(ts), 2 * self.bpo), np.float64)
            for p in np.unique(ph):
                rows = np.nonzero(ph == p)[0]
                X = xp[start[rows][:, None] + np.arange(2 * uh + 1)[None, :]]
                res[rows] = _bank_product(X, self.bank(o, int(p)), dtype, split_bf16)
            k0 = self.k0(o)
            out[k0:k0 + self.bpo] = (res[:, 0::2] + 1j * res[:, 1::2]).T
        return out


def _bank_product(X, W, dtype, split):
    """X (rows, taps) @ W (taps, columns) in the given arithmetic."""
    if split:
        Xh, Xl = split_bf16_pair(X)
        Wh, Wl = split_bf16_pair(W)
        terms = ((Xh, Wh), (Xl, Wh), (Xh, Wl))
    else:
        terms = ((X, W),)
    if dtype == np.float64:
        return sum(a.astype(np.float64) @ b.astype(np.float64) for a, b in terms)
    acc = np.zeros((X.shape[0], W.shape[1]), np.float32)
    for b0 in range(0, X.shape[1], 32):                                  # a float32 accumulator over 32-tap blocks in tap order
        for a, b in terms:
            acc += a[:, b0:b0 + 32].astype(np.float32) @ b[b0:b0 + 32].astype(np.float32)
    return acc.astype(np.float64)


def logmag(C, dtype=np.float64):
    """``log(1 + |C|)``; ``dtype=float32``: squares, sum, sqrt and log(1 + x) in float32 from float32 parts (the kernels' epilogue)."""
    if dtype == np.float64:
        return np.log1p(np.abs(C))
    re, im = C.real.astype(np.float32), C.imag.astype(np.float32)
    return np.log(np.float32(1) + np.sqrt(re * re + im * im))


def cqt_complex(y, sr, hop, n_bins=288, bins_per_octave=36, fmin=None, q_mode=0, half_len=23, beta=8.0, **kw):
    return MultirateCQT(sr, n_bins, bins_per_octave, fmin, q_mode, half_len, beta).cqt_complex(y, hop, **kw)


# ---- error measure --------------------------------------------------------------------------------------------------------------

def full_scale(y, lengths):
    """F_k = A sqrt(N_k) / 2, A = max|y|: |C| of a sinusoid of amplitude A at the centre of bin k
    (tests/test_oracle_cqt.py::test_sinusoid_peaks_at_its_bin)."""
    return float(np.max(np.abs(y))) * np.sqrt(np.asarray(lengths, np.float64)) / 2.0


def err_full_scale(mag_a, mag_b, y, lengths):
    """e[k, t] = | |C_a| - |C_b| | / F_k: per element, linear domain, relative to the bin's full-scale response -- not to the tensor's
    peak, which lets a loud component hide the rest.  ``mag_*``: magnitudes (n_bins, T) (complex input is taken by modulus)."""
    a = np.abs(mag_a) if np.iscomplexobj(mag_a) else np.asarray(mag_a, np.float64)
    b = np.abs(mag_b) if np.iscomplexobj(mag_b) else np.asarray(mag_b, np.float64)
    return np.abs(a - b) / full_scale(y, lengths)[:, None]


# ---- probe signals ----------------------------------------------------------------------------------------------------------------

CASCADE_TICK = 4096            # samples per tick of the fused decimator cascade; its frontier starts at -512 (fill_cascade_on)


def probe_set(n, sr=22050, hop=4410, n_bins=288, bins_per_octave=36, seed=0):
    """name -> float64 clip of n samples: the signals where a multirate CQT goes wrong.  Seeded; the CPU design tests and the GPU
    kernel tests use the same set."""
    rng = np.random.default_rng(seed)
    f = O.cqt_frequencies(n_bins, bins_per_octave)
    ti = np.arange(n, dtype=np.float64)

    def tone(hz, amp=0.5, phase=0.3):
        return amp * np.sin(2.0 * np.pi * hz * ti / sr + phase)

    def impulse(*at):
        y = np.zeros(n)
        for i in at:
            y[i] = 1.0
        return y

    centre = hop * max(1, (n // hop) // 2)
    tick = CASCADE_TICK * max(1, (n // 2) // CASCADE_TICK) - 512
    p = {
        "tone_top": tone(f[n_bins - bins_per_octave // 2]),              # bin centres: top, a middle and the lowest octave
        "tone_mid": tone(f[n_bins // 2 + 6]),
        "tone_low": tone(f[5]),
        "above_9k5": tone(sr * 9500.0 / 22050.0, 0.8),                   # above the top bin: everything is stop-band leakage
        "above_10k9": tone(sr * 10900.0 / 22050.0, 0.8),
        "bass_treble": tone(f[10], 0.8) + tone(f[n_bins - 28], 0.8e-4),  # a treble tone 80 dB under a loud bass tone
        "impulse_0": impulse(0),
        "impulse_last": impulse(n - 1),
        "impulse_centre": impulse(centre),                               # on a frame centre and one sample either side
        "impulse_centre_m1": impulse(centre - 1),
        "impulse_centre_p1": impulse(centre + 1),
        "impulse_tick": impulse(tick),                                   # on a cascade tick boundary
        "dc": np.full(n, 0.5),
        "chirp": 0.8 * np.sin(2.0 * np.pi * (30.0 * ti / sr + 0.5 * ((sr / 2.0 - 30.0) / (n / sr)) * (ti / sr) ** 2)),
        "white": rng.normal(0.0, 0.3, n),
    }
    # tones of the lowest octave switched on and off every 0.19 s: with an edge inside every frame's window the response follows the
    # window's position to 2 / N_k of full scale per sample -- what a neighbouring phase table (a window one sample off) changes
    gate = (np.floor(ti / (0.19 * sr)) % 2 == 0).astype(np.float64)
    p["tone_bursts"] = gate * (tone(f[3], 0.3) + tone(f[19], 0.3, 1.1) + tone(f[bins_per_octave - 2], 0.3, 2.3))
    for lvl in (1, 2, 3):                                                # the transition band of each of the first three decimators
        edge = sr / 2.0 ** (lvl + 1)                                     # 5512.5 Hz for level 1 at 22.05 kHz
        p[f"transition{lvl}_edge"] = tone(edge)
        p[f"transition{lvl}_above"] = tone(edge * 5800.0 / 5512.5)
    return p
