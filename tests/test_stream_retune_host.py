"""No GPU: the geometry of the retuner on audio that arrives in chunks (stream.retune_final, retune_tail) and its float64 model with a
carried ring (metrics.stream_retune) against metrics.retune_reference on the whole audio, which it must equal exactly."""
import math

import numpy as np
import pytest

from ake_amd import metrics, stream

CENTS = (50.0, -50.0, 49.99, -49.99, -17.3, 0.01, -0.01, 12.5, 33.3)
N_MAX = 3000
Z = metrics.RETUNE_ZEROS


def last_inputs(rho, count):
    """floor(float(k) * inv) + Z for k < count: the last input output k reads, in the double expression the kernel's position is."""
    return np.floor(np.arange(count, dtype=np.float64) * (1.0 / rho)).astype(np.int64) + Z


@pytest.mark.parametrize("cents", CENTS)
def test_final_outputs_against_a_brute_force_count(cents):
    c, rho = metrics.retune_ratio(cents)
    assert c == float(np.float32(cents)) and abs(rho - 2.0 ** (c / 1200.0)) <= 2.0 ** -50
    last = last_inputs(rho, int(N_MAX * 1.03) + 8)
    assert bool((np.diff(last) >= 0).all())                                          # so the final outputs are a prefix
    before = 0
    for n in range(N_MAX):
        got = stream.retune_final(n, rho)
        assert got == int(np.count_nonzero(last <= n - 1)), n                        # every k tested, one by one
        assert got >= before, n                                                      # monotone
        before = got
        whole = stream.retune_final(n, rho, finished=True)
        assert whole == math.floor(float(n) * rho) and got <= whole < metrics.retune_out_len(n), n


@pytest.mark.parametrize("cents", CENTS)
def test_the_count_far_out(cents):
    _, rho = metrics.retune_ratio(cents)
    inv = 1.0 / rho
    for n in (10 ** 6 + 7, 2 ** 33 + 5):
        k = stream.retune_final(n, rho)
        assert math.floor(float(k - 1) * inv) + Z <= n - 1 < math.floor(float(k) * inv) + Z
        assert k <= stream.retune_final(n, rho, finished=True) == math.floor(float(n) * rho)


@pytest.mark.parametrize("cents", CENTS)
def test_the_tail_a_push_leaves(cents):
    _, rho = metrics.retune_ratio(cents)
    inv = 1.0 / rho
    longest = 0
    for n in range(N_MAX):
        tail = stream.retune_tail(n, rho)
        first = math.floor(float(stream.retune_final(n, rho)) * inv) - Z + 1         # the first input still to be read
        assert tail == n - min(n, max(0, first)) and 0 <= tail <= 2 * Z - 1, n
        longest = max(longest, tail)
    assert longest == 2 * Z - 1                                                      # the ring of 64 is not a sample too long for its index


def test_zero_cents_is_a_copy_and_holds_nothing():
    for n in (0, 1, 999):
        assert stream.retune_final(n, 1.0) == n == stream.retune_final(n, 1.0, finished=True) and stream.retune_tail(n, 1.0) == 0
    rng = np.random.default_rng(3)
    pieces = [rng.standard_normal(m) for m in (5, 0, 100, 1)]
    for cents in (0.0, -0.0, float("nan")):                                          # NaN reads as 0
        assert metrics.retune_ratio(cents) == (0.0, 1.0)
        outs = metrics.stream_retune(pieces, cents)
        assert len(outs) == 5 and outs[4].shape == (0,)
        assert all(np.array_equal(o, p) for o, p in zip(outs, pieces))
    whole, n_out = metrics.retune_reference(np.concatenate(pieces), float("nan"))
    assert n_out == 106 and np.array_equal(whole[:106], np.concatenate(pieces))


def test_cents_beyond_the_clamp():
    assert metrics.retune_ratio(70.0) == (50.0, metrics.RETUNE_MAX_RATIO) == metrics.retune_ratio(50.0)
    assert metrics.retune_ratio(-1e9) == (-50.0, 1.0 / metrics.RETUNE_MAX_RATIO)
    rng = np.random.default_rng(4)
    pieces = [rng.standard_normal(m) for m in (70, 3, 500)]
    for beyond, at in ((70.0, 50.0), (-51.0, -50.0)):
        assert all(np.array_equal(a, b) for a, b in zip(metrics.stream_retune(pieces, beyond), metrics.stream_retune(pieces, at)))


def test_the_library_counts_as_the_model_does():
    """ake_stream_retune_out_count is host code: given the same double it gives the model's counts, far out too."""
    from ake_amd import _lib
    L = _lib.lib()
    for cents in CENTS + (0.0, float("nan"), 80.0):
        c, rho = metrics.retune_ratio(cents)
        for n in list(range(0, N_MAX, 7)) + [10 ** 6 + 7, 2 ** 33 + 5]:
            for flush in (0, 1):
                assert L.ake_stream_retune_out_count(cents, rho, n, flush) == stream.retune_final(n, rho, bool(flush), copy=c == 0.0), (cents, n, flush)
    assert L.ake_stream_retune_out_count(10.0, 1.0, -1, 0) == -1 and L.ake_stream_retune_out_count(10.0, 1.1, 5, 0) == -1
    assert L.ake_stream_retune_state_bytes(3) == 3 * 64 * 4


def random_cut(rng, n):
    """Pieces of 0 samples, of 1 sample, shorter than the 63 a push can leave, and longer, until n samples are cut."""
    pieces = []
    while sum(pieces) < n:
        kind = int(rng.integers(0, 5))
        m = (0, 1, int(rng.integers(2, 63)), int(rng.integers(63, 200)), int(rng.integers(200, 900)))[kind]
        pieces.append(min(m, n - sum(pieces)))
    return pieces


def test_any_cut_equals_the_reference_on_the_whole_exactly():
    rng = np.random.default_rng(11)
    sizes = set()
    for trial in range(200):
        cents = CENTS[trial % len(CENTS)]
        n = int(rng.integers(1, 1600))
        x = rng.standard_normal(n)
        cut = random_cut(rng, n) if trial % 20 else [n]                              # (now and then everything at once)
        sizes.update(cut)
        ref, n_out = metrics.retune_reference(x, cents)
        at, pieces = 0, []
        for m in cut:
            pieces.append(x[at:at + m])
            at += m
        outs = metrics.stream_retune(pieces, cents)
        _, rho = metrics.retune_ratio(cents)
        assert len(outs) == len(cut) + 1
        at = 0
        for m, o in zip(cut, outs):
            assert o.shape == (stream.retune_final(at + m, rho) - stream.retune_final(at, rho),), (trial, at, m)
            at += m
        got = np.concatenate(outs)
        assert got.shape == (n_out,) == (math.floor(n * rho),), trial
        assert np.array_equal(got, ref[:n_out]), (trial, cents, cut)                 # float64, the same products in the same order
    assert {0, 1} <= sizes and any(1 < m < 63 for m in sizes) and any(m > 200 for m in sizes)
