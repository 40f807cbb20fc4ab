"""No GPU: the geometry of the resampler on audio that arrives in chunks (stream.resampled_final, resample_first_input, resample_tail)
and its float64 model with a carried tail (metrics.stream_resample) against oracle.resample_oracle.prepare on the whole audio."""
import numpy as np
import pytest

from ake_amd import metrics, stream
from oracle import resample_oracle

RATE = 22050
RATES = (44100, 48000, 24000, 11025, 16000, 96000)
N_MAX = 3000
# the longest tail a push can leave, floor(2 * half / up): 2 * 20 / 1, 2 * 3200 / 147, 2 * 6400 / 147, 2 * 1600 / 147, and 20 when the
# rate goes up (half = 10 up)
LONGEST_TAIL = {44100: 40, 48000: 43, 96000: 87, 24000: 21, 11025: 20, 16000: 20}


def brute_final(n_in, up, down, half):
    """The k whose last input floor((k down + half) / up) has arrived; they form a prefix, counted one by one."""
    k = 0
    while (k * down + half) // up <= n_in - 1:
        k += 1
    return k


@pytest.mark.parametrize("rate", RATES)
def test_final_outputs_against_a_brute_force_count(rate):
    up, down, half = metrics.resample_ratio(rate, RATE)
    assert half == 10 * max(up, down) and up * rate == down * RATE
    last = 0
    for n in range(N_MAX):
        got = stream.resampled_final(n, up, down, half)
        assert got == brute_final(n, up, down, half), n
        assert got >= last, n                                                        # monotone
        last = got
        whole = stream.resampled_final(n, up, down, half, finished=True)
        assert whole == -(-n * up // down) and whole >= got, n
        if n in (0, 1, 2, 100, 333):
            assert whole == len(resample_oracle.resample_poly(np.zeros(n), rate, RATE))


def test_same_rate_passes_every_sample():
    for n in (0, 1, 999):
        assert stream.resampled_final(n, 1, 1, 10) == n == stream.resampled_final(n, 1, 1, 10, finished=True)
        assert stream.resample_tail(n, 1, 1, 10) == 0


@pytest.mark.parametrize("rate", RATES)
def test_the_tail_a_push_leaves(rate):
    up, down, half = metrics.resample_ratio(rate, RATE)
    longest = 0
    for n in range(N_MAX):
        k = stream.resampled_final(n, up, down, half)
        first = stream.resample_first_input(k, up, down, half)
        assert first == max(0, -((half - k * down) // up))
        assert first == 0 or (first * up >= k * down - half > (first - 1) * up)      # the ceiling
        tail = stream.resample_tail(n, up, down, half)
        assert tail == n - min(n, first) and 0 <= tail <= n
        longest = max(longest, tail)
    print(f"\n  STREAM RESAMPLE {rate} -> {RATE}: up {up} down {down} half {half}, longest tail {longest}")
    assert longest <= 2 * half // up + 1
    assert longest == LONGEST_TAIL[rate]


def random_cuts(rng, n):
    """Piece lengths that sum to n: zeros, ones, pieces shorter than any tail and longer ones, in random order."""
    cuts, left = [], n
    while left > 0:
        kind = rng.integers(0, 5)
        m = (0, 1, int(rng.integers(2, 20)), int(rng.integers(20, 100)), int(rng.integers(100, 600)))[kind]
        m = min(m, left)
        cuts.append(m)
        left -= m
    return cuts


@pytest.mark.parametrize("channel", [0, 1, -1])
def test_the_model_with_a_carried_tail_against_the_oracle_on_the_whole(channel):
    rng = np.random.default_rng(10 + channel)
    n, runs, worst = 900, 0, 0.0
    audio = rng.uniform(-1, 1, (2, n))
    refs = {rate: resample_oracle.prepare(audio, rate, RATE, channel) for rate in RATES + (RATE,)}
    kinds = set()
    while runs < 200:
        rate = (RATES + (RATE,))[runs % (len(RATES) + 1)]
        cuts = random_cuts(rng, n)
        kinds |= {min(c, 2) for c in cuts}
        pieces, at = [], 0
        for m in cuts:
            pieces.append(audio[:, at:at + m])
            at += m
        outs = metrics.stream_resample(pieces, rate, RATE, channel)
        assert len(outs) == len(cuts) + 1
        ref = refs[rate]
        assert sum(len(o) for o in outs) == len(ref) == stream.resampled_final(n, *metrics.resample_ratio(rate, RATE), finished=True)
        up, down, half = metrics.resample_ratio(rate, RATE)
        seen = 0
        for m, o in zip(cuts, outs):                                                 # every piece emits exactly what it made final
            before = stream.resampled_final(seen, up, down, half)
            seen += m
            assert len(o) == stream.resampled_final(seen, up, down, half) - before
        worst = max(worst, float(np.abs(np.concatenate(outs) - ref).max()))
        runs += 1
    assert kinds == {0, 1, 2}
    print(f"\n  STREAM RESAMPLE model, channel {channel}: 200 cuts, worst difference to the oracle on the whole {worst:.1e}")
    assert worst <= 1e-12


def test_a_single_channel_given_flat():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 500)
    outs = metrics.stream_resample([x[:7], x[7:7], x[7:]], 48000, RATE)
    assert float(np.abs(np.concatenate(outs) - resample_oracle.prepare(x[None], 48000, RATE, 0)).max()) <= 1e-12
