"""16-bit PCM input, host side (no GPU): what a sample means, and that the ABI table names the PCM entries."""
import numpy as np
import torch

import ake_amd
from ake_amd import _lib


def test_pcm16_to_float_is_exact_on_every_value():
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    got = ake_amd.pcm16_to_float(x)
    assert got.dtype == torch.float32
    ref = x.numpy().astype(np.float64) / 32768.0
    assert np.array_equal(got.numpy().astype(np.float64), ref)       # value / 32768 is a float32 for every int16
    assert got[0].item() == -1.0 and got[-1].item() == 32767.0 / 32768.0


def test_symbol_table_holds_the_pcm_entries():
    for name in ("ake_cqt_logmag_pcm16_f32", "ake_resample_pcm16_f32", "ake_pipeline_forward_pcm16_f32", "ake_pipeline_track_pcm16_f32"):
        assert name in _lib.SYMBOLS
