"""The two float -> (bf16 hi, bf16 lo) splits of csrc/bf16_split.h give the same bits for every non-NaN float: bf16_split2 (packed
conversion, v_cvt_pk_bf16_f32) replaced bf16_bits (integer rounding, twice per value) in pc2pc_fused_kernel, whose outputs must not
change by a bit.  tests/tools/bf16_split_check.hip is a stand-alone program whose kernel walks all 2^32 bit patterns through both
halves of the pack and counts the patterns that differ; it is built here, as tests/test_launch_host.py builds launch_check.hip."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
CSRC = os.path.join(REPO, "audio-key-estimation_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_packed_split_equals_the_integer_split_on_every_finite_float(tmp_path):
    exe = str(tmp_path / "bf16_split_check")
    # the library's own flags (csrc/build.sh): the denormal mode and the contraction of v - hi are part of what is compared
    build = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-x", "hip",
                            os.path.join(REPO, "tests", "tools", "bf16_split_check.hip"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = dict(line.split(" ", 1) for line in run.stdout.splitlines() if " " in line)
    print(run.stdout)
    assert int(out["patterns"]) == 2 << 32
    assert int(out["nan_patterns"]) == 2 * 2 * ((1 << 23) - 1)                 # both signs, through both halves
    assert int(out["differ"]) == 0
