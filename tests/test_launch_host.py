"""ake::launch (csrc/common.h), the one helper every kernel of the library is launched through: a launch the runtime rejects comes back
as AKE_ERR_HIP with the kernel's name, the runtime's text and the launch geometry in ake_last_error().  tests/tools/launch_check.hip is
a stand-alone program around one launch of an empty kernel; without a GPU the runtime rejects that launch, with one it succeeds."""
import os
import shutil
import subprocess

import pytest
import torch

from conftest import REPO

CSRC = os.path.join(REPO, "audio-key-estimation_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
AKE_OK, AKE_ERR_HIP = 0, -2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_launch_reports_a_rejected_launch_by_name(tmp_path):
    exe = str(tmp_path / "launch_check")
    build = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, "-x", "hip",
                            os.path.join(REPO, "tests", "tools", "launch_check.hip"), os.path.join(CSRC, "common.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    out = dict(line.split(" ", 1) for line in run.stdout.splitlines() if " " in line)
    code, error = int(out["code"]), out.get("error", "")
    print(run.stdout)
    if torch.cuda.is_available():
        assert code == AKE_OK, error
        return
    assert code == AKE_ERR_HIP
    assert "launch_check_kernel" in error
    assert out["no_device"] and out["no_device"] in error                    # the runtime's own text
    assert "grid 1 x 1 x 1" in error and "block 64 x 1 x 1" in error and "0 B" in error
