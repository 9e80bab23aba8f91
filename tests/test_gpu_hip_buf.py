"""The sized device buffers of csrc/hip_buf.h on a device: the check program camera_calibration_amd/host/hip_buf_check.cc (built by
build.build_host_test) round-trips transfers that fit and requires every transfer, fill or copy that does not fit to be refused with
CBA_ERR_STATE, the three numbers in the error text and the device contents unchanged; alloc(0), assign, reserve, moves, the pinned
pair and the device-to-device copy are among its cases."""
import subprocess

import pytest

from camera_calibration_amd import build

pytestmark = pytest.mark.gpu


def test_hip_buf_check_program_passes():
    run = subprocess.run([build.HIP_BUF_CHECK], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "hip_buf_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
