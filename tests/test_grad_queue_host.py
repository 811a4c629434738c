"""CPU test of the deferred gradient-reduction queue (csrc/grad_queue.h: make_rdesc, take_direct, resplit, plan_flush):
tests/host/grad_queue_test.cpp, a stand-alone program over fake addresses, built with the address and undefined-
behaviour sanitizers by the host compiler and run.  The header is host-only, so no HIP and no library is involved."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_grad_queue_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "grad_queue_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "lowlight_image_enhancement_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "grad_queue_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
