"""The layout of the table that a fuse or accumulate call puts on the device (webgpu-path-tracer_amd/csrc/ptmi_call_table.h), without a GPU: the sanitizer driver
tools/sanitize_call_table.cpp — the layout's promises over the cross product of edge counts, every part filled into a buffer of exactly the table's size and read
back — is built and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_the_sanitizer_driver_runs_clean(tmp_path):
    exe = str(tmp_path / "sanitize_call_table")
    # (the sanitizers' runtimes linked INTO the program: it needs nothing of the environment it is started in; the header needs none of ptmi_host.cpp's natives)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off",
           os.path.join(ROOT, "tools", "sanitize_call_table.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "sanitize_call_table: ok" in r.stdout, (r.returncode, r.stdout)
