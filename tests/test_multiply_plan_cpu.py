"""Which form of the top-n multiply runs (string_grouper_amd/csrc/sg_plan.h), without a GPU: the
stand-alone program tests/native/plan_cases.cpp holds every bar of the rule -- 0.65 / 0.45 / 0.40, 65 536 rows or 19 x 65 536
entries, 16 384 rows below the threshold, 128 entries a row, 32 768 rows and 0.004 x vocabulary for the pilot, its two looks
at the prices, 2^20 postings for the exact kernel's own index, the launch shape -- at the bar and one step under it, and every
switch once.  Built here with the host compiler (the header needs no HIP) and run; it names every case that fails.
tests/test_multiply_default_forms_gpu.py asks the library itself, on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "string_grouper_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def host_compiler():
    if shutil.which("c++"):
        return ["c++"]
    if os.path.exists(HIPCC) or shutil.which(HIPCC):
        return [HIPCC, "-x", "c++"]
    return None


def test_the_rule_at_every_bar(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "plan_cases")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "native", "plan_cases.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout
