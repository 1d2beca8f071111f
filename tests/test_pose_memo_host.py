"""The pose memo's bookkeeping (csrc/ss_memo.hpp) on its own, without HIP: tests/pose_memo_host.cpp - a stand-alone program
that drives the memo with the scripted walk of tests/test_vector.py's pose-cache test (stand still, leave and come back,
silence after the duration, a sound change, a scene change), a full pool whose rows freed by a tag change serve the same step,
pools too small and then grown, and two seeded walks, against a model of the reference's per-pose dicts written in the same
program - built with AddressSanitizer and UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("pose_memo") / "pose_memo_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "pose_memo_host.cpp"), "-o", out])
    return out


def test_memo_equals_the_reference_model_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pose memo: ok" in r.stdout and "FAIL" not in r.stdout
    assert r.stdout.count("walk seed") == 2
