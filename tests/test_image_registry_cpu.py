"""csrc/image_registry.cpp (the address-keyed table of image attributes and pending table refreshes) and the
layer-norm tail of csrc/dppo_layout.h, checked by a stand-alone program (tests/host/image_registry_main.cpp) built
with AddressSanitizer and UBSan and run as a child process. Nothing sanitizer-related is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusionpolicyoptimization_amd", "csrc")


def test_image_registry_and_layouts(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the registry's host check needs a C++17 compiler")
    exe = str(tmp_path / "image_registry_main")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(CSRC, "image_registry.cpp"),
                            os.path.join(ROOT, "tests", "host", "image_registry_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "image registry and layouts: ok" in run.stdout
