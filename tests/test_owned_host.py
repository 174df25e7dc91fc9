"""The ownership types of nerfpp_amd/csrc/owned.h (Buf, Scratch and the early-return macros) on the host: tests/helpers/owned_check.cpp is compiled with the host
compiler against the HIP API header alone -- no HIP library, no GPU -- and run; its exit status is the line of the first check that failed."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_owners_move_resize_and_give_back_on_every_early_return(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "owned_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nerfpp_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "owned_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "owned_check: ok" in out.stdout
