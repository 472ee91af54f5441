"""The index arithmetic of the lattice rows kernel (pynama_amd/csrc/pyn_lattice_rows.h) on the CPU: tools/lattice_rows_host_check.cpp
is a stand-alone program that includes the header the kernel decodes with and walks every run entry of small lattices (one rank and
z-slabs) against a brute-force CSR graph.  Built with the address and undefined-behaviour sanitizers (their runtimes linked
statically: the program needs nothing from its environment), run as its own process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_decode_against_brute_force(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in ("c++", "g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")) if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]      # (clang links its sanitizer runtimes statically anyway)
    exe = str(tmp_path / "lattice_rows_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                            "-I", os.path.join(ROOT, "pynama_amd", "csrc"), os.path.join(ROOT, "tools", "lattice_rows_host_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout + run.stderr
