"""The persistent form of the lattice rows kernel on the CPU: tools/lattice_rows_host_check.cpp includes the header the kernel
schedules and classifies with (pynama_amd/csrc/pyn_lattice_rows.h) and checks, besides the decode, that lat_rows_sched visits every
x-line exactly once for grids of 1 .. 2048 workgroups with one contiguous range of lines per XCD, and that the word of a line (class
+ end flags) equals a brute-force statement of it under structured and sampled Dirichlet sets.  Built WITHOUT the sanitizers here
(tests/test_lattice_rows_host.py runs the same program with them), run as its own process; the counts it prints are checked."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_and_line_classes(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in ("c++", "g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")) if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "lattice_rows_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pynama_amd", "csrc"),
                            os.path.join(ROOT, "tools", "lattice_rows_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout + run.stderr
    m = re.search(r"(\d+) scheduled trips, (\d+) line classes \((\d+) / (\d+) / (\d+) of class 0 / 1 / 2; class 2 reported lower: (\d+), "
                  r"class 0 or 1 reported as 2: (\d+)\)", run.stdout)
    assert m, run.stdout
    trips, lines, c0, c1, c2, unsafe, slow = map(int, m.groups())
    assert trips > 100000 and lines > 10000 and min(c0, c1, c2) > 1000     # all three classes well sampled
    assert unsafe == 0 and slow == 0
