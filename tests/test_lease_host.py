"""nsk::Lease / nsk::SlotLease (csrc/nsk_core.hpp) in a stand-alone host program: move, release on throw, no double release
(tests/lease_host_test.cpp; no GPU — the pool hands out host memory from its free list)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "navier_stokes_solver_amd")


def test_lease_host_program(tmp_path):
    exe = str(tmp_path / "lease_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "lease_host_test.cpp"), "-o", exe,
                           "-L" + PKG, "-lnsk_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "lease host test: ok" in out.stdout, out.stdout + out.stderr
