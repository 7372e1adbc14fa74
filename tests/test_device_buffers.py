"""CPU: csrc/device_buffers.hpp, the owner of every handle's memory, against a stand-in runtime (tests/device_buffers_main.cpp): 12
allocations of mixed kinds with the failure at every position, release and destructor, no block freed twice, none left."""
import os
import subprocess

from conftest import ROOT


def test_owner_frees_everything_once_wherever_an_allocation_fails(tmp_path):
    src = os.path.join(ROOT, "tests", "device_buffers_main.cpp")
    exe = str(tmp_path / "device_buffers_main")
    # the header needs the runtime API's declarations only: a host compiler, no HIP library
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "device_buffers ok" in run.stdout


def test_owner_header_stands_alone():
    """What lets a host compiler build it: the runtime API header and the standard library, nothing of the project's."""
    text = open(os.path.join(ROOT, "stdpar-nbody_amd", "csrc", "device_buffers.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert "<hip/hip_runtime_api.h>" in includes
    assert all(i.startswith("<") for i in includes) and "<hip/hip_runtime.h>" not in includes, includes
