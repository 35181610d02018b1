"""The owners of the host runtime's device and pinned memory (csrc/devmem.h), on the CPU:
tests/cpp/devmem_host.cpp defines the HIP allocation calls over malloc and drives every
owner through growth, failure, moves and destruction.  Host AddressSanitizer and UBSan
watch the run: a double free, a use after free or a leak fails the test like a wrong state."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_owners_under_host_sanitizers(tmp_path):
    exe = tmp_path / "devmem_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # the runtimes in the program: no library order to mind
                    "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "simple-raytracing-render_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "devmem_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 live at exit, 0 checks failed" in out.stdout
