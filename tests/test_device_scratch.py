"""csrc/device_scratch.h and csrc/pinned_buffer.h on the CPU: the scoped owner of device allocations, the grow-only device
and pinned buffers of a context and the error macros, compiled against a counting stand-in for the HIP runtime (tests/fake_include/hip_stub) with the address and undefined-behaviour sanitizers
and run as a program of its own (tests/cpp/device_scratch_test.cpp holds the assertions)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "fake_include", "hip_stub")
HEADERS = [os.path.join(ROOT, "art_planner_amd", "csrc", h) for h in ("device_scratch.h", "pinned_buffer.h")]


def test_header_compiles_alone():
    """each of the two: nothing but the HIP runtime header and the standard library, no artp_ctx, no other header of csrc/"""
    for header in HEADERS:
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + STUB, "-include", header, "-x", "c++",
                            os.devnull],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_device_scratch_under_sanitizers(tmp_path):
    exe = str(tmp_path / "device_scratch_test")
    # the sanitizer runtimes are linked into the program: it needs nothing preloaded and runs beside whatever is
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + STUB, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "device_scratch_test.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_scratch ok" in r.stdout
