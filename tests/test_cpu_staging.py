"""csrc/staging.hpp (the packed-block layout helper of the host layer) without a GPU.

tests/host/staging_layout.cpp is a stand-alone program that includes only that header:
the layouts of the api_*.cpp host entry points against offsets worked out by hand, the
properties of any sequence of takes, and every part of an exactly sized block written and
read back.  It is built with AddressSanitizer and UBSan and run as a child process.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb-ygz-slam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "staging_layout.cpp")


def test_staging_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "staging_layout")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
