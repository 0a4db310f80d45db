"""The switch table of libivg (csrc/switches.cpp) as a stand-alone host program under the address and undefined-behaviour sanitizers:
tools/switches_check.cpp asserts the documented defaults, the IVG_DEV gate, the normalisations, the generation rule of a reload and
that the retired names select nothing.  No GPU, and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_table_defaults_dev_gate_normalisations_and_generation(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "switches_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    os.path.join(ROOT, "tools", "switches_check.cpp"), "-o", exe], check=True, timeout=300)
    # the old tables are leaked by design (a launcher on another host thread may still hold one): no leak report
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    p =subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "switches_check: 14 switches, 9 retired names ok" in p.stdout
