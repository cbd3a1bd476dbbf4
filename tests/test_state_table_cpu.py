"""The host runtime's sampler table and chain-state table (csrc/host/tables.hpp) are plain C++: a stand-alone program
walks them under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_state_table_walk_is_clean_under_sanitizers(tmp_path):
    """every kind x layout x tuner at d in {1, 16, 17, 40, 200}, C in {1, 65}: what fork copies is allocated, what is
    allocated is copied or dead between steps, free covers all, and every ChainState pointer has one row"""
    exe = str(tmp_path / "state_table_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "state_table_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "660 configurations, 0 failures" in r.stdout, r.stdout
