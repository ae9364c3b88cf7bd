"""CPU: team_slice (csrc/hnsw_search_team.hpp), swept by the stand-alone host program
tests/cpp/test_search_team_slices.cpp under AddressSanitizer and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_search_team_slices.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_search_team_slices")


def test_team_slices_partition_the_rows_on_cpu_under_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", CPP, "-o", EXE], check=True)
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
