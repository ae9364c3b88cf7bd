"""CPU: the plan of the wide-k matrix-core exact search (csrc/search_plan.hpp
plan_exact_mfma_wide: splits, partial lists, candidate pools, workspace regions), swept by
the stand-alone host program tests/cpp/test_exact_wide_plan.cpp under AddressSanitizer and
UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_exact_wide_plan.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_exact_wide_plan")


def test_exact_wide_plan_invariants_on_cpu_under_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", CPP, "-o", EXE], check=True)
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
