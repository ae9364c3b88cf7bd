"""CPU: the arithmetic every device search is planned with (csrc/search_plan.hpp: the
partial-list shapes of the MFMA and VALU exact kernels, the visited-table size, the
workspace layout), checked by the stand-alone host program tests/cpp/test_search_plan.cpp
built with AddressSanitizer and UBSan: invariants swept over batch sizes, row counts and
k (every row in exactly one block, every list in exactly one merge group, regions
aligned, disjoint and in order), and fixed cases of the expressions the plans came from."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_search_plan.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_search_plan")


def build_search_plan() -> str:
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", CPP, "-o", EXE], check=True)
    return EXE


def test_search_plan_invariants_and_fixed_cases_on_cpu_under_sanitizers():
    out = subprocess.run([build_search_plan()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
