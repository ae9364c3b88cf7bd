"""CPU: the int8 sketch quantiser and its error bound (csrc/sketch.hpp), the header
function the sketch kernel and the prefiltered search share, checked by the stand-alone
host program tests/cpp/test_sketch_bound.cpp built with AddressSanitizer and UBSan:
random, heavy-tailed, denormal, all-zero and non-finite rows against 1,000 random unit
queries each, |q.x - q.x~| <= err in f64, and err = +inf for rows without a sketch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_sketch_bound.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_sketch_bound")


def build_sketch_bound() -> str:
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    CPP, "-o", EXE], check=True)
    return EXE


def test_sketch_bound_holds_on_cpu_under_sanitizers():
    out = subprocess.run([build_sketch_bound()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
