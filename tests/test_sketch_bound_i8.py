"""CPU: the integer sketch pass's query quantisation and bound (csrc/sketch.hpp: sketch_q16
and its two int8 planes, sketch_query, sketch_upper -- the functions the prefiltered search
calls on the device), checked by the stand-alone host program
tests/cpp/test_sketch_bound_i8.cpp built with AddressSanitizer and UBSan: dims 256 to 2048,
the row families of test_sketch_bound.cpp against unit, one-hot, constant, heavy-tailed,
scaled and un-normalised queries; planes and integer sums exact, the f32 bound above the
exact pass's value in any summation order, unusable queries unfiltered."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_sketch_bound_i8.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_sketch_bound_i8")


def build_sketch_bound_i8() -> str:
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    CPP, "-o", EXE], check=True)
    return EXE


def test_sketch_bound_i8_holds_on_cpu_under_sanitizers():
    out = subprocess.run([build_sketch_bound_i8()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
