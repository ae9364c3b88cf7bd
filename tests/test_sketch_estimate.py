"""CPU: the walk distance of the int8 traversal (csrc/sketch.hpp: sketch_estimate,
sketch_dist_dot / sketch_dist_l2, sketch_usable -- the functions the device code calls),
checked by the stand-alone host program tests/cpp/test_sketch_estimate.cpp built with
AddressSanitizer and UBSan: exact on integer data in [-127, 127] (dims 64 to 520: the
estimate is the integer dot product, the ip / l2sq distances the f32 sums), within
qn err + qe scale of q.x and below sketch_upper on float data (dims 64 to 2048), unusable
rows and queries reported as such."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_sketch_estimate.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_sketch_estimate")


def build_sketch_estimate() -> str:
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    CPP, "-o", EXE], check=True)
    return EXE


def test_sketch_estimate_exact_and_bounded_on_cpu_under_sanitizers():
    out = subprocess.run([build_sketch_estimate()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
