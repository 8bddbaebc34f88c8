"""The small dense pieces of the batched fit (glimpse_amd/csrc/glh_lm.h: the p x p solve, the damped system, the clamp into
the bounds, the damping rule, the forward-difference step) on the CPU: tests/hostcheck/ransac_hostcheck.cpp, a stand-alone
program, drives the header the kernel includes against a plain Gaussian elimination -- sizes 1 .. 18, singular systems, steps
that hit a bound.  It is built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Test-only: the
product never runs this code on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "ransac_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "ransac_hostcheck")


def test_solve_damping_and_clamp_against_gaussian_elimination():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "glimpse_amd", "csrc", "glh_lm.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
