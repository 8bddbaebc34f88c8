"""The one fit of the batched entry points (glimpse_amd/csrc/glh_lm.h) on the CPU: tests/hostcheck/ransac_hostcheck.cpp, a
stand-alone program, drives the header the kernels include.  Its small dense pieces (the p x p solve, the damped system,
the clamp into the bounds, the damping rule, the forward-difference step) against a plain Gaussian elimination -- sizes
1 .. 18, singular systems, steps that hit a bound -- and the whole loop (lm_begin, lm_first, lm_propose, lm_judge,
lm_finish) to its end, with a CPU function filling the sums: r = A x - b for 1, 3 and 18 parameters to the minimiser by
elimination, and one problem for every status (gtol, cap, singular, few rows, not finite, xtol).  It is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Test-only: the product never runs this code on the
CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "ransac_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "ransac_hostcheck")


def test_solve_damping_and_clamp_against_gaussian_elimination():
    """The linear fits end within 1e-7 of the minimiser by elimination, relative to its largest entry: ten times what the
    loop leaves with ftol = xtol = gtol = 1e-8 (measured and printed by the program: 4.1e-10, 6.95e-09 and 9.21e-09 for 1,
    3 and 18 parameters; the difference quotients over steps of sqrt(eps) carry 1.5e-8 of the residuals' rounding)."""
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "glimpse_amd", "csrc", "glh_lm.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
