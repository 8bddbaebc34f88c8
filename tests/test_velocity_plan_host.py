"""The LDS plan of the velocity field's stack kernel (glimpse_amd/csrc/glh_velocity_plan.h) on the CPU:
tests/hostcheck/velocity_plan_hostcheck.cpp, a stand-alone program, forms the plan the launch uses for every number of
pairs of 1 .. 1024 and requires that the parts of the region are inside the allowance of 163 840 bytes, aligned and apart,
that every index the kernel's expressions form lies inside its part (it runs them over a region of exactly the plan's
size), and that the bitonic network, with the kernel's index expressions, sorts lists of every length.  It is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Test-only: the product runs this code on the host,
before the launch, and in the kernel."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "velocity_plan_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "velocity_plan_hostcheck")
LDS_LIMIT = 163840


def test_every_plan_keeps_the_stack_inside_lds():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC] + [os.path.join(ROOT, "glimpse_amd", "csrc", name) for name in ("glh_velocity_plan.h", "glh_velocity.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
    plans = {int(p): (int(length), int(nodes), int(size))
             for p, length, nodes, size in re.findall(r"pairs (\d+): len (\d+), nodes (\d+), (\d+) bytes", run.stdout)}
    assert plans[1][:2] == (1, 32) and plans[256][:2] == (256, 32) and plans[257][:2] == (512, 16)
    assert plans[1024][:2] == (1024, 8)
    assert all(size <= LDS_LIMIT for _, _, size in plans.values())
    largest = int(re.search(r"largest (\d+) bytes", run.stdout).group(1))
    assert 64 * 1024 < largest <= LDS_LIMIT
