"""The LDS plan of the displacement kernels (glimpse_amd/csrc/glh_displace_plan.h) on the CPU:
tests/hostcheck/displace_plan_hostcheck.cpp, a stand-alone program, forms the plan the launch uses for every template of
3 .. 63 a side and every reach of 1 .. 32 per axis on both paths (7.6 million plans) and requires that the parts of the
region are aligned and do not overlap, that every LDS word and byte the integer kernel's loops read in a window row lies
inside the row's pitch, that the float path's pitch holds a row and is nxo modulo 32, and that the region stays within
the limit.  It is built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Test-only: the product
runs this code on the host, before the launch, and in the kernels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "displace_plan_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "displace_plan_hostcheck")
LDS_LIMIT = 160 * 1024


def test_every_plan_keeps_the_kernels_reads_inside_lds():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC] + [os.path.join(ROOT, "glimpse_amd", "csrc", name) for name in ("glh_displace_plan.h", "glh_displace.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
    largest = {name: int(size) for name, size in re.findall(r"largest (\w+) (\d+) bytes", run.stdout)}
    assert set(largest) == {"integer", "float"} and all(64 * 1024 < v <= LDS_LIMIT for v in largest.values())
    assert f"plans {2 * 61 * 61 * 32 * 32}, float fallbacks 0" in run.stdout
