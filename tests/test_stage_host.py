"""The plain part of a staging buffer (glimpse_amd/csrc/glh_stage_layout.h: where the arrays lie, the host bytes) on the
CPU: tests/hostcheck/stage_hostcheck.cpp, a stand-alone program, drives the header the library includes -- offsets against
a sequence of StageLayout::place calls, copies of exactly count * sizeof(T) bytes, empty arrays, the total -- and the
owner that frees the library's device resources (glh_owned.h) with a release that counts.  It is built
with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Test-only: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "stage_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "stage_hostcheck")


def test_offsets_and_copies_under_the_sanitizers():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "tests", "hostcheck", "owner_cases.h"),
            *(os.path.join(ROOT, "glimpse_amd", "csrc", h) for h in ("glh_stage_layout.h", "glh_owned.h"))]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
