"""The host plan of `glh_calib_ransac_groups` (glimpse_amd/csrc/glh_ransac_plan.h: what is refused before a device is
touched, the mask offsets, the chunking of a list of pairs) on the CPU: tests/hostcheck/ransac_pairs_hostcheck.cpp, a
stand-alone program, drives the header the library includes -- every refusal, offsets and chunk boundaries for group sizes
0, 1, 63, 64, 65 and 2^20 against brute-force restatements, the limits at 2^31 mask bytes.  It is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Test-only: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "ransac_pairs_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "ransac_pairs_hostcheck")


def test_refusals_offsets_and_chunks_under_the_sanitizers():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, *(os.path.join(ROOT, "glimpse_amd", "csrc", name) for name in ("glh_ransac_plan.h", "glh_calib.h"))]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
