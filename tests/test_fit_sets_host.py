"""What `glh_calib_fit_sets` refuses before a device is touched (glimpse_amd/csrc/glh_ransac_plan.h: fs_check) on the CPU:
tests/hostcheck/fit_sets_hostcheck.cpp, a stand-alone program, drives the header the library includes -- every refusal
with its whole message, a valid call accepted before and after each.  It is built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly.  Test-only: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glimpse_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hostcheck", "fit_sets_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "fit_sets_hostcheck")


def test_every_refusal_and_its_message_under_the_sanitizers():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "glh_ransac_plan.h"), os.path.join(CSRC, "glh_calib.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and not run.stderr.strip()
