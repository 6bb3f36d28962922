"""The mutual main pass's schedule (csrc/mutual_schedule.h), enumerated on the CPU as the kernels run it: a diagonal item sums
every ordered pair of its slice exactly once with the eight waves equally loaded, and for every slice count up to the 2^22-body
bound the units cover each slice pair once and fill whole rounds (tests/native/mutual_schedule_check.cpp).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mutual_schedule_covers_every_pair_once(tmp_path):
    exe = str(tmp_path / "mutual_schedule_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "mutual_schedule_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
