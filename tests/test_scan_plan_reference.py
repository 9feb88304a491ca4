"""The scan plan of the compacting stages without a device: sfm_amd/csrc/scan_plan.h built for the host and replayed as the
kernels of block_scan.h walk it (tests/native/scan_replay.h) against running sums, plain and under the sanitizers as a
stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "scan_plan_check.cpp")


def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_seeds(exe, seeds):
    for seed in seeds:
        run = subprocess.run([exe, str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
        assert int(run.stdout.split()[1]) >= 2 * 11              # the fixed block counts, random and largest counts


def test_scan_plan_against_running_sums(tmp_path):
    """The runs of the threads tile [0, n); the one-workgroup scan, out of place and in place, and both levels of the
    chunk scan at stride 1 and 2 equal a running sum, for 0, 1, 255 .. 257, 1,023 .. 1,025, 256 x 1,024 +- 1 blocks and
    seeded random block counts."""
    run_seeds(build_check(tmp_path, ["-O2"], "scan_plan_check"), (1, 2, 3))


def test_scan_plan_under_address_and_ub_sanitizers(tmp_path):
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "scan_plan_check_san")
    run_seeds(exe, (1, 2))
