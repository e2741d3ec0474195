"""The batched reader's pure header on the CPU: pyrecode_amd/csrc/rc_read_plan.h as the C++ itself (tests/native/read_plan_check.cpp - a
stand-alone program, also under AddressSanitizer / UBSan) against verdict and copy-back tables written out by hand in that program."""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "native", "read_plan_check.cpp")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_read_plan_header_against_the_written_out_tables(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there).  The program compares every answer of the header with its tables; its exit status is the verdict."""
    exe = tmp_path / "read_plan_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC] + flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == "ok"
