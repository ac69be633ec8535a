"""Build and run one host check program of ``csrc/kernels/tests`` under ASan/UBSan: a plain executable, nothing
preloaded."""

import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host_check(tmp_path, name, ok_line):
    """Compile ``csrc/kernels/tests/<name>.cpp`` with ``-fsanitize=address,undefined`` (skip when the compiler has
    no sanitizer runtime), run it, and assert a clean exit and ``ok_line`` in its output."""
    exe = str(tmp_path / name)
    src = os.path.join(REPO, "csrc", "kernels", "tests", name + ".cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        if "sanitizer" in r.stderr or "cannot find" in r.stderr:
            pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
        raise AssertionError(r.stderr)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert ok_line in r.stdout
