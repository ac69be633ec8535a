"""``row_index_ok`` (csrc/kernels/common.h), the host check in front of every kernel that evaluates a ``RowIndex``:
its table of refused and accepted selectors, run on the host alone."""

import shutil

import pytest

from tests.host_check import run_host_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_row_index_ok_table_under_asan_ubsan(tmp_path):
    """Every selector a kernel would not survive is refused, each mode's boundary is accepted, and the accepted
    small Feistel selectors walk to distinct rows inside their domain: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "row_index_check", "row index check ok")
