"""The stream piece gather's index arithmetic (csrc/kernels/tokens_stream_gather.h), replayed on the host alone."""

import shutil

import pytest

from tests.host_check import run_host_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stream_gather_arithmetic_under_asan_ubsan(tmp_path):
    """The kernel's chunk, group and lane loops over views that check every index, a source buffer that is exactly
    the corpus's 16-byte hull and a window of exactly rows * S elements: every position written exactly once, the
    units read exactly the hulls of the clipped pieces, at both element widths, every alignment, addresses past
    2^40 included: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "tokens_stream_gather_check", "stream gather check ok")
