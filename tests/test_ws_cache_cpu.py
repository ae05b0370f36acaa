"""The policy of the library-owned workspaces (csrc/ws_cache.h: hit, grow, refusal, independent keys, concurrent use, clear) on the host:
tests/host/ws_cache_main.cpp instantiates the cache with a counting fake allocator and asserts exact call counts.  The program is built
with the host compiler under the address + undefined-behaviour sanitizers and under the thread sanitizer, and both binaries are run as
programs of their own.  Plus: the two partial-buffer size exports, which now share one dW job table, still agree on the known value."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'ws_cache_main.cpp')


def _compiler():
    for c in (os.environ.get('CXX'), 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize('sanitize', ['address,undefined', 'thread'])
def test_ws_cache_policy_under_sanitizers(tmp_path, sanitize):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no C++ compiler on this machine')
    exe = str(tmp_path / 'ws_cache_main')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=' + sanitize, '-fno-sanitize-recover=all', '-pthread',
           SRC, '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    err = str(tmp_path / 'stderr.txt')      # the cache's own lines go here; a sanitizer report too (the program redirects stderr)
    r = subprocess.run([exe, err], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = open(err).read().splitlines() if os.path.exists(err) else None
    assert r.returncode == 0, (r.stdout, lines)
    assert r.stdout.strip().splitlines()[-1] == 'ws_cache: ok', r.stdout
    # three refusals in the program: each printed its one line, with the caller's text and the size
    assert lines == ['test: no memory for buffer A (1049.6 KB)', 'test: no memory for buffer A (1049.6 KB)',
                     'test: no memory for buffer A (1053.6 KB)'], lines


def test_partial_buffer_sizes_agree():
    """fastnerf_mlp_bf16_partial_floats and fastnerf_mlp_bwd_partial_floats size the same regions from one job table (csrc/dw_pair.h): both
    return what they returned when each had a table of its own -- 157 323 264 floats on a host without a GPU (the 256-CU default, pe_pad 96)
    and on any 256-CU part; 612 992 floats per CU + 1024 x 388 for the head partials in general."""
    from fastnerf import _lib
    lib = _lib.lib()
    ncu = int(lib.fastnerf_device_cus())
    if ncu <= 0:
        ncu = 256
    want = 612992 * ncu + 1024 * 388
    assert 612992 * 256 + 1024 * 388 == 157323264
    assert lib.fastnerf_mlp_bf16_partial_floats() == lib.fastnerf_mlp_bwd_partial_floats() == want
