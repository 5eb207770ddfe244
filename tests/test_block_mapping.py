"""The XCD block mapping of the kernels (yasph2d_amd/csrc/sphx_xcd.hpp) on the host: the header is compiled as plain C++ into a
small driver (tests/block_mapping_driver.cpp) with g++, like the oracle, and checked exhaustively.  Placement is a speed hint,
but only if the map is a bijection of the grid's blocks: a block mapped twice (or not at all) processes a particle range twice
(or never), silently."""
import os
import shutil
import subprocess

import pytest
from util import xcd_groups, xcd_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
XCD_SHIFT_MAX = 20
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the block-mapping driver"
    exe = str(tmp_path_factory.mktemp("block_mapping") / "block_mapping_driver")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "block_mapping_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout

    return run


def test_header_max_matches():
    src = open(os.path.join(CSRC, "sphx_xcd.hpp")).read()
    assert f"constexpr int XCD_SHIFT_MAX = {XCD_SHIFT_MAX};" in src


@pytest.mark.parametrize("check", ["perm_exhaustive", "perm_sampled", "scatter", "eighths"])
def test_mapping(driver, check):
    """perm_exhaustive: every grid 8 per, per in [1, 4096], every shift in [0, XCD_SHIFT_MAX], both directions, is a bijection of
    [0, grid).  perm_sampled: the same up to per = 65 536 (the 128 M particle grid).  scatter: the scatter's derived shift
    (shift - 2 over 1 024-particle blocks) and its packed argument, over its grids.  eighths: a grid of fewer than 8 << shift
    blocks gets the contiguous-eighths map (the default shift 7 below 1 024 blocks)."""
    rc, out = driver(check)
    assert rc == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) > 0


def test_shift_clamp(driver):
    """SPHX_XCD_CHUNK goes through xcd_shift_clamp: shifts of 29 and more would shift 32-bit operands by their width or more."""
    values = [-(2**31), -40, -1, 0, 1, 7, XCD_SHIFT_MAX - 1, XCD_SHIFT_MAX, XCD_SHIFT_MAX + 1, 28, 29, 31, 32, 40, INT_MAX]
    rc, out = driver("clamp", *values)
    assert rc == 0
    assert [int(v) for v in out.split()] == [min(max(v, 0), XCD_SHIFT_MAX) for v in values]


@pytest.mark.parametrize("grid", [8, 24, 8 * 9, 8 * 130, 8 * 1000, 8 * 1153])
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("rev", [0, 1])
def test_python_restatement_matches_header(driver, grid, shift, rev):
    """tests/util.py's xcd_map / xcd_groups (used by the GPU tests to pick scene sizes at which the chunked branch and the shorter
    last group are live) equal the header's map."""
    rc, out = driver("map", grid, rev, shift)
    assert rc == 0
    assert [int(v) for v in out.split()] == [xcd_map(b, grid, rev, shift) for b in range(grid)]


def test_default_shift_groups():
    """The arithmetic the comments state: with the default shift 7 a grid below 1 024 blocks has no full chunk; 9 blocks per XCD
    at shift 3 give one chunk of 8 and a last group of 1."""
    assert xcd_groups(8 * 127, 7) == (0, 127)
    assert xcd_groups(8 * 128, 7) == (1, 0)
    assert xcd_groups(8 * 9, 3) == (1, 1)
