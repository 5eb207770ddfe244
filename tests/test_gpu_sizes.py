"""Particle counts at the kernels' granularity, each against the oracle bit for bit: waves of 64 and workgroups of 256, the list
window of LIST_HALO = 116 slots either side (LIST_WIN = 488), the scatter's 1 024-particle blocks, grids rounded up to 8 blocks,
and the paired 16-byte loads (gat2) of [N|B] arrays of odd and even length, which read one record past an odd-length array and
take pairs that straddle the fluid/boundary split.  Each scene is a lattice blob of exactly N fluid particles over exactly B
boundary particles, uploaded into a fresh context (capacity = N), then stepped with the adaptive timer."""
import numpy as np
import pytest
from util import assert_same_state, lattice_scene, step_pair, xcd_groups

import yasph2d_amd as y
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 115, 116, 117, 255, 256, 257, 487, 488, 489, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
BOUNDARY = [0, 1, 37, 90]  # none, one, odd, even: N + B takes both parities for every N


def run_scene(n, b, steps=4):
    pos, boundary = lattice_scene(n, b)
    assert len(pos) == n and len(boundary) == b
    ctx, o = y.SphxContext(), Oracle()
    if b:
        ctx.set_boundary(boundary)
        o.set_boundary(boundary)
    ctx.upload(pos)
    o.set_particles(pos)
    timer = y.TimeManager()
    for s in range(steps):
        step_pair(ctx, o, timer, what=f"N {n} B {b} step {s}")
    assert_same_state(ctx, o, f"N {n} B {b}")


@pytest.mark.parametrize("b", BOUNDARY)
@pytest.mark.parametrize("n", SIZES)
def test_size_edges(n, b):
    run_scene(n, b)


@pytest.mark.parametrize("b", BOUNDARY)
@pytest.mark.parametrize("n", [4097, 10239])
def test_size_edges_chunked_mapping(monkeypatch, n, b):
    """SPHX_XCD_CHUNK=1: chunks of two blocks, so that the chunked branch and the last, shorter group of the block mapping are both
    live at these small grids (3 and 5 blocks per XCD)."""
    full, r = xcd_groups(((n + 255) // 256 + 7) & ~7, 1)
    assert full >= 1 and r >= 1
    monkeypatch.setenv("SPHX_XCD_CHUNK", "1")
    run_scene(n, b)
