"""The environment switches of the library against the oracle, bit for bit.  Every A/B form must compute the same step as the
default one; the product defaults of large contexts (streamed list loads, nontemporal cold stores: from 4 M / 6 M particles) are
also run at small N on the irregular scenes of test_gpu_random_scenes (dense clusters at the 64 cap, the 32-bit list fallback,
rim cells, sparse directories), which the large-N tests never reach.  Switches are read by sphx_create: each case sets them
before the context is created."""
import numpy as np
import pytest
import test_gpu_random_scenes as random_scenes
from util import assert_same_state, dam_break, step_pair, xcd_groups

import yasph2d_amd as y
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

# 16 928 fluid particles: 67 blocks of 256 -> a grid of 72 = 9 blocks per XCD; the scatter's 1 024-particle blocks: 24 = 3 per XCD
SCALE = 2.05


def lockstep(pos, boundary, steps, vel=None):
    ctx, o = y.SphxContext(), Oracle()
    ctx.set_boundary(boundary)
    o.set_boundary(boundary)
    ctx.upload(pos, vel)
    o.set_particles(pos, vel)
    timer = y.TimeManager()
    stats = [step_pair(ctx, o, timer, what=f"step {s}") for s in range(steps)]
    assert_same_state(ctx, o)
    return stats


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_xcd_chunk(monkeypatch, shift):
    """SPHX_XCD_CHUNK = shift: at 9 blocks per XCD every shift >= 1 has full chunks AND a non-empty last, shorter group; shift 3
    also chunks the scatter (derived shift 1 over its 3 blocks per XCD)."""
    pos, boundary = dam_break(SCALE)
    grid = ((len(pos) + 255) // 256 + 7) & ~7
    scatter_grid = ((len(pos) + 1023) // 1024 + 7) & ~7
    full, r = xcd_groups(grid, shift)
    assert shift == 0 or (full >= 1 and r >= 1), (grid, shift, full, r)
    if shift == 3:
        sfull, sr = xcd_groups(scatter_grid, shift - 2)
        assert sfull >= 1 and sr >= 1, (scatter_grid, sfull, sr)
    monkeypatch.setenv("SPHX_XCD_CHUNK", str(shift))
    lockstep(pos, boundary, 80)


@pytest.mark.parametrize("env", [{"SPHX_ALTERNATE_SWEEP": "0"}, {"SPHX_ALTERNATE_SWEEP": "2"}, {"SPHX_LAZY_TABLE": "0"},
                                 {"SPHX_STREAM_LISTS": "1"}, {"SPHX_NT_COLD_STORES": "1"},
                                 {"SPHX_STREAM_LISTS": "1", "SPHX_NT_COLD_STORES": "1", "SPHX_XCD_CHUNK": "3"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_switch(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pos, boundary = dam_break(SCALE)
    lockstep(pos, boundary, 80)


def test_fuse_warm_off_with_warm_starts(monkeypatch):
    """SPHX_FUSE_WARM=0: the divergence warm start as a walk of its own.  The reference scene from its impact on: the divergence loop
    takes several iterations from step ~60 on, so warm starts fire."""
    monkeypatch.setenv("SPHX_FUSE_WARM", "0")
    pos, boundary = dam_break(1.0)
    stats = lockstep(pos, boundary, 90)
    assert sum(s["warmstart_divergence"] for s in stats) >= 10
    assert sum(s["divergence_iterations"] > 1 for s in stats) >= 10


PRODUCT_FORM = {"SPHX_STREAM_LISTS": "1", "SPHX_NT_COLD_STORES": "1"}


@pytest.mark.parametrize("span", [0, 64])
@pytest.mark.parametrize("seed", [0, 1, 5, 9, 12])
def test_large_n_product_form_random_scene(monkeypatch, seed, span):
    """The large-N defaults on the random clouds (test_gpu_random_scenes.test_random_scene, the same assertions)."""
    for k, v in PRODUCT_FORM.items():
        monkeypatch.setenv(k, v)
    random_scenes.test_random_scene(seed, span)


@pytest.mark.parametrize("seed", [21, 23])
def test_large_n_product_form_dense_clusters(monkeypatch, seed):
    """The same on dense clusters at the 64-neighbour cap (test_random_dense_clusters_neighbor_lists: lists and densities, both
    list_span_limit 0 and 64).  The seeds are ones whose lists are capped without the would-be panic, so that the lists and the
    densities are compared, not only an error code; the oracle confirms it first."""
    pos, vel, boundary = random_scenes.scene(100 + seed, dense=True)
    o = Oracle()
    if len(boundary):
        o.set_boundary(boundary)
    o.set_particles(pos, vel)
    o.update_neighborhood()
    assert o.neighbor_flags() == 1  # bit 0: capped lists; bit 1 (panic) clear
    for k, v in PRODUCT_FORM.items():
        monkeypatch.setenv(k, v)
    random_scenes.test_random_dense_clusters_neighbor_lists(seed)
