"""Per-particle flow fields of a tiled run without a GPU: the C ABI exports the calls and checks its first argument, and the argument
behind consequence (b) of the contract (include/sphx.h, "per-particle flow fields of a tiled run") holds for the float32 restatement:
a tile that orders its particles by (Morton cell, id) like the single context does, and carries a ghost band of at least one
smoothing length, computes for every particle it owns the bits the uncut state gives — the neighbours of an owned particle are all
there, and they come in the same relative order, so every fp32 sum takes the same steps."""
import ctypes as C

import numpy as np
import pytest

import fields_reference as fr
import yasph2d_amd as y
from render_multi_reference import morton
from tiles_reference import cell_coord
from util import dam_break
from yasph2d_amd import _lib

F = np.float32


def test_symbols_exported_and_null_multi_rejected(sphx_lib):
    for name in ("sphx_multi_particle_fields", "sphx_tile_owned_count", "sphx_tile_particle_fields_enqueue", "sphx_tile_particle_fields_fetch"):
        assert hasattr(sphx_lib, name) and name in _lib.SIGNATURES, name
    d = np.zeros(4, F)
    out = _lib.SphxMultiFieldsOut(divergence=d.ctypes.data)
    n = C.c_uint64(4)
    assert sphx_lib.sphx_multi_particle_fields(None, 0, C.byref(out), C.byref(n)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_multi_particle_fields(None, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert n.value == 4 and not d.any()
    assert sphx_lib.sphx_tile_owned_count(None, None) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_tile_particle_fields_enqueue(None, 1, 0) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_tile_particle_fields_fetch(None, None, None, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert C.sizeof(_lib.SphxMultiFieldsOut) == 6 * C.sizeof(C.c_void_p)
    assert _lib.FIELD_BITS == dict(vel_grad=1, divergence=2, vorticity=4, color_grad=8) and tuple(_lib.FIELD_BITS) == y.FIELD_NAMES
    from yasph2d_amd.multi import MultiSolver

    assert hasattr(MultiSolver, "fields") and "fields" in vars(y.DFSPHMultiSolver)


def _oracle_state(steps):
    from oracle.oracle import Oracle

    pos, boundary = dam_break(1.0)
    o = Oracle()
    o.set_boundary(boundary)
    o.set_particles(pos)
    for _ in range(steps):
        o.dfsph_step()
    return dict(pos=o.positions(), vel=o.velocities(), density=o.densities(), boundary=o.boundary())


def _ordered(st, ids, keep, bkeep):
    """the particles `keep` of a state in (Morton cell, id) order with the boundary particles `bkeep` in the caller's order"""
    idx = np.nonzero(keep)[0]
    key = morton(cell_coord(st["pos"][idx], 0), cell_coord(st["pos"][idx], 1))
    idx = idx[np.lexsort((ids[idx], key))]
    return dict(pos=st["pos"][idx], vel=st["vel"][idx], density=st["density"][idx], boundary=st["boundary"][bkeep]), ids[idx]


@pytest.mark.parametrize("steps", [1, 60])
def test_owned_entries_of_hand_cut_strips_equal_the_uncut_state(steps):
    K = fr.Constants(y.default_params())
    st = _oracle_state(steps)
    n = len(st["pos"])
    ids = np.arange(n, dtype=np.uint32)  # (the oracle keeps the upload order)
    cx, bcx = cell_coord(st["pos"], 0), cell_coord(st["boundary"], 0)
    whole, whole_ids = _ordered(st, ids, np.ones(n, bool), np.ones(len(bcx), bool))
    counts, lists = fr.host_neighbours(K, whole["pos"], whole["boundary"])
    ref = fr.fields32(K, whole, counts, lists)
    by_id = np.argsort(whole_ids, kind="stable")
    cut, band = int(np.median(cx)), 2  # two cell columns of ghosts: every neighbour lies within one smoothing length = one cell
    seen = np.zeros(n, np.int64)
    for lo, hi in ((0, cut), (cut, 1 << 16)):
        keep = (cx >= lo - band) & (cx < hi + band)
        part, part_ids = _ordered(st, ids, keep, (bcx >= lo - band) & (bcx < hi + band))
        own = (cell_coord(part["pos"], 0) >= lo) & (cell_coord(part["pos"], 0) < hi)
        assert own.any() and (~own).any(), "the strip was meant to hold owned particles and ghosts"
        pc, pl = fr.host_neighbours(K, part["pos"], part["boundary"])
        got = fr.fields32(K, part, pc, pl)
        for f in fr.NAMES:
            a, b = got[f][own].view(np.uint32), ref[f][by_id][part_ids[own]].view(np.uint32)
            assert np.array_equal(a, b), (steps, (lo, hi), f, int((a != b).sum()))
        # a ghost at the outer edge of the band misses neighbours: its answer is not the particle's, which is why a ghost is never answered
        edge = ~own & ((cell_coord(part["pos"], 0) == lo - band) | (cell_coord(part["pos"], 0) == hi + band - 1))
        if edge.any():
            assert (pc[edge, 1] <= counts[by_id][part_ids[edge], 1]).all()
            assert not np.array_equal(got["color_grad"][edge].view(np.uint32), ref["color_grad"][by_id][part_ids[edge]].view(np.uint32))
        seen[part_ids[own]] += 1
    assert (seen == 1).all()
    assert np.abs(ref["color_grad"]).max() > 1.0 and (steps == 1 or np.abs(ref["vorticity"]).max() > 0.0)
