"""The picture of a tiled run (include/sphx.h, "picture of a tiled run") restated in numpy: a tile's layer and the composite rule.

layer32(tile_download, boundary, view) is render_reference.render32 over the particles a tile OWNS, in the tile's local order, with
the local index of a fluid owner replaced by its id and the Morton code of its cell added; merge(layers) folds layers in the order
given.  No GPU, no library call: the GPU tests compare the device with this bit for bit, and tests/test_render_multi_host.py checks that
the composite of the tiles' layers is the single context's picture.
"""
import numpy as np

import render_reference as rr
from tiles_reference import cell_coord, in_rect

F = np.float32
NONE, BOUNDARY = rr.NONE, rr.BOUNDARY
OWNED = np.uint32(0x80000000)
PARTICLE_RADIUS = F(0.005)  # default_params(): particle_radius = 0.5 / sqrt(particle_density)
SMOOTHING_LENGTH = F(0.02)
GRID_MIN = (-100.0, -100.0)


def morton(cx, cy):
    """morton.rs:49-51 encode: the bits of x at the even positions, those of y at the odd ones"""
    def part1by1(v):
        v = np.asarray(v, np.uint32) & np.uint32(0xFFFF)
        v = (v ^ (v << np.uint32(8))) & np.uint32(0x00FF00FF)
        v = (v ^ (v << np.uint32(4))) & np.uint32(0x0F0F0F0F)
        v = (v ^ (v << np.uint32(2))) & np.uint32(0x33333333)
        v = (v ^ (v << np.uint32(1))) & np.uint32(0x55555555)
        return v
    return (part1by1(cy) << np.uint32(1)) | part1by1(cx)


def _cells(pos, h, grid_min):
    return cell_coord(pos, 0, grid_min[0], h=h), cell_coord(pos, 1, grid_min[1], h=h)


def cell_keys(pos, h=SMOOTHING_LENGTH, grid_min=GRID_MIN):
    """morton(cell_of(x)) per particle: the grid's fp32 cell function (tiles_reference.cell_coord) and the encode above"""
    pos = np.asarray(pos, F).reshape(-1, 2)
    return morton(*_cells(pos, h, grid_min))


def layer32(tile_download, boundary, view, particle_radius=PARTICLE_RADIUS, rect=None, h=SMOOTHING_LENGTH, grid_min=GRID_MIN):
    """One tile's layer.  tile_download: dict(pos, vel, ids) of the tile's LOCAL arrays in local order (bit 31 of an id = owned; the
    ghosts are dropped here).  boundary: the boundary particles the tile holds.  rect = (x0, x1, y0, y1), the tile's cells: only the
    boundary particles whose cell lies in it are drawn (None: all of `boundary`).  particle_radius, h, grid_min: the parameter block's
    (defaults: default_params()).  Returns dict(key uint32 [H, W], owner uint32 [H, W],
    rgba uint8 [H, W, 4])."""
    ids = np.asarray(tile_download["ids"], np.uint32)
    own = (ids & OWNED) != 0
    pos = np.asarray(tile_download["pos"], F).reshape(-1, 2)[own]
    vel = np.asarray(tile_download["vel"], F).reshape(-1, 2)[own]
    ids = ids[own] & ~OWNED
    bnd = np.asarray(boundary, F).reshape(-1, 2)
    if rect is not None and len(bnd):
        bnd = bnd[in_rect(*_cells(bnd, h, grid_min), rect)]
    r = rr.render32(dict(pos=pos, vel=vel, boundary=bnd), view, particle_radius)
    idx = r["owner"]
    fluid = idx < BOUNDARY
    owner = idx.copy()
    key = np.zeros(idx.shape, np.uint32)
    if fluid.any():
        owner[fluid] = ids[idx[fluid]]
        key[fluid] = cell_keys(pos, h, grid_min)[idx[fluid]]
    return dict(key=key, owner=owner, rgba=r["rgba"])


def owner_class(owner):
    return np.where(owner == NONE, 0, np.where(owner == BOUNDARY, 1, 2))


def merge(layers):
    """The composite rule: the layers folded in the order given.  A later layer replaces what has accumulated only where its class
    (fluid 2, boundary 1, none 0) is higher, or both are fluid and its key is strictly greater.  key, owner and rgba travel together."""
    acc = {k: np.array(v, copy=True) for k, v in layers[0].items()}
    for l in layers[1:]:
        ca, cb = owner_class(acc["owner"]), owner_class(l["owner"])
        take = (cb > ca) | ((cb == 2) & (ca == 2) & (l["key"] > acc["key"]))
        for k in acc:
            acc[k][take] = l[k][take]
    return acc


def split(state, rects, h=SMOOTHING_LENGTH, grid_min=GRID_MIN):
    """A single context's state (pos, vel, boundary in device order, ids optional) cut into the tiles of `rects` (cell rectangles
    (x0, x1, y0, y1) that partition the domain): per tile the download a tile context would give — its owned particles in their
    relative order, ids with bit 31 — and the boundary particles of its cells."""
    pos = np.asarray(state["pos"], F).reshape(-1, 2)
    vel = np.asarray(state["vel"], F).reshape(-1, 2)
    ids = np.asarray(state["ids"], np.uint32) if "ids" in state else np.arange(len(pos), dtype=np.uint32)
    bnd = np.asarray(state["boundary"], F).reshape(-1, 2)
    (cx, cy), (bx, by) = _cells(pos, h, grid_min), _cells(bnd, h, grid_min)
    out = []
    for r in rects:
        m = in_rect(cx, cy, r)
        out.append((dict(pos=pos[m], vel=vel[m], ids=ids[m] | OWNED), bnd[in_rect(bx, by, r)]))
    return out


def seam_counts(layers):
    """(pixels two or more layers show a fluid particle at, pixels whose winner is not the lowest-rank such layer, pixels whose winner is
    not the highest-rank one): what a view has to put under load before it tests the composite rule"""
    fluid = np.stack([owner_class(l["owner"]) == 2 for l in layers])
    keys = np.stack([np.where(f, l["key"].astype(np.int64), -1) for f, l in zip(fluid, layers)])
    multi = fluid.sum(axis=0) >= 2
    win = keys.argmax(axis=0)  # (strictly greater keys win; equal keys do not occur between tiles)
    lowest = fluid.argmax(axis=0)
    highest = len(layers) - 1 - fluid[::-1].argmax(axis=0)
    return int(multi.sum()), int((multi & (win != lowest)).sum()), int((multi & (win != highest)).sum())
