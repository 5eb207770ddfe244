"""Reference for the edits of a tiled run (sphx_multi_append / sphx_multi_remove, include/sphx.h): the contract's equivalence says that the
state after an edit is the state that save, edit the part, load leaves.  edit_part is the middle step: it takes one part of a checkpoint
and writes the part without the removed particles and with the appended records.  Like the parser of tests/multi_state_reference.py it is
written from the layout comment at the top of yasph2d_amd/csrc/sphx_multi_state_format.hpp, not from the C++ below it.  The routing rule
and the rule of the id counter are restated here too (the C++ is yasph2d_amd/csrc/sphx_multi_edit.hpp)."""
import struct

import numpy as np

from multi_state_reference import CUTS_AT, DIGEST_AT, HEADER_BYTES, SECTIONS, TABLE_AT, digest_by_id, parse_part
from state_reference import digest

ID_LIMIT = 1 << 31


def edit_part(blob, keep_mask=None, appended=None, n_total=None):
    """blob: one part (bytes).  keep_mask: bool per particle of the part, False = removed (None: all stay).  appended: (pos [m, 2],
    vel [m, 2] or None, ids [m]) — records that go behind the survivors with kappa = stiffness = 0 (density and alpha 0 too: the loader
    does not read them).  n_total: the particle count of the whole edited run (None: this part is the whole run, or the caller edits one
    part of several and gives the new total).  -> the edited part (bytes)."""
    p = parse_part(blob)
    raw = bytes(blob)
    n = p["n_part"]
    keep = np.ones(n, bool) if keep_mask is None else np.asarray(keep_mask, bool)
    assert keep.shape == (n,)
    sec = {name: p[name][keep] for name in SECTIONS[:7]}
    if appended is not None:
        pos, vel, ids = appended
        pos = np.asarray(pos, "<f4").reshape(-1, 2)
        m = len(pos)
        vel = np.zeros((m, 2), "<f4") if vel is None else np.asarray(vel, "<f4").reshape(-1, 2)
        ids = np.asarray(ids, "<u4").reshape(m)
        assert not (ids >> 31).any() and np.isfinite(pos).all()
        zero = np.zeros(m, "<f4")
        new = dict(positions=pos, velocities=vel, particle_id=ids, density=zero, alpha=zero, kappa=zero, stiffness=zero)
        sec = {name: np.concatenate([sec[name], new[name]]) for name in sec}
    k = len(sec["particle_id"])
    if n_total is None:
        n_total = p["n_total"] - n + k
    head = bytearray(raw[:HEADER_BYTES])
    body = bytearray()
    at = HEADER_BYTES
    for s, name in enumerate(SECTIONS):
        data = (sec[name] if name != "boundary" else p["boundary"]).astype("<u4" if name == "particle_id" else "<f4").tobytes()
        dig = digest(p["boundary"].astype("<f4")) if name == "boundary" else digest_by_id(sec["particle_id"], sec[name])
        struct.pack_into("<QQQ", head, TABLE_AT + 24 * s, at, len(data), dig)
        body += data
        pad = (-len(data)) % 8
        body += b"\0" * pad
        at += len(data) + pad
    struct.pack_into("<Q", head, 16, at)  # total bytes
    struct.pack_into("<Q", head, 120, n_total)
    struct.pack_into("<I", head, 128, k)
    struct.pack_into("<Q", head, DIGEST_AT, digest(bytes(head[:DIGEST_AT])))
    out = bytes(head) + bytes(body)
    assert len(out) == at and CUTS_AT < TABLE_AT
    return out


# ---- routing: which tile owns a new record ------------------------------------------------------------------------------------------------
def cell_coord(v, grid_min, smoothing_length):
    """position -> cell index along one axis, in fp32 like the device: (v - grid_min) * (1 / h), NaN and negatives -> 0, saturating at 65535"""
    inv = np.float32(1.0) / np.float32(smoothing_length)
    c = (np.asarray(v, np.float32) - np.float32(grid_min)) * inv
    out = np.zeros(c.shape, np.int64)
    ok = c > 0
    out[ok] = np.minimum(c[ok], np.float32(65535.0)).astype(np.int64)
    return out


def layout_rects(part):
    """The tiles' cell rectangles (x0, x1, y0, y1), half-open, in ascending rank, from a parsed part's layout: strips along `axis` cut at
    cuts[], or nx columns cut at cuts[0 .. nx], column ix cut again at its own ny + 1 cuts behind them (rank = ix * ny + iy)."""
    cuts = part["cuts"]
    if part["axis"] >= 0:
        strips = [(cuts[r], cuts[r + 1]) for r in range(len(cuts) - 1)]
        return [(lo, hi, 0, 65536) if part["axis"] == 0 else (0, 65536, lo, hi) for lo, hi in strips]
    nx, ny = part["nx"], part["ny"]
    xc = cuts[:nx + 1]
    out = []
    for ix in range(nx):
        yc = cuts[nx + 1 + ix * (ny + 1):nx + 1 + (ix + 1) * (ny + 1)]
        out += [(xc[ix], xc[ix + 1], yc[iy], yc[iy + 1]) for iy in range(ny)]
    return out


def route(pos, rects, grid_min, smoothing_length):
    """owner[k] = the rank of the first rectangle that holds record k's cell (a record exactly on a cut has the cut's cell: the high side)"""
    pos = np.asarray(pos, np.float32).reshape(-1, 2)
    cx, cy = cell_coord(pos[:, 0], grid_min[0], smoothing_length), cell_coord(pos[:, 1], grid_min[1], smoothing_length)
    owner = np.full(len(pos), -1, np.int64)
    for r in reversed(range(len(rects))):
        x0, x1, y0, y1 = rects[r]
        owner[(cx >= x0) & (cx < x1) & (cy >= y0) & (cy < y1)] = r
    return owner


# ---- the id counter ------------------------------------------------------------------------------------------------------------------------------
def counter_after(ids, n):
    """after an upload of n particles: n without ids, 1 + the greatest id with them (0 for none); after a load: 1 + the greatest id"""
    if ids is None:
        return int(n)
    ids = np.asarray(ids, np.uint64)
    return int(ids.max()) + 1 if len(ids) else 0


def take_ids(counter, n_new):
    """-> (first_id, new counter), or None if an id would reach 2^31 (nothing is taken then)"""
    if counter + n_new > ID_LIMIT:
        return None
    return counter, counter + n_new
