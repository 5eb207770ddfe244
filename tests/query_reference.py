"""The neighbour-query contract of include/sphx.h (sphx_query_radius / sphx_select) restated in numpy.

* `query32` is the box rule in float32: the candidates of a point are the particles of the 3x3 cells around its cell in ascending device
  index (`cells_of` and `box_pairs` of tests/sample_reference.py — the candidates of sphx_sample_points), d2 = dx*dx + dy*dy unfused,
  accepted iff d2 <= radius*radius; entries in candidate order, points in the caller's order; nearest = the first smallest d2.
* `brute32` accepts by the same fp32 test over ALL particles (no grid): what the box rule equals for radius <= 0.9 h.
* `select32` is the predicate of sphx_remove, restated: the particles it would remove, in ascending index.

Inputs are the device-order arrays of an implementation: positions and ids from download(), the boundary from download_boundary().
numpy only.
"""
import numpy as np

from sample_reference import box_pairs, cells_of

F = np.float32
NONE = 0xFFFFFFFF
INF_WORD = 0x7F800000


def _d2(q, qi, pos, j):
    dx = (pos[j, 0] - q[qi, 0]).astype(F)
    dy = (pos[j, 1] - q[qi, 1]).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)


def _csr(m, qi, j, d2, ids):
    """(query, particle, d2) triples sorted by (query, particle) -> the outputs of the contract"""
    count = np.bincount(qi, minlength=m).astype(np.uint64)
    offsets = np.concatenate(([0], np.cumsum(count))).astype(np.uint64)
    nearest = np.full(m, NONE, np.uint32)
    nearest_d2 = np.full(m, INF_WORD, np.uint32).view(F).copy()
    if len(qi):
        # the first entry of each point with the point's smallest d2 (fp32 <, candidate order: ties keep the lower index)
        o = np.lexsort((np.arange(len(qi)), d2, qi))
        first = np.concatenate(([True], qi[o][1:] != qi[o][:-1]))
        w = o[first]
        nearest[qi[w]] = j[w].astype(np.uint32)
        nearest_d2[qi[w]] = d2[w]
    return dict(offsets=offsets, index=j.astype(np.uint32), id=np.asarray(ids, np.uint32)[j], dist_sq=d2.astype(F), nearest=nearest,
                nearest_dist_sq=nearest_d2, count=int(offsets[-1]))


def _set_of(state, boundary):
    if boundary:
        pos = np.asarray(state["boundary"], F).reshape(-1, 2)
        ids = state.get("boundary_ids")
    else:
        pos = np.asarray(state["pos"], F).reshape(-1, 2)
        ids = state.get("ids")
    return pos, (np.arange(len(pos), dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32))


def query32(constants, state, points, radius, boundary=False):
    """The contract in fp32.  state: dict(pos, ids, boundary, boundary_ids) in device order -> dict of the seven outputs."""
    q = np.ascontiguousarray(points, F).reshape(-1, 2)
    pos, ids = _set_of(state, boundary)
    r2 = F(F(radius) * F(radius))
    if len(pos) == 0 or len(q) == 0:
        z = np.zeros(0, np.int64)
        return _csr(len(q), z, z, np.zeros(0, F), ids)
    qi, j = box_pairs(cells_of(constants, q), cells_of(constants, pos))
    d2 = _d2(q, qi, pos, j)
    with np.errstate(invalid="ignore"):
        ok = d2 <= r2
    return _csr(len(q), qi[ok], j[ok], d2[ok], ids)


def brute32(state, points, radius, boundary=False, chunk=512):
    """Every particle against every point by the same fp32 acceptance test (no cells) -> as query32."""
    q = np.ascontiguousarray(points, F).reshape(-1, 2)
    pos, ids = _set_of(state, boundary)
    r2 = F(F(radius) * F(radius))
    qs, js, ds = [], [], []
    for k0 in range(0, len(q), chunk):
        qq = q[k0:k0 + chunk]
        dx = (pos[None, :, 0] - qq[:, None, 0]).astype(F)
        dy = (pos[None, :, 1] - qq[:, None, 1]).astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)
            a, b = np.nonzero(d2 <= r2)
        qs.append(a + k0)
        js.append(b)
        ds.append(d2[a, b])
    return _csr(len(q), np.concatenate(qs), np.concatenate(js), np.concatenate(ds).astype(F), ids)


def pairs(res):
    """the (point, index) pairs of a result as a set-comparable int64 array"""
    m = len(res["offsets"]) - 1
    qi = np.repeat(np.arange(m, dtype=np.int64), np.diff(res["offsets"].astype(np.int64)))
    return qi * (1 << 32) + res["index"].astype(np.int64)


def select32(pos, ids, rects, outside=False):
    """in(r, p) = p.x >= r.x0 && p.x < r.x1 && p.y >= r.y0 && p.y < r.y1 in fp32 (a NaN coordinate is in no rectangle); selected iff in
    any rectangle — with outside iff in none.  x0 > x1 or y0 > y1 is empty, infinite bounds are half planes.  -> dict(index, id, count)."""
    p = np.asarray(pos, F).reshape(-1, 2)
    r = np.asarray(rects, F).reshape(-1, 4)
    assert len(r) <= 8 and not np.isnan(r).any()
    hit = np.zeros(len(p), bool)
    with np.errstate(invalid="ignore"):
        for x0, y0, x1, y1 in r:
            hit |= (p[:, 0] >= x0) & (p[:, 0] < x1) & (p[:, 1] >= y0) & (p[:, 1] < y1)
    sel = np.nonzero(~hit if outside else hit)[0].astype(np.uint32)
    return dict(index=sel, id=np.asarray(ids, np.uint32)[sel], count=len(sel))
