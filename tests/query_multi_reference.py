"""Shared helpers of tests/test_gpu_query_multi.py and tests/query_multi_rank_worker.py: the contract of sphx_multi_query_radius /
sphx_multi_select (include/sphx.h, "neighbour queries of a tiled run") assembled from the single-context restatements of
tests/query_reference.py and tests/sample_reference.py, which are used as they are.

* `tile_states(m)`: every local tile's own arrays (ghosts included) and its clipped boundary with the boundary ids.
* `boundary_maps(states, boundary)`: clipped index -> index in the caller's array, recovered from the positions alone: the clipped set
  is a subsequence of the caller's array (equal positions share a cell, so they are kept or dropped together and a greedy match is exact).
* `owner_of`: the tile whose rectangle holds cells_of(q).
* `reference(...)`: query32 over the answering tile's own download per point, folded into one CSR list in the caller's order, ids translated.
numpy only.
"""
import numpy as np

import query_reference as qr
import sample_reference as sr

F = np.float32
NONE = 0xFFFFFFFF
INF_WORD = 0x7F800000
ENTRY = ("id", "dist_sq", "slot")
POINT = ("nearest_id", "nearest_slot", "nearest_dist_sq")


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind in "ui" else a.view(np.uint32)


def tile_states(m):
    out = []
    for k in range(m.info()["local_tiles"]):
        t = m.tile_context(k)
        d = t.download()
        bxy, bid = t.download_boundary()
        out.append(dict(pos=d["pos"], ids=d["ids"], boundary=bxy, boundary_ids=bid))
    return out


def boundary_maps(states, boundary):
    """per tile: uint32 [clipped count], the caller-order index of clipped boundary particle k"""
    key = np.ascontiguousarray(boundary, F).view(np.uint64).ravel()
    maps = []
    for st in states:
        n = len(st["boundary"])
        clipped = np.zeros(n, np.uint64)
        clipped[st["boundary_ids"]] = np.ascontiguousarray(st["boundary"], F).view(np.uint64).ravel()  # the clipped set in ITS caller order
        assert n == 0 or sorted(st["boundary_ids"].tolist()) == list(range(n))
        out, i = np.zeros(n, np.uint32), 0
        for k in range(n):
            while key[i] != clipped[k]:
                i += 1
            out[k] = i
            i += 1
        maps.append(out)
    return maps


def owner_of(K, rects, pts):
    c = sr.cells_of(K, pts)
    inside = np.stack([(c[:, 0] >= r[0]) & (c[:, 0] < r[1]) & (c[:, 1] >= r[2]) & (c[:, 1] < r[3]) for r in rects.tolist()], 0)
    assert (inside.sum(0) == 1).all(), "the rectangles do not partition the cell domain"
    return inside.argmax(0).astype(np.int32)


def reference(K, states, maps, owner, pts, radius, boundary=False, tiles=None):
    """The expected answer of MultiSolver.query(pts, radius, boundary, tiles=True).  tiles: the global ranks of `states` (default 0, 1, ..);
    a point whose owner is not among them gets an empty range, tile -1 and no nearest (a rank's part)."""
    m = len(pts)
    tiles = list(range(len(states))) if tiles is None else list(tiles)
    cnt = np.zeros(m, np.int64)
    res = dict(tile=np.full(m, -1, np.int32), nearest_id=np.full(m, NONE, np.uint32), nearest_slot=np.full(m, NONE, np.uint32),
               nearest_dist_sq=np.full(m, INF_WORD, np.uint32).view(F).copy())
    per = []
    for k, (t, st) in enumerate(zip(tiles, states)):
        idx = np.nonzero(owner == t)[0]
        r = qr.query32(K, st, pts[idx], radius, boundary)
        ids = r["id"] & np.uint32(0x7FFFFFFF) if not boundary else maps[k][r["id"]]
        src_ids = st["boundary_ids"] if boundary else st["ids"]
        cnt[idx] = np.diff(r["offsets"].astype(np.int64))
        res["tile"][idx] = t
        some = r["nearest"] != NONE
        res["nearest_slot"][idx] = r["nearest"]
        near = np.full(len(idx), NONE, np.uint32)
        nid = src_ids[r["nearest"][some]]
        near[some] = (nid & np.uint32(0x7FFFFFFF)) if not boundary else maps[k][nid]
        res["nearest_id"][idx] = near
        res["nearest_dist_sq"][idx] = r["nearest_dist_sq"]
        per.append((idx, r, ids))
    off = np.concatenate(([0], np.cumsum(cnt))).astype(np.uint64)
    total = int(off[-1])
    res.update(offsets=off, count=total, id=np.zeros(total, np.uint32), dist_sq=np.zeros(total, F), slot=np.zeros(total, np.uint32))
    for idx, r, ids in per:
        c = np.diff(r["offsets"].astype(np.int64))
        dst = np.repeat(off[idx].astype(np.int64), c) + (np.arange(r["count"]) - np.repeat(r["offsets"][:-1].astype(np.int64), c))
        res["id"][dst], res["dist_sq"][dst], res["slot"][dst] = ids, r["dist_sq"], r["index"]
    return res


def assert_same(got, ref, what, fields=None):
    fields = fields or [f for f in ("offsets", "tile") + ENTRY + POINT if f in got]
    assert got["count"] == ref["count"], "%s: count %d, expected %d" % (what, got["count"], ref["count"])
    for f in fields:
        a, b = bits(got[f]), bits(ref[f])
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs at %d places" % (what, f, int((a != b).sum()) if a.shape == b.shape else -1)


def point_id_pairs(res):
    """the (point, id) pairs of a result, sorted: comparable between a box walk and a search over all particles"""
    m = len(res["offsets"]) - 1
    qi = np.repeat(np.arange(m, dtype=np.int64), np.diff(res["offsets"].astype(np.int64)))
    return np.sort(qi * (1 << 32) + res["id"].astype(np.int64))
