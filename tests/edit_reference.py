"""numpy restatement of the sphx_append / sphx_remove contract (include/sphx.h): the predicate in fp32 with IEEE comparisons, and the
host-side round trip the device calls replace — filter or concatenate the downloaded arrays.  Its own hand cases are in
tests/test_edit_host.py; tests/test_gpu_edit.py compares the device with it."""
import numpy as np

MAX_RECTS = 8
INF = float("inf")


def as_rects(rects):
    """One (x0, y0, x1, y1) tuple or a sequence of them -> float32 [k, 4].  Refuses what the library refuses: more than 8, a NaN bound."""
    r = np.asarray(rects, np.float32)
    if r.size == 0:
        return np.zeros((0, 4), np.float32)
    if r.ndim == 1:
        r = r[None, :]
    if r.ndim != 2 or r.shape[1] != 4:
        raise ValueError("rects must be [k, 4]")
    if len(r) > MAX_RECTS:
        raise ValueError("more than %d rectangles" % MAX_RECTS)
    if np.isnan(r).any():
        raise ValueError("a rectangle bound is NaN")
    return r


def in_rect(r, pos):
    """in(r, p) = p.x >= r.x0 && p.x < r.x1 && p.y >= r.y0 && p.y < r.y1 — a NaN coordinate fails every comparison."""
    p = np.asarray(pos, np.float32).reshape(-1, 2)
    x0, y0, x1, y1 = (np.float32(v) for v in r)
    with np.errstate(invalid="ignore"):
        return (p[:, 0] >= x0) & (p[:, 0] < x1) & (p[:, 1] >= y0) & (p[:, 1] < y1)


def removed_mask(pos, rects, outside=False):
    """True where the particle goes: in any rectangle — with outside=True in none (the rectangles are a keep-box; NaN particles go)."""
    p = np.asarray(pos, np.float32).reshape(-1, 2)
    hit = np.zeros(len(p), bool)
    for r in as_rects(rects):
        hit |= in_rect(r, p)
    return ~hit if outside else hit


def remove(pos, vel, ids, rects, outside=False):
    """download, filter: the survivors in their order -> (pos, vel, ids, removed)."""
    gone = removed_mask(pos, rects, outside)
    keep = ~gone
    return np.asarray(pos)[keep], np.asarray(vel)[keep], np.asarray(ids)[keep], int(gone.sum())


def append(pos, vel, ids, new_pos, new_vel, first_id):
    """download, concatenate: the new records behind the present ones, ids first_id + k (new_vel None = zero) -> (pos, vel, ids)."""
    new_pos = np.asarray(new_pos, np.float32).reshape(-1, 2)
    new_vel = np.zeros_like(new_pos) if new_vel is None else np.asarray(new_vel, np.float32).reshape(-1, 2)
    new_ids = (np.uint64(first_id) + np.arange(len(new_pos), dtype=np.uint64)).astype(np.uint32)
    return (np.concatenate([np.asarray(pos, np.float32).reshape(-1, 2), new_pos]),
            np.concatenate([np.asarray(vel, np.float32).reshape(-1, 2), new_vel]),
            np.concatenate([np.asarray(ids, np.uint32), new_ids]))
