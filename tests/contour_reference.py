"""The contour contract of include/sphx.h (sphx_surface_contour / sphx_contour_chain, "free-surface extraction") restated in numpy.

* `contour32` is marching squares over a lattice of fp32 values in the contract's order of operations: b = f >= iso (NaN outside), case
  c = b0 | b1<<1 | b2<<2 | b3<<3, the saddles resolved by the centre ((f0+f1)+(f2+f3))*0.25f, the crossing of an edge a-b (a = the node
  of the lower lattice index) at t = (iso - f_a) / (f_b - f_a), p = a + t*(b - a), one fp32 rounding per operation.  numpy rounds every
  float32 operation correctly and never fuses, so it reproduces the device bit for bit.  Segments come cell after cell.
* `chain` is the stitching rule, with Python dicts (float == on both coordinates: NaN matches nothing, -0 matches +0).
* `lines_of`, `shoelace` and `dangling` serve the properties the tests assert.

numpy only; the lattice values come from the caller (hand-made, sample_reference.sample32, or a device's own download).
"""
import numpy as np

F = np.float32
EDGE_B, EDGE_R, EDGE_T, EDGE_L = 0, 1, 2, 3
# case -> [(from, to), ...]; the saddles (5, 10) are listed as (centre inside, centre outside)
SEGMENTS = {1: [(EDGE_B, EDGE_L)], 2: [(EDGE_R, EDGE_B)], 4: [(EDGE_T, EDGE_R)], 8: [(EDGE_L, EDGE_T)], 3: [(EDGE_R, EDGE_L)],
            6: [(EDGE_T, EDGE_B)], 12: [(EDGE_L, EDGE_R)], 9: [(EDGE_B, EDGE_T)], 14: [(EDGE_L, EDGE_B)], 13: [(EDGE_B, EDGE_R)],
            11: [(EDGE_R, EDGE_T)], 7: [(EDGE_T, EDGE_L)]}
SADDLES = {5: ([(EDGE_B, EDGE_R), (EDGE_T, EDGE_L)], [(EDGE_B, EDGE_L), (EDGE_T, EDGE_R)]),
           10: ([(EDGE_R, EDGE_T), (EDGE_L, EDGE_B)], [(EDGE_R, EDGE_B), (EDGE_L, EDGE_T)])}


def _cross(xa, ya, xb, yb, fa, fb, iso):
    with np.errstate(all="ignore"):
        t = ((iso - fa).astype(F) / (fb - fa).astype(F)).astype(F)
        return np.stack([(xa + (t * (xb - xa).astype(F)).astype(F)).astype(F), (ya + (t * (yb - ya).astype(F)).astype(F)).astype(F)], -1)


def contour32(values, x0, y0, dx, dy, nx, ny, iso):
    """-> dict(segments [n, 2, 2] float32, cell [n] uint32, count, case [cells] (the case of every cell), centre_inside [cells])."""
    iso = F(iso)
    if nx < 2 or ny < 2:
        return dict(segments=np.zeros((0, 2, 2), F), cell=np.zeros(0, np.uint32), count=0, case=np.zeros(0, np.int64), centre_inside=np.zeros(0, bool))
    f = np.asarray(values, F).reshape(ny, nx)
    xs = (F(x0) + (np.arange(nx, dtype=F) * F(dx)).astype(F)).astype(F)
    ys = (F(y0) + (np.arange(ny, dtype=F) * F(dy)).astype(F)).astype(F)
    shape = (ny - 1, nx - 1)
    f0, f1, f2, f3 = (np.ascontiguousarray(a).ravel() for a in (f[:-1, :-1], f[:-1, 1:], f[1:, 1:], f[1:, :-1]))
    xl, xr = (np.broadcast_to(a[None, :], shape).ravel() for a in (xs[:-1], xs[1:]))
    yb, yt = (np.broadcast_to(a[:, None], shape).ravel() for a in (ys[:-1], ys[1:]))
    with np.errstate(invalid="ignore", over="ignore"):
        b = [(v >= iso) for v in (f0, f1, f2, f3)]  # (a comparison with NaN is False: outside)
        centre = ((((f0 + f1).astype(F) + (f2 + f3).astype(F)).astype(F) * F(0.25)).astype(F)) >= iso
    case = b[0].astype(np.int64) | b[1].astype(np.int64) << 1 | b[2].astype(np.int64) << 2 | b[3].astype(np.int64) << 3
    cells = len(case)
    # the crossing of every edge of every cell (only those of differing nodes are used)
    P = np.zeros((4, cells, 2), F)
    P[EDGE_B] = _cross(xl, yb, xr, yb, f0, f1, iso)
    P[EDGE_R] = _cross(xr, yb, xr, yt, f1, f2, iso)
    P[EDGE_T] = _cross(xl, yt, xr, yt, f3, f2, iso)
    P[EDGE_L] = _cross(xl, yb, xl, yt, f0, f3, iso)
    frm, to, cnt = np.zeros((cells, 2), np.int64), np.zeros((cells, 2), np.int64), np.zeros(cells, np.int64)
    for c, segs in SEGMENTS.items():
        m = case == c
        frm[m, 0], to[m, 0], cnt[m] = segs[0][0], segs[0][1], 1
    for c, (inside, outside) in SADDLES.items():
        for segs, m in ((inside, (case == c) & centre), (outside, (case == c) & ~centre)):
            for k in range(2):
                frm[m, k], to[m, k] = segs[k]
            cnt[m] = 2
    ci, k = np.nonzero(np.arange(2)[None, :] < cnt[:, None])  # (C order: cell after cell, then the segment within the cell)
    seg = np.stack([P[frm[ci, k], ci], P[to[ci, k], ci]], 1).astype(F)
    return dict(segments=seg, cell=ci.astype(np.uint32), count=len(ci), case=case, centre_inside=centre)


def _key(p):
    x, y = float(p[0]), float(p[1])
    if x != x or y != y:
        return None
    return (x + 0.0, y + 0.0)  # (-0.0 == 0.0 and hashes alike)


def chain(segments):
    """-> (order [n] uint32, line_first [lines + 1] uint32, closed [lines] bool) by the rule of sphx_contour_chain."""
    seg = np.asarray(segments, F).reshape(-1, 4)
    n = len(seg)
    starts, ends, cursor = {}, set(), {}
    skey, ekey = [_key(s[0:2]) for s in seg], [_key(s[2:4]) for s in seg]
    for i in range(n):
        if skey[i] is not None:
            starts.setdefault(skey[i], []).append(i)
        if ekey[i] is not None:
            ends.add(ekey[i])
    used = np.zeros(n, bool)

    def successor(s):
        e = ekey[s]
        run = starts.get(e) if e is not None else None
        if run is None:
            return None
        at = cursor.get(e, 0)
        while at < len(run) and used[run[at]]:
            at += 1
        cursor[e] = at
        return run[at] if at < len(run) else None

    order, first, closed = [], [], []

    def follow(s0, may_close):
        first.append(len(order))
        s, last = s0, s0
        while s is not None:
            used[s] = True
            order.append(s)
            last = s
            s = successor(s)
        closed.append(bool(may_close and seg[s0, 0] == seg[last, 2] and seg[s0, 1] == seg[last, 3]))

    for i in range(n):
        if not used[i] and not (skey[i] is not None and skey[i] in ends):
            follow(i, False)
    for i in range(n):
        if not used[i]:
            follow(i, True)
    first.append(n)
    return np.array(order, np.uint32).reshape(-1), np.array(first, np.uint32), np.array(closed, bool).reshape(-1)


def lines_of(segments, chained=None):
    """The polylines: (list of [k, 2] point arrays — the first segment's start, then every end — and the closed flags)."""
    seg = np.asarray(segments, F).reshape(-1, 2, 2)
    order, first, closed = chain(seg) if chained is None else chained
    return [np.concatenate([seg[order[first[k]:first[k] + 1], 0], seg[order[first[k]:first[k + 1]], 1]]) for k in range(len(closed))], list(closed)


def shoelace(points):
    """Signed area (float64) of the polygon through `points` (closed implicitly); counter-clockwise is positive."""
    p = np.asarray(points, np.float64)
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def enclosed_area(segments):
    """Sum of the signed areas of the closed lines (inside on the left: outer rings count positive, holes negative)."""
    lines, closed = lines_of(segments)
    return sum(shoelace(l[:-1]) for l, c in zip(lines, closed) if c)


def dangling(segments):
    """(starts that are no segment's end, ends that are no segment's start), as counts, by bit-level point equality (no NaN expected)."""
    seg = np.asarray(segments, F).reshape(-1, 4)
    s = {_key(p) for p in seg[:, 0:2]}
    e = {_key(p) for p in seg[:, 2:4]}
    return len(s - e), len(e - s)
