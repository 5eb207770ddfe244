"""The tiled gauge contract of include/sphx.h ("gauges and probes of a tiled run") restated in numpy, from the header's words alone.

* `owned` is the brute-force ownership of a ray's samples: the cell sat_u16((q - grid_min) * cell_inv) of every sample against a cell
  rectangle — what the device's lanes test.
* `intervals` turns such masks into {lo, count} and asserts fact 1 (one contiguous interval per tile) and fact 2 (every sample is owned
  exactly once) on the way.
* `part_of` is what a tile's reduce pass stores for the interval it owns; `fold` is the host fold of such parts into a record, with the
  refusals (a gap, an overlap, a wrong count).  `fold(parts)` must equal gauge_reference.reduce_one(values) bit for bit.
* The `variant` argument of fold builds the mutants tests/test_gauge_multi_host.py must see rejected.

numpy only.
"""
import numpy as np

import gauge_reference as gr

F = np.float32
NONE = gr.NONE
QNAN = gr.QNAN
PART_DTYPE = np.dtype([("lo", "<u4"), ("count", "<u4"), ("first", "<u4"), ("last", "<u4"), ("inside", "<u4"), ("f_lo", "<f4"), ("f_last", "<f4"),
                       ("f_next", "<f4")])
VARIANTS = ("contract", "next_from_owner_only", "max_for_first", "ignore_count")


class Refused(Exception):
    pass


def cells(points, gmin, cell_inv):
    """cell_of per axis, int64 [n, 2]: every operation rounded to fp32 (an overflow saturates, no NaN can arise from finite gauges)"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((np.asarray(points, F) - np.asarray(gmin, F)).astype(F) * F(cell_inv)).astype(F)
        return np.fmin(np.fmax(v, F(0.0)), F(65535.0)).astype(np.int64)


def sample_points(gauge):
    with np.errstate(over="ignore", invalid="ignore"):
        return gr.gauge_points(*gauge)


def owned(gauge, gmin, cell_inv, rect):
    """bool [n]: sample k of the gauge lies in the cell rectangle (x0, x1, y0, y1), half-open"""
    c = cells(sample_points(gauge), gmin, cell_inv)
    return (c[:, 0] >= rect[0]) & (c[:, 0] < rect[1]) & (c[:, 1] >= rect[2]) & (c[:, 1] < rect[3])


def intervals(gauge, gmin, cell_inv, rects):
    """-> int64 [len(rects), 2] of {lo, count} from the brute-force masks; asserts contiguity and that the tiles partition the samples"""
    masks = np.stack([owned(gauge, gmin, cell_inv, r) for r in rects], 0)
    assert (masks.sum(0) == 1).all(), "a sample is not owned exactly once"
    out = np.zeros((len(rects), 2), np.int64)
    for t, m in enumerate(masks):
        k = np.nonzero(m)[0]
        if len(k):
            assert k[-1] - k[0] + 1 == len(k), "the owned samples of a tile are not contiguous"
            out[t] = (k[0], len(k))
    return out


def _qnan():
    return np.array([QNAN], np.uint32).view(F)[0]


def part_of(f, lo, count, iso):
    """the sphx_gauge_part of the interval [lo, lo + count) of a gauge whose values are f"""
    f = np.asarray(f, F)
    p = np.zeros((), PART_DTYPE)
    p["lo"], p["count"] = lo, count
    p["first"] = p["last"] = NONE
    p["f_lo"] = p["f_last"] = p["f_next"] = _qnan()
    with np.errstate(invalid="ignore"):
        wet = lo + np.nonzero(f[lo:lo + count] >= F(iso))[0]
    if count:
        p["f_lo"] = f[lo]
    if len(wet):
        p["first"], p["last"], p["inside"] = wet[0], wet[-1], len(wet)
        p["f_last"] = f[wet[-1]]
        if wet[-1] + 1 < lo + count:
            p["f_next"] = f[wet[-1] + 1]
    return p


def parts_of(f, cuts, iso):
    """parts of the intervals between consecutive cuts (0 = cuts[0] <= ... <= cuts[-1] = n; equal cuts give empty parts)"""
    return np.array([part_of(f, a, b - a, iso) for a, b in zip(cuts[:-1], cuts[1:])], PART_DTYPE)


def fold(gauge, iso, parts, variant="contract"):
    """-> the gauge_reference.REC_DTYPE record of the parts, or raises Refused"""
    assert variant in VARIANTS
    n = gauge[4]
    parts = np.asarray(parts, PART_DTYPE).reshape(-1)
    live = [p for p in parts if p["count"] > 0]
    if variant != "ignore_count":
        if any(p["count"] == 0 and p["inside"] != 0 for p in parts):
            raise Refused("an empty part reports samples inside")
        at = 0
        for p in sorted(live, key=lambda p: int(p["lo"])):
            if p["lo"] > at:
                raise Refused("gap")
            if p["lo"] < at:
                raise Refused("overlap")
            at += int(p["count"])
        if at != n:
            raise Refused("gap at the end")
    wet = sorted((p for p in live if p["inside"] > 0), key=lambda p: int(p["lo"]))
    if not wet:
        return gr.reduce_one(gauge, np.full(n, _qnan(), F), iso)
    first = max(int(p["first"]) for p in wet) if variant == "max_for_first" else min(int(p["first"]) for p in wet)
    last = max(int(p["last"]) for p in wet)
    inside = sum(int(p["inside"]) for p in wet)
    holder = [p for p in wet if int(p["last"]) == last][0]
    f_last, f_next = holder["f_last"], F(0.0)
    if last + 1 < n:
        if last + 1 < int(holder["lo"]) + int(holder["count"]) or variant == "next_from_owner_only":
            f_next = holder["f_next"]
        else:
            owner = [p for p in live if int(p["lo"]) == last + 1]  # (exists where the parts tile the ray; only the mutant gets past a gap)
            f_next = owner[0]["f_lo"] if owner else _qnan()
    # the record is the rule's: formed by gauge_reference over an array that has the same inside test and the same two values
    rec = gr.reduce_one(gauge, _synthetic(n, first, last, f_last, f_next, iso), iso)
    rec["first"], rec["inside"] = first, inside
    return rec


def _synthetic(n, first, last, f_last, f_next, iso):
    """values whose `last`, f[last] and f[last + 1] are the given ones (first and inside are set by the caller)"""
    f = np.full(n, _qnan(), F)  # NaN: outside
    f[last] = f_last
    if last + 1 < n:
        f[last + 1] = f_next
    return f


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()
