"""The gauge contract of include/sphx.h (sphx_gauge_levels / sphx_gauge_reduce, "gauges and probes") restated in numpy, from the header's
words alone.

* `gauge_points` are the samples of a gauge: (x0 + (float)k * dx, y0 + (float)k * dy), one fp32 rounding per operation.
* `reduce32` is the rule over given values: b_k = f_k >= iso (NaN outside), first / last / inside, and behind `last` the crossing
  t = (iso - f_a) / (f_b - f_a), p = a + t * (b - a) with a = last, b = last + 1 — numpy rounds every float32 operation correctly and never
  fuses, so it reproduces the device bit for bit.  A ray that ends wet has t = 0 and the last sample as its point; a ray with nothing
  inside holds SPHX_GAUGE_NONE and the quiet-NaN word 0x7FC00000.
* `levels32` samples with sample_reference.sample32 and reduces.
* The `variant` argument of reduce32 builds the mutants tests/test_gauge_host.py must see rejected.

numpy only.
"""
import numpy as np

import sample_reference as sr

F = np.float32
NONE = 0xFFFFFFFF
QNAN = 0x7FC00000
REC_DTYPE = np.dtype([("first", "<u4"), ("last", "<u4"), ("inside", "<u4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("f_last", "<f4"),
                      ("f_next", "<f4")])
VARIANTS = ("contract", "strict_greater", "b_lower", "fused", "float64")


def gauge_rows(gauges):
    """[g, 5] rows of x0, y0, dx, dy, n -> list of (F x0, F y0, F dx, F dy, int n)"""
    a = np.asarray(gauges, np.float64).reshape(-1, 5)
    return [(F(r[0]), F(r[1]), F(r[2]), F(r[3]), int(r[4])) for r in a]


def gauge_points(x0, y0, dx, dy, n):
    k = np.arange(n, dtype=F)
    return np.stack([(F(x0) + (k * F(dx)).astype(F)).astype(F), (F(y0) + (k * F(dy)).astype(F)).astype(F)], -1)


def _qnan():
    return np.array([QNAN], np.uint32).view(F)[0]


def _fma32(a, b, c):
    """fl32(a * b + c) with one rounding: the product of two floats is exact in float64, the sum is rounded to float64 and then to
    float32 (double rounding can only differ from a true fma in a tie no test input constructs)"""
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def reduce_one(gauge, f, iso, variant="contract"):
    x0, y0, dx, dy, n = gauge
    f = np.asarray(f, F).reshape(-1)
    assert len(f) == n and n >= 1 and variant in VARIANTS
    iso = F(iso)
    rec = np.zeros((), REC_DTYPE)
    with np.errstate(all="ignore"):
        b = (f > iso) if variant == "strict_greater" else (f >= iso)  # (a comparison with NaN is False: outside)
        wet = np.nonzero(b)[0]
        if len(wet) == 0:
            rec["first"] = rec["last"] = NONE
            for name in ("t", "x", "y", "f_last", "f_next"):
                rec[name] = _qnan()
            return rec
        first, last = int(wet[0]), int(wet[-1])
        rec["first"], rec["last"], rec["inside"] = first, last, len(wet)
        pt = lambda k: (F(x0 + F(F(k) * dx)), F(y0 + F(F(k) * dy)))
        xa, ya = pt(last)
        rec["f_last"] = f[last]
        if last == n - 1:
            rec["t"], rec["x"], rec["y"], rec["f_next"] = F(0), xa, ya, _qnan()
            return rec
        xb, yb = pt(last + 1)
        fa, fb = f[last], f[last + 1]
        rec["f_next"] = fb
        if variant == "b_lower":  # the edge written from the upper sample: a = last + 1, b = last
            t = F(F(iso - fb) / F(fa - fb))
            rec["t"], rec["x"], rec["y"] = t, F(xb + F(t * F(xa - xb))), F(yb + F(t * F(ya - yb)))
        elif variant == "fused":
            t = F(F(iso - fa) / F(fb - fa))
            rec["t"], rec["x"], rec["y"] = t, _fma32(t, F(xb - xa), xa), _fma32(t, F(yb - ya), ya)
        elif variant == "float64":
            d = np.float64
            t = (d(iso) - d(fa)) / (d(fb) - d(fa))
            rec["t"], rec["x"], rec["y"] = F(t), F(d(xa) + t * (d(xb) - d(xa))), F(d(ya) + t * (d(yb) - d(ya)))
        else:
            t = F(F(iso - fa) / F(fb - fa))
            rec["t"], rec["x"], rec["y"] = t, F(xa + F(t * F(xb - xa))), F(ya + F(t * F(yb - ya)))
    return rec


def reduce32(values, gauges, iso, variant="contract"):
    """-> REC_DTYPE array [g]; values: float32, n per gauge, gauge after gauge"""
    rows = gauge_rows(gauges)
    v = np.asarray(values, F).reshape(-1)
    assert len(v) == sum(r[4] for r in rows)
    out, at = np.zeros(len(rows), REC_DTYPE), 0
    for k, g in enumerate(rows):
        out[k] = reduce_one(g, v[at:at + g[4]], iso, variant)
        at += g[4]
    return out


def all_points(gauges):
    rows = gauge_rows(gauges)
    return np.concatenate([gauge_points(*g) for g in rows]) if rows else np.zeros((0, 2), F)


def levels32(C_, state, gauges, iso, field="fraction", kind=sr.KERNEL_WENDLAND):
    """-> (records, values) of the restated sampling (sample_reference.sample32) at the gauges' points"""
    values = sr.sample32(C_, state, all_points(gauges), kind)[field]
    return reduce32(values, gauges, iso), values


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()
