"""Neighbour queries without a GPU: the restatement tests/query_reference.py against a brute force on the golden dam break (which pins
the box rule include/sphx.h states), the two calls' refusals without a device, and the ctypes layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import query_reference as qr
import sample_reference as sr
import yasph2d_amd as y
from yasph2d_amd import _lib

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dam_break_4050.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    st = dict(pos=g["s100_pos"].astype(F), boundary=g["in_boundary"].astype(F))
    K = sr.Constants(y.default_params())
    rng = np.random.default_rng(7)
    both = np.concatenate([st["pos"], st["boundary"]])
    lo, hi = both.min(0) - 2 * K.h, both.max(0) + 2 * K.h
    pts = [(lo + rng.random((20000, 2)) * (hi - lo)).astype(F),  # over the scene and a margin
           st["pos"][rng.choice(len(st["pos"]), 1000, replace=False)],  # on particles
           st["boundary"][rng.choice(len(st["boundary"]), 1000, replace=False)]]
    return K, st, np.concatenate(pts).astype(F)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("factor", [0.9, 0.5])
def test_box_rule_equals_brute_force_below_h(golden, factor, boundary):
    K, st, pts = golden
    r = F(K.h * F(factor))
    a, b = qr.query32(K, st, pts, r, boundary), qr.brute32(st, pts, r, boundary)
    assert a["count"] == b["count"] > 1000
    for k in a:
        x, z = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype == F:
            x, z = x.view(np.uint32), z.view(np.uint32)
        assert np.array_equal(x, z), k


def test_box_rule_at_h_is_a_subset(golden):
    """radius == h: the fluid agrees here; the boundary misses pairs a search over all particles accepts (a particle exactly h away can
    sit two cells off after the rounding of cell_of) — the box rule is the contract.  This point set: 78 of 20 167 boundary pairs."""
    K, st, pts = golden
    missed = {}
    for boundary in (False, True):
        a, b = qr.pairs(qr.query32(K, st, pts, K.h, boundary)), qr.pairs(qr.brute32(st, pts, K.h, boundary))
        assert len(np.setdiff1d(a, b)) == 0  # a subset
        missed[boundary] = len(np.setdiff1d(b, a))
    assert missed[False] == 0 and missed[True] > 0, missed


def test_reference_hand_cases():
    K = sr.Constants(y.default_params())
    h = K.h
    pos = np.array([[0.5, 0.5], [0.5, 0.5], [0.5 + 0.25 * h, 0.5], [0.7, 0.7]], F)
    st = dict(pos=pos, ids=np.array([7, 5, 9, 11], np.uint32), boundary=np.zeros((0, 2), F))
    q = np.array([[0.5, 0.5], [np.nan, 0.5], [0.5 + 0.0625 * h, 0.5], [1e6, 1e6]], F)
    r = qr.query32(K, st, q, h)
    assert r["offsets"].tolist() == [0, 3, 3, 6, 6] and r["index"].tolist() == [0, 1, 2, 0, 1, 2] and r["id"].tolist() == [7, 5, 9, 7, 5, 9]
    assert r["nearest"].tolist() == [0, qr.NONE, 0, qr.NONE]  # ties go to the lowest index
    assert r["nearest_dist_sq"].view(np.uint32)[[1, 3]].tolist() == [qr.INF_WORD] * 2 and r["dist_sq"][0] == 0
    tiny = qr.query32(K, st, q, np.finfo(F).tiny)  # r2 underflows to 0: only d2 == 0
    assert tiny["offsets"].tolist() == [0, 2, 2, 2, 2]
    assert qr.query32(K, st, q, h, boundary=True)["count"] == 0
    s = qr.select32(np.array([[0.1, 0.1], [np.nan, 0.1], [0.5, 0.5]], F), [3, 4, 5], [(0.0, 0.0, 0.5, 0.5)])
    assert s["index"].tolist() == [0] and s["id"].tolist() == [3]
    s = qr.select32(np.array([[0.1, 0.1], [np.nan, 0.1], [0.5, 0.5]], F), [3, 4, 5], [(0.0, 0.0, 0.5, 0.5)], outside=True)
    assert s["index"].tolist() == [1, 2]
    assert qr.select32(np.zeros((2, 2), F), [0, 1], [(1.0, -1.0, -1.0, 1.0)])["count"] == 0  # x0 > x1: empty
    assert qr.select32(np.zeros((2, 2), F), [0, 1], [(-np.inf, -np.inf, np.inf, np.inf)])["count"] == 2
    assert qr.select32(np.zeros((2, 2), F), [0, 1], [])["count"] == 0 and qr.select32(np.zeros((2, 2), F), [0, 1], [], True)["count"] == 2


def test_calls_without_a_device(sphx_lib):
    E = _lib.ERR_INVALID_ARGUMENT
    cnt = np.zeros(1, np.uint64)
    q = _lib.SphxQueryOut(count=cnt.ctypes.data)
    s = _lib.SphxSelectOut(count=cnt.ctypes.data)
    assert sphx_lib.sphx_query_radius(None, None, 0, 0.02, 0, 0, C.byref(q)) == E
    assert sphx_lib.sphx_query_radius(None, None, 0, 0.02, 0, 0, None) == E
    assert sphx_lib.sphx_select(None, None, 0, 0, 0, C.byref(s)) == E
    assert sphx_lib.sphx_select(None, None, 0, 0, 0, None) == E


def test_struct_layouts():
    assert C.sizeof(_lib.SphxQueryOut) == 56 and C.sizeof(_lib.SphxSelectOut) == 24
    assert [f for f, _ in _lib.SphxQueryOut._fields_] == ["offsets", "index", "id", "dist_sq", "nearest", "nearest_dist_sq", "count"]
    assert [f for f, _ in _lib.SphxSelectOut._fields_] == ["index", "id", "count"]
