"""Neighbour queries of a tiled run (sphx_multi_query_radius / sphx_multi_select, include/sphx.h), the parts that need no GPU: the fold
of the tiles' (ranks') parts into one CSR list in the caller's order (csrc/sphx_query_merge.hpp) as a sanitized stand-alone program and
through the exported sphx_query_merge, both against a numpy restatement of the fold; the exports, the bindings and the struct sizes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yasph2d_amd as ya
from yasph2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
GUARD, GUARD_WORD = 8, 0xDEADBEEF
NONE, INF_WORD = 0xFFFFFFFF, 0x7F800000
MULTI_CALLS = ("sphx_multi_query_radius", "sphx_query_merge", "sphx_multi_select")
TILE_CALLS = ("sphx_tile_query_radius", "sphx_tile_query_fetch", "sphx_tile_select", "sphx_tile_select_fetch")


# ------------------------------------------------------------------------------------------------------ parts and the restatement
def make_part(rng, m, answered, tile, counts=None, part_cap=None, entries=True, id_map=None):
    """A full-form part: the points `answered` (bool [m]) carry tile `tile` and counts[i] entries, the others -1 and an empty range."""
    cnt = np.where(answered, rng.integers(0, 6, m) if counts is None else counts, 0).astype(np.uint64)
    off = np.zeros(m + 1, np.uint64)
    off[1:] = np.cumsum(cnt, dtype=np.uint64)
    total = int(off[m])
    held = total if part_cap is None else min(total, part_cap)
    p = dict(offsets=off, tile=np.where(answered, tile, -1).astype(np.int32), rank=tile, total=total, held=held if entries else 0,
             id_map=id_map)
    for f in ("nearest_id", "nearest_slot", "nearest_d2"):
        p[f] = rng.integers(0, 2**31, m, dtype=np.uint64).astype(np.uint32)
    if id_map is not None:
        p["nearest_id"] = rng.integers(0, len(id_map), m).astype(np.uint32)
    p["nearest_id"][~answered] = NONE
    if entries:
        for f in ("id", "d2", "slot"):
            p[f] = rng.integers(0, 2**31, held, dtype=np.uint64).astype(np.uint32)
        if id_map is not None:
            p["id"] = rng.integers(0, len(id_map), held).astype(np.uint32)
    return p


def fold(m, parts, cap, entries=True):
    """The fold, restated: per point the part with tile >= 0 and the lowest tile; its entries appended in point order."""
    off = np.zeros(m + 1, np.uint64)
    tile = np.full(m, -1, np.int32)
    near = {f: np.full(m, INF_WORD if f == "nearest_d2" else NONE, np.uint32) for f in ("nearest_id", "nearest_slot", "nearest_d2")}
    ent = {f: [] for f in ("id", "d2", "slot")}
    pos, rc = 0, 0
    for i in range(m):
        off[i] = pos
        who = [p for p in parts if p["tile"][i] >= 0]
        if not who:
            continue
        p = min(who, key=lambda q: q["tile"][i])
        tile[i] = p["tile"][i]
        for f in near:
            near[f][i] = p[f][i]
        if p["id_map"] is not None and near["nearest_id"][i] != NONE:
            near["nearest_id"][i] = p["id_map"][near["nearest_id"][i]]
        a, b = int(p["offsets"][i]), int(p["offsets"][i + 1])
        if entries:
            for e in range(a, min(b, a + max(cap - pos, 0))):
                if e >= p["held"]:
                    rc = _lib.ERR_CAPACITY
                    break
                for f in ent:
                    v = p[f][e]
                    ent[f].append(p["id_map"][v] if f == "id" and p["id_map"] is not None else v)
        pos += b - a
    off[m] = pos
    return rc, pos, off, tile, near, {f: np.array(v, np.uint32) for f, v in ent.items()}


def compact(p):
    """The compact form of a full-form part: records of the answered points only."""
    k = np.nonzero(p["tile"] >= 0)[0]
    q = dict(p)
    q.update(point=k.astype(np.uint32), offsets=p["offsets"][k], compact=True)
    for f in ("nearest_id", "nearest_slot", "nearest_d2"):
        q[f] = p[f][k]
    return q


def write_case(path, m, parts, cap, entries):
    with open(path, "wb") as f:
        np.array([m, len(parts), cap, int(entries)], np.uint64).tofile(f)
        for p in parts:
            c = bool(p.get("compact"))
            n = len(p["point"]) if c else m
            n_map = 0 if p["id_map"] is None else len(p["id_map"])
            np.array([int(c), n, p["total"], p["rank"], p["held"], n_map], np.uint64).tofile(f)
            if c:
                p["point"].tofile(f)
            p["offsets"].astype(np.uint64).tofile(f)
            if not c:
                p["tile"].tofile(f)
            for k in ("nearest_id", "nearest_slot", "nearest_d2"):
                p[k].tofile(f)
            if entries:
                for k in ("id", "d2", "slot"):
                    p[k].tofile(f)
            if n_map:
                np.asarray(p["id_map"], np.uint32).tofile(f)


def read_result(path, m, cap, entries):
    raw = np.fromfile(path, np.uint8)
    head = raw[:16 + 8 * (m + 1)].view(np.uint64)
    rest = raw[16 + 8 * (m + 1):].view(np.uint32)
    out = dict(rc=int(head[0]), count=int(head[1]), offsets=head[2:], tile=rest[:m].view(np.int32))
    for k, f in enumerate(("nearest_id", "nearest_slot", "nearest_d2")):
        out[f] = rest[(k + 1) * m:(k + 2) * m]
    if entries:
        ent = rest[4 * m:].reshape(3, cap + GUARD)
        out.update(id=ent[0], d2=ent[1], slot=ent[2])
    return out


def cases():
    """name -> (m, parts, cap, entries, expected rc, the parts in the full form)"""
    rng = np.random.default_rng(20261021)
    out = {}
    for form in ("full", "compact"):
        shape = (lambda p: compact(p)) if form == "compact" else (lambda p: p)
        m = 700
        owner = rng.integers(0, 3, m)
        owner[100:400] = 1  # (a long run one part answers: one memcpy)
        owner[400:600] = np.arange(200) % 2  # (alternating owners: runs of one)
        parts = [make_part(rng, m, owner == k, [5, 2, 9][k]) for k in range(3)]
        total = fold(m, parts, 1 << 40)[1]
        out[form + "-disjoint"] = (m, [shape(p) for p in parts], total, True, 0, parts)
        # cap inside a point's run, at a run boundary (the end of the 300-point run), at 0, one below the total
        off = fold(m, parts, 0, False)[2]
        i = next(k for k in range(150, 400) if int(off[k + 1]) - int(off[k]) >= 2)
        for name, cap in (("inside", int(off[i]) + 1), ("boundary", int(off[400])), ("zero", 0), ("below", total - 1)):
            out[form + "-cap-" + name] = (m, [shape(p) for p in parts], cap, True, 0, parts)
        # two parts claim the same points: the lowest TILE wins, not the first part
        both = rng.random(m) < 0.4
        parts2 = [make_part(rng, m, (owner == 0) | both, 7), make_part(rng, m, (owner == 1) | both, 3), make_part(rng, m, owner == 2, 4)]
        out[form + "-claimed-twice"] = (m, [shape(p) for p in parts2], fold(m, parts2, 1 << 40)[1], True, 0, parts2)
        # points nobody answers, an empty part, a part that answers points without entries
        nobody = rng.random(m) < 0.3
        parts3 = [make_part(rng, m, (owner == 0) & ~nobody, 0), make_part(rng, m, np.zeros(m, bool), 1),
                  make_part(rng, m, (owner != 0) & ~nobody, 2, counts=np.zeros(m, np.uint64))]
        out[form + "-nobody-and-empty"] = (m, [shape(p) for p in parts3], fold(m, parts3, 1 << 40)[1], True, 0, parts3)
        # a truncated part whose missing entry is needed / is not needed
        short = [make_part(rng, m, owner == k, k, part_cap=40 if k == 1 else None) for k in range(3)]
        need = fold(m, short, 1 << 40)[1]
        out[form + "-truncated-needed"] = (m, [shape(p) for p in short], need, True, _lib.ERR_CAPACITY, short)
        out[form + "-truncated-unneeded"] = (m, [shape(p) for p in short], 20, True, 0, short)
        # totals above 2^32: synthetic offsets, no entry arrays
        big = [make_part(rng, m, owner == k, k, counts=rng.integers(1 << 29, 1 << 31, m), entries=False) for k in range(3)]
        out[form + "-above-2^32"] = (m, [shape(p) for p in big], 16, False, 0, big)
        # boundary ids: every part translates through its own map
        maps = [rng.permutation(5000)[:300 + 50 * k].astype(np.uint32) for k in range(3)]
        mapped = [make_part(rng, m, owner == k, k, id_map=maps[k]) for k in range(3)]
        out[form + "-id-map"] = (m, [shape(p) for p in mapped], fold(m, mapped, 1 << 40)[1], True, 0, mapped)
    out["no-parts"] = (50, [], 10, True, 0, [])
    nothing = [make_part(rng, 0, np.zeros(0, bool), 0)]
    out["no-points"] = (0, nothing, 4, True, 0, nothing)
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------------------ 1. the header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the query-merge driver"
    d = tmp_path_factory.mktemp("query_merge")
    exe = str(d / "query_merge_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "query_merge_driver.cpp"), "-o", exe])

    def run(name, m, parts, cap, entries):
        src, dst = str(d / (name + ".in")), str(d / (name + ".out"))
        write_case(src, m, parts, cap, entries)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
        return read_result(dst, m, cap, entries)

    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_query_merge_host(driver, name):
    """Seeded parts in the full and the compact form through csrc/sphx_query_merge.hpp, compiled with the address and undefined-behaviour
    sanitizers, against the numpy restatement: disjoint owners (a 300-point run of one part, 200 alternating points), points two parts
    claim (the lowest tile wins), points nobody answers, an empty part, no parts, no points, capacities inside a run, at a run boundary,
    at 0 and one below the total (the guard words behind every capacity stay), a truncated part whose entry is needed
    (SPHX_ERR_CAPACITY) and one whose is not, totals above 2^32 without entry arrays, boundary ids translated per part."""
    m, parts, cap, entries, want_rc, full = CASES[name]
    got = driver(name, m, parts, cap, entries)
    rc, count, off, tile, near, ent = fold(m, full, cap, entries)
    assert rc == want_rc and got["rc"] == want_rc
    assert got["count"] == count and np.array_equal(got["offsets"], off) and np.array_equal(got["tile"], tile)
    if name.endswith("above-2^32"):
        assert count > 2**32
    for f in near:
        assert np.array_equal(got[f], near[f]), f
    if entries:
        n = min(count, cap)
        for f in ent:
            assert np.all(got[f][cap:] == GUARD_WORD), f  # nothing at or behind the capacity
            if rc == 0:
                assert np.array_equal(got[f][:n], ent[f][:n]), f
            # (rc != 0: offsets, count and the guards hold; the entries of a refused fold are not specified)


def test_merge_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_query_merge.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


# ------------------------------------------------------------------------------------------------------ 2. the exported merge
def as_query_part(p):
    d = dict(offsets=p["offsets"], tile=p["tile"], count=p["total"], nearest_id=p["nearest_id"], nearest_slot=p["nearest_slot"],
             nearest_dist_sq=p["nearest_d2"].view(np.float32))
    if "id" in p:
        d.update(id=p["id"], dist_sq=p["d2"].view(np.float32), slot=p["slot"])
    return d


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if n.startswith("full-") and not n.endswith("id-map")])
def test_query_merge_exported(name):
    """yasph2d_amd.query_merge (sphx_query_merge through the bindings) on the full-form cases, against the same restatement."""
    m, parts, cap, entries, want_rc, _ = CASES[name]
    if want_rc:
        with pytest.raises(ya.SphxError) as e:
            ya.query_merge([as_query_part(p) for p in parts], cap)
        assert e.value.code == want_rc and "sphx_query_merge" in str(e.value)
        return
    got = ya.query_merge([as_query_part(p) for p in parts], cap)
    rc, count, off, tile, near, ent = fold(m, parts, cap, entries)
    assert got["count"] == count and np.array_equal(got["offsets"], off) and np.array_equal(got["tile"], tile)
    for f, g in (("nearest_id", "nearest_id"), ("nearest_slot", "nearest_slot"), ("nearest_d2", "nearest_dist_sq")):
        assert np.array_equal(got[g].view(np.uint32), near[f])
    if entries:
        n = min(count, cap)
        for f, g in (("id", "id"), ("d2", "dist_sq"), ("slot", "slot")):
            assert len(got[g]) == n and np.array_equal(got[g].view(np.uint32), ent[f][:n])


def test_query_merge_arguments():
    L = _lib.lib()
    bad = _lib.ERR_INVALID_ARGUMENT
    m = 3
    off, til, cnt = np.zeros(m + 1, np.uint64), np.zeros(m, np.int32), np.zeros(1, np.uint64)
    ids = np.zeros(4, np.uint32)
    caps = (C.c_uint64 * 1)(4)

    def struct(**kw):
        o = _lib.SphxMultiQueryOut()
        for k, v in kw.items():
            setattr(o, k, v.ctypes.data)
        return o

    part = struct(offsets=off, tile=til)
    out = struct(offsets=off.copy(), count=cnt)
    assert L.sphx_query_merge(m, C.byref(part), caps, 1, 4, None) == bad and b"out is NULL" in L.sphx_multi_last_error(None)
    assert L.sphx_query_merge(m, C.byref(part), caps, 1, 4, C.byref(struct(offsets=off))) == bad and b"out->count" in L.sphx_multi_last_error(None)
    assert L.sphx_query_merge(m, None, caps, 1, 4, C.byref(out)) == bad and b"parts is NULL" in L.sphx_multi_last_error(None)
    assert L.sphx_query_merge(m, C.byref(struct(tile=til)), caps, 1, 4, C.byref(out)) == bad and b"offsets" in L.sphx_multi_last_error(None)
    assert L.sphx_query_merge(m, C.byref(struct(offsets=off)), caps, 1, 4, C.byref(out)) == bad and b"tile" in L.sphx_multi_last_error(None)
    wants_id = struct(count=cnt, id=ids)
    assert L.sphx_query_merge(m, C.byref(part), caps, 1, 4, C.byref(wants_id)) == bad and b"lacks" in L.sphx_multi_last_error(None)
    assert L.sphx_query_merge(m, C.byref(struct(offsets=off, tile=til, id=ids)), None, 1, 4, C.byref(wants_id)) == bad
    assert b"parts_cap" in L.sphx_multi_last_error(None)
    cnt[0] = 99
    assert L.sphx_query_merge(m, None, None, 0, 4, C.byref(out)) == 0 and cnt[0] == 0  # the all-absent answer


# ------------------------------------------------------------------------------------------------------ 3. exports, bindings, sizes
def test_exports_and_bindings():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sphx.h")).read()
    for name in MULTI_CALLS + TILE_CALLS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    from yasph2d_amd.multi import MultiSolver

    for name in ("query", "select"):
        assert callable(getattr(MultiSolver, name)) and callable(getattr(ya.DFSPHMultiSolver, name))
    assert callable(ya.query_merge) and "query_merge" in ya.__all__


def test_struct_sizes_match_the_header(tmp_path):
    """sizeof of the new structs as a C compiler sees them in include/sphx.h equals what ctypes lays out (and the sizes the header states)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "sphx.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(sphx_multi_query_out), '
                   'sizeof(sphx_multi_select_out), sizeof(sphx_tile_query_part)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert sizes == [C.sizeof(_lib.SphxMultiQueryOut), C.sizeof(_lib.SphxMultiSelectOut), C.sizeof(_lib.SphxTileQueryPart)] == [72, 32, 88]
