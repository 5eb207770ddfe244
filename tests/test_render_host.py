"""Rendering without a GPU: the camera and the colour map against the reference's own known answers, the float32 restatement of the
rendering contract (tests/render_reference.py — what the GPU tests compare the device with bit for bit) against an independent float64
brute force on the golden states, the scenes' power to exercise the rule, the pixel-rectangle header under hostile values (compiled
for the host: tests/render_rect_driver.cpp), the coverage rule of min_pixel_radius, and the PNG writer."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import render_reference as rr
import yasph2d_amd as y
from yasph2d_amd import _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dam_break_4050.npz"))
RADIUS = F(y.default_params().particle_radius) if os.path.exists(_lib.LIB_PATH) else F(0.005)


def golden_state(step):
    return dict(pos=GOLD["s%d_pos" % step], vel=GOLD["s%d_vel" % step], boundary=GOLD["in_boundary"])


def test_render_symbols_exported_and_null_arguments_rejected(sphx_lib):
    assert hasattr(sphx_lib, "sphx_render") and hasattr(sphx_lib, "sphx_render_fit")
    assert "sphx_render" in _lib.SIGNATURES and "sphx_render_fit" in _lib.SIGNATURES
    assert C.sizeof(_lib.SphxRenderView) == 48 and C.sizeof(_lib.SphxRenderOut) == 16
    v = _lib.SphxRenderView()
    assert sphx_lib.sphx_render(None, C.byref(v), 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_render_fit(4, 4, 0.0, 0.0, 1.0, 1.0, None) == _lib.ERR_INVALID_ARGUMENT
    for bad in ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, -1.0), (float("nan"), 0.0, 1.0, 1.0), (0.0, 0.0, float("inf"), 1.0)):
        assert sphx_lib.sphx_render_fit(4, 4, *bad, C.byref(v)) == _lib.ERR_INVALID_ARGUMENT, bad
    assert (_lib.RENDER_NONE, _lib.RENDER_BOUNDARY) == (rr.NONE, rr.BOUNDARY)


def test_render_fit_is_center_around_world_rect(sphx_lib):
    """camera.rs:71-84 (construction_from_world_rect), and the app's defaults."""
    v = y.render_fit(200, 100, (10.0, 10.0, 20.0, 40.0))
    assert (v.width, v.height) == (200, 100)
    assert v.pixel_per_world_unit == 2.5 and tuple(v.center) == (20.0, 30.0)
    assert v.radius == 0 and v.min_pixel_radius == 0 and F(v.speed_scale) == F(0.1)
    assert tuple(v.background) == rr.BACKGROUND == (102, 102, 115, 255) and tuple(v.boundary) == rr.BOUNDARY_COLOR == (51, 51, 51, 255)
    assert tuple(v.reserved) == (0, 0)
    # the numpy camera is the same camera, also where the divisions round
    for (w, h, rect) in ((200, 100, (10.0, 10.0, 20.0, 40.0)), (640, 360, rr.SCENE_RECT), (1920, 1080, rr.SCENE_RECT), (17, 13, (-3.3, 0.7, 0.9, 7.1))):
        a, b = y.render_fit(w, h, rect), rr.fit(w, h, rect)
        assert F(a.pixel_per_world_unit) == b.pixel_per_world_unit and (F(a.center[0]), F(a.center[1])) == b.center, (w, h, rect)
    v = y.render_fit(64, 32, radius=0.015, min_pixel_radius=0.75, center=(1.0, 2.0), background=(1, 2, 3, 4))
    assert F(v.radius) == F(0.015) and v.min_pixel_radius == 0.75 and tuple(v.center) == (1.0, 2.0) and tuple(v.background) == (1, 2, 3, 4)
    with pytest.raises(TypeError):
        y.render_fit(64, 32, raduis=1.0)


@pytest.mark.parametrize("position,screen_xy,cases", [
    ((0.0, 0.0), (0.0, 0.0), [((0, 0), (100, 50)), ((1, 1), (110, 40)), ((-1, -1), (90, 60))]),
    ((1.0, 1.0), (0.0, 0.0), [((0, 0), (90, 60)), ((1, 1), (100, 50)), ((-1, -1), (80, 70))]),
    ((0.0, 0.0), (1.0, 2.0), [((0, 0), (101, 52)), ((1, 1), (111, 42)), ((-1, -1), (91, 62))]),
])
def test_world_to_screen_and_the_pixel_formula_are_inverses(position, screen_xy, cases):
    """camera.rs:86-125 (world_to_screen_conversion): the three cameras' known answers, and each of them back through the contract's
    pixel formula (the pixel whose centre is the screen point minus the screen's offset: ix + 0.5 = sx)."""
    v = rr.View(200, 100, position, 10.0)
    inv = F(F(1.0) / v.pixel_per_world_unit)
    for world, screen in cases:
        s = rr.world_to_screen(v, world, screen_xy)
        assert (float(s[0]), float(s[1])) == tuple(float(t) for t in screen)
        sx, sy = F(s[0] - F(screen_xy[0])), F(s[1] - F(screen_xy[1]))
        qx = F(v.center[0] + F(F(sx - F(F(0.5) * F(v.width))) * inv))
        qy = F(v.center[1] - F(F(sy - F(F(0.5) * F(v.height))) * inv))
        assert (float(qx), float(qy)) == tuple(float(t) for t in world)
    # and pixel_centres() is that formula at ix + 0.5
    qx, qy = rr.pixel_centres(v)
    half = F(F(0.5) * inv)
    assert qx[100] == F(v.center[0] + half) and qy[50] == F(v.center[1] - half) and qy[0] > qy[99]  # row 0 is the top row


def test_heatmap_knots():
    """heatmap_color (main.rs:74-80) at its knots, beyond them, negative and NaN."""
    third = F(1.0) / F(3.0)
    t = np.array([0.0, third, F(2.0) * third, 1.0, 7.5, -2.0, np.nan, np.inf, -np.inf, 0.5 * third], F)
    got = rr.heatmap_bytes(t)
    want = [(0, 0, 0), (255, 0, 0), (255, 255, 0), (255, 255, 255), (255, 255, 255), (0, 0, 0), (0, 0, 0), (255, 255, 255), (0, 0, 0),
            (128, 0, 0)]
    assert [tuple(int(c) for c in g[:3]) for g in got] == want
    assert (got[:, 3] == 255).all()


@pytest.mark.parametrize("step", [1, 10, 100])
@pytest.mark.parametrize("radius", [0.005, 0.015])
def test_restatement_against_float64_brute_force(step, radius):
    """Owners of the fp32 restatement and of a float64 gather may differ only where some particle's distance is within fp32 rounding of
    the radius; at most 0.1 % of the covered pixels may be such (a condition on the scene, not a measurement)."""
    st = golden_state(step)
    v = rr.fit(640, 360, radius=radius)
    a = rr.render32(st, v, RADIUS)["owner"]
    b, amb = rr.render64(st, v, RADIUS)
    covered = int((b != rr.NONE).sum())
    diff = a != b
    print("step %d radius %g: covered %d, ambiguous %d, differing %d" % (step, radius, covered, int(amb.sum()), int(diff.sum())))
    assert covered > 10000
    assert not (diff & ~amb).any(), "owners differ at %d unambiguous pixels" % int((diff & ~amb).sum())
    assert int(diff.sum()) <= covered // 1000


def test_window_mode_equals_full_mode():
    """The two ways render32 finds a particle's candidate pixels (module docstring) give the same image."""
    st = golden_state(100)
    for v in (rr.fit(640, 360), rr.fit(640, 360, radius=0.015), rr.fit(160, 120, min_pixel_radius=0.75),
              rr.View(333, 77, (0.4, 0.3), 2000.0), rr.View(64, 48, (30.0, 30.0), 50.0)):
        a, b = rr.render32(st, v, RADIUS, mode="full"), rr.render32(st, v, RADIUS, mode="window")
        assert np.array_equal(a["owner"], b["owner"]) and np.array_equal(a["rgba"], b["rgba"])


def test_scenes_exercise_the_rule():
    """What the GPU tests render must contain every case of the rule: all three classes of pixels, fluid over fluid, fluid over boundary,
    and speeds that move every colour channel."""
    st = golden_state(100)
    n = 640 * 360
    r = rr.render32(st, rr.fit(640, 360), RADIUS, counts=True)
    fluid = r["owner"] < rr.BOUNDARY
    frac = [float(fluid.sum()) / n, float((r["owner"] == rr.BOUNDARY).sum()) / n, float((r["owner"] == rr.NONE).sum()) / n]
    over, fob = int((r["fluid_count"] >= 2).sum()), int((fluid & r["boundary_cover"]).sum())
    print("reference radius: fluid %.3f boundary %.3f background %.3f, overdrawn %d, fluid over boundary %d" % (*frac, over, fob))
    assert min(frac) >= 0.02
    assert over > 0 and fob > 0
    rgb = r["rgba"][fluid][:, :3]
    assert (rgb[:, 0] > 0).any() and (rgb[:, 1] > 0).any() and (rgb[:, 2] > 0).any()
    assert (r["rgba"][~fluid & r["boundary_cover"]] == rr.BOUNDARY_COLOR).all() and (r["rgba"][r["owner"] == rr.NONE] == rr.BACKGROUND).all()
    big = rr.render32(st, rr.fit(640, 360, radius=0.015), RADIUS, counts=True)
    over, fob = int((big["fluid_count"] >= 2).sum()), int(((big["owner"] < rr.BOUNDARY) & big["boundary_cover"]).sum())
    print("radius 0.015: overdrawn %d, fluid over boundary %d" % (over, fob))
    assert over >= 1000 and fob >= 100
    # the owner is the HIGHEST covering index: at an overdrawn pixel a lower one covers too
    iy, ix = np.argwhere(big["fluid_count"] >= 2)[0]
    v = rr.fit(640, 360, radius=0.015)
    qx, qy = rr.pixel_centres(v)
    d = st["pos"] - np.array([qx[ix], qy[iy]], F)
    cov = np.nonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) <= F(F(0.015) * F(0.015)))[0]
    assert len(cov) == big["fluid_count"][iy, ix] and big["owner"][iy, ix] == cov.max() > cov.min()


@pytest.mark.parametrize("ppu", [60.0, 20.0])
def test_min_pixel_radius_lets_every_particle_in_view_cover_a_pixel(ppu):
    """Every point of the image is within sqrt(0.5) pixels of a pixel centre: with min_pixel_radius = 0.75 every particle inside the image
    covers at least one pixel; with the reference's radius most of them fall between the pixel centres."""
    st = golden_state(100)
    v = rr.View(160, 120, (0.95, 0.7), ppu)
    s = (st["pos"].astype(np.float64) - np.array([0.95, 0.7])) * ppu
    inside = (np.abs(s[:, 0]) <= 80.0) & (np.abs(s[:, 1]) <= 60.0)
    assert inside.sum() == len(s)  # the whole fluid is in view

    def uncovered(view):
        hits = np.zeros(len(s), np.int64)
        r = rr.disc_radius(view, RADIUS)
        rr._scatter(st["pos"], view, F(r * r), "full", lambda j, p: np.add.at(hits, j, 1))
        return int((inside & (hits == 0)).sum())

    plain, wide = uncovered(v), uncovered(v.replace(min_pixel_radius=0.75))
    print("%g pixels per unit: %d of %d particles cover no pixel with the reference radius, %d with min_pixel_radius 0.75" % (ppu, plain, inside.sum(), wide))
    assert wide == 0
    assert plain > inside.sum() // 2


# ---- the pixel rectangle of the scatter kernel, on the host -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rect_driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the pixel-rectangle driver"
    exe = str(tmp_path_factory.mktemp("render_rect") / "render_rect_driver")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "render_rect_driver.cpp"), "-o", exe])

    def run(view, r, xy):
        xy = np.ascontiguousarray(xy, F).reshape(-1, 2)
        head = struct.pack("<IIffffI", view.width, view.height, view.center[0], view.center[1], view.pixel_per_world_unit, r, len(xy))
        out = subprocess.run([exe], input=head + xy.tobytes(), capture_output=True, timeout=300)
        assert out.returncode == 0
        return np.frombuffer(out.stdout, np.uint32).reshape(-1, 4).astype(np.int64)

    return run


HOSTILE = [1e30, -1e30, 3.4e38, -3.4e38, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-38, 65536.0, -65536.0, 1e9, -1e9]


def rect_views():
    vs = [rr.fit(640, 360), rr.fit(1920, 1080), rr.View(1, 1, (0.5, 0.5), 10.0), rr.View(1, 777, (0.5, 0.5), 300.0), rr.View(333, 1, (0.5, 0.5), 300.0),
          rr.View(17, 13, (1.0, 0.2), 4000.0), rr.View(160, 120, (0.95, 0.7), 20.0), rr.View(64, 64, (1e6, -1e6), 100.0),
          rr.View(64, 64, (0.0, 0.0), 1e-3), rr.View(32, 32, (0.0, 0.0), 1e7), rr.View(8, 8, (3e38, 3e38), 1.0), rr.View(1 << 20, 200, (5.0, 0.0), 1e5)]
    return vs


@pytest.mark.parametrize("vi", range(12))
def test_pixel_rectangle_under_hostile_values(rect_driver, vi):
    """0 <= x0 <= x1 <= width and 0 <= y0 <= y1 <= height whatever the particle, and no pixel the contract calls covered lies outside
    the rectangle: hostile coordinates, discs straddling every edge and corner of the image, 1-pixel images, random particles."""
    v = rect_views()[vi]
    rng = np.random.default_rng(100 + vi)
    inv = F(F(1.0) / v.pixel_per_world_unit)
    qx, qy = rr.pixel_centres(v)
    for r in (F(0.005), F(0.02), F(F(0.75) * inv), F(F(4.0) * inv)):
        pts = [(a, b) for a in HOSTILE for b in HOSTILE]
        # edges and corners: particles around every edge at distances of about r, in units of a pixel and of r
        ex = [qx[0], qx[-1], F(qx[0] - F(0.5) * inv), F(qx[-1] + F(0.5) * inv)]
        ey = [qy[0], qy[-1], F(qy[0] + F(0.5) * inv), F(qy[-1] - F(0.5) * inv)]
        offs = [F(0), r, -r, F(r * F(1.0001)), F(-r * F(1.0001)), F(r * F(0.9999)), inv, -inv, F(r + inv), F(-r - inv)]
        with np.errstate(all="ignore"):
            pts += [(F(a + o), F(b + p)) for a in ex for b in ey for o in offs for p in offs]
            pts += [(F(a + o), F(v.center[1])) for a in ex for o in offs] + [(F(v.center[0]), F(b + p)) for b in ey for p in offs]
            span = np.array([v.width, v.height], np.float64) / float(v.pixel_per_world_unit)
            rnd = np.array([float(v.center[0]), float(v.center[1])]) + (rng.random((3000, 2)) - 0.5) * span * 1.2
        xy = np.concatenate([np.array(pts, F).reshape(-1, 2), rnd.astype(F)])
        rect = rect_driver(v, float(r), xy)
        x0, x1, y0, y1 = rect.T
        assert ((0 <= x0) & (x0 <= x1) & (x1 <= v.width) & (0 <= y0) & (y0 <= y1) & (y1 <= v.height)).all()
        # every covered pixel of the restatement lies inside its particle's rectangle
        seen = [0]

        def visit(j, p):
            iy, ix = p // v.width, p % v.width
            bad = ~((x0[j] <= ix) & (ix < x1[j]) & (y0[j] <= iy) & (iy < y1[j]))
            assert not bad.any(), "view %d r %g: particle %s covers pixel (%d, %d) outside its rectangle %s" % (
                vi, r, xy[j[bad][0]], ix[bad][0], iy[bad][0], rect[j[bad][0]])
            seen[0] += len(j)

        if v.width * len(xy) <= 1 << 28:
            rr._scatter(xy, v, F(r * r), "full", visit)
            if vi < 8 and vi != 7:
                assert seen[0] > 0
        # the work stays bounded: a rectangle is no larger than the disc's bounding box plus a margin
        if vi < 7:
            rp = float(r) * float(v.pixel_per_world_unit)
            assert ((x1 - x0) <= 2 * rp + 3).all() and ((y1 - y0) <= 2 * rp + 3).all()
        # non-finite and far-away particles get the empty rectangle
        with np.errstate(all="ignore"):
            far = ~np.isfinite(xy).all(axis=1) | (np.abs(xy.astype(np.float64) - np.array([float(v.center[0]), float(v.center[1])])).max(axis=1) > 1e20)
        if vi != 10:
            assert (rect[far] == 0).all()


def test_write_png_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    for shape in ((13, 17, 4), (1, 1, 4), (9, 5, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / ("t%d.png" % shape[0]))
        y.write_png(path, img)
        raw = open(path, "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n"
        pos, chunks = 8, []
        while pos < len(raw):
            n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
            data = raw[pos + 8:pos + 8 + n]
            assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
            chunks.append((kind, data))
            pos += 12 + n
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        w, h, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
        assert (h, w, depth, colour, comp, filt, inter) == (shape[0], shape[1], 8, 6 if shape[2] == 4 else 2, 0, 0, 0)
        rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * shape[2])
        assert (rows[:, 0] == 0).all()  # filter type None: the row is the pixels
        assert np.array_equal(rows[:, 1:].reshape(shape), img)
    with pytest.raises(ValueError):
        y.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4), np.uint8))
