"""Gauges without a GPU: the C ABI exports the gauge and probe calls; the numpy restatement of the gauge rule (tests/gauge_reference.py),
which the GPU tests hold the device to bit for bit, is compared on constructed value arrays with sphx_gauge_rule.hpp compiled alone
(tests/gauge_rule_driver.cpp, under the address and undefined-behaviour sanitizers) and with the library's sphx_gauge_reduce; mutants of
the restatement are rejected by those inputs; the crossing is the contour's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import contour_reference as cr
import gauge_reference as gr
import sample_reference as sr
import yasph2d_amd as y
from util import uniform_points
from yasph2d_amd import _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
NAN = F(np.nan)


def test_gauge_symbols_exported_and_null_context_rejected(sphx_lib):
    for name in ("sphx_gauge_levels", "sphx_gauge_reduce", "sphx_probe_record", "sphx_probe_get_status", "sphx_probe_read"):
        assert hasattr(sphx_lib, name) and name in _lib.SIGNATURES
    rec = np.zeros(1, y.GAUGE_REC_DTYPE)
    g = np.zeros(1, y.GAUGE_DTYPE)
    assert sphx_lib.sphx_gauge_levels(None, g.ctypes.data, 1, 0, 0, 0.5, 0, rec.ctypes.data, None) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_probe_record(None, None, 0, g.ctypes.data, 1, 0, 0, 0.5, 4, 1) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_probe_get_status(None, None) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_probe_read(None, 0, 0, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    for t in (_lib.SphxGauge, _lib.SphxGaugeRec, _lib.SphxProbeRec, _lib.SphxProbeStatus):
        assert C.sizeof(t) == 32
    for d in (y.GAUGE_DTYPE, y.GAUGE_REC_DTYPE, y.PROBE_REC_DTYPE):
        assert d.itemsize == 32
    assert y.GAUGE_REC_DTYPE == gr.REC_DTYPE and _lib.GAUGE_NONE == gr.NONE and _lib.GAUGE_MAX == 1024
    for name in ("gauges", "probe_record", "probe_status", "probe_frames"):
        assert hasattr(y.SphxContext, name)


# ------------------------------------------------------------------------------------------------------------- constructed inputs
def _random_case(seed, lengths):
    """oblique rays with inexact steps over decreasing noisy profiles: t, the products and the sums all round"""
    rng = np.random.default_rng(seed)
    gauges, values = [], []
    for n in lengths:
        gauges.append([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.01, 0.013), rng.uniform(0.003, 0.011), n])
        prof = np.clip(1.1 - np.arange(n) / max(n * rng.uniform(0.2, 1.3), 1.0), 0, 1) + rng.normal(0, 0.04, n)
        values.append(prof.astype(F))
    return gauges, np.concatenate(values), 0.5


def cases():
    """name -> (gauges [g, 5], values, iso): what the issue lists, on rays whose points are not all exact"""
    ray = [0.3, -0.2, 0.0, 0.0125, 6]
    obl = [0.1, 0.7, 0.003, -0.007, 6]
    c = {}
    c["nothing inside"] = ([ray, obl], np.array([0.1, 0.2, 0.3, 0.4, 0.3, 0.2] * 2, F), 0.5)
    c["everything inside"] = ([ray, obl], np.array([0.9, 0.8, 0.7, 0.6, 0.7, 0.8] * 2, F), 0.5)
    c["last = 0"] = ([ray, obl], np.array([0.9, 0.3, 0.2, 0.1, 0.0, 0.0] * 2, F), 0.5)
    c["last = n-1 alone"] = ([ray, obl], np.array([0.1, 0.3, 0.2, 0.1, 0.0, 0.7] * 2, F), 0.5)
    c["n = 1"] = ([[0.3, 0.1, 0.5, 0.5, 1], [0.3, 0.1, 0.5, 0.5, 1], [1.5, -2.0, 0.0, 0.0, 1]], np.array([0.7, 0.2, 0.5], F), 0.5)
    c["a bubble"] = ([ray, obl], np.array([0.9, 0.8, 0.1, 0.9, 0.2, 0.1, 0.2, 0.9, 0.1, 0.1, 0.8, 0.3], F), 0.5)
    c["NaN values"] = ([ray, obl, ray], np.array([0.9, NAN, 0.9, NAN, 0.1, NAN, NAN, NAN, NAN, NAN, NAN, NAN, 0.9, 0.8, 0.7, 0.6, NAN, 0.1], F), 0.5)
    c["inf values"] = ([ray, obl], np.array([np.inf, 0.9, 0.6, -np.inf, 0.1, 0.0, 0.9, np.inf, 0.2, 0.1, 0.1, 0.1], F), 0.5)
    c["+0 and -0 at iso +0"] = ([ray, obl], np.array([1.0, -0.0, -1.0, -1.0, -1.0, -1.0, 1.0, 0.0, -0.0, -2.0, -1.0, -1.0], F), 0.0)
    c["+0 and -0 at iso -0"] = ([ray, obl], np.array([1.0, 0.0, -1.0, -1.0, -1.0, -1.0, -0.0, 0.0, -0.0, -2.0, -1.0, -1.0], F), -0.0)
    c["f == iso exactly"] = ([ray, obl], np.array([0.9, 0.5, 0.25, 0.1, 0.0, 0.0, 0.5, 0.5, 0.5, 0.5, 0.4, 0.3], F), 0.5)
    c["f == iso at the end"] = ([ray], np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.5], F), 0.5)
    c["iso negative"] = ([ray, obl], np.array([-0.1, -0.3, -0.7, -0.9, -1.0, -2.0, 3.0, 2.0, -0.25, -0.75, -0.8, -0.625], F), -0.5)
    c["zero and negative steps"] = ([[0.5, 0.5, 0.0, 0.0, 4], [0.5, 0.5, -0.125, -0.0625, 4]], np.array([0.9, 0.8, 0.2, 0.1, 0.9, 0.7, 0.3, 0.1], F), 0.5)
    c["huge coordinates"] = ([[3e38, -3e38, 1e37, 1e37, 5]], np.array([0.9, 0.8, 0.7, 0.1, 0.0], F), 0.5)
    c["subnormal difference"] = ([ray], np.array([1e-45, 0.0, 0.0, 0.0, 0.0, 0.0], F), 1e-45)
    c["mixed lengths"] = _random_case(1, [1, 2, 63, 64, 65, 255, 256, 257, 1025])
    c["many gauges"] = _random_case(2, [17] * 300)
    return c


CASES = cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed to compile the gauge-rule driver"
    d = tmp_path_factory.mktemp("gauge_rule")
    exe = str(d / "gauge_rule_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "gauge_rule_driver.cpp"), "-o", exe])

    def run(gauges, values, iso):
        g = y._gauge_array(gauges)
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([len(g)], np.uint32).tobytes() + np.array([iso], F).tobytes() + g.tobytes() + np.asarray(values, F).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return int(r.stdout.split()[1]), np.fromfile(dst, y.GAUGE_REC_DTYPE)

    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_header_equals_the_restatement(driver, sphx_lib, name):
    gauges, values, iso = CASES[name]
    want = gr.reduce32(values, gauges, iso)
    rc, got = driver(gauges, values, iso)
    assert rc == _lib.OK and gr.same_bytes(got, want), (name, got, want)
    assert gr.same_bytes(y.gauge_reduce(values, gauges, iso), want)  # the library's sphx_gauge_reduce is the same header


def test_constructed_cases_are_what_they_say():
    r = lambda name: gr.reduce32(CASES[name][1], CASES[name][0], CASES[name][2])
    word = lambda a: np.asarray(a, F).view(np.uint32)
    a = r("nothing inside")
    assert (a["first"] == gr.NONE).all() and (a["last"] == gr.NONE).all() and (a["inside"] == 0).all()
    for m in ("t", "x", "y", "f_last", "f_next"):
        assert (word(a[m]) == gr.QNAN).all()
    a = r("everything inside")
    assert (a["first"] == 0).all() and (a["last"] == 5).all() and (a["inside"] == 6).all() and (a["t"] == 0).all() and (word(a["f_next"]) == gr.QNAN).all()
    assert gr.same_bytes(np.stack([a["x"], a["y"]], -1), np.stack([gr.gauge_points(*g)[5] for g in gr.gauge_rows(CASES["everything inside"][0])]))
    assert (r("last = 0")["last"] == 0).all() and (r("last = 0")["inside"] == 1).all()
    a = r("last = n-1 alone")
    assert (a["first"] == 5).all() and (a["last"] == 5).all() and (a["t"] == 0).all()
    a = r("n = 1")
    assert a["last"].tolist() == [0, gr.NONE, 0] and a["t"][0] == 0 and a["t"][2] == 0  # (0.5 >= 0.5: inside)
    a = r("a bubble")
    assert (a["inside"] < a["last"] - a["first"] + 1).all()
    a = r("NaN values")
    assert a["last"].tolist() == [2, gr.NONE, 3] and np.isnan(a["x"][0]) and np.isnan(a["t"][2])  # (f_next NaN: the crossing is NaN, not a fault)
    assert word(a["f_last"][0]) == word(F(0.9)) and a["inside"].tolist() == [2, 0, 4]
    a = r("+0 and -0 at iso +0")
    assert a["last"].tolist() == [1, 2] and a["inside"].tolist() == [2, 3]  # (-0 >= +0)
    assert r("+0 and -0 at iso -0")["last"].tolist() == [1, 2]
    a = r("f == iso exactly")
    assert a["last"].tolist() == [1, 3] and (a["t"] == 0).all()  # equality is inside; the crossing sits on the sample itself
    assert gr.same_bytes(np.stack([a["x"], a["y"]], -1)[0], gr.gauge_points(*gr.gauge_rows(CASES["f == iso exactly"][0])[0])[1])
    assert r("iso negative")["last"].tolist() == [1, 2]
    a = r("zero and negative steps")
    assert a["last"].tolist() == [1, 1] and a["x"][0] == F(0.5) and a["y"][0] == F(0.5) and a["x"][1] < F(0.375)
    assert r("subnormal difference")["t"][0] == 0  # (gradual underflow: f_b - f_a = -1e-45 is not zero)
    a = r("mixed lengths")
    assert (a["inside"] > 0).all() and len(set(a["last"].tolist())) > 5


def test_mutants_of_the_restatement_are_rejected():
    """> for >=, the edge written from the upper sample, a fused multiply-add in the point, float64 interpolation: each differs from the
    contract on some constructed input (and the driver equals the contract on all of them, above)."""
    killed = {v: [] for v in gr.VARIANTS[1:]}
    for name, (gauges, values, iso) in CASES.items():
        want = gr.reduce32(values, gauges, iso)
        for v in killed:
            if not gr.same_bytes(gr.reduce32(values, gauges, iso, v), want):
                killed[v].append(name)
    assert all(killed.values()), killed
    assert "f == iso exactly" in killed["strict_greater"]
    # the random rays alone kill the three arithmetic mutants, each on many gauges
    gauges, values, iso = CASES["many gauges"]
    want = gr.reduce32(values, gauges, iso)
    for v in ("b_lower", "fused", "float64"):
        got = gr.reduce32(values, gauges, iso, v)
        differ = sum(not gr.same_bytes(got[k], want[k]) for k in range(len(want)))
        # (a fused or float64 point differs only where an inner rounding reaches the result's last bit: rarer than a changed t)
        assert differ > (20 if v == "b_lower" else 0), (v, differ)
        assert all(gr.same_bytes(got[m], want[m]) for m in ("first", "last", "inside", "f_last", "f_next"))


# ------------------------------------------------------------------------------------------------------------- the contour's crossing
def test_crossing_is_the_contours():
    rng = np.random.default_rng(7)
    n, x0, y0, dy = 40, F(0.37), F(0.013), F(0.0071)
    for trial in range(20):
        f = (np.clip(1.2 - np.arange(n) / rng.uniform(8, 45), 0, 1) + rng.normal(0, 0.05, n)).astype(F)
        rec = gr.reduce32(f, [[x0, y0, 0.0, dy, n]], 0.5)[0]
        last = int(rec["last"])
        if not 0 <= last < n - 1:
            continue
        # the contour's formula on the edge a = (0, last), b = (0, last + 1) of a lattice whose column 0 is the gauge
        ys = (y0 + (np.arange(n, dtype=F) * dy).astype(F)).astype(F)
        xa = np.array([F(x0 + F(F(0) * F(0.01)))], F)
        p = cr._cross(xa, ys[last:last + 1], xa, ys[last + 1:last + 2], f[last:last + 1], f[last + 1:last + 2], F(0.5))[0]
        assert gr.same_bytes(p, np.array([rec["x"], rec["y"]], F))
        # ... and the whole contour restatement on a two-column lattice: the point is an end of a segment of cell (0, last)
        for col1 in (f, np.zeros(n, F), np.ones(n, F), rng.random(n, dtype=F)):
            lat = np.stack([f, col1], -1)  # [ny, nx = 2]
            c = cr.contour32(lat, x0, y0, F(0.01), dy, 2, n, 0.5)
            ends = {e.tobytes() for e in c["segments"][c["cell"] == last].reshape(-1, 2)}
            assert np.array([rec["x"], rec["y"]], F).tobytes() in ends, (trial, last)


def test_restated_sampling_through_the_library_rule(sphx_lib):
    """columns, a bed ray and an oblique ray through 700 scattered particles: the restated sampling reduced by the restatement and by
    the library's host rule give the same bytes (the GPU tests repeat this with the device's own values)"""
    K = sr.Constants(y.default_params())
    pos = (uniform_points(700, 2500.0, 11) + F(0.3)).astype(F)
    st = dict(pos=pos, vel=np.zeros_like(pos), density=np.zeros(len(pos), F), boundary=np.zeros((0, 2), F))
    st["density"] = np.maximum(sr.sample32(K, dict(st, density=np.ones(len(pos), F)), pos, sr.KERNEL_WENDLAND)["density"], K.rho0)
    lo, hi = pos.min(0), pos.max(0)
    gauges = [[x, lo[1] - 0.03, 0.0, 0.008, 80] for x in np.linspace(lo[0] + 0.02, hi[0] - 0.02, 5)]
    gauges += [[lo[0] - 0.03, lo[1] + 0.05, 0.005, 0.0, 60], [hi[0] + 0.03, hi[1] + 0.03, -0.004, -0.0035, 90], [5.0, 5.0, 0.01, 0.01, 9]]
    rec, values = gr.levels32(K, st, gauges, 0.5)
    assert gr.same_bytes(y.gauge_reduce(values, gauges, 0.5), rec)
    assert (rec["inside"][:7] > 0).all() and rec["inside"][7] == 0 and (rec["last"][:5] < 79).all()
    # the level of a column lies between its last wet sample and the next one
    for k in range(5):
        ys = gr.gauge_points(*gr.gauge_rows(gauges)[k])[:, 1]
        assert ys[rec["last"][k]] <= rec["y"][k] <= ys[rec["last"][k] + 1] and rec["x"][k] == F(gauges[k][0])


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_gauge_reduce_argument_errors(sphx_lib):
    ok, bad = _lib.OK, _lib.ERR_INVALID_ARGUMENT
    v = np.array([0.9, 0.1, 0.0], F)
    rec = np.zeros(4, y.GAUGE_REC_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(g, n_gauges=None, values=v, iso=0.5, out=rec):
        g = y._gauge_array(g)
        return sphx_lib.sphx_gauge_reduce(p(values) if values is not None else None, p(g) if len(g) else None, len(g) if n_gauges is None else n_gauges,
                                          iso, p(out) if out is not None else None)

    good = [0.0, 0.0, 0.0, 0.1, 3]
    assert call([good]) == ok
    assert call([good], out=None) == bad
    assert call([], n_gauges=1) == bad  # gauges NULL with n_gauges > 0
    assert call([], values=None) == ok and call([]) == ok  # n_gauges == 0 succeeds
    assert call([good], values=None) == bad
    big = np.zeros(_lib.GAUGE_MAX + 1, y.GAUGE_DTYPE)
    big["n"] = 1
    many = np.zeros(_lib.GAUGE_MAX + 1, F)
    assert call(big, values=many, out=np.zeros(_lib.GAUGE_MAX + 1, y.GAUGE_REC_DTYPE)) == bad
    assert call(big[:-1], values=many, out=np.zeros(_lib.GAUGE_MAX, y.GAUGE_REC_DTYPE)) == ok
    assert call([[0, 0, 0, 0.1, 0]]) == bad and call([[0, 0, 0, 0.1, 2 ** 20 + 1]]) == bad
    assert call([[0, 0, 0, 0.1, 2 ** 20]] * 17) == bad  # 17 * 2^20 > 2^24 samples (refused before a value is read)
    for k in range(4):
        for x in (np.nan, np.inf, -np.inf):
            g = list(good)
            g[k] = x
            assert call([g]) == bad, (k, x)
    for iso in (np.nan, np.inf, -np.inf):
        assert call([good], iso=iso) == bad
    assert call([[0.0, 0.0, -0.5, 0.0, 3], [1.0, 1.0, 0.0, 0.0, 3]], values=np.zeros(6, F)) == ok  # negative and zero steps are legal
    with pytest.raises(ValueError):
        y.gauge_reduce(v, [[0, 0, 0, 0.1, 4]])
    with pytest.raises(y.SphxError):
        y.gauge_reduce(v, [[0, np.nan, 0, 0.1, 3]])
