"""Shared helpers for the parity tests: scenes (inputs) and oracle-vs-device comparison."""
import numpy as np


def dam_break(scale=1.0):
    """The reference scene (main.rs:177-196) through the host mirror: (positions, boundary)."""
    import yasph2d_amd as y

    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    return w.positions, w.boundary_particles


def bench_world():
    """benches/benchmarks/update_densities.rs:72-80: 1x1 m rect with jitter 0.5 + a 20-thick boundary line."""
    import yasph2d_amd as y

    w = y.FluidParticleWorld()
    w.add_fluid_rect(0.0, 0.0, 1.0, 1.0, 0.5)
    w.add_boundary_thick_line((-0.5, 0.5), (1.5, 0.5), 20)
    return w.positions, w.boundary_particles


def uniform_points(n, density, seed):
    """benches/benchmarks/neighborhood_search.rs:10-17 / neighborhood_search.rs:531-538: n uniform points in a
    sqrt(n/density)-sided square (own RNG: the reference's SmallRng stream is not reproducible here)."""
    rng = np.random.default_rng(seed)
    side = np.float32(np.sqrt(np.float32(n) / np.float32(density)))
    return (rng.random((n, 2), dtype=np.float32) * side).astype(np.float32)


def brute_force_neighbors(pos, radius, i):
    d = pos - pos[i]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]  # f32, un-fused like the reference
    m = d2 <= np.float32(radius) * np.float32(radius)
    m[i] = False
    return np.nonzero(m)[0].astype(np.uint32)


def assert_same_neighbors(a, b):
    """a, b = (counts[N,2], start, lists)"""
    ca, sa, la = a
    cb, sb, lb = b
    assert ca.shape == cb.shape
    bad = np.nonzero((ca != cb).any(axis=1))[0]
    assert bad.size == 0, f"neighbor counts differ at {bad[:10]} ({bad.size} particles): {ca[bad[:5]]} vs {cb[bad[:5]]}"
    assert la.shape == lb.shape
    diff = np.nonzero(la != lb)[0]
    assert diff.size == 0, f"neighbor lists differ at {diff.size} entries, first at flat index {diff[:5]}"


def assert_bits_equal(a, b, what):
    """fp32 arrays must be numerically identical element by element (+0 == -0 allowed, NaN never)."""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    assert np.isfinite(a).all() and np.isfinite(b).all(), f"{what}: non-finite values"
    bad = np.nonzero(a != b)
    if bad[0].size:
        i = tuple(x[0] for x in bad)
        raise AssertionError(f"{what}: {bad[0].size} of {a.size} elements differ; first at {i}: {a[i]!r} vs {b[i]!r}")


def xcd_groups(grid, shift):
    """The XCD block mapping's split of a grid (yasph2d_amd/csrc/sphx_xcd.hpp, xcd_map): (full chunks per XCD of 2^shift blocks, r =
    blocks per XCD in the last, shorter group).  shift 0: no chunks, (0, grid / 8).  Checked against the header by
    tests/test_block_mapping.py."""
    per = grid >> 3
    if shift == 0:
        return 0, per
    full = per >> shift
    return full, per - (full << shift)


def xcd_map(block, grid, rev, shift):
    """Python restatement of xcd_map (sphx_xcd.hpp) for the host tests."""
    per, q0, x = grid >> 3, block >> 3, block & 7
    q = per - 1 - q0 if rev else q0
    if shift == 0:
        return x * per + q
    full, r = xcd_groups(grid, shift)
    g = q >> shift
    if g < full:
        return (g << (shift + 3)) + (x << shift) + (q - (g << shift))
    return (full << (shift + 3)) + x * r + (q - (full << shift))


def step_pair(ctx, o, timer, diam=np.float32(0.01), what=""):
    """One DFSPH step on the device (phase B started by the device's own timer law) and in the oracle; the dt, vmax, iteration
    counts, warm starts and neighbour-list entries of the step must agree.  -> the device's step stats."""
    import yasph2d_amd as y

    vmax = ctx.step_begin(timer.simulation_step(), timer.law(diam))
    dt_ns = timer.update_simulation_step(diam, vmax)
    st = ctx.step_finish(y.duration_as_secs_f32(dt_ns))
    so = o.dfsph_step()
    assert dt_ns == o.timer_step_ns(), what
    assert np.float32(vmax) == np.float32(so["vmax"]), (what, vmax, so["vmax"])
    for k in ("density_iterations", "divergence_iterations", "warmstart_density", "warmstart_divergence", "neighbor_entries"):
        assert st[k] == so[k], (what, k, st[k], so[k])
    return st


def assert_same_state(ctx, o, what=""):
    """ids, positions, velocities, densities, kappa, stiffness and the neighbour lists, bit for bit."""
    d = ctx.download()
    np.testing.assert_array_equal(d["ids"], o.ids(), what + " ids")
    assert_bits_equal(d["pos"], o.positions(), what + " positions")
    assert_bits_equal(d["vel"], o.velocities(), what + " velocities")
    assert_bits_equal(d["density"], o.densities(), what + " densities")
    ss = ctx.download_solver_state()
    assert_bits_equal(ss["kappa"], o.kappa(), what + " kappa")
    assert_bits_equal(ss["stiffness"], o.stiffness(), what + " stiffness")
    assert_same_neighbors(ctx.download_neighbors(), o.neighbors())


def lattice_scene(n, b, spacing=np.float32(1.0 / 90.0), origin=(0.5, 0.5)):
    """Exactly n fluid particles on a square lattice at the reference's fluid spacing (row-major, the last row partly filled) and
    exactly b boundary particles at the boundary spacing (0.01) in rows of up to 64 under it, the first one spacing below."""
    side = max(1, int(np.ceil(np.sqrt(n))))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n].astype(np.float32)
    o = np.array(origin, np.float32)
    pos = (o + g * np.float32(spacing)).astype(np.float32).reshape(-1, 2)
    k = np.arange(b)
    row, col = k // 64, k % 64
    x0 = o[0] + np.float32(side) * np.float32(spacing) * np.float32(0.5) - np.float32(0.01) * np.float32(min(b, 64)) * np.float32(0.5)
    bnd = np.stack([x0 + col.astype(np.float32) * np.float32(0.01), o[1] - np.float32(spacing) - row.astype(np.float32) * np.float32(0.01)], -1)
    return pos, bnd.astype(np.float32).reshape(-1, 2)
