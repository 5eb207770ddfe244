"""The oracle's DFSPH sub-steps against the float64 restatement of the Rust solver (tests/dfsph_reference64.py), lock-step.

The oracle and the device are compared with each other bit for bit elsewhere; neither is compared with the reference's formulas
there, and a slip made in both would pass.  Here the oracle's tile backend (one tile over the whole domain) runs the sub-steps of
TiledDFSPH.step; after each one its state must be what the restatement computes from the state before it, within the round-off
bound of tests/dfsph_lockstep.py (C = 2, per-output allowances K there).  Every mutant of the restatement — one plausible slip each —
must be rejected by the same comparison on the same recorded data; the ratio by which each one exceeds the bound is printed."""
import numpy as np
import pytest
from dfsph_lockstep import (MUTANTS, Bounds, check_trace, make_plan, membership_of_trace, mutant, restatement, run_plan,
                            single_tile)
from util import dam_break, lattice_scene

H = 0.02


def disturbed(pos, seed, sigma=0.5):
    return np.random.default_rng(seed).normal(0.0, sigma, pos.shape).astype(np.float32)


def spray(seed=5):
    """Sparse spray: isolated particles (alpha floor 1e-6 -> alpha = 1e6), particles with 1..8 neighbours and small clumps
    around the <9 gate, converging velocities (positive density change), over an odd-length boundary line."""
    rng = np.random.default_rng(seed)
    far = rng.uniform(0.0, 1.0, (300, 2))
    clumps = []
    for k in range(40):
        c = rng.uniform(0.05, 0.95, 2)
        m = 3 + k % 12
        clumps.append(c + rng.uniform(-0.012, 0.012, (m, 2)))
    pos = np.concatenate([far] + clumps).astype(np.float32)
    vel = (rng.normal(0.0, 0.3, pos.shape) - 0.5 * (pos - pos.mean(0))).astype(np.float32)
    xs = np.arange(0.0, 1.0, 0.01, dtype=np.float32)[:99]
    boundary = np.stack([xs, np.full_like(xs, -0.01)], -1)
    return pos, vel, boundary


def boundary_only():
    """Fluid particles 1.5 h apart right above a boundary line: their only neighbours are boundary particles."""
    xs = np.arange(0.1, 0.9, 0.03, dtype=np.float32)
    pos = np.stack([xs, np.full_like(xs, 0.007)], -1).astype(np.float32)
    vel = np.stack([np.zeros_like(xs), -np.linspace(0.2, 1.0, len(xs), dtype=np.float32)], -1)
    bx = np.arange(0.0, 1.0, 0.01, dtype=np.float32)[:101]
    boundary = np.stack([bx, np.zeros_like(bx)], -1)
    return pos, vel, boundary


def lattice_at_h(seed=7):
    """A lattice of spacing h (pairs at q = 1 up to fp32 rounding, just inside or outside), pairs exactly h apart (q = 1: in the
    list, contributing zero), near-coincident twins (d^2 <= 1e-10: not neighbours of each other) and boundary rows below."""
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24)), -1).reshape(-1, 2).astype(np.float32)
    pos = (np.float32(0.5) + g * np.float32(H)).astype(np.float32)
    twins = pos[::37] + np.float32(4e-6)
    pos = np.concatenate([pos, twins]).astype(np.float32)
    # half-spacing rows so that neighbours exist besides the q = 1 pairs
    half = (pos[:200] + np.float32(H / 2)).astype(np.float32)
    pos = np.concatenate([pos, half]).astype(np.float32)
    # pairs exactly h apart in fp32 (x = -h/2 and +h/2: halving is exact), each on its own
    hh = np.float32(H) / np.float32(2)
    ys = (np.float32(0.1) + np.float32(0.06) * np.arange(10, dtype=np.float32)).astype(np.float32)
    pairs = np.concatenate([np.stack([np.full_like(ys, -hh), ys], -1), np.stack([np.full_like(ys, hh), ys], -1)])
    pos = np.concatenate([pos, pairs]).astype(np.float32)
    bx = np.arange(0.48, 1.0, 0.01, dtype=np.float32)
    boundary = np.concatenate([np.stack([bx, np.full_like(bx, 0.485 - 0.01 * r)], -1) for r in range(2)]).astype(np.float32)[:-1]
    return pos, disturbed(pos, seed, 0.3), boundary


def random_scene(seed, dense=False):
    import test_gpu_random_scenes

    return test_gpu_random_scenes.scene(seed, dense=dense)


def dense_cluster():
    """Clusters at 0.4 x the usual spacing: lists capped at 64 entries.  Without the random scene's floor segment: a static hit
    after 64 dynamic neighbours is the reference's panic (neighborhood_search.rs:373), an error on the device."""
    pos, vel, _ = random_scene(101, dense=True)
    return pos, vel, np.zeros((0, 2), np.float32)


def dam_break_disturbed():
    pos, boundary = dam_break(1.0)
    return pos, disturbed(pos, 1), boundary


def sized(n, b=37):
    pos, boundary = lattice_scene(n, b)
    return pos, disturbed(pos, n), boundary


# name -> (scene, steps, fixed iterations)
SCENES = {
    "dam_break": (dam_break_disturbed, 2, (3, 2)),
    "random": (lambda: random_scene(3), 2, (3, 2)),
    "dense_cluster": (dense_cluster, 1, (2, 1)),
    "spray": (spray, 2, (3, 2)),
    "boundary_only": (boundary_only, 2, (2, 2)),
    "lattice_at_h": (lattice_at_h, 2, (3, 2)),
}
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
for _n in SIZES:
    SCENES[f"n{_n}"] = ((lambda n=_n: sized(n)), 2, (2, 2))


def oracle_backend():
    from tile_oracle_backend import OracleTileBackend

    return OracleTileBackend()


_traces = {}


def oracle_trace(name):
    if name not in _traces:
        if name == "dam_break_300":
            _traces[name] = dam_break_after_300()
        else:
            make, steps, fixed = SCENES[name]
            pos, vel, boundary = make()
            b = oracle_backend()
            boundary = single_tile(b, pos, vel, boundary)
            _traces[name] = run_plan(b, make_plan(steps, fixed))
    return _traces[name]


def dam_break_after_300():
    """The reference scene after 300 oracle steps (adaptive timer): impact, live warm-start values in their slots."""
    from oracle.oracle import Oracle

    pos, boundary = dam_break(1.0)
    o = Oracle()
    o.set_boundary(boundary)
    o.set_particles(pos)
    stats = [o.dfsph_step() for _ in range(300)]
    assert sum(s["warmstart_density"] + s["warmstart_divergence"] for s in stats[-50:]) > 0
    p, v, kappa, stiff = o.positions(), o.velocities(), o.kappa(), o.stiffness()
    assert np.abs(kappa).max() > 0 and np.abs(stiff).max() > 0
    b = oracle_backend()
    boundary = single_tile(b, p, v, boundary, kappa, stiff)
    return run_plan(b, make_plan(2, (3, 2), warm_from=0))


ALL = list(SCENES) + ["dam_break_300"]


@pytest.mark.parametrize("name", ALL)
def test_oracle_substeps_match_float64_restatement(name):
    trace = oracle_trace(name)
    bounds = check_trace(trace, restatement(), Bounds(), name)
    print(f"\n{name}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    membership_of_trace(trace, H)


def test_scenes_reach_the_edges():
    """The scenes exercise what they are there for: alpha at its 1e-6 floor, particles with 1..8 and exactly 9 neighbours,
    fluid particles whose only neighbours are boundary particles, capped lists, q = 1 pairs and excluded near-coincident twins."""
    def final(name):
        return oracle_trace(name)[-1][3]

    seen = set()
    for op, _, _, s in oracle_trace("spray"):
        if op[0] == "regrid":
            tot = s["counts"][:, 1]
            assert (tot == 0).any() and (s["alpha"][tot == 0] == np.float32(1e6)).all()
            seen |= set(tot.tolist())
    assert set(range(10)) <= seen, sorted(seen)
    s = final("boundary_only")
    assert (s["counts"][:, 0] == 0).all() and (s["counts"][:, 1] > 0).all()
    assert (final("dense_cluster")["counts"][:, 1] == 64).any()
    s = oracle_trace("lattice_at_h")[0][3]
    d = s["pos"][:, None, :] - s["pos"][None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    hsq = np.float32(H) * np.float32(H)
    assert (d2 == hsq).any()                              # q = 1
    assert ((d2 > 0) & (d2 <= np.float32(1e-10))).any()     # twins
    assert (s["counts"][:, 1] == 1).sum() >= 20              # the exact-h pairs list each other


_mutant_ratios = {}


@pytest.mark.parametrize("cls", MUTANTS, ids=lambda c: c.__name__)
def test_mutant_is_rejected_on_oracle_data(cls):
    """The comparison must be able to fail: replayed through a mutated restatement, the recorded sub-steps of the disturbed dam
    break, the spray and the 300-step state must exceed the bound.  The smallest excess ratio is printed."""
    ratio = 0.0
    for name in ("dam_break", "spray", "dam_break_300"):
        b = check_trace(oracle_trace(name), mutant(cls), Bounds(), name)
        ratio = max(ratio, b.max_ratio())
    _mutant_ratios[cls.__name__] = ratio
    print(f"\n{cls.__name__}: {ratio:.3g} x the bound")
    assert ratio > 1.0, f"mutant '{cls.__doc__}' passes the comparison (ratio {ratio:.3g})"
