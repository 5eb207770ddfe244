"""Parameter sets away from the reference app's constants (smoothing factor 2, particle density 10 000, rest density 100, gravity
(0, -9.81), grid_min (-100, -100)) and one scene that scales with the particle spacing, for the parity tests that run the oracle,
the float64 restatement and the device at those sets.

A set is (smoothing factor, particle density, rest density, gravity, grid_min); everything else follows as in
fluidparticleworld.rs:53-89: radius = 0.5 / sqrt(particle density), h = 2 radius smoothing_factor, m = rho0 / particle density."""
import numpy as np

DEFAULT_GRAVITY = (0.0, -9.81)
DEFAULT_GRID_MIN = (-100.0, -100.0)

# id -> (smoothing factor, particle density, rest density, gravity, grid_min)
SETS = {
    "wide": (3.0, 1.0e4, 100.0, DEFAULT_GRAVITY, DEFAULT_GRID_MIN),          # h = 0.03: ~28 neighbours, 9 particles per cell
    "coarse_water": (2.0, 2500.0, 1000.0, DEFAULT_GRAVITY, DEFAULT_GRID_MIN),  # h = 0.04, m = 0.4, radius 0.01
    "fine": (2.0, 4.0e4, 997.0, (1.3, -4.0), (-3.0, -7.5)),                   # h = 0.01, m = 0.024925, oblique gravity, shifted grid
    "tiny": (2.5, 1.0e6, 1.0, DEFAULT_GRAVITY, (-1.0, -1.0)),                 # h = 0.0025000002 (not a round float), m = 1e-6
    "odd": (2.0, 123.0, 3.7, (0.0, -1.62), (-500.0, -500.0)),                 # h = 0.18033393, fl(h fl(1/h)) = 0.99999994
}
SET_IDS = list(SETS)
# section "saturated cell coordinates": every position of the scene lies beyond cell 65535 on both axes
SATURATED = (2.0, 4.0e6, 100.0, DEFAULT_GRAVITY, DEFAULT_GRID_MIN)
ORIGIN = (0.3737, 0.2143)  # no lattice point of any set's cell grid ((0.37, 0.21) is one at h = 0.01, grid_min (-3, -7.5))
STEP_N = 1500          # the stepping tests' block
CHEAP_N = (63, 257, 1025)


def _set(name):
    return SETS[name] if isinstance(name, str) else tuple(name)


def particle_density(name):
    return _set(name)[1]


def spacing(name):
    """Particle spacing s = 1 / sqrt(particle density), fp32."""
    return np.float32(1.0) / np.sqrt(np.float32(_set(name)[1]))


def properties(name):
    """smoothing_length, particle_mass, particle_radius, fluid_density in the reference's fp32 operations (fluidparticleworld.rs:53-89)."""
    sf, pd, rho0, _, _ = _set(name)
    radius = np.float32(0.5) / np.sqrt(np.float32(pd))
    return dict(smoothing_length=np.float32(2.0) * radius * np.float32(sf), particle_mass=np.float32(rho0) / np.float32(pd),
                particle_radius=radius, fluid_density=np.float32(rho0))


def diameter(name):
    """The CFL diameter: 2 particle_radius of the set."""
    return np.float32(2.0) * properties(name)["particle_radius"]


def params(name, **kw):
    """The library's parameter block of a set (keywords as yasph2d_amd.default_params: fixed_iterations, viscosity, ...)."""
    import yasph2d_amd as y

    sf, pd, rho0, gravity, grid_min = _set(name)
    p = y.default_params(sf, pd, rho0, **kw)
    p.gravity[0], p.gravity[1] = gravity
    p.grid_min[0], p.grid_min[1] = grid_min
    return p


def oracle(name, **kw):
    from oracle.oracle import Oracle

    sf, pd, rho0, gravity, grid_min = _set(name)
    return Oracle(sf, pd, rho0, gravity, grid_min, **kw)


def scene(name, n=STEP_N, seed=0, velocity_scale=0.5, jitter=0.03, origin=ORIGIN):
    """A jittered lattice block of n particles at spacing s (row-major in a square of side ceil(sqrt(n)), the last row partly filled)
    resting one spacing above a three-row floor at spacing s that is four particles wider than the block on each side.  Velocities:
    seeded normal of sigma velocity_scale s per second, so that the block settles instead of scattering.  (A lattice at spacing s is
    a few per cent denser than rho0 under the Wendland kernel, 3.5 % at smoothing factor 2: the first steps, at the timer's smallest
    dt, push it apart at some m/s.  That is the solver's answer to the state, the same in the oracle and on the device.)
    -> (positions, velocities, boundary), fp32."""
    s = spacing(name)
    rng = np.random.default_rng(seed)
    side = max(1, int(np.ceil(np.sqrt(n))))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n].astype(np.float32)
    o = np.array(origin, np.float32)
    pos = (o + (g + rng.uniform(-jitter, jitter, g.shape).astype(np.float32)) * s).astype(np.float32).reshape(-1, 2)
    vel = (rng.normal(0.0, 1.0, pos.shape) * (velocity_scale * float(s))).astype(np.float32)
    cols = np.arange(-4, side + 4, dtype=np.float32)
    boundary = np.concatenate([np.stack([o[0] + cols * s, np.full_like(cols, o[1] - np.float32(1 + row) * s)], -1) for row in range(3)])
    return pos, vel, boundary.astype(np.float32).reshape(-1, 2)


TILED_N = 6000                    # the tiled scene's block
TILED_DRIFT = (1500.0, 900.0)     # spacings per second: the block crosses cell columns and rows within ten steps
TILED_STEPS = 10
TILED_HALO = 8


def tiled_scene(name, n=TILED_N, drift=TILED_DRIFT, seed=0):
    """scene(name, n) with a uniform drift velocity (in spacings per second) on top of the seeded one, so that particles change tile
    within a ten-step run.  -> (positions, velocities, boundary), fp32."""
    pos, vel, boundary = scene(name, n, seed=seed)
    vel = (vel + (np.array(drift, np.float32) * spacing(name)).astype(np.float32)).astype(np.float32)
    return pos, vel, boundary


def cells(name, xy):
    """Cell coordinates of positions under the set's own constants: sat_u16((p - grid_min) * fl(1 / h)) per axis, int64 [n, 2]."""
    gm, inv = np.array(_set(name)[4], np.float32), np.float32(1.0) / properties(name)["smoothing_length"]
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((np.asarray(xy, np.float32) - gm).astype(np.float32) * inv).astype(np.float32)
    return np.fmin(np.fmax(v, np.float32(0.0)), np.float32(65535.0)).astype(np.int64)


def tile_cuts(name, pos):
    """A 2 x 2 layout of the set's cell grid: the x-cut at the 40 % quantile of the particles' cell columns, every column cut again at
    the median of its own cell rows.  -> (xcuts [3], ycuts [2][3])."""
    c = cells(name, pos)
    xcuts = [0, int(np.sort(c[:, 0])[int(0.4 * len(c))]), 65536]
    ycuts = []
    for ix in range(2):
        col = c[(c[:, 0] >= xcuts[ix]) & (c[:, 0] < xcuts[ix + 1]), 1]
        ycuts.append([0, int(np.sort(col)[len(col) // 2]), 65536])
    return xcuts, ycuts


def tile_rects(xcuts, ycuts):
    """The rectangles (x0, x1, y0, y1) of tile_cuts' layout in rank order ix * 2 + iy, as MultiSolver.tile_rects() reports them."""
    return np.array([(xcuts[ix], xcuts[ix + 1], ycuts[ix][iy], ycuts[ix][iy + 1]) for ix in range(2) for iy in range(2)], np.int64)


def owner(rects, c):
    """The tile whose rectangle holds each cell of c [n, 2]; exactly one does."""
    inside = np.stack([(c[:, 0] >= r[0]) & (c[:, 0] < r[1]) & (c[:, 1] >= r[2]) & (c[:, 1] < r[3]) for r in np.asarray(rects).tolist()], 0)
    assert (inside.sum(0) == 1).all(), "the rectangles do not partition the cell domain"
    return inside.argmax(0).astype(np.int32)
