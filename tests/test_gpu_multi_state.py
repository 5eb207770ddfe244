"""The checkpoint of a tiled run on the device (include/sphx.h, "checkpoint of a tiled run"): sphx_multi_state_size / _save / _load /
_digest and their files, the solver object's checkpoint / restore, against tests/multi_state_reference.py and sphx_multi_download.  All
scenes are the dam break of tests/util.py at scale 1.0 (4 050 particles, every tile on device 0): small, and it has ghosts, migration and
re-partitioning.  The format's validation, the digest's hand cases and the exports are checked without a GPU in
tests/test_multi_state_host.py."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import multi_state_reference as mref
import state_reference as sref
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)  # every sphx_step_stats field
FIVE = ("positions", "velocities", "particle_id", "kappa", "stiffness")
BAD, NOT_READY, CAPACITY = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY, _lib.ERR_CAPACITY


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, params=None, rebalance_every=4, halo=10, invariant=False, grid=True):
    layout = _lib.LAYOUT_AUTO if grid else _lib.LAYOUT_STRIPS
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every, layout=layout)
    if invariant:
        m.set_tiling_invariant(True)
    return m


def make_multi(world, **kw):
    m = new_multi(world, **kw)
    m.set_boundary(BOUNDARY)
    m.upload(POS)
    return m


def by_id(d):
    """a download sorted by id"""
    o = np.argsort(d["ids"], kind="stable")
    return {k: v[o] for k, v in d.items()}


def owned_solver_state(m, world):
    """ids and alpha / kappa / stiffness of the particles the tiles own, tile after tile in device order (what the part holds)"""
    ids, out = [], dict(alpha=[], kappa=[], stiffness=[])
    for k in range(world):
        c = m.tile_context(k)
        t, s = c.download(), c.download_solver_state()
        own = (t["ids"] >> 31) == 1
        ids.append(t["ids"][own] & 0x7FFFFFFF)
        for name in out:
            out[name].append(s[name][own])
    return np.concatenate(ids), {k: np.concatenate(v) for k, v in out.items()}


def digests_of_part(p):
    return {s: p["table"][s][2] for s in mref.SECTIONS}


def same_stats(a, b):
    return all(x[k] == y_[k] or (x[k] != x[k] and y_[k] != y_[k]) for x, y_ in zip(a, b) for k in STEP_FIELDS) and len(a) == len(b)


# ---- 1. content ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run40():
    """4 tiles, 40 adaptive steps with a re-partition every 4; saves and digests between the steps"""
    m = make_multi(4)
    timer = y.TimeManager()
    stats, blobs = [], []
    for k in range(40):
        stats.append(m.step(timer))
        if k % 10 == 9:
            blobs.append(m.save_state())
            m.state_digest()
    return m, timer, stats, blobs


def test_the_part_holds_what_the_tiles_own(run40):
    m, _, stats, blobs = run40
    assert m.info()["rebalances"] > 0
    blob = m.save_state()
    assert blob == m.save_state() == blobs[-1], "two saves of one state must be byte-identical"
    p = mref.parse_part(blob)
    d = m.download()
    assert (p["n_total"], p["n_part"], p["b"], p["part"], p["n_parts"], p["world"], p["steps"]) == (N, N, len(BOUNDARY), 0, 1, 4, 40)
    assert p["tiling_invariant"] == 0 and p["axis"] == -1 and (p["nx"], p["ny"]) == (2, 2) and len(p["cuts"]) == 9
    assert (p["num_density_iters"], p["num_divergence_iters"]) == (stats[-1]["density_iterations"], stats[-1]["divergence_iterations"])
    assert (p["last_div_iters"], p["last_div_warm"]) == (stats[-1]["divergence_iterations"], stats[-1]["warmstart_divergence"])
    # the part in the tiles' device order IS the download (tile after tile, owned particles in local order)
    assert np.array_equal(p["particle_id"], d["ids"]) and p["positions"].tobytes() == d["pos"].tobytes()
    assert p["velocities"].tobytes() == d["vel"].tobytes() and p["density"].tobytes() == d["density"].tobytes()
    assert sorted(p["particle_id"].tolist()) == list(range(N))
    assert p["boundary"].tobytes() == np.ascontiguousarray(BOUNDARY, np.float32).tobytes()
    ids, s = owned_solver_state(m, 4)
    assert np.array_equal(ids, p["particle_id"]) and p["alpha"].tobytes() == s["alpha"].tobytes()
    for name, cnt in (("kappa", p["num_density_iters"]), ("stiffness", p["num_divergence_iters"])):
        want = s[name] if cnt > 1 else np.zeros(N, np.float32)
        assert p[name].tobytes() == want.tobytes(), name
    # digests: the table, the live digest and the reference over the download agree; for ids 0 .. N-1 they are the section digests by id
    table, live = digests_of_part(p), m.state_digest()
    want = mref.run_digests(d["ids"], d["pos"], d["vel"], d["density"], p["alpha"], p["kappa"], p["stiffness"], BOUNDARY)
    assert table == live == want
    di = by_id(d)
    assert table["positions"] == sref.digest(di["pos"]) and table["velocities"] == sref.digest(di["vel"]) and table["density"] == sref.digest(di["density"])
    assert table["particle_id"] == sref.digest(np.arange(N, dtype=np.uint32))


def test_saves_and_digests_do_not_change_the_run(run40):
    m, timer, stats, _ = run40
    plain = make_multi(4)
    t2 = y.TimeManager()
    stats2 = [plain.step(t2) for _ in range(40)]
    assert same_stats(stats, stats2) and t2.simulation_step_ns() == timer.simulation_step_ns()
    a, b = m.download(), plain.download()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert m.info()["exchanges"] == plain.info()["exchanges"]
    plain.close()


def test_canonical_zeros_with_one_iteration_loops():
    m = make_multi(4, params=y.default_params(fixed_iterations=(1, 1)))
    timer = y.TimeManager()
    m.steps(timer, 6)
    p = mref.parse_part(m.save_state())
    assert (p["num_density_iters"], p["num_divergence_iters"]) == (1, 1)
    zero = np.zeros(N, np.float32).tobytes()  # +0.0: all bits clear
    assert p["kappa"].tobytes() == zero and p["stiffness"].tobytes() == zero
    assert p["table"]["kappa"][2] == p["table"]["stiffness"][2] == (N * mref.LEN) & mref.MASK
    m.close()


def test_part_of_one_tile_and_of_strips_and_size():
    # (three strips along x of which the third lies to the right of the fluid and owns nothing)
    for world, strips in ((1, None), (2, None), (3, (0, [0, 5017, 5100, 65536]))):
        m = new_multi(world, rebalance_every=4 if strips is None else 0)
        if strips:
            m.set_strips(*strips)
        m.set_boundary(BOUNDARY)
        m.upload(POS)
        timer = y.TimeManager()
        m.steps(timer, 5)
        blob = m.save_state()
        p = mref.parse_part(blob)
        d = m.download()
        assert p["world"] == world and p["axis"] in (0, 1) and len(p["cuts"]) == world + 1 and (p["nx"], p["ny"]) == (1, 1)
        assert strips is None or (p["axis"], p["cuts"]) == strips
        assert p["positions"].tobytes() == d["pos"].tobytes() and np.array_equal(p["particle_id"], d["ids"])
        assert digests_of_part(p) == m.state_digest()
        m.close()


# ---- 2. tiling-invariant mode: the loaded run continues bit for bit, whatever the loader's tiling ------------------------------------------
@pytest.fixture(scope="module")
def invariant_run():
    params = y.default_params(fixed_iterations=(2, 2))
    m = make_multi(4, params=params, invariant=True)
    timer = y.TimeManager()
    first = m.steps(timer, 6)
    blob, tstate, dig = m.save_state(), timer.get_state(), m.state_digest()
    rest = m.steps(timer, 6)
    assert all(s["warmstart_density"] == 1 and s["warmstart_divergence"] == 1 for s in rest), "both warm starts must fire"
    end = by_id(m.download())
    m.close()
    return params, blob, tstate, dig, rest, end, timer.simulation_step_ns()


@pytest.mark.parametrize("world", [4, 2, 1], ids=["2x2", "2 strips", "one tile"])
def test_invariant_mode_continues_bit_identically(invariant_run, world):
    params, blob, tstate, dig, rest, end, dt_ns = invariant_run
    m = new_multi(world, params=params, invariant=True)
    m.load_state(blob)  # (before any upload: the checkpoint brings the boundary too)
    assert m.state_digest() == dig == digests_of_part(mref.parse_part(blob)), "all eight digests after the load equal the checkpoint's"
    timer = y.TimeManager()
    timer.set_state(tstate)
    got = m.steps(timer, 6)
    assert same_stats(got, rest) and timer.simulation_step_ns() == dt_ns
    d = by_id(m.download())
    for k in ("ids", "pos", "vel", "density"):
        assert d[k].tobytes() == end[k].tobytes(), k
    m.close()


# ---- 3. default mode --------------------------------------------------------------------------------------------------------------------------
def run_default(world, steps, grid=True):
    m = make_multi(world, grid=grid)
    timer = y.TimeManager()
    m.steps(timer, steps)
    return m, timer


def max_abs_by_id(a, b):
    a, b = by_id(a), by_id(b)
    assert np.array_equal(a["ids"], b["ids"])
    return max(float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in ("pos", "vel", "density"))


def test_default_mode_load_holds_the_saved_particles_and_two_loads_agree():
    m, timer = run_default(4, 12)
    blob, tstate = m.save_state(), timer.get_state()
    saved, p = by_id(m.download()), mref.parse_part(m.save_state())
    ids_s, sol_s = owned_solver_state(m, 4)
    m.close()
    loaded = []
    for _ in range(2):
        k = new_multi(4)
        k.load_state(blob)
        d = by_id(k.download())
        for name in ("ids", "pos", "vel"):
            assert d[name].tobytes() == saved[name].tobytes(), name
        dig = k.state_digest()
        assert all(dig[s] == p["table"][s][2] for s in FIVE + ("boundary",))
        # kappa and stiffness by id, bit for bit (canonical where the loops will not read them)
        ids_l, sol_l = owned_solver_state(k, 4)
        for name in ("kappa", "stiffness"):
            want = np.zeros(N, np.float32)
            want[p["particle_id"]] = p[name]
            got = np.zeros(N, np.float32)
            got[ids_l] = sol_l[name]
            cnt = p["num_density_iters"] if name == "kappa" else p["num_divergence_iters"]
            if cnt > 1:
                assert got.tobytes() == want.tobytes(), name
        i = k.info()
        assert (i["world"], i["grid_layout"]) == (4, 1)
        loaded.append(k)
    runs = []
    for k in loaded:
        t = y.TimeManager()
        t.set_state(tstate)
        runs.append((k.steps(t, 10), k.download(), t.simulation_step_ns()))
        k.close()
    assert same_stats(runs[0][0], runs[1][0]) and runs[0][2] == runs[1][2]
    for name in runs[0][1]:
        assert runs[0][1][name].tobytes() == runs[1][1][name].tobytes(), name


def test_default_mode_restart_is_within_the_spread_between_tilings():
    """Restart versus uninterrupted run after 10 steps, judged against the spread the project already has between two tilings of one run:
    max |difference| by id over pos, vel and density between the uninterrupted 2-strip and 2 x 2 default-mode runs of the same 10 steps.
    The restart may differ from its uninterrupted twin by at most 4 x that (one realisation of rounding noise against another)."""
    a, _ = run_default(2, 10)
    b, _ = run_default(4, 10)
    yard = max_abs_by_id(a.download(), b.download())
    a.close()
    m, timer = run_default(4, 5)
    blob, tstate = m.save_state(), timer.get_state()
    m.close()
    k = new_multi(4)
    k.load_state(blob)
    t = y.TimeManager()
    t.set_state(tstate)
    k.steps(t, 5)
    diff = max_abs_by_id(k.download(), b.download())
    print("default mode, 10 steps: spread between 2 strips and 2x2 %.6g, restart (saved at step 5) against uninterrupted 2x2 %.6g" % (yard, diff))
    assert diff <= 4.0 * yard
    b.close()
    k.close()


def test_a_checkpoint_of_2x2_loads_into_other_tilings_and_layouts():
    m, _ = run_default(4, 8)
    blob = m.save_state()
    saved = by_id(m.download())
    p = mref.parse_part(blob)
    m.close()
    for world, strips in ((2, None), (3, (0, [0, 5017, 5100, 65536])), (1, None), (2, (1, [0, 5055, 65536]))):
        k = new_multi(world, rebalance_every=4 if world != 3 else 0)
        if strips:
            k.set_strips(*strips)
        k.load_state([blob])
        d = by_id(k.download())
        for name in ("ids", "pos", "vel"):
            assert d[name].tobytes() == saved[name].tobytes(), (world, name)
        dig = k.state_digest()
        assert all(dig[s] == p["table"][s][2] for s in FIVE + ("boundary",))
        if strips:
            assert mref.parse_part(k.save_state())["cuts"] == strips[1] and k.info()["axis"] == strips[0]
        t = y.TimeManager()
        st = k.steps(t, 2)
        assert all(s["flags"] == 0 for s in st)
        k.close()


# ---- 4. refusals and states -----------------------------------------------------------------------------------------------------------------------
def reseal(raw):
    """the header's digest recomputed (a forgery the structural checks have to catch)"""
    raw = bytearray(raw)
    struct.pack_into("<Q", raw, mref.DIGEST_AT, sref.digest(bytes(raw[:mref.DIGEST_AT])))
    return bytes(raw)


def test_refusals_leave_the_multi_untouched_and_a_mismatch_asks_for_a_load(tmp_path):
    params = y.default_params()
    fresh = new_multi(2)
    for fn in (fresh.save_state, fresh.state_digest):
        assert "before the first" in refused(NOT_READY, fn)
    m, timer = run_default(2, 6)
    blob = m.save_state()
    before = (m.save_state(), m.info()["exchanges"])

    def untouched():
        assert (m.save_state(), m.info()["exchanges"]) == before

    L = m.L
    n = C.c_uint64()
    buf = np.zeros(len(blob), np.uint8)
    # flags, capacity, NULL
    assert L.sphx_multi_state_save(m.h, buf.ctypes.data_as(C.c_void_p), len(blob), 1, C.byref(n)) == BAD
    assert L.sphx_multi_state_save(m.h, buf.ctypes.data_as(C.c_void_p), len(blob) - 1, 0, C.byref(n)) == CAPACITY and n.value == len(blob)
    assert L.sphx_multi_state_save(m.h, None, 0, 0, C.byref(n)) == BAD and n.value == len(blob)
    assert L.sphx_multi_state_size(m.h, C.byref(n)) == 0 and n.value == len(blob)
    ptrs, sizes = (C.c_void_p * 1)(buf.ctypes.data), (C.c_uint64 * 1)(len(blob))
    buf[:] = np.frombuffer(blob, np.uint8)
    assert L.sphx_multi_state_load(m.h, ptrs, sizes, 1, 1) == BAD and L.sphx_multi_state_load(m.h, ptrs, sizes, 0, 0) == BAD
    untouched()
    # between step_begin and step_finish
    v = m.step_begin(timer.simulation_step())
    for fn, args in ((m.save_state, ()), (m.state_digest, ()), (m.load_state, (blob,)), (m.save_state_file, (tmp_path / "x",))):
        assert "step_finish" in refused(NOT_READY, fn, *args)
    m.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(np.float32(0.01), v)))
    blob = m.save_state()
    before = (blob, m.info()["exchanges"])
    # malformed parts: truncated, damaged header, forged counts, a single-context blob, sets that are none
    assert "truncated" in refused(BAD, m.load_state, blob[:-8])
    assert "truncated" in refused(BAD, m.load_state, blob[:100])
    assert "damaged" in refused(BAD, m.load_state, blob[:130] + b"\x01" + blob[131:])
    forged = bytearray(blob)
    struct.pack_into("<I", forged, 128, N + 1)
    assert "N_part" in refused(BAD, m.load_state, reseal(forged))
    forged = bytearray(blob)
    struct.pack_into("<Q", forged, mref.TABLE_AT + 24, struct.unpack_from("<Q", blob, mref.TABLE_AT)[0])
    assert "overlap" in refused(BAD, m.load_state, reseal(forged))
    forged = bytearray(blob)
    struct.pack_into("<II", forged, 136, 1, 2)
    assert "missing" in refused(BAD, m.load_state, reseal(forged))
    assert "more parts" in refused(BAD, m.load_state, [blob, blob])
    p = mref.parse_part(blob)
    forged = bytearray(blob)
    forged[p["table"]["particle_id"][0] + 3] |= 0x80
    assert "2^31" in refused(BAD, m.load_state, bytes(forged))
    forged = bytearray(blob)
    forged[p["table"]["boundary"][0]] ^= 1
    assert "boundary" in refused(BAD, m.load_state, bytes(forged))
    forged = bytearray(blob)
    forged[p["table"]["density"][0] + p["table"]["density"][1]] = 1  # the padding behind an odd count of 4-byte words
    assert N % 2 == 0 or "padding" in refused(BAD, m.load_state, bytes(forged))
    ctx = y.SphxContext(params)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    assert "single-context" in refused(BAD, m.load_state, ctx.save_state())
    ctx.close()
    untouched()
    # params that differ in one field; the other mode
    other = new_multi(2, params=y.default_params(fixed_iterations=(0, 3)))
    assert "fixed_divergence_iterations" in refused(BAD, other.load_state, blob)
    refused(NOT_READY, other.save_state)
    other.close()
    inv = new_multi(2, invariant=True)
    assert "tiling-invariant" in refused(BAD, inv.load_state, blob)
    inv.set_boundary(BOUNDARY)
    inv.upload(POS)
    assert "tiling-invariant" in refused(BAD, m.load_state, inv.save_state())
    inv.close()
    untouched()
    # files
    path = tmp_path / "ckpt.bin"
    m.save_state_file(path)
    assert path.read_bytes() == blob and not os.path.exists(str(path) + ".tmp")
    assert "neither" in refused(BAD, m.load_state_file, tmp_path / "nothing_here")
    refused(BAD, m.save_state_file, tmp_path / "no_such_dir" / "x")
    (tmp_path / "set.r000of002").write_bytes(blob)
    assert "incomplete" in refused(BAD, m.load_state_file, tmp_path / "set")
    untouched()
    k = new_multi(2)
    k.load_state_file(path)
    q = mref.parse_part(k.save_state())  # (density and alpha are recomputed by the load's re-grid: default mode promises the other six)
    assert all(q["table"][s] == p["table"][s] for s in FIVE + ("boundary",)) and all(q[s].tobytes() == p[s].tobytes() for s in FIVE + ("boundary",))
    # one payload word corrupted: the host checks pass, the device digest does not
    forged = bytearray(blob)
    forged[p["table"]["velocities"][0] + 8 * (N // 2)] ^= 0x10
    assert "velocities" in refused(BAD, k.load_state, bytes(forged))
    t2 = y.TimeManager()
    for fn, args in ((k.step, (t2,)), (k.save_state, ()), (k.state_digest, ()), (k.stats, ())):
        refused(NOT_READY, fn, *args)
    k.load_state(blob)  # ... and a load puts it right
    assert all(k.state_digest()[s] == p["table"][s][2] for s in FIVE + ("boundary",))
    assert k.step(t2)["flags"] == 0
    k.close()
    m.close()
    fresh.close()


def test_a_statistics_recording_survives_a_load():
    m, timer = run_default(2, 4)
    m.stats_record([(-1e30, -1e30, 1e30, 1e30)], 8)
    m.steps(timer, 2)
    blob = m.save_state()
    m.load_state(blob)
    m.steps(timer, 2)
    st = m.stats_status()
    assert (st["recording"], st["frames"]) == (1, 4)
    m.close()


# ---- 5. one process per tile ------------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_load_in_process_and_into_the_ranks_again(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars, and with them the digests), tiling-invariant mode,
    fixed 2 + 2: each rank writes its part; the set loads into the two ranks again and into an in-process 2-tile multi, and all three
    continue bit-identically; state_digest() returns the same 64 bytes on both ranks."""
    before, after = 6, 6
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29553",
           os.path.join(HERE, "multi_state_rank_worker.py"), str(tmp_path), str(before), str(after)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    for k in ("dig_saved", "dig_loaded", "stats_a", "stats_b", "timer", "dt_ns"):
        assert r[0][k].tobytes() == r[1][k].tobytes(), k
    assert r[0]["dig_saved"].tobytes() == r[0]["dig_loaded"].tobytes(), "all eight digests after the load equal the checkpoint's"
    assert r[0]["stats_a"].tobytes() == r[0]["stats_b"].tobytes()
    parts = [(tmp_path / ("ckpt.r%03dof002" % k)).read_bytes() for k in range(2)]
    heads = [mref.parse_part(b) for b in parts]
    for k in range(2):
        assert parts[k] == r[k]["part"].tobytes() and (heads[k]["part"], heads[k]["n_parts"], heads[k]["n_total"]) == (k, 2, N)
        for name in ("ids", "pos", "vel", "density"):
            assert r[k][name + "_a"].tobytes() == r[k][name + "_b"].tobytes(), (k, name)  # the ranks, loaded again, repeat their run
    assert heads[0]["n_part"] + heads[1]["n_part"] == N
    table = [sum(h["table"][s][2] for h in heads) & mref.MASK for s in mref.SECTIONS[:7]]
    assert table == [int(v) for v in r[0]["dig_saved"][:7]] and int(r[0]["dig_saved"][7]) == heads[0]["table"]["boundary"][2]
    # the in-process multi: the same parts (given in the other order), the same continuation
    m = new_multi(2, params=y.default_params(fixed_iterations=(2, 2)), invariant=True)
    m.load_state([parts[1], parts[0]])
    assert [m.state_digest()[s] for s in mref.SECTIONS] == [int(v) for v in r[0]["dig_saved"]]
    timer = y.TimeManager()
    timer.set_state(_lib.SphxTimerState.from_buffer_copy(r[0]["timer"].tobytes()))
    st = m.steps(timer, after)
    assert np.array([[float(s[k]) for k in STEP_FIELDS] for s in st]).tobytes() == r[0]["stats_a"].tobytes()
    assert timer.simulation_step_ns() == int(r[0]["dt_ns"][0])
    d = by_id(m.download())
    ranks = by_id({k: np.concatenate([r[0][k + "_a"], r[1][k + "_a"]]) for k in ("ids", "pos", "vel", "density")})
    for name in ("ids", "pos", "vel", "density"):
        assert d[name].tobytes() == ranks[name].tobytes(), name
    m.close()


# ---- 6. the solver object ----------------------------------------------------------------------------------------------------------------------
def test_solver_checkpoint_and_restore_round_trip_the_timer(tmp_path):
    def world_and_solver():
        w = y.FluidParticleWorld()
        w.reset_fluid(1.0)
        s = y.DFSPHMultiSolver(w, [0, 0], params=y.default_params(fixed_iterations=(2, 2)))
        s.multi().set_tiling_invariant(True)  # (promise 2: the restored run then repeats the uninterrupted one bit for bit)
        return w, s

    w, s = world_and_solver()
    timer = y.TimeManager()
    path = tmp_path / "run.ckpt"
    with pytest.raises(y.SphxError) as e:
        s.checkpoint(w, timer, path)
    assert e.value.code == NOT_READY
    s.simulation_steps(w, timer, 6, sync_world=False)
    s.checkpoint(w, timer, path)
    tstate = bytes(timer.get_state())
    # the old calls still refuse this solver
    for fn in (s.save, s.load):
        with pytest.raises(y.SphxError) as e:
            fn(w, timer, tmp_path / "old.bin")
        assert e.value.code == BAD and "multi-GPU" in str(e.value)
    rest = s.simulation_steps(w, timer, 4, sync_world=False)
    s.sync_world(w)
    end = by_id(dict(pos=w.positions, vel=w.velocities, ids=w.particle_ids))
    w2, s2 = world_and_solver()
    t2 = y.TimeManager(fixed_ns=999)
    s2.restore(w2, t2, path)
    assert bytes(t2.get_state()) == tstate and w2.num_dynamic_particles == N
    assert np.array(w2.boundary_particles).tobytes() == np.array(w.boundary_particles).tobytes()
    got = s2.simulation_steps(w2, t2, 4, sync_world=False)
    assert same_stats(got, rest) and t2.num_steps == timer.num_steps and bytes(t2.get_state()) == bytes(timer.get_state())
    s2.sync_world(w2)
    d = by_id(dict(pos=w2.positions, vel=w2.velocities, ids=w2.particle_ids))
    assert d["ids"].tolist() == list(range(N))
    for name in ("ids", "pos", "vel"):
        assert d[name].tobytes() == end[name].tobytes(), name
    # a single-context solver is refused, and so is a file that is none
    w3 = y.FluidParticleWorld()
    w3.reset_fluid(1.0)
    s3 = y.DFSPHSolver(w3)
    assert s3.L.sphx_solver_multi_checkpoint(s3.h, w3.h, timer.h, str(path).encode()) == BAD
    assert s3.L.sphx_solver_multi_restore(s3.h, w3.h, timer.h, str(path).encode()) == BAD
    bad = tmp_path / "bad.ckpt"
    bad.write_bytes(path.read_bytes()[:-4])
    with pytest.raises(y.SphxError) as e:
        s2.restore(w2, t2, bad)
    assert e.value.code == BAD and "truncated" in str(e.value)
