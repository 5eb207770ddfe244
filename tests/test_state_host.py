"""Saving and restoring a context (sphx_state_*, include/sphx.h), the parts that need no GPU: the reference digest on hand cases, the
blob format's validation as a sanitized stand-alone program, the timer state, and the exports / bindings / NULL handling / harness
options."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import state_reference as ref

import yasph2d_amd as y
from yasph2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
STATE_CALLS = ("sphx_state_size", "sphx_state_save", "sphx_state_load", "sphx_state_digest", "sphx_state_save_file", "sphx_state_load_file",
               "sphx_timer_get_state", "sphx_timer_set_state", "sphx_solver_save", "sphx_solver_load")


# ------------------------------------------------------------------------------------------------------ 1. the reference digest
def test_digest_hand_cases():
    M, L, K = ref.MUL, ref.LEN, ref.MASK
    assert ref.digest_ints([]) == 0 == ref.digest(np.zeros(0, np.uint32))                       # an empty section
    assert ref.digest_ints([1]) == (M + L) & K == ref.digest(np.array([1], np.uint32))           # one word: 1 * (1 * M) + 1 * L
    assert ref.digest_ints([5]) == (5 * M + L) & K
    a, b = ref.digest_ints([1, 2]), ref.digest_ints([2, 1])                                      # position-weighted
    assert a == (1 * M + 2 * ((3 * M) & K) + 2 * L) & K and b == (2 * M + 1 * ((3 * M) & K) + 2 * L) & K and a != b
    assert ref.digest_ints([0] * 3) == (3 * L) & K != ref.digest_ints([0] * 4) == (4 * L) & K    # zeros of two lengths
    # wrap-around past 2^64: one product alone is ~2^95, and the reduced sum differs from the unreduced one
    big = [0xFFFFFFFF] * 8
    unreduced = sum(w * ((2 * i + 1) * M) for i, w in enumerate(big)) + 8 * L
    assert unreduced >> 64 and ref.digest_ints(big) == unreduced & K
    assert 0xFFFFFFFF * M >= 1 << 64
    # the multiplier of a word is reduced before the product too: (2 i + 1) * M wraps at i = 1 already (3 M > 2^64)
    assert 3 * M >= 1 << 64 and ref.digest_ints([0, 7]) == (7 * ((3 * M) & K) + 2 * L) & K


def test_digest_vectorised_equals_formula():
    rng = np.random.default_rng(7)
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 4097):
        w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        assert ref.digest(w) == ref.digest_ints(w.tolist())
    f = rng.standard_normal((33, 2)).astype(np.float32)
    assert ref.digest(f) == ref.digest_ints(f.view(np.uint32).reshape(-1).tolist()) == ref.digest(f.tobytes())


# ------------------------------------------------------------------------------------------------------ 2. the format driver
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the state-format driver"
    exe = str(tmp_path_factory.mktemp("state_format") / "state_format_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "state_format_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["valid", "corrupt_bytes", "corrupt_fields", "truncations", "solver_file", "params"])
def test_format_validation(driver, check):
    """valid: the built header (and the empty state) pass.  corrupt_bytes: every byte of the header, three damaged values each, is
    refused.  corrupt_fields: every field forged with the header's digest recomputed — magic, version, endianness, sizes, counts that
    disagree, sections out of range / overlapping / misaligned / misplaced, sizes that overflow 64 bits — is refused for the stated
    reason.  truncations: every length below the blob's is refused.  The sanitizers stay clean (any report aborts the program)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) > 0


def test_format_header_has_no_hip():
    """The format header is plain host C++ (the driver above compiled it with g++): it includes nothing of HIP."""
    src = open(os.path.join(CSRC, "sphx_state_format.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


def test_driver_digest_equals_reference(driver):
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 7, 100):
        w = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        rc, out, _ = driver("digest", *["%x" % v for v in w])
        assert rc == 0 and int(out, 16) == ref.digest_ints(w.tolist())


def test_reference_parser_reads_the_drivers_header(driver):
    """The parser of tests/state_reference.py (written from the layout's text) and the C++ header agree on a header the C++ built."""
    rc, out, _ = driver("header")
    assert rc == 0
    head = bytes.fromhex(out.strip())
    assert len(head) == ref.HEADER_BYTES
    (total,) = np.frombuffer(head, "<u8", 1, 16)
    p = ref.parse_blob(head + bytes(int(total) - len(head)))
    assert (p["n"], p["b"], p["cached_n"], p["wcsph_n"], p["ids_issued"]) == (1001, 33, 900, 7, 1200)
    assert (p["num_density_iters"], p["num_divergence_iters"], p["lists_current"], p["sampling_allowed"], p["set_changed"]) == (3, 2, 1, 1, 0)
    assert p["params"]["max_density_iterations"] == 200 and p["params"]["smoothing_length"] == np.float32(0.02)
    assert [p["table"][s][2] for s in ref.SECTIONS] == [0x1111111111111111 * (k + 1) for k in range(9)]
    assert p["alpha"].shape == (900,) and p["accel"].shape == (7, 2) and p["boundary"].shape == (33, 2)


# ------------------------------------------------------------------------------------------------------ 3. the timer state
def drive(timer, vmaxes):
    out = []
    for v in vmaxes:
        timer.on_step_started()
        out.append(timer.update_simulation_step(np.float32(0.01), np.float32(v)))
    return out


def make_timer(kind):
    if kind == "fixed":
        return y.TimeManager(fixed_ns=123456)
    t = y.TimeManager()
    if kind == "target_frame":
        t.set_target_frame(16666667 // 8)
    return t


@pytest.mark.parametrize("kind", ["adaptive", "fixed", "target_frame"])
def test_timer_state_continues(sphx_lib, kind):
    rng = np.random.default_rng(3)
    vmax = np.concatenate([rng.uniform(0.0, 0.3, 40), rng.uniform(0.5, 12.0, 80), [0.0, 1e-7, 1e4]]).astype(np.float32)
    half = len(vmax) // 2
    a = make_timer(kind)
    first = drive(a, vmax[:half])
    state = a.get_state()
    assert state.num_simulation_steps == half and state.simulation_step_ns == first[-1] and state.fixed == (kind == "fixed")
    rest = drive(a, vmax[half:])
    if kind != "fixed":
        assert len(set(first + rest)) > 10, "the sequence must exercise the adaptive law"
    # a timer of ANOTHER kind and history takes the state over completely
    b = y.TimeManager(fixed_ns=999) if kind != "fixed" else y.TimeManager()
    drive(b, vmax[:7])
    b.set_state(state)
    assert bytes(b.get_state()) == bytes(state)
    assert drive(b, vmax[half:]) == rest
    assert b.total_simulated_ns == a.total_simulated_ns and b.num_steps == a.num_steps == len(vmax)
    assert b.simulation_step_ns() == a.simulation_step_ns()
    assert bytes(b.get_state()) == bytes(a.get_state())


def test_timer_state_layout_and_refusals(sphx_lib):
    assert C.sizeof(_lib.SphxTimerState) == 56
    t = y.TimeManager()
    before = bytes(t.get_state())
    L = sphx_lib
    assert L.sphx_timer_get_state(None, C.byref(_lib.SphxTimerState())) == _lib.ERR_INVALID_ARGUMENT
    assert L.sphx_timer_get_state(t.h, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.sphx_timer_set_state(t.h, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.sphx_timer_set_state(None, C.byref(t.get_state())) == _lib.ERR_INVALID_ARGUMENT
    for field, value in (("fixed", 2), ("reserved", 1), ("cfl_factor", float("nan"))):
        s = t.get_state()
        setattr(s, field, value)
        with pytest.raises(y.SphxError) as e:
            t.set_state(s)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
        assert bytes(t.get_state()) == before, "a refused state must leave the timer unchanged"


# ------------------------------------------------------------------------------------------------------ 4. exports, bindings, NULL, harness
def test_header_declares_and_library_exports(sphx_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphx.h")).read(), flags=re.S)
    for name in STATE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES
    assert re.search(r"SPHX_STATE_DEVICE_BUFFER\s*=\s*1u", src) and re.search(r"#define\s+SPHX_STATE_SECTIONS\s+9\b", src)
    assert _lib.STATE_DEVICE_BUFFER == 1 and len(_lib.STATE_SECTIONS) == 9 == len(ref.SECTIONS)
    assert "sphx_timer_state" in src and "SPHX_ABI_VERSION 5" in src
    # the header says what the digest is not, and that sphx_multi_* has no counterpart
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    assert "NOT a cryptographic hash" in full and re.search(r"sphx_multi_\* has NO counterpart", full)


def test_null_arguments_are_refused(sphx_lib, tmp_path):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    n = C.c_uint64(123)
    buf = (C.c_uint8 * 512)()
    out = (C.c_uint64 * 9)()
    path = str(tmp_path / "never_written.bin").encode()
    assert L.sphx_state_size(None, C.byref(n)) == bad and L.sphx_state_size(None, None) == bad
    assert L.sphx_state_save(None, buf, 512, 0, C.byref(n)) == bad and L.sphx_state_save(None, None, 0, 0, None) == bad
    assert L.sphx_state_load(None, buf, 512, 0) == bad and L.sphx_state_load(None, None, 0, 0) == bad
    assert L.sphx_state_digest(None, out) == bad and L.sphx_state_digest(None, None) == bad
    assert L.sphx_state_save_file(None, path) == bad and L.sphx_state_save_file(None, None) == bad
    assert L.sphx_state_load_file(None, path) == bad and L.sphx_state_load_file(None, None) == bad
    assert not os.path.exists(path.decode())
    w, t = y.FluidParticleWorld(), y.TimeManager()
    for args in ((None, w.h, t.h, path), (None, None, None, None)):
        assert L.sphx_solver_save(*args) == bad and L.sphx_solver_load(*args) == bad


def test_harness_help_names_the_options(sphx_lib):
    exe = os.path.join(ROOT, "yasph2d_amd", "sphx_harness")
    assert os.path.exists(exe), "sphx_harness is built by __graft_entry__.build()"
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--load-state FILE" in r.stdout and "--save-state FILE[:at=STEP]" in r.stdout
    for args in (["--save-state"], ["--save-state", "x:at=-1"], ["--save-state", "x:at=1.5"], ["--save-state", ":at=3"], ["--load-state"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "invalid --" in r.stderr, (args, r.stderr)
