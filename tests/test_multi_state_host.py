"""The checkpoint of a tiled run (sphx_multi_state_*, include/sphx.h), the parts that need no GPU: the id-keyed digest against the section
digest and on hand cases, the part format's validation as a sanitized stand-alone program, and the exports / bindings / NULL handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import multi_state_reference as mref
import numpy as np
import pytest
import state_reference as ref

import yasph2d_amd as y
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
CALLS = ("sphx_multi_state_size", "sphx_multi_state_save", "sphx_multi_state_load", "sphx_multi_state_digest", "sphx_multi_state_save_file",
         "sphx_multi_state_load_file", "sphx_solver_multi_checkpoint", "sphx_solver_multi_restore", "sphx_tile_state_pack", "sphx_tile_state_fetch",
         "sphx_tile_upload_state", "sphx_get_tiling_invariant")


# ------------------------------------------------------------------------------------------------------ 1. the id-keyed digest
def test_digest_by_id_equals_section_digest_for_ids_0_to_n():
    """For ids 0 .. N-1 the id-keyed digest is the section digest of the id-ordered array, whatever order the particles come in."""
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 64, 65, 257, 4050):
        for k in (1, 2):
            a = rng.integers(0, 1 << 32, (n, k), dtype=np.uint64).astype(np.uint32)
            by_id = ref.digest(a)
            assert mref.digest_by_id(np.arange(n), a) == by_id
            perm = rng.permutation(n)
            assert mref.digest_by_id(perm, a[perm]) == by_id  # device order is any order
            if n <= 65:
                assert mref.digest_by_id_ints(perm.tolist(), a[perm].tolist()) == by_id
            # the digest of the whole is the plain sum of the pieces' (mod 2^64)
            cut = n // 3
            parts = (perm[:cut], perm[cut:])
            assert sum(mref.digest_by_id(p, a[p]) for p in parts) & ref.MASK == by_id


def test_digest_by_id_hand_cases():
    M, L, K = ref.MUL, ref.LEN, ref.MASK
    assert mref.digest_by_id_ints([], []) == 0 == mref.digest_by_id([], np.zeros((0, 1), np.uint32))
    assert mref.digest_by_id_ints([0], [[1]]) == (M + L) & K                                   # id 0, one word: index 0
    assert mref.digest_by_id_ints([5], [[1]]) == (((11 * M) & K) + L) & K                      # sparse: id 5 -> index 5, multiplier 11 M
    assert mref.digest_by_id_ints([5], [[1, 2]]) == (((21 * M) & K) + 2 * ((23 * M) & K) + 2 * L) & K  # k = 2: indices 10 and 11
    # sparse ids: as if the missing ids held zero words, but for the length term
    dense = ref.digest_ints([0, 0, 7, 0, 9])
    assert mref.digest_by_id_ints([2, 4], [[7], [9]]) == (dense - 3 * L) & K
    # equal ids share their multipliers: the words add up, and the order among them does not matter
    a = mref.digest_by_id_ints([3, 3], [[1], [2]])
    assert a == mref.digest_by_id_ints([3, 3], [[2], [1]]) == (3 * ((7 * M) & K) + 2 * L) & K
    assert a == mref.digest_by_id(np.array([3, 3]), np.array([[1], [2]], np.uint32))
    # the largest id a tile can hold, wrap-around included
    big = (1 << 31) - 1
    assert mref.digest_by_id_ints([big], [[0xFFFFFFFF, 1]]) == mref.digest_by_id(np.array([big]), np.array([[0xFFFFFFFF, 1]], np.uint32))


# ------------------------------------------------------------------------------------------------------ 2. the format driver
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the multi-state-format driver"
    exe = str(tmp_path_factory.mktemp("multi_state_format") / "multi_state_format_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "multi_state_format_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["valid", "corrupt_bytes", "corrupt_fields", "truncations", "sets", "params", "file"])
def test_format_validation(driver, check):
    """valid: well-formed parts (one part, a part of four, the empty run, 64 strips, a 64 x 1 grid) pass.  corrupt_bytes: every byte of the
    header, three damaged values each, is refused.  corrupt_fields: every field forged with the header's digest recomputed — counts that
    disagree, a layout no multi could have had, sections out of range / overlapping / misaligned / misplaced — is refused for the stated
    reason.  truncations: every shorter length.  sets: a missing or duplicated part index, parts whose scalars, params, layout or boundary
    digest differ, counts that do not add up.  params: one field differs — that field is named.  file: the solver's checkpoint file.
    The sanitizers stay clean (any report aborts the program)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) > 0


def test_format_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_multi_state_format.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


def test_driver_digest_equals_reference(driver):
    rng = np.random.default_rng(13)
    for n, k in ((0, 1), (1, 1), (1, 2), (7, 2), (100, 1), (50, 2)):
        ids = rng.integers(0, 1 << 31, n, dtype=np.uint64)
        ids[: n // 4] = ids[n // 2: n // 2 + n // 4]  # some equal ids
        w = rng.integers(0, 1 << 32, (n, k), dtype=np.uint64)
        args = ["%d:%s" % (i, ",".join("%x" % v for v in row)) for i, row in zip(ids, w)]
        rc, out, _ = driver("digest", k, *args)
        assert rc == 0 and int(out, 16) == mref.digest_by_id_ints(ids.tolist(), w.tolist()) == mref.digest_by_id(ids, w.astype(np.uint32))
    rc, out, _ = driver("digest", 1, *["%d:%x" % (i, v) for i, v in enumerate((3, 1, 4, 1, 5))])
    assert int(out, 16) == ref.digest_ints([3, 1, 4, 1, 5])


def test_reference_parser_reads_the_drivers_header(driver):
    """The parser of tests/multi_state_reference.py (written from the layout's text) and the C++ header agree on a header the C++ built."""
    rc, out, _ = driver("header")
    assert rc == 0
    head = bytes.fromhex(out.strip())
    assert len(head) == mref.HEADER_BYTES
    (total,) = np.frombuffer(head, "<u8", 1, 16)
    p = mref.parse_part(head + bytes(int(total) - len(head)))
    assert (p["n_total"], p["n_part"], p["b"], p["part"], p["n_parts"]) == (1001, 1001, 33, 0, 1)
    assert (p["num_density_iters"], p["num_divergence_iters"], p["last_div_iters"], p["last_div_warm"], p["steps"]) == (3, 2, 2, 1, 40)
    assert (p["tiling_invariant"], p["world"], p["axis"], p["nx"], p["ny"]) == (1, 4, -1, 2, 2)
    assert p["cuts"] == [0, 40, 65536, 0, 17, 65536, 0, 23, 65536]
    assert p["params"]["max_density_iterations"] == 200 and p["params"]["smoothing_length"] == np.float32(0.02)
    assert [p["table"][s][2] for s in mref.SECTIONS] == [0x1111111111111111 * (k + 1) for k in range(8)]
    assert p["kappa"].shape == (1001,) and p["positions"].shape == (1001, 2) and p["boundary"].shape == (33, 2)


# ------------------------------------------------------------------------------------------------------ 3. exports, bindings, NULL
def test_header_declares_and_library_exports(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES
        # as many parameters in the binding as in the declaration
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(",") if a.strip()]), name
    assert re.search(r"#define\s+SPHX_MULTI_STATE_SECTIONS\s+8\b", src) and len(_lib.MULTI_STATE_SECTIONS) == 8 == len(mref.SECTIONS)
    assert re.search(r"SPHX_TILE_STATE_ZERO_KAPPA\s*=\s*1u", src) and re.search(r"SPHX_TILE_STATE_ZERO_STIFFNESS\s*=\s*2u", src)
    assert (_lib.TILE_STATE_ZERO_KAPPA, _lib.TILE_STATE_ZERO_STIFFNESS) == (1, 2)
    assert "SPHX_ABI_VERSION 5" in src and sphx_lib.sphx_abi_version() == 5
    # the single-context section still says what it does not do, and now points at this one
    assert re.search(r"sphx_multi_\* has NO counterpart", full) and "checkpoint of a tiled run" in full
    for cls, names in ((MultiSolver, ("save_state", "load_state", "state_digest", "save_state_file", "load_state_file")),
                       (y.DFSPHMultiSolver, ("checkpoint", "restore"))):
        for nm in names:
            assert callable(getattr(cls, nm))


def test_null_arguments_are_refused(sphx_lib, tmp_path):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    n = C.c_uint64(123)
    buf = (C.c_uint8 * 2048)()
    out = (C.c_uint64 * 8)()
    path = str(tmp_path / "never_written.bin").encode()
    ptrs, sizes = (C.c_void_p * 1)(C.addressof(buf)), (C.c_uint64 * 1)(2048)
    assert L.sphx_multi_state_size(None, C.byref(n)) == bad and L.sphx_multi_state_size(None, None) == bad
    assert L.sphx_multi_state_save(None, buf, 2048, 0, C.byref(n)) == bad and L.sphx_multi_state_save(None, None, 0, 0, None) == bad
    assert L.sphx_multi_state_load(None, ptrs, sizes, 1, 0) == bad and L.sphx_multi_state_load(None, None, None, 0, 0) == bad
    assert L.sphx_multi_state_digest(None, out) == bad and L.sphx_multi_state_digest(None, None) == bad
    assert L.sphx_multi_state_save_file(None, path) == bad and L.sphx_multi_state_save_file(None, None) == bad
    assert L.sphx_multi_state_load_file(None, path) == bad and L.sphx_multi_state_load_file(None, None) == bad
    assert L.sphx_tile_state_pack(None, 0, None, None, None) == bad and L.sphx_tile_state_fetch(None, None, None) == bad
    assert L.sphx_tile_upload_state(None, None, None, None, None, None, 0) == bad
    assert L.sphx_get_tiling_invariant(None) == 0
    assert not os.path.exists(path.decode())
    w, t = y.FluidParticleWorld(), y.TimeManager()
    for args in ((None, w.h, t.h, path), (None, None, None, None)):
        assert L.sphx_solver_multi_checkpoint(*args) == bad and L.sphx_solver_multi_restore(*args) == bad
