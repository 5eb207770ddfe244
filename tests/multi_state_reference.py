"""Reference for the parts of a tiled checkpoint (sphx_multi_state_save, include/sphx.h): a numpy restatement of the id-keyed section
digest and a parser of one part.

The parser is written from the layout table in the comment at the top of yasph2d_amd/csrc/sphx_multi_state_format.hpp and from the contract
in include/sphx.h, not from the C++ below that comment: offsets and sizes are spelled out here a second time, so that a change of the
format that is not also a change of its documentation fails the tests."""
import struct

import numpy as np
from state_reference import LEN, MASK, MUL, PARAM_FIELDS, digest

SECTIONS = ("positions", "velocities", "particle_id", "density", "alpha", "kappa", "stiffness", "boundary")
WORDS = dict(positions=2, velocities=2, particle_id=1, density=1, alpha=1, kappa=1, stiffness=1)
HEADER_BYTES = 1176
PARAMS_AT, PARAMS_BYTES = 40, 80
TABLE_AT, DIGEST_AT, CUTS_AT, MAX_CUTS = 976, 1168, 192, 196


def digest_by_id_ints(ids, rows):
    """The formula of sphx.h in Python integers: rows[i] are the k words of the particle with id ids[i]."""
    s, words = 0, 0
    for pid, row in zip(ids, rows):
        k = len(row)
        for c, w in enumerate(row):
            s += int(w) * (((2 * (int(pid) * k + c) + 1) * MUL) & MASK)
        words += k
    return (s + words * LEN) & MASK


def digest_by_id(ids, a):
    """The same over an array whose first axis is the particle (read as little-endian 32-bit words); vectorised, uint64 wraps."""
    ids = np.asarray(ids).astype(np.uint64)
    n = len(ids)
    w = np.frombuffer(np.ascontiguousarray(a).tobytes(), "<u4").astype(np.uint64).reshape(n, -1) if n else np.zeros((0, 1), np.uint64)
    k = w.shape[1] if n else 1
    with np.errstate(over="ignore"):
        idx = ids[:, None] * np.uint64(k) + np.arange(k, dtype=np.uint64)[None, :]
        mult = (idx * np.uint64(2) + np.uint64(1)) * np.uint64(MUL)
        s = int((w * mult).sum(dtype=np.uint64)) if n else 0
    return (s + n * k * LEN) & MASK


def run_digests(ids, pos, vel, density, alpha, kappa, stiffness, boundary):
    """{section: digest} of a whole run from its arrays in ANY common particle order."""
    arrays = dict(positions=np.asarray(pos, "<f4"), velocities=np.asarray(vel, "<f4"), particle_id=np.asarray(ids, "<u4"), density=np.asarray(density, "<f4"),
                  alpha=np.asarray(alpha, "<f4"), kappa=np.asarray(kappa, "<f4"), stiffness=np.asarray(stiffness, "<f4"))
    out = {name: digest_by_id(ids, a) for name, a in arrays.items()}
    out["boundary"] = digest(np.asarray(boundary, "<f4"))
    return out


def parse_part(blob):
    """-> dict(total_bytes, params{...}, params_bytes, n_total, n_part, b, part, n_parts, num_density_iters, num_divergence_iters,
    last_div_iters, last_div_warm, steps, tiling_invariant, world, axis, nx, ny, cuts, table{name: (offset, bytes, digest)}, and one array
    per section).  Asserts everything the layout promises."""
    raw = bytes(blob)
    assert len(raw) >= HEADER_BYTES
    assert raw[0:8] == b"SPHXMULT"
    version, endian = struct.unpack_from("<II", raw, 8)
    assert version == 1 and endian == 0x01020304
    (total,) = struct.unpack_from("<Q", raw, 16)
    header_bytes, n_sections, params_bytes, zero = struct.unpack_from("<IIII", raw, 24)
    assert total == len(raw) and header_bytes == HEADER_BYTES and n_sections == len(SECTIONS) and params_bytes == PARAMS_BYTES and zero == 0
    out = dict(total_bytes=total, params={})
    for name, fmt, off in PARAM_FIELDS:
        v = struct.unpack_from("<" + fmt, raw, PARAMS_AT + off)
        out["params"][name] = v[0] if len(v) == 1 else v
    out["params_bytes"] = raw[PARAMS_AT:PARAMS_AT + PARAMS_BYTES]
    assert out["params"]["device"] == 0
    (out["n_total"],) = struct.unpack_from("<Q", raw, 120)
    out["n_part"], out["b"], out["part"], out["n_parts"] = struct.unpack_from("<IIII", raw, 128)
    out["num_density_iters"], out["num_divergence_iters"], out["last_div_iters"], out["last_div_warm"] = struct.unpack_from("<IIII", raw, 144)
    (out["steps"],) = struct.unpack_from("<Q", raw, 160)
    out["tiling_invariant"], out["world"] = struct.unpack_from("<II", raw, 168)
    out["axis"], out["nx"], out["ny"], n_cuts = struct.unpack_from("<iIII", raw, 176)
    cuts = struct.unpack_from("<%dI" % MAX_CUTS, raw, CUTS_AT)
    assert n_cuts <= MAX_CUTS and not any(cuts[n_cuts:])
    out["cuts"] = list(cuts[:n_cuts])
    assert CUTS_AT + 4 * MAX_CUTS == TABLE_AT and TABLE_AT + 24 * len(SECTIONS) == DIGEST_AT and DIGEST_AT + 8 == HEADER_BYTES
    n, b = out["n_part"], out["b"]
    assert out["part"] < out["n_parts"] and n <= out["n_total"]
    want_bytes = (8 * n, 8 * n, 4 * n, 4 * n, 4 * n, 4 * n, 4 * n, 8 * b)
    out["table"] = {}
    at = HEADER_BYTES
    covered = np.zeros(len(raw), bool)
    covered[:HEADER_BYTES] = True
    for k, name in enumerate(SECTIONS):
        off, nbytes, dig = struct.unpack_from("<QQQ", raw, TABLE_AT + 24 * k)
        assert off == at and off % 8 == 0 and nbytes == want_bytes[k], (name, off, at, nbytes, want_bytes[k])
        out["table"][name] = (off, nbytes, dig)
        covered[off:off + nbytes] = True
        at = (off + nbytes + 7) & ~7
    assert at == total
    (out["header_digest"],) = struct.unpack_from("<Q", raw, DIGEST_AT)
    assert out["header_digest"] == digest(raw[:DIGEST_AT])
    assert not np.frombuffer(raw, np.uint8)[~covered].any(), "padding bytes are not zero"

    def arr(name, dtype, shape):
        off, nbytes, _ = out["table"][name]
        return np.frombuffer(raw, dtype, count=nbytes // 4, offset=off).reshape(shape).copy()

    out["positions"] = arr("positions", "<f4", (n, 2))
    out["velocities"] = arr("velocities", "<f4", (n, 2))
    out["particle_id"] = arr("particle_id", "<u4", (n,))
    for name in ("density", "alpha", "kappa", "stiffness"):
        out[name] = arr(name, "<f4", (n,))
    out["boundary"] = arr("boundary", "<f4", (b, 2))
    return out
