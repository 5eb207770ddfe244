"""Reference for the state blob of sphx_state_save (include/sphx.h): a numpy restatement of the section digest and a parser of the blob.

The parser is written from the layout table in the comment at the top of yasph2d_amd/csrc/sphx_state_format.hpp and from the contract in
include/sphx.h, not from the C++ below that comment: offsets and sizes are spelled out here a second time, so that a change of the
format that is not also a change of its documentation fails the tests."""
import struct

import numpy as np

MUL = 0x9E3779B97F4A7C15
LEN = 0xD6E8FEB86659FD93
MASK = (1 << 64) - 1

SECTIONS = ("positions", "velocities", "particle_id", "density", "alpha", "kappa", "stiffness", "accel", "boundary")
HEADER_BYTES = 392
PARAMS_AT, PARAMS_BYTES = 40, 80
# sphx_params (include/sphx.h), natural alignment: name, struct format, offset inside the struct
PARAM_FIELDS = (("smoothing_length", "f", 0), ("particle_mass", "f", 4), ("fluid_density", "f", 8), ("particle_radius", "f", 12),
                ("gravity", "2f", 16), ("grid_min", "2f", 24), ("xsph_epsilon", "f", 32), ("max_avg_density_error", "f", 36),
                ("max_density_iterations", "I", 40), ("max_divergence_error", "f", 44), ("max_divergence_iterations", "I", 48),
                ("fixed_density_iterations", "I", 52), ("fixed_divergence_iterations", "I", 56), ("device", "i", 60),
                ("list_span_limit", "I", 64), ("viscosity_model", "I", 68), ("fluid_viscosity", "f", 72), ("reserved", "I", 76))


def digest_ints(words):
    """The formula of sphx.h in Python integers: sum_i w[i] * ((2 i + 1) * MUL) + W * LEN, mod 2^64."""
    s = 0
    for i, w in enumerate(words):
        s += int(w) * (((2 * i + 1) * MUL) & MASK)
    return (s + len(words) * LEN) & MASK


def digest(a):
    """The same over the bytes of an array (or bytes), read as little-endian 32-bit words; vectorised (uint64 arithmetic wraps)."""
    raw = a if isinstance(a, (bytes, bytearray, memoryview)) else np.ascontiguousarray(a).tobytes()
    assert len(raw) % 4 == 0
    w = np.frombuffer(raw, "<u4").astype(np.uint64)
    n = len(w)
    with np.errstate(over="ignore"):
        k = (np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * np.uint64(MUL)
        s = int((w * k).sum(dtype=np.uint64)) if n else 0
    return (s + n * LEN) & MASK


def state_digests(pos, vel, ids, density, alpha, kappa, stiffness, accel, boundary):
    """{section: digest} over arrays as the blob stores them."""
    arrays = (np.asarray(pos, "<f4"), np.asarray(vel, "<f4"), np.asarray(ids, "<u4"), np.asarray(density, "<f4"), np.asarray(alpha, "<f4"),
              np.asarray(kappa, "<f4"), np.asarray(stiffness, "<f4"), np.asarray(accel, "<f4"), np.asarray(boundary, "<f4"))
    return {name: digest(a) for name, a in zip(SECTIONS, arrays)}


def parse_blob(blob):
    """-> dict(version, total_bytes, params{...}, n, b, cached_n, wcsph_n, ids_issued, num_density_iters, num_divergence_iters, set_changed,
    tiling_invariant, lists_current, sampling_allowed, table{name: (offset, bytes, digest)}, header_digest, and one array per section).
    Asserts everything the layout promises."""
    raw = bytes(np.asarray(blob, np.uint8).tobytes()) if not isinstance(blob, (bytes, bytearray)) else bytes(blob)
    assert len(raw) >= HEADER_BYTES
    assert raw[0:8] == b"SPHXSTAT"
    version, endian = struct.unpack_from("<II", raw, 8)
    assert version == 1 and endian == 0x01020304
    (total,) = struct.unpack_from("<Q", raw, 16)
    header_bytes, n_sections, params_bytes, zero = struct.unpack_from("<IIII", raw, 24)
    assert total == len(raw) and header_bytes == HEADER_BYTES and n_sections == len(SECTIONS) and params_bytes == PARAMS_BYTES and zero == 0
    out = dict(version=version, total_bytes=total, params={})
    for name, fmt, off in PARAM_FIELDS:
        v = struct.unpack_from("<" + fmt, raw, PARAMS_AT + off)
        out["params"][name] = v[0] if len(v) == 1 else v
    out["params_bytes"] = raw[PARAMS_AT:PARAMS_AT + PARAMS_BYTES]
    assert out["params"]["device"] == 0
    out["n"], out["b"], out["cached_n"], out["wcsph_n"] = struct.unpack_from("<IIII", raw, 120)
    (out["ids_issued"],) = struct.unpack_from("<Q", raw, 136)
    out["num_density_iters"], out["num_divergence_iters"] = struct.unpack_from("<II", raw, 144)
    out["set_changed"], out["tiling_invariant"], out["lists_current"], out["sampling_allowed"] = struct.unpack_from("<IIII", raw, 152)
    n, b, w = out["n"], out["b"], min(out["n"], out["cached_n"])
    want_bytes = (8 * n, 8 * n, 4 * n, 4 * n, 4 * w, 4 * w, 4 * w, 8 * out["wcsph_n"], 8 * b)
    out["table"] = {}
    at = HEADER_BYTES
    covered = np.zeros(len(raw), bool)
    covered[:HEADER_BYTES] = True
    for k, name in enumerate(SECTIONS):
        off, nbytes, dig = struct.unpack_from("<QQQ", raw, 168 + 24 * k)
        assert off == at and off % 8 == 0 and nbytes == want_bytes[k], (name, off, at, nbytes, want_bytes[k])
        out["table"][name] = (off, nbytes, dig)
        covered[off:off + nbytes] = True
        at = (off + nbytes + 7) & ~7
    assert at == total
    (out["header_digest"],) = struct.unpack_from("<Q", raw, 384)
    assert out["header_digest"] == digest(raw[:384])
    pad = np.frombuffer(raw, np.uint8)[~covered]
    assert not pad.any(), "padding bytes are not zero"

    def arr(name, dtype, shape):
        off, nbytes, _ = out["table"][name]
        return np.frombuffer(raw, dtype, count=nbytes // 4, offset=off).reshape(shape).copy()

    out["positions"] = arr("positions", "<f4", (n, 2))
    out["velocities"] = arr("velocities", "<f4", (n, 2))
    out["particle_id"] = arr("particle_id", "<u4", (n,))
    out["density"] = arr("density", "<f4", (n,))
    for name in ("alpha", "kappa", "stiffness"):
        out[name] = arr(name, "<f4", (w,))
    out["accel"] = arr("accel", "<f4", (out["wcsph_n"], 2))
    out["boundary"] = arr("boundary", "<f4", (b, 2))
    return out
