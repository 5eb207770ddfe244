"""Reference for following particles by id (include/sphx.h, "following particles by id"), in a few lines of numpy: slot_of from a
download by the "highest device index wins" rule, and the outputs and absent words built from it.  Everything is compared as raw
32-bit words."""
import numpy as np

ABSENT = np.uint32(0xFFFFFFFF)       # SPHX_TRACK_ABSENT
ABSENT_WORD = np.uint32(0x7FC00000)  # every float of an absent id


def slot_of(device_ids, ids):
    """-> uint32 [len(ids)]: the highest index j with device_ids[j] == ids[k], or ABSENT"""
    device_ids = np.asarray(device_ids, np.uint32)
    ids = np.asarray(ids, np.uint32).reshape(-1)
    last = {}
    for j, v in enumerate(device_ids.tolist()):
        last[v] = j  # (ascending j: the highest index stays)
    return np.array([last.get(v, int(ABSENT)) for v in ids.tolist()], np.uint32)


def gather(d, slot):
    """d = ctx.download() -> {slot, pos, vel, density} as uint32 words (shapes [m], [m, 2], [m, 2], [m])"""
    slot = np.asarray(slot, np.uint32)
    here = slot != ABSENT
    j = slot[here].astype(np.int64)
    out = {"slot": slot.copy()}
    for f, width in (("pos", 2), ("vel", 2), ("density", 1)):
        a = np.full((len(slot), width), ABSENT_WORD, np.uint32)
        a[here] = np.ascontiguousarray(d[f], np.float32).view(np.uint32).reshape(-1, width)[j]
        out[f] = a if width == 2 else a[:, 0]
    return out


def fetch(d, ids):
    """what sphx_track_fetch returns for the tracked ids, from a download"""
    return gather(d, slot_of(d["ids"], ids))


def by_id(d, first, count):
    """what sphx_download_by_id(first, count) returns -> (outputs, present)"""
    out = fetch(d, (np.arange(count, dtype=np.uint64) + np.uint64(first)).astype(np.uint32))
    return out, int((out["slot"] != ABSENT).sum())


def frame(d, ids):
    """one recorder frame: uint32 [m, 4] = x, y, vx, vy"""
    r = fetch(d, ids)
    return np.concatenate([r["pos"], r["vel"]], 1)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)
