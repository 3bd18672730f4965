"""CPU oracle of the XTC encoder (include/dcv.h, dcv_xtc_encode / dcv_xtc_pack): the quantisation in NumPy float32, the
policy that chooses the *script* of a frame, and ``encode``, which hands both to the structural encoder of
tests/xtc_oracle.py (``encode_frame``: integers plus a script give the legal stream that says exactly that).

This file is the definition where the contract in include/dcv.h could be read two ways:

* a run always begins with the water swap: when ``q[p]`` is not within reach of ``q[p + 1]`` the group is the single atom
  ``p`` (r = 0) and nothing behind it is tried;
* differences and their absolute sums are exact integers (64 bits on the device), never wrapped;
* a frame is marked NONFINITE (1) when any coordinate is not finite, otherwise RANGE (2) when any ``lf`` fails
  ``|lf| < 2147483520``; a raw frame (at most 9 atoms) is only checked for non-finite coordinates;
* the descriptor of a marked frame keeps ``offset``, ``precision`` and ``raw`` and has zeros elsewhere; the descriptor of
  a raw frame is the one ``trajectory.index_xtc`` gives (nbytes, smallidx, precision, minint, maxint all zero);
* the *slot* of a frame holds the payload padded with zeros to a multiple of 4 (the floats of a raw frame); the nine
  fields in front of the payload are in the descriptor and are written by the pack step."""
from __future__ import annotations

import struct
from typing import List, Optional, Tuple

import numpy as np

from tests import xtc_oracle as xo

OK, NONFINITE, RANGE = 0, 1, 2
LIMIT = np.float32(2147483520.0)   # the largest float32 below 2^31
FRAME_DTYPE = np.dtype([("offset", "<i8"), ("nbytes", "<i4"), ("smallidx", "<i4"), ("precision", "<f4"), ("raw", "<i4"),
                        ("minint", "<i4", (3,)), ("maxint", "<i4", (3,))], align=True)


def slot_bytes(natoms: int) -> int:
    """ceil(102 natoms / 8) rounded up to 4: no frame needs more (96 bits of a full-range atom, 6 of flag and run)."""
    return ((102 * natoms + 7) // 8 + 3) // 4 * 4


def scaled(xyz, inv_scale: float = 0.1) -> np.ndarray:
    return np.asarray(xyz, dtype=np.float32) * np.float32(inv_scale)


def quantise(xyz, precision: float = 1000.0, inv_scale: float = 0.1) -> Tuple[np.ndarray, int]:
    """(int64 integers, status) of one frame or a batch: lf = (x * inv_scale) * precision and
    i = trunc(lf + copysign(0.5, lf)), every operation in float32.  Integers of a marked array are zero."""
    x = np.asarray(xyz, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        lf = (x * np.float32(inv_scale)) * np.float32(precision)
        if not np.isfinite(x).all():
            return np.zeros(x.shape, dtype=np.int64), NONFINITE
        if not (np.abs(lf) < LIMIT).all():
            return np.zeros(x.shape, dtype=np.int64), RANGE
        r = np.trunc(lf + np.copysign(np.float32(0.5), lf))
    assert r.dtype == np.float32
    return r.astype(np.int64), OK


def _reach(a, b, smallnum: int, sizesmall: int) -> bool:
    return all(0 <= int(a[c]) - int(b[c]) + smallnum < sizesmall for c in range(3))


def policy(q: np.ndarray) -> Tuple[xo.Script, int]:
    """(script, starting smallidx) of the integers q [natoms, 3]."""
    q = np.asarray(q, dtype=np.int64)
    N = len(q)
    mindiff = min(int(np.abs(q[a] - q[a - 1]).sum()) for a in range(1, N))
    s = xo.FIRSTIDX
    while s < xo.LASTIDX and xo.MAGIC[s] < mindiff:
        s += 1
    s0, script, run, p = s, [], 0, 0
    while p < N:
        smallnum, sizesmall = xo.MAGIC[s] // 2, xo.MAGIC[s]
        r, diffs = 0, []
        if p + 1 < N and _reach(q[p], q[p + 1], smallnum, sizesmall):
            r, prev = 1, q[p]
            diffs.append(q[p] - q[p + 1])
            while r < 8 and p + 1 + r < N and _reach(q[p + 1 + r], prev, smallnum, sizesmall):
                diffs.append(q[p + 1 + r] - prev)
                prev = q[p + 1 + r]
                r += 1
        if r == 0:
            step = 1 if s < xo.LASTIDX else 0
        else:
            smaller = xo.MAGIC[max(xo.FIRSTIDX, s - 1)] // 2
            step = -1 if s > xo.FIRSTIDX and all(abs(int(v)) < smaller for d in diffs for v in d) else 0
        reuse = 3 * r == run and step == 0
        if not reuse:
            run = 3 * r
        script.append((r, step, reuse))
        s += step
        p += 1 + r
    return script, s0


def encode_frame(x, precision: float = 1000.0, inv_scale: float = 0.1) -> Tuple[bytes, dict, int]:
    """(body, descriptor fields, status) of one frame x [natoms, 3] (Angstrom): body = the nine fields and the padded
    payload (the floats for a raw frame), empty for a marked frame."""
    x = np.asarray(x, dtype=np.float32)
    natoms = len(x)
    d = dict(nbytes=0, smallidx=0, precision=np.float32(0.0 if natoms <= 9 else precision), raw=int(natoms <= 9), minint=(0, 0, 0), maxint=(0, 0, 0))
    if natoms <= 9:
        if not np.isfinite(x).all():
            return b"", d, NONFINITE
        return scaled(x, inv_scale).astype(">f4").tobytes(), d, OK
    q, status = quantise(x, precision, inv_scale)
    if status:
        return b"", d, status
    script, s0 = policy(q)
    frame = xo.encode_frame(q, script, s0, precision)
    body = frame[56:]
    nbytes = struct.unpack_from(">i", body, 32)[0]
    d.update(nbytes=nbytes, smallidx=s0, minint=tuple(int(v) for v in q.min(0)), maxint=tuple(int(v) for v in q.max(0)))
    return body, d, OK


def encode(xyz, precision: float = 1000.0, inv_scale: float = 0.1) -> Tuple[List[bytes], np.ndarray, np.ndarray]:
    """(bodies, descriptors [n] of FRAME_DTYPE with ``offset`` = f * slot_bytes, status [n] int32) of xyz [n, natoms, 3]."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n, natoms = xyz.shape[:2]
    desc = np.zeros(n, dtype=FRAME_DTYPE)
    status = np.zeros(n, dtype=np.int32)
    bodies = []
    for f in range(n):
        body, d, status[f] = encode_frame(xyz[f], precision, inv_scale)
        bodies.append(body)
        desc[f]["offset"] = f * slot_bytes(natoms)
        for k, v in d.items():
            desc[f][k] = v
    return bodies, desc, status


def slot_payload(body: bytes, natoms: int) -> bytes:
    """What the frame's slot holds: the body without its nine fields (a raw body as it is)."""
    return body if natoms <= 9 else body[36:]


def file_image(bodies: List[bytes], status, natoms: int, step=None, time=None, box=None, frames=None) -> bytes:
    """The file the pack step writes: header and body of every frame that is not marked.  Defaults as the writer's: step
    is the source frame index, time that index as float32, the box zeros."""
    n = len(bodies)
    frames = np.arange(n) if frames is None else np.asarray(frames)
    step = frames if step is None else step
    time = np.asarray(frames, dtype=np.float32) if time is None else time
    out = []
    for f in range(n):
        if status[f]:
            continue
        b = np.zeros(9) if box is None else np.asarray(box[f]).ravel()
        out.append(xo.header(natoms, int(step[f]), float(time[f]), b) + bodies[f])
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ synthetic inputs
CASES = ("chain", "water", "scattered", "tight", "identical", "negative", "bigsize", "bits72", "run_at_end", "precision100")


def case_precision(name: str) -> float:
    return {"bigsize": 1.0e5, "precision100": 100.0}.get(name, 1000.0)


def synthetic(name: str, n_frames: int, natoms: int, seed: int = 0) -> np.ndarray:
    """xyz [n_frames, natoms, 3] float32 (Angstrom) of a case; every frame from its own seed."""
    out = np.zeros((n_frames, natoms, 3), dtype=np.float32)
    for f in range(n_frames):
        rng = np.random.Generator(np.random.PCG64([seed, CASES.index(name), natoms, f]))
        if name in ("chain", "negative", "precision100", "run_at_end"):
            x = np.cumsum(rng.normal(0.0, 2.2, size=(natoms, 3)), axis=0) + rng.uniform(-20, 60, size=3)
            if name == "negative":
                x -= 400.0
            if name == "run_at_end":      # the last atoms sit on top of each other: the last group is a run that ends the frame
                x[-3:] = x[-4] + rng.normal(0.0, 0.01, size=(3, 3))
        elif name == "water":             # O, H, H triplets: 1 Angstrom bonds, molecules far apart
            x = np.repeat(rng.uniform(0.0, 40.0, size=((natoms + 2) // 3, 3)), 3, axis=0)[:natoms]
            x = x + rng.normal(0.0, 0.6, size=(natoms, 3)) * (np.arange(natoms) % 3 != 0)[:, None]
        elif name == "scattered":
            x = rng.uniform(-300.0, 300.0, size=(natoms, 3))
        elif name == "tight":
            x = rng.uniform(-50, 50, size=3) + rng.normal(0.0, 0.004 * (1 + f % 5), size=(natoms, 3))
        elif name == "identical":
            x = np.tile(rng.uniform(-50, 50, size=3), (natoms, 1))
        elif name == "bigsize":           # precision 1e5: extents over 0xffffff integers, bitsize = 0
            x = rng.uniform(-2000.0, 2000.0, size=(natoms, 3))
            x[1] = x[0] + rng.normal(0.0, 0.001, size=3)
        elif name == "bits72":            # sizeint just below 2^24 in every component: a 72-bit pack3
            x = rng.uniform(-83880.0, 83880.0, size=(natoms, 3))
            x[0], x[1] = -83886.0 + rng.uniform(0, 0.5, size=3), 83885.5 + rng.uniform(0, 0.5, size=3)
        else:
            raise KeyError(name)
        out[f] = x.astype(np.float32)
    return out
