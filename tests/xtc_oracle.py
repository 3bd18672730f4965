"""CPU oracle of the XTC reader (include/dcv.h, dcv_xtc_decode): a plain Python decoder of the format description, and a
*structural* encoder for synthetic streams.

The decoder restates the description field by field with Python integers (no limbs, no window) and keeps the guards of
the device decoder: zero bits behind ``nbytes`` mark the frame (status 1), a run that would pass ``natoms`` marks it and
stops (2), a ``smallidx`` that leaves [9, 72] marks it and stops (3), ``maxint < minint`` or a precision that is not
finite and positive mark it before anything is read (4).

The encoder is not GROMACS's: it takes the integer coordinates and a *script* -- per atom group the number of small
atoms that follow the full-range atom (0 to 8), the step of ``smallidx`` (-1, 0, +1) and whether the group reuses the
previous run length through ``flag = 0`` -- and emits the legal stream that says exactly that.  Any legal stream must
decode, whether or not GROMACS's heuristics would have chosen it.  ``decode(encode(ints)) == ints`` is its own check
(tests/test_xtc_cpu.py)."""
from __future__ import annotations

import functools
import math
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

FIRSTIDX, LASTIDX = 9, 72
MAGIC = [0] * 9 + [8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812, 1024, 1290, 1625, 2048, 2580,
                   3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072, 165140,
                   208063, 262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304,
                   5284491, 6658042, 8388607, 10568983, 13316085, 16777216]
assert len(MAGIC) == LASTIDX + 1
XTC_MAGIC = 1995
OK, SHORT, RUN, SMALLIDX, HEADER = 0, 1, 2, 3, 4


def _wrap(v: int) -> int:
    """A 32-bit two's complement sum, as the C code computes it."""
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


# ------------------------------------------------------------------------------------------------ file frames
def frames(data: bytes) -> List[Dict]:
    """The frames of an XTC file: header fields and where the payload (or the raw floats) lies."""
    out, pos = [], 0
    while pos < len(data):
        magic, natoms, step = struct.unpack_from(">iii", data, pos)
        assert magic == XTC_MAGIC, magic
        time = struct.unpack_from(">f", data, pos + 12)[0]
        box = struct.unpack_from(">9f", data, pos + 16)
        natoms2 = struct.unpack_from(">i", data, pos + 52)[0]
        assert natoms2 == natoms
        pos += 56
        fr = {"natoms": natoms, "step": step, "time": time, "box": box}
        if natoms <= 9:
            fr.update(raw=True, offset=pos)
            pos += 12 * natoms
        else:
            precision = struct.unpack_from(">f", data, pos)[0]
            ints = struct.unpack_from(">8i", data, pos + 4)
            fr.update(raw=False, precision=precision, minint=ints[0:3], maxint=ints[3:6], smallidx=ints[6], nbytes=ints[7], offset=pos + 36)
            pos += 36 + (ints[7] + 3) // 4 * 4
        out.append(fr)
    assert pos == len(data)
    return out


# ------------------------------------------------------------------------------------------------ decoder
class _Bits:
    def __init__(self, payload: bytes):
        self.value = int.from_bytes(payload, "big")
        self.total = 8 * len(payload)
        self.taken = 0

    def get(self, n: int) -> int:
        """n bits, most significant first; zero behind the payload."""
        lo = self.total - self.taken - n
        self.taken += n
        if n == 0:
            return 0
        v = self.value >> lo if lo >= 0 else self.value << -lo
        return v & ((1 << n) - 1)

    @property
    def overrun(self) -> bool:
        return self.taken > self.total


def _unpack3(bits: _Bits, nbits: int, sizes: Sequence[int]) -> List[int]:
    v = 0
    for k in range(nbits // 8):
        v |= bits.get(8) << (8 * k)
    if nbits % 8:
        v |= bits.get(nbits % 8) << (8 * (nbits // 8))
    n2 = v % sizes[2]
    v //= sizes[2]
    return [(v // sizes[1]) & 0xffffffff, v % sizes[1], n2]


def decode_payload(payload: bytes, natoms: int, precision: float, minint, maxint, smallidx: int) -> Tuple[np.ndarray, int]:
    """(ints [natoms, 3] int64 in output order, status).  Rows behind the first inconsistency stay at the int64 minimum."""
    out = np.full((natoms, 3), np.iinfo(np.int64).min, dtype=np.int64)
    if not (math.isfinite(precision) and precision > 0) or any(maxint[k] < minint[k] for k in range(3)):
        return out, HEADER
    sizeint = [maxint[k] - minint[k] + 1 for k in range(3)]
    if any(s >= 1 << 32 for s in sizeint):
        return out, HEADER
    if not FIRSTIDX <= smallidx <= LASTIDX:
        return out, SMALLIDX
    if any(s > 0xffffff for s in sizeint):
        bitsizeint = [min(s.bit_length(), 32) for s in sizeint]
        bitsize = 0
    else:
        bitsize = (sizeint[0] * sizeint[1] * sizeint[2]).bit_length()
    smaller = MAGIC[max(FIRSTIDX, smallidx - 1)] // 2
    smallnum = MAGIC[smallidx] // 2
    sizesmall = MAGIC[smallidx]
    bits = _Bits(payload)
    emitted = 0

    def emit(v):
        nonlocal emitted
        if emitted < natoms:
            out[emitted] = v
        emitted += 1

    run, i = 0, 0
    while i < natoms:
        if bitsize == 0:
            this = [bits.get(bitsizeint[k]) for k in range(3)]
        else:
            this = _unpack3(bits, bitsize, sizeint)
        i += 1
        this = [_wrap(this[k] + minint[k]) for k in range(3)]
        prev = this
        is_smaller = 0
        if bits.get(1):
            run = bits.get(5)
            is_smaller = run % 3
            run -= is_smaller
            is_smaller -= 1
        if run > 0:
            if i + run // 3 > natoms:
                return out, RUN
            for k in range(0, run, 3):
                this = _unpack3(bits, smallidx, [sizesmall] * 3)
                i += 1
                this = [_wrap(this[c] + prev[c] - smallnum) for c in range(3)]
                if k == 0:
                    this, prev = prev, this
                    emit(prev)
                else:
                    prev = this
                emit(this)
                if bits.overrun:
                    return out, SHORT
        else:
            emit(this)
        if bits.overrun:
            return out, SHORT
        smallidx += is_smaller
        if not FIRSTIDX <= smallidx <= LASTIDX:
            return out, (SMALLIDX if i < natoms else OK)
        if is_smaller < 0:
            smallnum = smaller
            smaller = MAGIC[smallidx - 1] // 2 if smallidx > FIRSTIDX else 0
        elif is_smaller > 0:
            smaller = smallnum
            smallnum = MAGIC[smallidx] // 2
        sizesmall = MAGIC[smallidx]
    return out, OK


def to_float(ints: np.ndarray, precision: float, scale: float = 10.0) -> np.ndarray:
    """x = (float)i * (1.0f / precision), then x * scale: two float32 multiplications."""
    inv = np.float32(1.0) / np.float32(precision)
    return (np.asarray(ints).astype(np.int32).astype(np.float32) * inv) * np.float32(scale)


def decode(data: bytes, scale: float = 10.0, descriptors: Optional[List[Dict]] = None):
    """(ints [n, A, 3] int64 -- None for raw files --, xyz [n, A, 3] float32, status [n] int32) of the frames of a file,
    or of ``descriptors`` (entries of :func:`frames`, possibly altered) read from ``data``.  The coordinates of a frame
    behind its first inconsistency are NaN."""
    frs = frames(data) if descriptors is None else descriptors
    natoms = frs[0]["natoms"]
    xyz = np.full((len(frs), natoms, 3), np.nan, dtype=np.float32)
    status = np.zeros(len(frs), dtype=np.int32)
    if frs[0]["raw"]:
        for f, fr in enumerate(frs):
            xyz[f] = np.frombuffer(data, dtype=">f4", count=3 * natoms, offset=fr["offset"]).astype(np.float32).reshape(natoms, 3) * np.float32(scale)
        return None, xyz, status
    ints = np.zeros((len(frs), natoms, 3), dtype=np.int64)
    for f, fr in enumerate(frs):
        payload = data[fr["offset"]:fr["offset"] + fr["nbytes"]]
        ints[f], status[f] = decode_payload(payload, natoms, fr["precision"], fr["minint"], fr["maxint"], fr["smallidx"])
        good = ints[f, :, 0] != np.iinfo(np.int64).min
        xyz[f, good] = to_float(ints[f, good], fr["precision"], scale)
    return ints, xyz, status


# ------------------------------------------------------------------------------------------------ encoder
class _Writer:
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v: int, n: int) -> None:
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.value = (self.value << n) | v
        self.n += n

    def bytes(self) -> bytes:
        nbytes = (self.n + 7) // 8
        return (self.value << (8 * nbytes - self.n)).to_bytes(nbytes, "big")


def _pack3(w: _Writer, nbits: int, sizes: Sequence[int], n: Sequence[int]) -> None:
    assert all(0 <= n[k] < sizes[k] for k in range(3)), (n, sizes)
    v = (n[0] * sizes[1] + n[1]) * sizes[2] + n[2]
    assert v < 1 << nbits
    for _ in range(nbits // 8):
        w.put(v & 0xff, 8)
        v >>= 8
    if nbits % 8:
        w.put(v, nbits % 8)


Script = List[Tuple[int, int, bool]]   # per atom group: small atoms behind the full-range atom, smallidx step, reuse the run by flag = 0


def header(natoms: int, step: int = 0, time: float = 0.0, box=None) -> bytes:
    box = np.eye(3).ravel() * 3.0 if box is None else box
    return struct.pack(">iiif9fi", XTC_MAGIC, natoms, step, time, *[float(b) for b in box], natoms)


def encode_frame(ints: np.ndarray, script: Script, smallidx: int, precision: float = 1000.0, minint=None, maxint=None, step: int = 0,
                 time: float = 0.0) -> bytes:
    """One compressed frame (header and padded payload) whose decode is ``ints`` ([natoms, 3], natoms > 9, output order)."""
    ints = np.asarray(ints, dtype=np.int64)
    natoms = len(ints)
    assert natoms > 9 and sum(1 + r for r, _, _ in script) == natoms
    minint = [int(v) for v in (ints.min(0) if minint is None else minint)]
    maxint = [int(v) for v in (ints.max(0) if maxint is None else maxint)]
    assert all(minint[k] <= ints[:, k].min() and ints[:, k].max() <= maxint[k] for k in range(3))
    assert all(-(1 << 31) <= minint[k] and maxint[k] < 1 << 31 for k in range(3))
    sizeint = [maxint[k] - minint[k] + 1 for k in range(3)]
    if any(s > 0xffffff for s in sizeint):
        bitsizeint, bitsize = [min(s.bit_length(), 32) for s in sizeint], 0
    else:
        bitsize = (sizeint[0] * sizeint[1] * sizeint[2]).bit_length()
    smallidx0 = smallidx
    w = _Writer()
    run, p = 0, 0
    for r, step_idx, reuse in script:
        assert 0 <= r <= 8 and step_idx in (-1, 0, 1) and FIRSTIDX <= smallidx <= LASTIDX
        big = ints[p + 1] if r else ints[p]   # the water swap: the full-range atom of a run is the SECOND atom written
        n = [int(big[k]) - minint[k] for k in range(3)]
        if bitsize == 0:
            for k in range(3):
                w.put(n[k], bitsizeint[k])
        else:
            _pack3(w, bitsize, sizeint, n)
        if reuse:
            assert run == 3 * r and step_idx == 0, "flag = 0 keeps the last run length and does not move smallidx"
            w.put(0, 1)
        else:
            w.put(1, 1)
            w.put(3 * r + step_idx + 1, 5)
            run = 3 * r
        sizesmall, smallnum = MAGIC[smallidx], MAGIC[smallidx] // 2
        prev = big
        for k in range(r):
            cur = ints[p] if k == 0 else ints[p + 1 + k]
            _pack3(w, smallidx, [sizesmall] * 3, [int(cur[c]) - int(prev[c]) + smallnum for c in range(3)])
            prev = cur
        p += 1 + r
        smallidx += step_idx
    payload = w.bytes()
    body = struct.pack(">f3i3iii", precision, *minint, *maxint, smallidx0, len(payload)) + payload + b"\0" * (-len(payload) % 4)
    return header(natoms, step, time) + body


def encode_raw_frame(xyz_nm: np.ndarray, step: int = 0, time: float = 0.0) -> bytes:
    """One frame of at most 9 atoms: the float32 coordinates (nm) as they are."""
    xyz_nm = np.asarray(xyz_nm, dtype=np.float32)
    assert 1 <= len(xyz_nm) <= 9
    return header(len(xyz_nm), step, time) + xyz_nm.astype(">f4").tobytes()


# ------------------------------------------------------------------------------------------------ synthetic cases
def make_ints(rng: np.random.Generator, script: Script, smallidx: int, lo, hi) -> np.ndarray:
    """Integer coordinates a script can encode: full-range atoms anywhere in [lo, hi] (per component), the small atoms of
    a run anywhere the current ``smallidx`` reaches from their predecessor, clipped to [lo, hi]."""
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.int64), 3), np.broadcast_to(np.asarray(hi, dtype=np.int64), 3)
    out = []
    for r, step_idx, _ in script:
        big = rng.integers(lo, hi, endpoint=True)
        smallnum, sizesmall = MAGIC[smallidx] // 2, MAGIC[smallidx]
        group, prev = [], big
        for k in range(r):
            cur = rng.integers(np.maximum(lo, prev - smallnum), np.minimum(hi, prev - smallnum + sizesmall - 1), endpoint=True)
            group.append(cur)
            prev = cur
        out.extend([group[0], big] + group[1:] if r else [big])
        smallidx += step_idx
    return np.asarray(out, dtype=np.int64)


def _fill(natoms: int, groups: Script) -> Script:
    """``groups`` followed by single atoms (flag = 1, run 0) up to ``natoms``."""
    used = sum(1 + r for r, _, _ in groups)
    assert used <= natoms
    return list(groups) + [(0, 0, False)] * (natoms - used)


def _case_scripts(name: str, rng: np.random.Generator) -> Tuple[int, Script, int]:
    """(natoms, script, first smallidx) of one frame of a synthetic case."""
    if name in ("atoms10", "negative", "precision100"):
        n = 10 if name == "atoms10" else 23
        script, left = [], n
        while left:
            r = int(rng.integers(0, min(8, left - 1), endpoint=True))
            idx = int(rng.integers(12, 40))
            script.append((r, 0, False))
            left -= 1 + r
        return n, script, idx
    if name == "runs":          # all eight run codes, each with the swap, in a random order between single atoms
        groups = [(int(r), 0, False) for r in rng.permutation(np.arange(1, 9))]
        for _ in range(3):
            groups.insert(int(rng.integers(0, len(groups) + 1)), (0, 0, False))
        return sum(1 + r for r, _, _ in groups), groups, int(rng.integers(14, 30))
    if name == "run_at_end":    # 30 atoms, the last group a run that ends exactly at the last atom
        r = int(rng.integers(1, 9))
        return 30, _fill(30 - 1 - r, [(2, 0, False)]) + [(r, 0, False)], int(rng.integers(14, 30))
    if name == "walk_down":     # smallidx down to 9 (where smaller = 0) and back up, with runs on the way
        start = int(rng.integers(12, 16))
        steps = [-1] * (start - FIRSTIDX) + [1] * (start - FIRSTIDX) + [-1, 1]
        groups = [(int(rng.integers(0, 3)), s, False) for s in steps]
        return 48, _fill(48, groups), start
    if name == "walk_up":       # smallidx up past 60, to the last index
        start = int(rng.integers(56, 60))
        groups = [(int(rng.integers(0, 3)), 1, False) for _ in range(LASTIDX - start)]
        return 60, _fill(60, groups), start
    if name == "flag0":         # flag = 0 behind a run (the run length persists) and behind single atoms
        r = int(rng.integers(1, 5))
        groups = [(0, 0, True), (0, 0, True), (r, 0, False), (r, 0, True), (r, 0, True), (0, 0, False), (0, 0, True), (r, 1, False), (r, 0, True)]
        return 40, _fill(40, groups), int(rng.integers(14, 30))
    if name in ("bigsize", "bits72"):
        n = 16
        script, left = [], n
        while left:
            r = int(rng.integers(0, min(3, left - 1), endpoint=True))
            script.append((r, 0, False))
            left -= 1 + r
        return n, script, int(rng.integers(20, 50))
    raise KeyError(name)


CASES = ("atoms10", "raw9", "raw1", "runs", "run_at_end", "walk_down", "walk_up", "flag0", "bigsize", "bits72", "negative", "precision100")
N_SYNTHETIC_FRAMES = 65   # two waves, one of them partial


@functools.lru_cache(maxsize=None)
def synthetic(name: str, seed: int = 0) -> Tuple[bytes, Optional[np.ndarray], float]:
    """(file bytes, ints [65, A, 3] or None for the raw cases, precision) of a synthetic case: 65 frames of unequal byte
    length whose ``nbytes`` are no multiples of 4 (a frame is drawn again until that holds).  Cached: callers share the
    result and leave it unchanged."""
    rng = np.random.Generator(np.random.PCG64([seed, CASES.index(name)]))
    if name.startswith("raw"):
        natoms = int(name[3:])
        xyz = rng.uniform(-5.0, 5.0, size=(N_SYNTHETIC_FRAMES, natoms, 3)).astype(np.float32)
        return b"".join(encode_raw_frame(x, step=500 * f, time=float(f)) for f, x in enumerate(xyz)), None, 0.0
    precision = 100.0 if name == "precision100" else 1000.0
    data, all_ints = [], []
    for f in range(N_SYNTHETIC_FRAMES):
        for _ in range(64):
            natoms, script, smallidx = _case_scripts(name, rng)
            minint = maxint = None
            if name == "bigsize":     # one component wider than 0xffffff, up to the whole int32 range: fields of up to 32 bits
                width = int(rng.integers(1 << 24, (1 << 32) - 1)) if f % 2 else (1 << 32) - 2
                lo = np.array([-(1 << 31) + 1 if f % 2 == 0 else int(rng.integers(-(1 << 31), (1 << 31) - width)), -3000, 100])
                hi = np.array([lo[0] + width - 1, 4000 + 37 * f, 100 + int(rng.integers(0, 1 << 20))])
            elif name == "bits72":    # three sizes just below 2^24: a 72-bit unpack3 for every full-range atom
                lo = rng.integers(-(1 << 23), 1 << 20, size=3)
                size = (1 << 24) - 1 - rng.integers(0, 3, size=3)
                hi = lo + size - 1
                minint, maxint = lo, hi
            elif name == "negative":
                lo = -rng.integers(20000, 30000, size=3)
                hi = lo + rng.integers(50, 9000, size=3)
            else:
                centre = rng.integers(-2000, 8000, size=3)
                half = rng.integers(30, 6000 + 90 * f, size=3)
                lo, hi = centre - half, centre + half
            ints = make_ints(rng, script, smallidx, lo, hi)
            frame = encode_frame(ints, script, smallidx, precision, minint, maxint, step=500 * f, time=float(f))
            nbytes = struct.unpack_from(">i", frame, 56 + 32)[0]
            if nbytes % 4:
                break
        else:
            raise AssertionError(f"{name}: no frame with nbytes % 4 != 0 in 64 draws")
        data.append(frame)
        all_ints.append(ints)
    natoms_all = {len(i) for i in all_ints}
    assert len(natoms_all) == 1, "the frames of a file have one atom count"
    return b"".join(data), np.asarray(all_ints), precision
