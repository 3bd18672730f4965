"""Oracle of the MLP engine's dropout masks: Philox-4x32 restated in NumPy integer arithmetic from the published algorithm
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox.h), and on top of it
the keying include/dcv.h documents for dcv_mlp_desc.dropout.  Nothing here calls the engine: tests/test_dropout_oracle_cpu.py
pins the restatement to Random123's known-answer vectors, tests/test_dropout_bn_gpu.py pins the engine to the restatement."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # key increments (golden ratio, sqrt(3) - 1)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """counter: four words, key: two words (scalars or arrays that broadcast against each other), each taken mod 2^32.
    Returns the four output words as uint32 arrays of the broadcast shape."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _MASK for c in counter])
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0      # 32 x 32 -> 64 bit products: no overflow in uint64
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> _S32, p0 & _MASK
        hi1, lo1 = p1 >> _S32, p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & _MASK
        k1 = (k1 + np.uint64(W1)) & _MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    """keep iff draw >= thr: p * 2^32 in float64 from the float32 p, clamped to [1, 2^32 - 1], truncated"""
    t = float(np.float32(p)) * 4294967296.0
    return int(min(max(t, 1.0), 4294967295.0))


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def mask(seed, rank, layer, step, rows, width, p):
    """[rows, width] float32 multipliers (0 or 1 / (1 - p)) of the dropout behind Linear `layer` in training step `step` of an
    engine created with `seed`, on data-parallel rank `rank`: counter (row, col >> 2, layer, step), key (seed & 0xffffffff,
    (seed >> 32) + 0x9E3779B9 * rank), the four output words on columns 4 q .. 4 q + 3."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, ((seed >> 32) + W0 * int(rank)) & 0xFFFFFFFF)
    quads = (int(width) + 3) // 4
    r = np.arange(int(rows), dtype=np.uint64)[:, None]
    q = np.arange(quads, dtype=np.uint64)[None, :]
    words = philox4x32((r, q, int(layer) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF), key, rounds=7)
    draws = np.stack(words, axis=-1).reshape(int(rows), 4 * quads)[:, :int(width)]
    return np.where(draws >= np.uint32(threshold(p)), scale(p), np.float32(0.0)).astype(np.float32)
