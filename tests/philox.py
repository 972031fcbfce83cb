"""Philox4x32-10 (Salmon et al., Random123) and the executors' dropout mask in
numpy: a restatement of molclr_amd/csrc/dropout.h the tests compare the
kernels' masks against."""
import numpy as np

U = np.uint64
M0, M1 = U(0xD2511F53), U(0xCD9E8D57)
W0, W1 = U(0x9E3779B9), U(0xBB67AE85)
MASK32, S32 = U(0xFFFFFFFF), U(32)


def philox4x32_10(ctr, key):
    """ctr: four and key: two uint32 values or arrays (broadcastable, held in
    uint64); returns the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=U) & MASK32 for x in ctr]
    k0, k1 = (np.asarray(k, dtype=U) & MASK32 for k in key)
    for _ in range(10):
        p0 = M0 * c[0]  # 32 x 32 -> 64 bits: exact in uint64
        p1 = M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK32, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + W0) & MASK32
        k1 = (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def threshold(p: float) -> int:
    return int(p * 4294967296.0)


def dropout_mask(seed: int, call: int, layer: int, p: float, N: int, D: int) -> np.ndarray:
    """[N, D] uint8 keep-mask: counter (row, column / 4, layer, call_lo), key
    (seed_lo, seed_hi ^ call_hi); word j of a call decides column 4 c + j; kept
    iff word >= (uint32)(p * 2^32)."""
    seed &= 0xFFFFFFFFFFFFFFFF  # a signed 64-bit value's bit pattern
    call &= 0xFFFFFFFFFFFFFFFF
    rows = np.arange(N, dtype=U)[:, None]
    cols = np.arange(D // 4, dtype=U)[None, :]
    words = philox4x32_10((rows, cols, layer, call & 0xFFFFFFFF),
                          (seed & 0xFFFFFFFF, (seed >> 32) ^ (call >> 32)))
    words = np.stack([np.broadcast_to(w, (N, D // 4)) for w in words], axis=-1).reshape(N, D)
    return (words >= np.uint32(threshold(p))).astype(np.uint8)
