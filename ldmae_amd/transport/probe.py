"""The Rademacher probe of the Hutchinson trace estimator, restated on the host in numpy: Philox4x32-10 (Salmon, Moraes, Dror & Shaw, "Parallel
random numbers: as easy as 1, 2, 3", SC'11) exactly as csrc/ode.hip's ldmae_rademacher_f32 evaluates it.  A counter-based generator: the sign of
element i of the draw with (seed, counter) is a function of those three numbers alone, so the device draw can be checked bit for bit and a
likelihood can be reproduced from its seed.  `normal` is the standard-normal draw of the SDE sampler (ldmae_normal_f32) from the same generator, in f64."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                      # the two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                      # the key schedule: golden ratio, sqrt(3) - 1
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (uint32, broadcastable) -> the four output words [..., 4] of the 10-round bijection."""
    c = [np.asarray(ctr[..., j], dtype=np.uint64) for j in range(4)]
    k = [np.asarray(key[..., j], dtype=np.uint64) for j in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                 # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def rademacher(n, seed, counter):
    """The n signs (+-1.0, f32) ldmae_rademacher_f32 writes: key = (seed low, seed high), counter words = (counter low, counter high, v low, v high)
    with v = i // 4; element i takes word i % 4 of block v and is +1 when that word's top bit is set."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    v = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([np.full_like(v, counter & 0xFFFFFFFF), np.full_like(v, counter >> 32), v & _MASK, v >> np.uint64(32)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    words = philox4x32_10(ctr, key).reshape(-1)[:n]
    return np.where(words >> np.uint32(31), np.float32(1), np.float32(-1)).astype(np.float32)


def normal(n, seed, counter):
    """The n standard normals ldmae_normal_f32 draws, in f64 (the specification evaluated without rounding; the kernel's f32 evaluation differs by
    a few 1e-6).  Blocks, key and counter as `rademacher`; word w_j of a block gives u_j = ((w_j >> 9) + 0.5) 2^-23, strictly inside (0, 1);
    Box-Muller on (u0, u1) and (u2, u3): r = sqrt(-2 ln u_a), values r cos(2 pi u_b), r sin(2 pi u_b); element i takes value i % 4 of block
    i // 4.  |z| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    v = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([np.full_like(v, counter & 0xFFFFFFFF), np.full_like(v, counter >> 32), v & _MASK, v >> np.uint64(32)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    u = ((philox4x32_10(ctr, key) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r, a = np.sqrt(-2.0 * np.log(u[:, 0::2])), 2.0 * np.pi * u[:, 1::2]                 # [blocks, 2]: the pairs (u0, u1), (u2, u3)
    return np.stack([r * np.cos(a), r * np.sin(a)], -1).reshape(-1)[:n]
