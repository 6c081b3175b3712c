"""NumPy restatement of the sampler noise generator (include/diffsal.h, "sampler noise"): Philox4x32-10 keyed by the seed and
counted by (quad, draw, clip id), then Box-Muller in fp64.  Test-side only: the package never imports it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # < 2^64: exact in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def bits(seed, ids, draw, per):
    """[N, per] uint32: element e of clip n is word e % 4 of the call with counter (e // 4, draw, id_lo, id_hi)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (per + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    out = np.empty((len(ids), nq * 4), dtype=np.uint32)
    for n, cid in enumerate(ids):
        cid = int(cid)
        assert cid >= 0
        r = philox4x32_10((q, np.uint64(draw), np.uint64(cid & MASK), np.uint64(cid >> 32)), (seed & MASK, seed >> 32))
        out[n] = np.stack(r, axis=1).reshape(-1)
    return out[:, :per]


def normals(seed, ids, draw, per, dtype=np.float64):
    """[N, per] normals in ``dtype`` arithmetic (fp64: the reference; fp32: what a plain fp32 evaluation of the formulas gives)."""
    nq = (per + 3) // 4
    r = bits(seed, ids, draw, nq * 4).reshape(len(ids), nq, 4)
    out = np.empty((len(ids), nq, 4), dtype=dtype)
    two_pi = dtype(2.0 * np.pi)
    for a in (0, 2):
        u1 = ((r[..., a] >> np.uint32(8)).astype(dtype) + dtype(1)) * dtype(2.0 ** -24)
        u2 = (r[..., a + 1] >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
        rad = np.sqrt(dtype(-2.0) * np.log(u1))
        out[..., a] = rad * np.cos(two_pi * u2)
        out[..., a + 1] = rad * np.sin(two_pi * u2)
    return out.reshape(len(ids), nq * 4)[:, :per]
