"""Reference of the counter-based dropout bits (include/mgcn_hip.h (12)), written from the definition in numpy:
SplitMix64 keys, Philox4x32-10 words, keep iff word < T. Vectorised over whole [rows, cols] blocks; nothing here is ported from
csrc/dropout.hip, which the tests hold against it."""
import numpy as np

M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

SITE_FEATURE, SITE_HIDDEN = 0x1000, 0x1001


def sm(x):
    """One SplitMix64 step of a Python int, mod 2^64."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, step, site):
    return sm(sm(sm(seed & M64) ^ (step & M64)) ^ (site & M64))


def threshold(p):
    return min((1 << 32) - 1, int(np.floor((1.0 - float(p)) * 4294967296.0)))


def layer_site(li, which):
    """which: 0 = in, 1 = out, 2 = gcn_drop."""
    return 4 * li + which


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays that hold 32-bit words (broadcast against each other); returns four uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    lo32 = np.uint64(0xffffffff)
    s32 = np.uint64(32)
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + PHILOX_W0) & 0xffffffff, (k1 + PHILOX_W1) & 0xffffffff
        p0 = np.uint64(PHILOX_M0) * c0          # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(PHILOX_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & lo32, p1 >> s32, p1 & lo32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
    return c0, c1, c2, c3


def words(k, rows, cols, row0=0):
    """The 32-bit word of every element of a [rows, cols] block whose first row is the global row `row0`: uint64 [rows, cols]."""
    ncb = (cols + 3) // 4
    row = [(int(row0) + r) & M64 for r in range(rows)]
    r_lo = np.array([v & 0xffffffff for v in row], dtype=np.uint64).reshape(rows, 1)
    r_hi = np.array([v >> 32 for v in row], dtype=np.uint64).reshape(rows, 1)
    cb = np.arange(ncb, dtype=np.uint64).reshape(1, ncb)
    out = philox4x32_10(r_lo, r_hi, cb, np.zeros((1, 1), dtype=np.uint64), k & 0xffffffff, k >> 32)
    w = np.stack([np.broadcast_to(o, (rows, ncb)) for o in out], axis=2).reshape(rows, ncb * 4)
    return w[:, :cols]


def mask(k, rows, cols, row0, thr):
    """Keep bits as uint8 [rows, cols]."""
    return (words(k, rows, cols, row0) < np.uint64(thr)).astype(np.uint8)


def apply(x, k, row0, p):
    """Dropout of a float32 numpy block [rows, cols]: kept -> x * inv_keep (one f32 multiply), dropped -> +0.0."""
    inv_keep = np.float32(0.0) if p >= 1 else np.float32(1.0 / (1.0 - p))
    m = mask(k, x.shape[0], x.shape[1], row0, threshold(p)).astype(bool)
    with np.errstate(all='ignore'):
        return np.where(m, x.astype(np.float32) * inv_keep, np.float32(0.0)).astype(np.float32)
