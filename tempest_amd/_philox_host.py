"""Philox4x32-10 on the host for the few draws the host control flow needs itself (the offset of the systematic comb, the
multinomial split of draws across ranks), and, over NumPy arrays, for the host twin of a plugin's noise (trace.Noise).  Same stream
layout as csrc/common.h: counter (item, draw, tick, tag), key = seed."""

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1):
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniform_scalar(seed, tick, tag, item=0, draw=0):
    r = philox4x32(item & _MASK, draw & _MASK, tick & _MASK, tag & _MASK, seed & _MASK, (seed >> 32) & _MASK)
    k = ((r[0] >> 5) << 26) | (r[1] >> 6)
    return k * 2.0 ** -53


def _words(seed, item, draw, tick, tag):
    """The four 32-bit words of every (item, draw, tick, tag) -- broadcast uint64 arrays with at least one axis."""
    import numpy as np
    c = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype=np.uint64)) & np.uint64(_MASK) for v in (item, draw, tick, tag)))
    seed = int(seed)
    return philox4x32(*c, seed & _MASK, (seed >> 32) & _MASK)


def _k53(hi, lo):
    """53-bit integers from two 32-bit words: the 27 high bits of hi, the 26 high bits of lo."""
    import numpy as np
    return ((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))


def uniform_pair(seed, item, draw, tick, tag):
    """The two U[0, 1) doubles of every (item, draw, tick, tag): k 2^-53, the device's bits."""
    import numpy as np
    r = _words(seed, item, draw, tick, tag)
    return _k53(r[0], r[1]).astype(np.float64) * 2.0 ** -53, _k53(r[2], r[3]).astype(np.float64) * 2.0 ** -53


def normal_pair(seed, item, draw, tick, tag):
    """The two N(0, 1) doubles of every (item, draw, tick, tag) by Box-Muller on the device's two uniforms: r = sqrt(-2 log u1) with
    u1 = (k + 1) 2^-53 in (0, 1], angle 2 pi u2.  log, cos and sin are NumPy's: equal to the device's to rounding, not to the bit."""
    import numpy as np
    w = _words(seed, item, draw, tick, tag)
    u1 = (_k53(w[0], w[1]).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = _k53(w[2], w[3]).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    th = 2.0 * np.pi * u2
    return r * np.cos(th), r * np.sin(th)
