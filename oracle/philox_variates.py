"""CPU ORACLE -- test infrastructure only: a numpy mirror of the device's Philox variates.

The kernels draw every variate as a pure function of (seed, chain, sweep, tag, index)
(csrc/philox.hpp): Philox4x32-10 on the counter (index, tag, sweep, chain) with the key
(seed low word, seed high word); one draw gives two 53-bit uniforms, (words 0, 1) and (words
2, 3).  This module restates that layout and the maps the Metropolis blocks build on it
(csrc/gst_kernel.hpp mh_variates, csrc/gst_draws.h mh_variate), vectorised over any
broadcastable chain / sweep / index arrays, so a test can write the tape a Philox-mode launch
must be equivalent to.
"""
from __future__ import annotations

import numpy as np

TAG_WHITE, TAG_HYPER, TAG_BDRAW, TAG_THETA = 1 << 24, 2 << 24, 3 << 24, 4 << 24
TAG_Z, TAG_ALPHA, TAG_DF = 5 << 24, 6 << 24, 7 << 24
TAPE_WHITE, TAPE_HYPER = 0, 80            # _abi.TAPE_WHITE / TAPE_HYPER
N_WHITE_STEPS, N_HYPER_STEPS = 20, 10     # gibbs.py:121,88

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11): four counter words and two key words (each
    broadcastable, taken modulo 2^32) -> the four output words as uint64 arrays < 2^32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(v).astype(np.uint64) & _LO
                                           for v in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u01(lo, hi):
    """53-bit uniform in [0, 1) from two 32-bit words (philox.hpp u01)."""
    x = (np.asarray(hi, np.uint64) << _S32) | np.asarray(lo, np.uint64)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniform2(seed, chain, sweep, tag, index=0):
    """Rng::uniform2: the two uniforms of draw (index, tag) of global chain ``chain`` at
    global sweep ``sweep`` (both truncated to 32 bits, as make_rng does)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10(index, tag, sweep, chain, seed & 0xFFFFFFFF, seed >> 32)
    return u01(r[0], r[1]), u01(r[2], r[3])


def normal_from_uniforms(a, b):
    """The cosine half of Box-Muller (gst_draws.h normal_from)."""
    return np.sqrt(-2.0 * np.log1p(-a)) * np.cos(2.0 * np.pi * b)


def normal_from(seed, chain, sweep, tag, index=0):
    return normal_from_uniforms(*uniform2(seed, chain, sweep, tag, index))


def choice_index(u, nind):
    """k = min(int(u * nind), nind - 1): the position in the white / hyper index list."""
    return np.minimum((np.asarray(u) * nind).astype(np.int64), nind - 1)


def scale_class(us, cdf):
    """The jump-scale class of mh_variate: the number of cdf entries <= us, at most 4."""
    return np.minimum((np.asarray(cdf)[:, None] <= np.asarray(us).reshape(1, -1)).sum(axis=0),
                      4).reshape(np.shape(us))


def mh_tape(seed, chains, sweeps, wind, hind):
    """The Metropolis entries of the tape that a Philox-mode launch is equivalent to.

    ``chains`` [C] and ``sweeps`` [S] are *global* ids (chain0 + c, sweep0 + it).  Returns
    [C, S, 120]: per step the four entries (u_scale, parameter, jump normal, u_accept) at
    TAPE_WHITE + 4 step (20 steps, TAG_WHITE) and TAPE_HYPER + 4 step (10 steps, TAG_HYPER),
    from draws 3 step (both uniforms), 3 step + 1 (the normal) and 3 step + 2 (the index).
    """
    ch = np.asarray(chains, np.int64)[:, None, None]
    sw = np.asarray(sweeps, np.int64)[None, :, None]
    out = np.zeros((ch.shape[0], sw.shape[1], TAPE_HYPER + 4 * N_HYPER_STEPS))
    for tag, off, nsteps, ind in ((TAG_WHITE, TAPE_WHITE, N_WHITE_STEPS, wind),
                                  (TAG_HYPER, TAPE_HYPER, N_HYPER_STEPS, hind)):
        ind = np.asarray(ind, np.int64)
        if ind.size == 0:
            continue
        step = np.arange(nsteps)[None, None, :]
        us, ua = uniform2(seed, ch, sw, tag | (3 * step))
        xi = normal_from(seed, ch, sw, tag | (3 * step + 1))
        uidx, _ = uniform2(seed, ch, sw, tag | (3 * step + 2))
        e = np.stack([us, ind[choice_index(uidx, len(ind))].astype(np.float64), xi, ua], axis=-1)
        out[:, :, off:off + 4 * nsteps] = e.reshape(e.shape[0], e.shape[1], -1)
    return out
