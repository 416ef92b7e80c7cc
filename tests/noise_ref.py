"""tests/noise_ref.py -- NumPy restatement of the device noise generator (racinglmpc_amd/csrc/lmpc_noise.hip.h), test infrastructure only.

Block function: Philox4x64-10 (only its four constants are shared with the device code); addressing: the words of (seed, stream, lap, t, car) are the block
function on the counter [t + 1, car, lap, stream] with the key [seed, 0] -- what numpy.random.Philox(counter=[t, car, lap, stream], key=[seed, 0]).random_raw(4)
returns (numpy_words below: NumPy's own generator, the independent side the restatement is checked against).  Transform: Box-Muller in float64 with NumPy's
log / sqrt / cos / sin."""
import numpy as np

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157            # round multipliers
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B            # Weyl constants the key is bumped by after every round
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(a):
    """uint64 array of Python integers / arrays taken modulo 2**64."""
    if isinstance(a, np.ndarray) and a.dtype == np.uint64:
        return a
    return np.array([int(v) % 2 ** 64 for v in np.ravel(np.asarray(a, dtype=object))], dtype=np.uint64).reshape(np.shape(a))


def _mulhilo(m, b):
    """(high, low) 64-bit halves of the 128-bit product of the constant m and the uint64 array b, from 32-bit limbs (no intermediate passes 2**64)."""
    m = np.uint64(m)
    a0, a1 = m & _LO, m >> _S32
    b0, b1 = b & _LO, b >> _S32
    t = a0 * b0
    k = t >> _S32
    t = a1 * b0 + k
    w1, w2 = t & _LO, t >> _S32
    t = a0 * b1 + w1
    k = t >> _S32
    return a1 * b1 + w2 + k, m * b


def philox4x64_10(c0, c1, c2, c3, k0, k1):
    """The block function on uint64 arrays of one shape: returns the four output words."""
    c0, c1, c2, c3, k0, k1 = [np.array(_u64(v), dtype=np.uint64, ndmin=1) for v in np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])]
    for _ in range(10):
        hi0, lo0 = _mulhilo(M0, c0)
        hi1, lo1 = _mulhilo(M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = k0 + np.uint64(W0); k1 = k1 + np.uint64(W1)
    return c0, c1, c2, c3


def words(seed, stream, lap, t, car):
    """(..., 4) uint64: the raw words of (seed, stream, lap, t, car); t and car may be arrays (broadcast against each other)."""
    t = _u64(t); car = _u64(car)
    w = philox4x64_10(t + np.uint64(1), car, _u64(lap), _u64(stream), _u64(seed), np.uint64(0))
    shape = np.broadcast(t, car).shape
    return np.stack([v.reshape(shape) for v in w], axis=-1)


def numpy_words(seed, stream, lap, t, car):
    """The same four words from NumPy's Philox bit generator (one (t, car) at a time)."""
    ctr = np.array([int(t) % 2 ** 64, int(car) % 2 ** 64, int(lap) % 2 ** 64, int(stream) % 2 ** 64], dtype=np.uint64)
    key = np.array([int(seed) % 2 ** 64, 0], dtype=np.uint64)
    return np.asarray(np.random.Philox(counter=ctr, key=key).random_raw(4), dtype=np.uint64)


def box_muller(wa, wb):
    """(za, zb) float64 of the uint64 word pair (wa, wb)."""
    u1 = ((wa >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53         # (0, 1]
    u2 = (wb >> np.uint64(11)).astype(np.float64) * 2.0 ** -53                          # [0, 1)
    r = np.sqrt(-2.0 * np.log(u1))
    a = (2.0 * np.pi) * u2
    return r * np.cos(a), r * np.sin(a)


def raw(seed, stream, lap, t0, T, car0, B):
    """(T, B, 4) uint64: what Context.noise_raw returns."""
    t = np.array([int(t0) + i for i in range(T)], dtype=object)[:, None]
    car = np.array([int(car0) + b for b in range(B)], dtype=object)[None, :]
    return words(seed, stream, lap, np.broadcast_to(t, (T, B)), np.broadcast_to(car, (T, B)))


def fill(seed, stream, lap, t0, T, car0, B, width=3):
    """(T, B, width) float64: what Context.noise_fill returns, to rounding of log / cos / sin."""
    w = raw(seed, stream, lap, t0, T, car0, B)
    z0, z1 = box_muller(w[..., 0], w[..., 1])
    z2, _ = box_muller(w[..., 2], w[..., 3])
    return np.ascontiguousarray(np.stack([z0, z1, z2][:width], axis=-1))
