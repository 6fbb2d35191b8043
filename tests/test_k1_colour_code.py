"""K1's packed colour code (csrc/jbf_fast.hip, jbf_pk_kernel) restated in numpy.

Per tap the kernel forms -cd = 2 a.b - |a|^2 - |b|^2 (a = centre colour, b = tap colour, 8-bit BGR) as
    u   = float with the bits 0x4B000000 + a.b                        (v_dot4_u32_u8 with the accumulator input) = 2^23 + a.b
    w   = fma(u, 2, h_q),   h_q = -(2^24 - 2^18 + |b|^2)  staged in LDS   (one rounding)
    ncd = w + negC,         negC = -(2^18 + |a|^2)                       (one rounding)
Every step is evaluated here in binary64 and rounded to binary32 at the three rounding points (the staged constant, the
fma, the add); the test demands that no rounding changes a value (every intermediate is an exact float32) and that
ncd == -cd as an integer."""
import itertools

import numpy as np

K_MAGIC = 0x4B000000          # bits of the float 2^23
H_BIAS = 16515072.0           # 2^24 - 2^18
C_BIAS = 262144.0             # 2^18


def _exact32(x):
    """x (binary64) rounded to binary32; asserts that the rounding changed nothing"""
    r = np.asarray(x, np.float64).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), x), "an intermediate of the colour code is not an exact float32"
    return r


def colour_code(a, b):
    """a, b: [n, 3] integer colours -> ncd as float32 [n], by the kernel's sequence"""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    dot = (a * b).sum(axis=1)
    na = (a * a).sum(axis=1)
    nb = (b * b).sum(axis=1)
    assert dot.max() < (1 << 18) and nb.max() < (1 << 18)
    # the integer accumulate stays inside the mantissa field of 2^23: the bit pattern IS the float 2^23 + a.b
    u_bits = (K_MAGIC + dot).astype(np.uint32)
    u = u_bits.view(np.float32)
    assert np.array_equal(u.astype(np.float64), 8388608.0 + dot)
    h = _exact32(-(H_BIAS + nb.astype(np.float64)))                       # rounding point 1: the staged constant
    negc = _exact32(-(C_BIAS + na.astype(np.float64)))
    w = _exact32(u.astype(np.float64) * 2.0 + h.astype(np.float64))       # rounding point 2: the fma (product and sum exact in binary64)
    assert w.min() >= 67069.0 and w.max() <= 652294.0
    ncd = _exact32(w.astype(np.float64) + negc.astype(np.float64))        # rounding point 3: the add
    return ncd


def _check(a, b):
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    cd = ((a - b) ** 2).sum(axis=1)
    ncd = colour_code(a, b)
    assert np.array_equal(ncd.astype(np.float64), -cd.astype(np.float64))
    # +0, not -0, for equal colours (the sign would survive into the argument fma)
    assert not np.signbit(ncd[cd == 0]).any()


def test_corner_colours_against_each_other():
    corners = np.array(list(itertools.product((0, 255), repeat=3)), np.int64)
    a, b = zip(*itertools.product(corners, corners))
    a, b = np.array(a), np.array(b)
    assert ((a - b) ** 2).sum(axis=1).max() == 195075
    _check(a, b)


def test_all_parities_of_the_squared_norms():
    # |x|^2 mod 2 = (number of odd channels) mod 2; values next to the ends of the range in every parity combination
    vals = (0, 1, 2, 127, 128, 253, 254, 255)
    cols = np.array(list(itertools.product(vals, repeat=3)), np.int64)
    a, b = np.meshgrid(np.arange(len(cols)), np.arange(len(cols)), indexing="ij")
    a, b = cols[a.ravel()], cols[b.ravel()]
    par = set(zip(((a * a).sum(axis=1) & 1).tolist(), ((b * b).sum(axis=1) & 1).tolist()))
    assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}
    _check(a, b)


def test_random_colour_pairs():
    rng = np.random.default_rng(20240611)
    a = rng.integers(0, 256, (100000, 3))
    b = rng.integers(0, 256, (100000, 3))
    _check(a, b)
    near = np.clip(a + rng.integers(-1, 2, a.shape), 0, 255)              # +-1 neighbours: cd in 0..3
    _check(a, near)
