"""The rBRIEF loop of k_describe rounds a rotated pattern coordinate v (|v| <= 18.385) with ONE binary32 addition, v + 1.5 * 2^23, and reads
rint(v) out of the sum's bits (k_describe_body.hpp) where it used rintf and a conversion.  Checked here with numpy's binary32 arithmetic
(IEEE, round to nearest even - the mode the kernels run in): the sum's bits are 0x4B400000 + rint(v) for EVERY float of [-20, 20], and the
address arithmetic built on those bits gives 40 r + q."""
import numpy as np

MAGIC = np.float32(12582912.0)          # 1.5 * 2^23
MAGIC_BITS = 0x4B400000
STRIDE = 40                             # kBlurStride


def _check(bits):
    v = bits.view(np.float32)
    got = (v + MAGIC).view(np.uint32).astype(np.int64) - MAGIC_BITS
    want = np.rint(v).astype(np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (v[bad[:4]], got[bad[:4]], want[bad[:4]])


def test_magic_constant():
    assert MAGIC.view(np.uint32) == MAGIC_BITS


def test_every_float_up_to_20_rounds_as_rintf():
    top = int(np.float32(20.0).view(np.uint32))          # the bit patterns 0 .. top are the floats 0 .. 20 in ascending order (zero and denormals included)
    chunk = 1 << 24
    for sign in (0, 0x80000000):
        for lo in range(0, top + 1, chunk):
            bits = np.arange(lo, min(lo + chunk, top + 1), dtype=np.uint32) | np.uint32(sign)
            _check(bits)


def test_ties_round_to_even():
    v = np.arange(-18.5, 19.0, 1.0, dtype=np.float32)
    got = (v + MAGIC).view(np.uint32).astype(np.int64) - MAGIC_BITS
    assert np.array_equal(got, np.rint(v).astype(np.int64))
    assert got[0] == -18 and got[-1] == 18 and 0 in got and np.all(got % 2 == 0)


def test_address_arithmetic_on_the_sums_bits():
    """v_mad_u32_u24 takes the low 24 bits of the row's sum, 0x400000 + r, times the stride, plus all 32 bits of the column's sum; the lane's base
    carries - (STRIDE * 0x400000 + MAGIC_BITS) modulo 2^32."""
    off = (STRIDE * 0x400000 + MAGIC_BITS) & 0xffffffff
    r, q = np.meshgrid(np.arange(-18, 19), np.arange(-18, 19), indexing="ij")
    rb = (r.astype(np.float32) + MAGIC).view(np.uint32).astype(np.int64)
    qb = (q.astype(np.float32) + MAGIC).view(np.uint32).astype(np.int64)
    base = 12345
    addr = ((base - off) + (rb & 0xffffff) * STRIDE + qb) & 0xffffffff
    assert np.array_equal(addr, base + STRIDE * r + q)
