"""IC_Angle's static weight words (k_describe_body.hpp: kWeightsPb / kWeightsPlain, the arrays the description kernels' __constant__ tables
are initialised from and a workgroup copies into LDS) against a restatement written from the reference: umax by the constructor's formula
(ORBextractor.cc:459-474), then the two layout rules of the staged tile rows.  CPU only: orbx_debug_describe_tables copies the host's arrays."""
import math
import os
import re

import numpy as np

import extractorb_amd as X

HALF_PATCH = 15      # HALF_PATCH_SIZE, ORBextractor.cc:71
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbx.h")


def reference_umax():
    """ORBextractor.cc:459-474 (cvFloor / cvCeil / cvRound: floor, ceil, round half to even; sqrt(2.f) is a binary32 constant)"""
    umax = [0] * (HALF_PATCH + 2)
    r2 = float(np.sqrt(np.float32(2.0)))
    vmax = math.floor(HALF_PATCH * r2 / 2 + 1)
    vmin = math.ceil(HALF_PATCH * r2 / 2)
    hp2 = float(HALF_PATCH * HALF_PATCH)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(hp2 - v * v)))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:HALF_PATCH + 1]


def restated(words, u_of_byte):
    """[2][16][words] weight words: byte b of dword j of row |v| = a is u + 16 (plane 0) or 1 (plane 1) where u = u_of_byte(4 j + b) lies in the
    disc's row, 0 elsewhere"""
    umax = reference_umax()
    t = np.zeros((2, 16, words), np.uint32)
    for which in range(2):
        for a in range(16):
            for j in range(words):
                for b in range(4):
                    u = u_of_byte(4 * j + b)
                    if abs(u) <= HALF_PATCH and abs(u) <= umax[a]:
                        t[which, a, j] |= np.uint32((1 if which else u + 16) << (8 * b))
    return t


def test_umax_is_the_table_the_library_computes():
    assert reference_umax() == X.compute_tables()["umax"].tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_static_weight_words_equal_the_restatement():
    pb, plain = X.describe_tables()
    assert pb.shape == (2, 16, 12) and plain.shape == (2, 16, 8)
    want_pb = restated(12, lambda t: t - 22)          # patch-blur form: byte t of the re-aligned 44-byte tile row <-> u = t - 22, |u| <= 15
    want_plain = restated(8, lambda k: k - 15)        # plain form: byte k from the patch's first column on <-> u = k - 15
    for got, want, name in ((pb, want_pb, "PB"), (plain, want_plain, "plain")):
        for which in range(2):
            for a in range(16):
                for j in range(got.shape[2]):
                    for b in range(4):
                        g, w = (int(got[which, a, j]) >> (8 * b)) & 255, (int(want[which, a, j]) >> (8 * b)) & 255
                        assert g == w, "%s plane %d row %d dword %d byte %d: %d, want %d" % (name, which, a, j, b, g, w)
    # what the layout rules imply: a row of the disc holds 2 umax + 1 ones, its u + 16 weights sum to 16 x that (the u cancel)
    umax = reference_umax()
    for t in (pb, plain):
        by = t.view(np.uint8).reshape(2, 16, -1).astype(np.int64)
        assert by[1].sum(axis=1).tolist() == [2 * u + 1 for u in umax]
        assert by[0].sum(axis=1).tolist() == [16 * (2 * u + 1) for u in umax]


def test_null_pointers_are_refused():
    bad_argument = int(re.search(r"ORBX_ERR_BAD_ARGUMENT\s*=\s*(-?\d+)", open(HEADER).read()).group(1))      # the header's value
    L = X.load_library()
    buf = np.zeros(384, np.uint32)
    assert L.orbx_debug_describe_tables(None, buf.ctypes.data) == bad_argument and L.orbx_debug_describe_tables(buf.ctypes.data, None) == bad_argument
