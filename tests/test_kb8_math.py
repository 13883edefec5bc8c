"""extractorb_amd/csrc/k_camera_kb8.hpp compiled for the host (tests/cpp/kb8_host_check.cpp behind tests/cpp/host_shim) against the host libm:
atan2f32 on a structured set and on 10^8 pseudo-random pairs, the sine / cosine on every float of [-pi, pi], kb8Project against a plain
statement of KannalaBrandt8::project (reference src/CameraModels/KannalaBrandt8.cpp:28-44).  Equality of bytes, with one stated exception: two NaN results count as equal whatever their payload.  A NaN comes out only where a NaN
went in (atan2f's `x + y`, the propagation through the polynomials), and which operand's payload such an addition keeps is the hardware's
choice, not the algorithm's.
The header restates glibc 2.35's algorithms: on another glibc a mismatch skips with that reason, on 2.35 it fails."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "cpp"),
              "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"), "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"),
              "-I" + os.path.join(ROOT, "include")]


def build_kb8_host(directory):
    """tests/cpp/kb8_host_check.cpp as a shared library (also used by tests/test_last_frame_two_eyes.py)"""
    so = os.path.join(str(directory), "libkb8_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "kb8_host_check.cpp"), "-o", so])
    L = C.CDLL(so)
    L.kb8_check_atan2_structured.restype = C.c_long
    L.kb8_check_atan2_structured.argtypes = [C.POINTER(C.c_long)]
    L.kb8_check_atan2_random.restype = C.c_long
    L.kb8_check_atan2_random.argtypes = [C.c_long, C.c_ulonglong]
    L.kb8_check_sincos.restype = C.c_long
    L.kb8_check_sincos.argtypes = [C.c_int]
    L.kb8_check_project.restype = C.c_long
    L.kb8_check_project.argtypes = [C.c_long, C.c_ulonglong]
    L.kb8_project.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.kb8_project_libm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_kb8_host(tmp_path_factory.mktemp("kb8"))


def glibc_version():
    f = C.CDLL(None).gnu_get_libc_version
    f.restype = C.c_char_p
    return f().decode()


def settle(mismatches, what):
    if mismatches and glibc_version() != "2.35":
        pytest.skip("%d mismatches in %s against glibc %s: the header restates glibc 2.35" % (mismatches, what, glibc_version()))
    assert mismatches == 0, "%s: %d results differ from libm in their bytes (two NaN results, which only NaN inputs give, count as equal)" % (what, mismatches)


def test_atan2_on_the_structured_set(host):
    parts = (C.c_long * 3)()
    bad = host.kb8_check_atan2_structured(parts)
    assert parts[0] == 256 * 256 * 16 * 4 and parts[1] > 900 and parts[2] > 300      # exponent pairs, thresholds and k boundaries, specials
    settle(bad, "atan2f32 / atanf32, structured set")


def test_atan2_on_pseudo_random_pairs(host):
    settle(host.kb8_check_atan2_random(100_000_000, 1), "atan2f32, 10^8 pairs (half raw bit patterns, half a 2^-16 grid over +-128)")


@pytest.mark.parametrize("negative", [1, 0])
def test_sine_and_cosine_on_every_float_up_to_pi(host, negative):
    settle(host.kb8_check_sincos(negative), "kb8SinCos on every float of %s" % ("[-pi, -0]" if negative else "[0, pi]"))


def test_projection_against_the_plain_statement(host):
    settle(host.kb8_check_project(5_000_000, 1), "kb8Project")
