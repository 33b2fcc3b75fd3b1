"""What the host computes once per launch for the fused v210 kernel (phaneron_amd/csrc/ph_kernels.h: fused_lut_k, fused_wg_magic,
fused_job_of) - host code of the product, no device: the lookup constants of a table bit for bit as the kernels' make_lut_k
(ph_ldslut.h) derives them, and the job division by reciprocal exact for every group size and workgroup a launch can have."""
import ctypes as C

import numpy as np
import pytest

import luts
from phaneron_amd import capi

MAGIC = np.float32(12582912.0)  # kRoundMagic, 1.5 * 2^23


def host_lut_k(lut):
    k5 = (C.c_uint32 * 5)()
    fn = capi.lib().ph_debug_fused_lut_k
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    lut = np.ascontiguousarray(lut, np.float32)
    n = fn(lut.ctypes.data_as(C.POINTER(C.c_float)), k5)
    return n, np.array(list(k5), np.uint32)


def make_lut_k(layout):
    """make_lut_k of ph_ldslut.h with numpy's float32 (IEEE, denormals kept): the LutView of ph_lut.cpp's lut_view, then the same
    operations in the same order; g_lds is at LDS address 0"""
    bias, a_scale = np.float32(layout["index_bias"]), np.float32(layout["a_scale"])
    delta_scale = np.array([2], np.uint32).view(np.float32)[0]                                             # 2^-148
    delta_base = np.array([layout["delta_off"] - 2 * layout["index_bias"]], np.uint32).view(np.float32)[0]  # a denormal
    lds0 = np.array([0], np.uint32).view(np.float32)[0]
    small = (delta_base + lds0) + bias * delta_scale
    b = small - MAGIC * delta_scale
    a_base = -((MAGIC - bias) * a_scale)
    f = np.array([a_scale, a_base, delta_scale, b], np.float32).view(np.uint32)
    return np.concatenate([f, np.array([layout["shift"] - 2], np.uint32)])


def check_table(lut, what):
    layout, _ = capi.lut_layout(lut)
    assert layout is not None, what
    n, got = host_lut_k(lut)
    assert n == layout["lds_bytes"], what
    want = make_lut_k(layout)
    assert np.array_equal(got, want), "%s: host LutK %r, make_lut_k %r" % (what, ["%08x" % x for x in got], ["%08x" % x for x in want])
    # and the record means what the lookup needs (exact in float64): the delta fma's bit pattern is delta_off + 2 * idx,
    # the anchor fma is (idx + bias) * a_scale
    f = got[:4].view(np.float32).astype(np.float64)
    idx = np.array([0, 1, 2, 255, 256, 32767, 32768, 65534, 65535], np.float64)
    y = idx + np.float64(MAGIC)
    assert np.array_equal((y * f[2] + f[3]) / 2.0 ** -149, layout["delta_off"] + 2 * idx), what
    assert np.array_equal(y * f[0] + f[1], (idx + layout["index_bias"]) * f[0]), what
    return layout


@pytest.mark.parametrize("layout", luts.LAYOUTS, ids=lambda l: "bias%d-m%d" % l)
def test_host_lut_k_of_every_layout(layout):
    """a table that only `layout` can hold (tests/luts.py): all twelve layouts lut_compress chooses among"""
    got = check_table(luts.layout_table(layout[0], layout[1], 0xA115 + 16 * layout[0] + layout[1]), "layout %r" % (layout,))
    assert (got["index_bias"], 23 - got["shift"], got["lds_bytes"]) == (layout[0], layout[1], luts.LDS_BYTES[layout])


@pytest.mark.parametrize("spec", ["709", "2020", "601-625", "601-525", "sRGB"])
def test_host_lut_k_of_the_colour_tables(spec):
    check_table(capi.gamma2linear_lut(spec), "gamma2linear " + spec)
    check_table(capi.linear2gamma_lut(spec), "linear2gamma " + spec)


def test_a_plain_table_has_no_record():
    n, _ = host_lut_k(np.random.default_rng(7).random(65536, dtype=np.float32))
    assert n == 0


def test_job_division_by_reciprocal_is_exact():
    """blockIdx.x / wg_per_job for every group size 1 .. 256 and every workgroup 0 .. 1023, from the library's own
    fused_wg_magic / fused_job_of"""
    fn = capi.lib().ph_debug_fused_job_of
    fn.restype, fn.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32]
    for d in range(1, 257):
        got = np.array([fn(d, b) for b in range(1024)], np.uint32)
        want = np.arange(1024, dtype=np.uint32) // np.uint32(d)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "wg_per_job %d: block %d gives %d, not %d" % (d, bad[0], got[bad[0]], want[bad[0]])
    # the bound ph_kernels.h states, at its edge: (block + 1) * d <= 2^30
    for d, b in ((1, 2 ** 30 - 1), (256, 2 ** 22 - 1), (85, (2 ** 30) // 85 - 1), (3, (2 ** 30) // 3 - 1)):
        assert fn(d, b) == b // d, (d, b)
