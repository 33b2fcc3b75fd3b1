"""Every LDS layout of a gamma table on the host (ph_lut_layout_of: lut_compress of ph_lut.cpp; no device): tests/luts.py makes a table
per layout, and the inputs the GPU tests of test_lut_layouts_gpu.py rely on are shown - by the oracle alone - to visit what they
claim to visit, so that an edit to an input that loses coverage fails on any machine."""
import numpy as np
import pytest

import luts
import packfmt
from phaneron_amd import capi


def seed_of(bias, m):
    return 0x1A7 + 16 * bias + m


@pytest.mark.parametrize("bias,m", luts.LAYOUTS)
def test_a_forced_table_lands_in_its_layout_and_decodes_exactly(bias, m):
    table = luts.layout_table(bias, m, seed_of(bias, m))
    assert np.isfinite(table).all() and 0.015 < table.min() and table.max() < 1.01
    layout, image = capi.lut_layout(table)
    assert layout is not None, "the (%d, %d) table must fit the LDS" % (bias, m)
    assert (layout["index_bias"], layout["shift"], layout["hole"]) == (bias, 23 - m, 4 << m), layout
    n = luts.n_blocks(bias, m)
    assert layout["lds_bytes"] == image.size == (4 << m) + 4 * ((n + 3) & ~3) + 131072 == luts.LDS_BYTES[(bias, m)] <= 160 * 1024
    assert layout["delta_off"] == layout["lds_bytes"] - 131072
    assert not image[: layout["hole"]].any()
    idx = np.arange(65536, dtype=np.uint32)
    assert np.array_equal(luts._lds_lookup(layout, image, idx), table.view(np.uint32))


def test_the_twelve_footprints():
    got = [[luts.lds_bytes(b, m) for m in luts.MS] for b in luts.BIASES]
    assert got == [[137744, 144400, 157712], [137232, 143376, 155664], [136720, 142352, 153616], [136208, 141328, 151568]]
    assert luts.LDS_BYTES[luts.LARGEST] == max(luts.LDS_BYTES.values()) and luts.LDS_BYTES[luts.SMALLEST] == min(luts.LDS_BYTES.values())


@pytest.mark.parametrize("bias", luts.BIASES)
def test_a_table_that_needs_m_10_is_refused(bias):
    """no m = 10 layout fits 160 KiB, and every coarser one puts two of the table's anchors into one block"""
    assert luts.lds_bytes(bias, 10) > 160 * 1024
    layout, image = capi.lut_layout(luts.layout_table(bias, 10, seed_of(bias, 10)))
    assert layout is None and image is None


# ---- the coverage the GPU tests rely on, by the oracle alone ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["std", "general"])
@pytest.mark.parametrize("fmt", packfmt.NAMES)
def test_reader_frames_visit_every_index(fmt, kind):
    """all 65536 indices in R, in G and in B (10-bit formats under both matrices, 8-bit planar ones under the general matrix);
    every input code in every plane where an 8-bit frame cannot do that"""
    why = luts.reader_coverage(fmt, kind)
    assert why is None, why


def test_the_v210_reader_frame_has_tails_and_the_two_matrices_take_the_two_paths():
    y, _, _ = luts.codes10("std")
    assert y.shape[1] % 6 == 4 and y.shape[1] % 48 != 0  # a tail quad: vectors with last = 0
    assert y.size < 2046 * 1024 // 8  # selected from the 2046 x 1024 frame that is the upper bound
    std, gen = luts.std_matrix().reshape(3, 4), luts.general_matrix().reshape(3, 4)
    is_std = lambda k: k[0][1] == 0 and k[2][2] == 0 and k[0][0] == k[1][0] == k[2][0]  # ycbcr_matrix_is_standard (ph_ldslut.h)
    assert is_std(std) and not is_std(gen)
    assert is_std(luts.std_matrix(8).reshape(3, 4)) and not is_std(luts.general_matrix(8).reshape(3, 4))


def test_the_writer_image_holds_every_index_every_tie_and_their_neighbours():
    why = luts.writer_coverage()
    assert why is None, why
    v = luts.writer_values()
    k = np.float32(65535.0)
    assert np.array_equal(np.rint(v[:65536] * k), np.arange(65536, dtype=np.float32))  # rint(t * 65535) == i for t = f32(i / 65535)
    x = v * k
    ties = v[(x - np.floor(x)) == 0.5]
    assert ties.size >= 65535 // 2, "only %d exact ties found" % ties.size
    for t in ties[:: max(1, ties.size // 97)]:  # both neighbours of a tie are in the list, and they are no ties
        for nb in (np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))):
            assert nb in v
    img = luts.writer_image()
    assert img.shape[1] % 6 == 4 and img.shape[0] % 2 == 0
    for ch in range(3):  # a different order per channel
        assert not np.array_equal(img[..., ch], img[..., (ch + 1) % 3], equal_nan=True)
    assert np.isnan(img[..., :3]).any() and np.isinf(img[..., :3]).any()  # the specials are there
