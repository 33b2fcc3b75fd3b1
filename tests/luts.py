"""Gamma tables that force each LDS layout (phaneron_amd/csrc/ph_lut.h, lut_compress in ph_lut.cpp), and inputs that make a kernel
visit every index of such a table.

A table is held in the LDS as anchors (one u32 per logarithmic block of the index) plus a u16 delta per entry; lut_compress takes
the smallest of the 12 layouts bias 16 / 32 / 64 / 128 x m = 7 / 8 / 9 in which every block's bit patterns span less than 65536.
The product's own colour tables land in three of them; layout_table() makes a table for any one.

Inputs are chosen and judged with the ORACLE alone: index_probe() as the table and an identity gamut make the oracle's reader
return the table index it used, so "this frame visits all 65536 entries" is a statement about the reference's arithmetic, never
about the code under test."""
import contextlib
import functools

import numpy as np

import fmt10
import frames
from oracle import orc

BIASES, MS = (16, 32, 64, 128), (7, 8, 9)
LAYOUTS = [(b, m) for b in BIASES for m in MS]
# hole + 4 * roundup4(n_blocks) + 131072, from ph_lut.cpp's arithmetic (test_lut_layouts_cpu.py derives them again)
LDS_BYTES = {(16, 7): 137744, (16, 8): 144400, (16, 9): 157712, (32, 7): 137232, (32, 8): 143376, (32, 9): 155664,
             (64, 7): 136720, (64, 8): 142352, (64, 9): 153616, (128, 7): 136208, (128, 8): 141328, (128, 9): 151568}
SMALLEST, LARGEST = (128, 7), (16, 9)   # 136208 and 157712 bytes
THREE = [(16, 9), (128, 7), (32, 8)]    # the layouts every single-table kernel is taken through
IDENTITY = np.eye(3, dtype=np.float32).reshape(-1)   # the gamut matrix under which a reader's f32 output IS the table entry


def blocks(bias, m):
    """blk(i) of ph_lut.h for i = 0 .. 65535: (bits(f32(i) + bias) >> (23 - m)) - blk(0)"""
    b = (np.arange(65536, dtype=np.float32) + np.float32(bias)).view(np.uint32) >> np.uint32(23 - m)
    return (b - b[0]).astype(np.int64)


def n_blocks(bias, m):
    return int(blocks(bias, m)[-1]) + 1


def lds_bytes(bias, m):
    return (4 << m) + 4 * ((n_blocks(bias, m) + 3) & ~3) + 131072


def layout_table(bias, m, seed):
    """a float32 table of 65536 entries that lut_compress can hold in layout (bias, m) only: every block has a random anchor (the
    bit pattern of a value in [1/64, 1)) and every entry a random 16-bit delta on top of its block's anchor.  Any coarser layout
    puts two anchors into one block, whose span then exceeds 16 bits.  The values are finite, in (0.015, 1.01) and not monotone -
    the operation is table[idx] - and spread over the unit range, so a wrong anchor or delta moves an 8-bit or 10-bit output code
    as well as an f32 bit pattern.

    For WRITER cases mind that a wrong delta shows only where it moves the output code (a delta is at most 2^16 ulps, about
    0.4 % of the value; a 10-bit code is 0.1 % of the range): the f32 reader cases are the exact ones, bit for bit."""
    blk = blocks(bias, m)
    anchor = frames.uniform_f32(int(blk[-1]) + 1, seed, 1.0 / 64, 1.0).view(np.uint32)
    delta = (frames.splitmix64(seed + 1, 65536) % np.uint64(65536)).astype(np.uint32)
    return (anchor[blk] + delta).view(np.float32)


@contextlib.contextmanager
def register(table):
    """upload a table, register it with the library, yield the device tensor, unregister on exit (such tables must not stay in
    hip_harness.ColourParams' cache: the next test may get the same device address for another table)"""
    import hip_harness as hh
    t = hh.dev(table)
    assert hh.ctx().register_lut(t, table), "the table has no LDS form"
    try:
        yield t
    finally:
        hh.host(t)  # (drains the library's queue and torch's: nothing still reads the table)
        hh.ctx().unregister_lut(t)


def index_probe():
    """the table whose entry IS its index: through the oracle with an identity gamut, the output is the index that was used"""
    return np.arange(65536, dtype=np.float32)


def missing(indices):
    """how many of the 65536 table indices do not occur in `indices` (the oracle's output under index_probe())"""
    seen = np.zeros(65536, bool)
    seen[np.asarray(indices, np.float32).astype(np.int64).reshape(-1)] = True
    return int(65536 - seen.sum())


def _lds_lookup(layout, image, idx):
    """The table kernels' lookup (phaneron_amd/csrc/ph_ldslut.h) restated with numpy on the LDS image: every float operation of it
    is exact, so float64 arithmetic narrowed to float32 reproduces it."""
    magic = np.float64(12582912.0)  # 1.5 * 2^23: y = idx + magic is what the rounding add leaves
    y = idx.astype(np.float64) + magic
    a_scale = np.float64(layout["a_scale"])
    fs = (y * a_scale - (magic - layout["index_bias"]) * a_scale).astype(np.float32)
    assert np.array_equal(fs.astype(np.float64), (idx.astype(np.float64) + layout["index_bias"]) * a_scale)  # exact
    a_addr = (fs.view(np.uint32) >> np.uint32(layout["shift"] - 2)) & np.uint32(0xFFFFFFFC)
    d_addr = np.uint32(layout["delta_off"]) + 2 * idx.astype(np.uint32)
    assert a_addr.min() >= layout["hole"] and a_addr.max() + 4 <= layout["delta_off"] and d_addr.max() + 2 <= layout["lds_bytes"]
    anchors = image[: layout["delta_off"]].view(np.uint32)
    deltas = image[layout["delta_off"]:].view(np.uint16)
    return anchors[a_addr >> 2] + deltas[idx].astype(np.uint32)


# ---- reader inputs: frames under which the oracle visits every index in R, in G and in B ------------------------------------------
def std_matrix(bits=10):
    """the 709 Loader matrix of a 10-bit / 8-bit format: the shape every matrix of the reference's colour maths has (read_px_lds' STD path)"""
    return orc.ycbcr2rgb_matrix("709", *((10, 64, 940, 896) if bits == 10 else (8, 16, 235, 224)))


def general_matrix(bits=10):
    """a matrix of another shape (the kernels' general dot products): index = 64 Y + Cr | 64 Y + Cb | 64 Y + Cr for 10-bit codes,
    256 Y + Cb | 256 Y + Cr | 256 Y + Cb for 8-bit ones - B has a Cr term, R (8-bit) a Cb term, so the STD test fails"""
    g = 64.0 if bits == 10 else 256.0
    rows = [(g, 0, 1, 0), (g, 1, 0, 0), (g, 0, 1, 0)] if bits == 10 else [(g, 1, 0, 0), (g, 0, 1, 0), (g, 1, 0, 0)]
    return (np.array(rows, np.float64) / 65535.0).astype(np.float32).reshape(-1)


def planes_of(fmt, y, cb, cr):
    """code planes (y [h][w], cb / cr [h][w / 2]) as a frame of any YCbCr pack format; 4:2:0 formats take the chroma of the even lines"""
    h, w = y.shape
    if fmt == "v210":
        return [frames.v210_pack_codes(y, cb, cr, w, h)]
    p = frames.pack_pitch(fmt, w) if fmt in orc.FORMATS else fmt10.pitch(w)
    wide = fmt in ("yuv422p10", "yuv420p10", "p010")
    dt = np.uint16 if wide else np.uint8
    Y, U, V = np.zeros((h, p), dt), np.zeros((h, p // 2), dt), np.zeros((h, p // 2), dt)
    Y[:, :w], U[:, : w // 2], V[:, : w // 2] = y, cb, cr
    if fmt not in ("yuv422p10", "yuv422p8"):
        U, V = U[0::2], V[0::2]
    if fmt == "p010":
        Y, U, V = Y << 6, U << 6, V << 6
    if fmt in ("nv12", "p010"):
        out = [Y, np.stack([U, V], axis=-1)]
    else:
        out = [Y, U, V]
    return [np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy() for a in out]


@functools.lru_cache(maxsize=None)
def _pairs10(kind):
    """pixel pairs (Y0, Y1, C) with Cb = Cr = C of 10-bit codes under which the oracle's reader, with the `kind` matrix, uses every
    table index in R, in G and in B.  Chosen from the pool Y = 0 .. 1023 x C = 0 .. 1023 by the oracle's own answer: per channel
    the first pixel that reaches each index."""
    cm = std_matrix() if kind == "std" else general_matrix()
    w, h = 1026, 1024  # whole quads: every pixel is read with the matrix's offset column
    y = np.broadcast_to((np.arange(w, dtype=np.uint32) % 1024)[None, :], (h, w))
    c = np.broadcast_to(np.arange(h, dtype=np.uint32)[:, None], (h, w // 2))
    idx = orc.v210_read(frames.v210_pack_codes(y, c, c, w, h), w, h, cm, index_probe(), IDENTITY)
    chosen = np.zeros(h * w, bool)
    for ch in range(3):
        found, first = np.unique(idx[..., ch].reshape(-1), return_index=True)
        assert found.size == 65536, "the pool reaches %d indices in channel %d under the %s matrix" % (found.size, ch, kind)
        chosen[first] = True
    px = np.flatnonzero(chosen)
    line, col = px // w, px % w  # (sorted by line: pixels of one chroma value are neighbours)
    yy, cc = (col % 1024).astype(np.uint32), line.astype(np.uint32)
    out = []
    for cval in np.unique(cc):
        ys = yy[cc == cval]
        if ys.size & 1:
            ys = np.append(ys, ys[-1])
        out.append(np.stack([ys[0::2], ys[1::2], np.full(ys.size // 2, cval, np.uint32)], axis=1))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def codes10(kind, w=1282, v420=False):
    """code planes of a 10-bit frame under which the oracle visits every index in every channel with the `kind` ("std" / "general")
    matrix.  w = 1282: lines of 213 whole v210 quads and a 4-pixel tail, whose vectors have last = 0 - the chosen pairs fill the
    whole quads, the tails repeat some of them.  v420: every line twice, so that a 4:2:0 frame keeps each pair's chroma."""
    pairs = _pairs10(kind)
    per_line = (w // 6) * 3
    h = -(-pairs.shape[0] // per_line)
    h += h & 1
    fill = pairs[np.arange(h * (w // 2)) % pairs.shape[0]].reshape(h, w // 2, 3)
    body = np.resize(pairs, (h * per_line, 3)).reshape(h, per_line, 3)  # (np.resize repeats the pairs to fill the last line)
    fill[:, :per_line] = body
    y = np.stack([fill[..., 0], fill[..., 1]], axis=-1).reshape(h, w)
    c = fill[..., 2]
    if v420:
        y, c = np.repeat(y, 2, axis=0), np.repeat(c, 2, axis=0)
    return np.ascontiguousarray(y), np.ascontiguousarray(c), np.ascontiguousarray(c)


@functools.lru_cache(maxsize=None)
def codes8():
    """code planes of an 8-bit frame (512 x 256) that holds every (Y, C) combination with Cb = Cr = C, 4:2:0 included: every code
    in every plane, and under general_matrix(8) every index in every channel"""
    w, h = 512, 256
    y = np.broadcast_to((np.arange(w, dtype=np.uint32) % 256)[None, :], (h, w))
    c = 2 * (np.arange(h, dtype=np.uint32)[:, None] // 2) + (np.arange(w // 2, dtype=np.uint32)[None, :] >= 128)
    return np.ascontiguousarray(y), np.ascontiguousarray(c), np.ascontiguousarray(c)


@functools.lru_cache(maxsize=None)
def rgb8_codes():
    """a packed 8-bit RGB frame (256 x 8 pixels x 4 bytes) with every code in every byte lane, a different order per lane"""
    n = 256 * 8
    i = np.arange(n, dtype=np.uint32)
    px = np.stack([i % 256, (i * 7 + 3) % 256, (255 - i) % 256, (i * 13 + 5) % 256], axis=-1).astype(np.uint8)
    return 256, 8, px.reshape(-1)


def reader_case(fmt, kind):
    """(planes, w, h, colMatrix or None) of a frame of `fmt` for the reader tests; kind "std" / "general" (RGB formats: None)"""
    import packfmt
    f = packfmt.get(fmt)
    if f.code_range is None:
        w, h, px = rgb8_codes()
        return [px], w, h, None
    bits = f.code_range[0]
    y, cb, cr = codes10(kind, v420=f.v420) if bits == 10 else codes8()
    cm = std_matrix(bits) if kind == "std" else general_matrix(bits)
    return planes_of(fmt, y, cb, cr), y.shape[1], y.shape[0], cm


def reader_coverage(fmt, kind):
    """why this frame is enough, judged by the oracle: None, or the failure message"""
    import packfmt
    f = packfmt.get(fmt)
    planes, w, h, cm = reader_case(fmt, kind)
    if f.code_range is None or (f.code_range[0] == 8 and kind == "std"):
        # an 8-bit frame cannot reach every index under its standard matrix: every input code in every plane (byte lane) instead
        lanes = [planes[0].reshape(-1, 4)[:, k] for k in range(4)] if f.code_range is None else \
            [a.reshape(-1) for a in codes8()]
        short = [k for k, a in enumerate(lanes) if np.unique(a).size != 256]
        return "%s %s: planes %r lack some of the 256 input codes" % (fmt, kind, short) if short else None
    idx = f.oracle_read(planes, w, h, cm, index_probe(), IDENTITY)
    gaps = [missing(idx[..., ch]) for ch in range(3)]
    return "%s %s %dx%d: the oracle leaves out %r of the 65536 indices in R, G, B" % (fmt, kind, w, h, gaps) if any(gaps) else None


# ---- writer inputs: an image whose R, G and B each hold every index, every tie and the ties' neighbours --------------------------
@functools.lru_cache(maxsize=None)
def writer_values():
    """f32 values t: i / 65535 for every i (rint(t * 65535) == i), every t whose f32 product t * 65535 is exactly i + 0.5 (the ties
    of the rounding index; found by search among the neighbours of (i + 0.5) / 65535), and the values one ulp either side of each"""
    k = np.float32(65535.0)
    base = (np.arange(65536, dtype=np.float64) / 65535.0).astype(np.float32)
    assert np.array_equal(np.rint(base * k), np.arange(65536, dtype=np.float32))
    half = np.arange(65535, dtype=np.float64) + 0.5
    cand = (half / 65535.0).astype(np.float32)
    ties = []
    for step in range(-3, 4):
        t = cand.copy()
        for _ in range(abs(step)):
            t = np.nextafter(t, np.float32(2.0 if step > 0 else -1.0))
        ties.append(t[(t * k).astype(np.float64) == half])
    ties = np.unique(np.concatenate(ties))
    assert ties.size > 0
    return np.concatenate([base, ties, np.nextafter(ties, np.float32(-1.0)), np.nextafter(ties, np.float32(2.0))])


@functools.lru_cache(maxsize=None)
def writer_image(w=1282):
    """an f32 RGBA image [h][w][4] for the writer tests: every channel holds writer_values() in an order of its own (three seeded
    permutations), random alpha, and below that eight lines of frames.rgba_specials.  w = 1282: each line ends in a 4-pixel v210
    tail, whose indices are truncated, not rounded.  The height is even (4:2:0 writers)."""
    vals = writer_values()
    lines = -(-vals.size // w)
    lines += lines & 1
    img = np.zeros((lines + 8, w, 4), np.float32)
    for ch in range(3):
        order = np.argsort(frames.splitmix64(0x7AB1E + ch, vals.size), kind="stable")
        img[:lines, :, ch] = np.resize(vals[order], lines * w).reshape(lines, w)
    img[:lines, :, 3] = frames.uniform_f32(lines * w, 0x7AB1E + 3).reshape(lines, w)
    img[lines:] = frames.rgba_specials(w, 8, 0x7AB1E + 4)
    return img


def writer_coverage(w=1282):
    """None, or why writer_image() is not enough: judged on the image and the reference's index arithmetic (rint of the f32 product)"""
    img = writer_image(w)
    k = np.float32(65535.0)
    with np.errstate(invalid="ignore", over="ignore"):
        x = img[..., :3] * k
        frac = x - np.floor(x)
    gaps = [missing(np.clip(np.rint(np.nan_to_num(x[..., ch], nan=0.0)), 0, 65535)) for ch in range(3)]
    if any(gaps):
        return "the writer image leaves out %r of the 65536 indices in R, G, B" % (gaps,)
    n_ties = [int(np.unique(x[..., ch][(frac[..., ch] == 0.5) & (x[..., ch] < 65535)]).size) for ch in range(3)]
    xv = writer_values() * k
    want = int(np.unique(xv[(xv - np.floor(xv)) == 0.5]).size)
    if min(n_ties) < want:
        return "the writer image holds %r of the %d exact ties in R, G, B" % (n_ties, want)
    return None
