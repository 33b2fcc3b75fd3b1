"""The 10-bit 4:2:0 decoder frames (yuv420p10le, p010le) and the 4:2:2 frames that define them (include/phaneron_hip.h,
DESIGN.md 2): random frames, the equivalent yuv422p10 frame F' a read is defined on, and the 4:2:0 planes a write makes from
what the yuv422p10 Writer makes.  Plane layouts: P = the width rounded up to 8 samples, 16-bit little-endian words;
yuv420p10 Y [h][P], Cb / Cr [h/2][P/2] (LSB-aligned); p010 Y [h][P], CbCr [h/2][P] (Cb first, MSB-aligned)."""
import numpy as np

FORMATS = ("yuv420p10", "p010")


def pitch(w):
    return w + 7 - ((w - 1) % 8)


def plane_bytes(fmt, w, h):
    p = pitch(w)
    return [2 * p * h, p * h // 2, p * h // 2] if fmt == "yuv420p10" else [2 * p * h, p * h]


def random_frame(fmt, w, h, seed):
    """raw 16-bit words (as uint16 arrays, one per plane): yuv420p10 words use all 16 bits (samples above 1023 included), p010
    words carry non-zero low bits below the sample"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << 16, n // 2, dtype=np.uint16) for n in plane_bytes(fmt, w, h)]


def as_bytes(planes):
    return [np.ascontiguousarray(p).view(np.uint8) for p in planes]


def to_422(fmt, planes, w, h):
    """F': the yuv422p10 frame (uint16 planes Y [h][P], Cb / Cr [h][P/2]) whose read is this frame's read - chroma line r is the
    source's chroma line r >> 1, a p010 sample is its word >> 6"""
    p = pitch(w)
    y = planes[0].reshape(h, p)
    if fmt == "yuv420p10":
        u, v = planes[1].reshape(h // 2, p // 2), planes[2].reshape(h // 2, p // 2)
    else:
        y = y >> 6
        c = planes[1].reshape(h // 2, p // 2, 2) >> 6
        u, v = c[:, :, 0], c[:, :, 1]
    rows = np.arange(h) >> 1
    return [np.ascontiguousarray(y).reshape(-1), np.ascontiguousarray(u[rows]).reshape(-1), np.ascontiguousarray(v[rows]).reshape(-1)]


def from_422_write(fmt, planes422, w, h, interlace):
    """the 4:2:0 planes a write makes, from the yuv422p10 Writer's planes of the same call (uint16, as to_422 lays them out):
    chroma row g is the 4:2:2 row 2g + (interlace == 3); p010 samples are (s << 6) & 0xffff, Cb and Cr interleaved"""
    p = pitch(w)
    y = planes422[0].reshape(h, p)
    rows = 2 * np.arange(h // 2) + (1 if interlace == 3 else 0)
    u, v = planes422[1].reshape(h, p // 2)[rows], planes422[2].reshape(h, p // 2)[rows]
    if fmt == "yuv420p10":
        return [np.ascontiguousarray(a).reshape(-1) for a in (y, u, v)]
    shl = lambda a: ((a.astype(np.uint32) << 6) & 0xFFFF).astype(np.uint16)
    c = np.stack([shl(u), shl(v)], axis=-1)
    return [shl(y).reshape(-1), np.ascontiguousarray(c).reshape(-1)]


def rows_written(h, interlace):
    """the luma rows a write call makes"""
    return np.arange(h) if interlace == 0 else np.arange(1 if interlace == 3 else 0, h, 2)
