"""The fused v210 kernel's layers below the top carry a NaN witness per pixel, not eighteen sums (ph_kernels_lds.hip
fused_layer_combine): a v210 reader emits alpha = 1, every combine is acc = fma(acc, 0, t), and a lower layer reaches the
picture only through whether one of its values is non-finite.  The witness is W = r * 0, fma(g, 0, W), fma(b, 0, W) of the
pixel's three table entries; the last layer combines with W.  That stands for the old arithmetic only where no finite table
entry can overflow in the gamut matrix, which a guard decides once per launch (ph_kernels.h fused_witness_holds); where it
fails the kernel keeps the accumulators through every layer.

Every GPU case runs ph_fused_v210_combine and compares its v210 words bit for bit with orc.pipeline_v210_combine on the same
inputs.  The last test needs no GPU: the guard as a launch gets it against a restatement in numpy.
"""
import ctypes as C

import numpy as np
import pytest

import frames
from oracle import orc
from phaneron_amd import capi

gpu = pytest.mark.gpu

WR_O = (orc.rgb2ycbcr_matrix("2020"), orc.linear2gamma_lut("2020"))
F32 = np.float32
TWO_126 = F32(2.0) ** F32(126)
TWO_125 = F32(2.0) ** F32(125)


def _bits_equal(got, want, what):
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %08x vs %08x" % (what, bad.size, w.size, bad[0], g[bad[0]], w[bad[0]])


def _lut_with(entry0):
    lut = orc.gamma2linear_lut("709").copy()
    lut[0] = entry0  # entry 0 is a block of its own in the LDS form (ph_lut.h), so it stays exact
    return lut


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


# the poisons at entry 0 whose table keeps its LDS form (decided here, on the CPU: a variant that cannot register is not a case)
_POISONS = [(name, v) for name, v in (("+inf", F32(np.inf)), ("-inf", F32(-np.inf)), ("nan", _bits(0x7FC00000)))
            if capi.lut_layout(_lut_with(v))[0] is not None]
assert any(name == "+inf" for name, _ in _POISONS), "the +Inf table must keep its LDS form"
_POISON_IDS = [name for name, _ in _POISONS]
_POISON_VALUES = [v for _, v in _POISONS]


def _standard():
    return orc.ycbcr2rgb_matrix("709"), orc.rgb2rgb_matrix("709", "2020")


def _flat(w, h, y, cb, cr):
    return frames.v210_pack_codes(np.full((h, w), y, np.uint32), np.full((h, w // 2), cb, np.uint32), np.full((h, w // 2), cr, np.uint32), w, h)


def _indices(cm, y, cb, cr):
    """the three reader-table indices of one code triple (v210.ts:64-70), in f32 as the kernels compute them"""
    m = np.asarray(cm, F32).reshape(3, 4)
    v = np.array([y, cb, cr, 1], F32)
    t = np.array([np.sum(m[i] * v, dtype=np.float64) for i in range(3)])
    return np.rint(np.clip(t, 0.0, 1.0) * 65535.0).astype(np.int64)


def _guard(lut, gm):
    """(lmax, holds) as a launch with this reader table and gamut matrix gets them (device-free)"""
    fn = capi.lib().ph_debug_fused_witness
    fn.restype = C.c_int
    fn.argtypes = [np.ctypeslib.ndpointer(np.float32, flags="C"), np.ctypeslib.ndpointer(np.float32, flags="C"), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lmax, holds = C.c_float(), C.c_int()
    assert fn(np.ascontiguousarray(lut, F32), np.ascontiguousarray(np.asarray(gm, F32).reshape(-1)[:9]), C.byref(lmax), C.byref(holds)) == 0
    return F32(lmax.value), bool(holds.value)


def _fused(layers, w, h, cm, lut, gm):
    """the kernel's words and the oracle's for one stack; cm (12), lut (65536), gm (9) as the oracle takes them"""
    import torch
    import hip_harness as hh
    k = hh.ctx()
    dlut = hh.dev(lut)
    assert k.register_lut(dlut, lut) == 1, "the reader table must keep its LDS form"
    try:
        wcm, wlut = hh.ColourParams.writer("2020")
        out = torch.full((frames.v210_pitch_bytes(w) * h // 4,), 0x2AAAAAAA, dtype=torch.int32, device="cuda")
        k.fused_v210_combine([hh.dev(l) for l in layers], out, w, h, hh.dev(cm), dlut,
                             hh.dev(np.concatenate([gm, np.zeros(3, np.float32)]).astype(np.float32)), wcm, wlut)
        got = hh.host(out, np.uint32)
    finally:
        k.unregister_lut(dlut)
    with np.errstate(all="ignore"):
        return got, orc.pipeline_v210_combine(layers, w, h, cm, lut, gm, *WR_O)


def _noise(w, h, channel, n):
    return [frames.v210_random(w, h, frames.layer_seed(channel, i), legal=False) for i in range(n)]


@gpu
@pytest.mark.parametrize("poison", _POISON_VALUES, ids=_POISON_IDS)
def test_poison_value_at_entry_0(poison):
    """the headline stack (N = 4) on noise that reaches index 0 in every layer: +Inf, -Inf and NaN all end as a NaN witness"""
    w, h = 1920, 32
    cm, gm = _standard()
    lut = _lut_with(poison)
    assert _guard(lut, gm)[1], "the witness path is the one under test"
    got, want = _fused(_noise(w, h, 20, 4), w, h, cm, lut, gm)
    _bits_equal(got, want, "entry 0 = %r" % poison)


@gpu
@pytest.mark.parametrize("n,where", [(3, (0,)), (3, (1,)), (3, (2,)), (3, (0, 1)), (4, (0,)), (4, (2,)), (4, (3,)), (4, (0, 2)), (4, (1, 2))],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else "n%d" % v)
def test_poison_position(n, where):
    """Index 0 of the +Inf table reached from the listed layers only: an all-zero-code layer there (R and B clamp to index 0),
    mid-grey layers elsewhere.  From the last layer the Inf is the value that is clamped; from any layer below it arrives as NaN."""
    w, h = 1920, 32
    cm, gm = _standard()
    lut = _lut_with(F32(np.inf))
    grey, zero = _flat(w, h, 512, 512, 512), _flat(w, h, 0, 0, 0)
    assert (_indices(cm, 0, 0, 0)[[0, 2]] == 0).all() and (_indices(cm, 512, 512, 512) > 0).all()
    layers = [zero if l in where else grey for l in range(n)]
    got, want = _fused(layers, w, h, cm, lut, gm)
    _bits_equal(got, want, "%d layers, poison in %r" % (n, where))
    clean = orc.pipeline_v210_combine([grey] * n, w, h, cm, lut, gm, *WR_O)
    assert not np.array_equal(want, clean), "the poison does not show"


def _gamut(kind):
    gm = _standard()[1].copy()
    if kind == "identity":
        gm = np.eye(3, dtype=F32).reshape(-1)
    elif kind == "zero-row":
        gm[3:6] = 0.0
    return gm.astype(F32)


@gpu
@pytest.mark.parametrize("kind", ["standard", "identity", "zero-row"])
@pytest.mark.parametrize("n,at", [(2, 0), (3, 1)], ids=["first", "middle"])
def test_poison_in_one_channel_only(kind, n, at):
    """A lower layer whose R clamps to index 0 while G and B do not: the one non-finite entry makes ALL three channels of the
    pixel's gamut product non-finite (Inf * c, Inf * 0 = NaN, NaN + x), so all three channels above it are NaN - with the
    standard matrix, with the identity (R's Inf meets a zero in the other two rows) and with a row of zeros."""
    w, h = 1920, 32
    cm, _ = _standard()
    gm = _gamut(kind)
    lut = _lut_with(F32(np.inf))
    idx = _indices(cm, 300, 512, 0)
    assert idx[0] == 0 and idx[1] > 0 and idx[2] > 0, idx
    layers = _noise(w, h, 21, n)
    layers[at] = _flat(w, h, 300, 512, 0)
    assert _guard(lut, gm)[1]
    got, want = _fused(layers, w, h, cm, lut, gm)
    _bits_equal(got, want, "R only, %s gamut matrix" % kind)
    top_alone = orc.pipeline_v210_combine(layers[-1:], w, h, cm, lut, gm, *WR_O)
    assert not np.array_equal(want, top_alone), "the poisoned channel does not show"


@gpu
@pytest.mark.parametrize("n", [2, 5])
def test_stack_depths(n):
    """N = 2: first and last, no middle layer; N = 5: the rolled loop of pairs and the odd middle layer behind it"""
    w, h = 1920, 32
    cm, gm = _standard()
    got, want = _fused(_noise(w, h, 22, n), w, h, cm, _lut_with(F32(np.inf)), gm)
    _bits_equal(got, want, "%d layers" % n)


@gpu
def test_general_matrix_copy():
    """a near-miss of the standard matrix shape (Cb feeds R): the general dot-product copy of the layer bodies"""
    w, h, n = 1920, 32, 3
    cm, gm = _standard()
    cm = cm.copy()
    cm[1] = F32(3.0e-4)
    got, want = _fused(_noise(w, h, 23, n), w, h, cm, _lut_with(F32(np.inf)), gm)
    _bits_equal(got, want, "cb in red")


@gpu
def test_ragged_lines():
    """1280 x 6: lines that end in a tail quad and two cleared slots, the kernel's other instantiation"""
    w, h, n = 1280, 6, 3
    cm, gm = _standard()
    got, want = _fused(_noise(w, h, 24, n), w, h, cm, _lut_with(F32(np.inf)), gm)
    _bits_equal(got, want, "ragged lines")


@gpu
def test_two_slices_per_workgroup():
    """1920 x 1080 is 1 350 quads per workgroup: one full slice and a second that only some waves hold - the smallest frame at
    which the prefetch chain crosses a slice boundary and a wave skips a slice"""
    w, h, n = 1920, 1080, 4
    cm, gm = _standard()
    got, want = _fused(_noise(w, h, 25, n), w, h, cm, _lut_with(F32(np.inf)), gm)
    _bits_equal(got, want, "two slices")


def _guard_cases():
    """(id, lut, gm, guard holds) - what the guard has to tell apart, each case stated with the side it must fall on"""
    cm, std = _standard()
    clean = orc.gamma2linear_lut("709").copy()
    eye = np.eye(3, dtype=F32).reshape(-1)
    below = np.nextafter(TWO_126, F32(0), dtype=F32)
    huge = clean.copy()
    huge[0] = F32(2.0) ** F32(127)  # finite, and the all-zero-code layer visits it
    nan_gm, inf_gm = std.copy(), std.copy()
    nan_gm[4] = F32(np.nan)
    inf_gm[0] = F32(np.inf)
    return [("bound-just-holds", clean, (eye * below).astype(F32), True),
            ("bound-just-fails", clean, (eye * TWO_126).astype(F32), False),
            ("gamut-overflows", clean, (std * F32(2.0) ** F32(127)).astype(F32), False),  # real Inf in the lower layers
            ("huge-entry", huge, (std * F32(4)).astype(F32), False),  # 2^127 * 4 * 0.63: real Inf from a finite entry
            ("gamut-nan", clean, nan_gm, False),
            ("gamut-inf", clean, inf_gm, False)]


_GUARD_CASES = _guard_cases()


@gpu
@pytest.mark.parametrize("case", _GUARD_CASES, ids=[c[0] for c in _GUARD_CASES])
def test_guard(case):
    """Each side of the guard against the oracle, the Inf and NaN that real overflow leaves in the lower layers included: an
    all-zero-code layer (index 0) at the bottom, noise above it"""
    name, lut, gm, holds = case
    w, h, n = 1920, 32, 4
    cm, _ = _standard()
    assert lut[65535] == F32(1.0) and _guard(lut, gm) == (max(F32(1.0), F32(np.abs(lut[0]))), holds), name
    layers = _noise(w, h, 26, n)
    layers[0] = _flat(w, h, 0, 0, 0)
    got, want = _fused(layers, w, h, cm, lut, gm)
    _bits_equal(got, want, name)


@gpu
@pytest.mark.parametrize("w,h,n", [(1280, 6, 3), (1920, 1080, 3), (1920, 32, 2), (1920, 32, 5)], ids=["ragged", "two-slices", "n2", "n5"])
def test_guard_failed_shapes(w, h, n):
    """where the guard fails the accumulators are kept through every layer: that path on the ragged form, across a slice
    boundary and at other depths, with a gamut matrix that overflows for real"""
    cm, std = _standard()
    gm = (std * F32(2.0) ** F32(127)).astype(F32)
    lut = _lut_with(F32(np.inf))
    assert not _guard(lut, gm)[1]
    got, want = _fused(_noise(w, h, 27, n), w, h, cm, lut, gm)
    _bits_equal(got, want, "guard failed, %d x %d, %d layers" % (w, h, n))


def _guard_restated(lut, gm):
    """the bound in numpy, f32 throughout: lmax * max_row(|g0| + |g1| + |g2|) < 2^126 and lmax < 2^125, false for any NaN or Inf"""
    lut = np.asarray(lut, F32)
    finite = np.abs(lut[np.isfinite(lut)])
    lmax = finite.max() if finite.size else F32(0)
    a = np.abs(np.asarray(gm, F32).reshape(-1)[:9]).reshape(3, 3)
    with np.errstate(all="ignore"):
        rows = (a[:, 0] + a[:, 1]) + a[:, 2]
        worst = rows.max()  # (NaN if any row is)
        return lmax, bool(F32(lmax * worst) < TWO_126) and bool(lmax < TWO_125)


def test_guard_expression_on_the_cpu():
    """what a launch is given (the table's largest finite magnitude) and what the kernel's expression makes of it, against the
    restatement above - for the guard cases, the poisoned tables, a table of Inf alone and bounds on either side of 2^125"""
    cm, std = _standard()
    cases = [(lut, gm) for _, lut, gm, _ in _GUARD_CASES]
    cases += [(_lut_with(v), std) for v in _POISON_VALUES]
    cases += [(np.full(65536, np.inf, F32), std), (_lut_with(F32(-3.0)), std)]
    eye = np.eye(3, dtype=F32).reshape(-1)
    for top in (np.nextafter(TWO_125, F32(0), dtype=F32), TWO_125):
        cases += [(_lut_with(top), eye), (_lut_with(-top), (eye * F32(0.5)).astype(F32))]
    for name, lut, gm, holds in _GUARD_CASES:
        assert _guard_restated(lut, gm)[1] == holds, name  # (the side each case is stated to fall on)
    for lut, gm in cases:
        want = _guard_restated(lut, gm)
        got = _guard(lut, gm)
        assert got[0].view(np.uint32) == F32(want[0]).view(np.uint32) and got[1] == want[1], (got, want)
