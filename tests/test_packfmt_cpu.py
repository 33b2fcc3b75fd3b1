"""CPU checks that pin tests/packfmt.py - the tests' one description of the pack formats - to the library, and the GPU sweeps'
format lists to it: a tenth name in capi.FORMATS fails here until it has a row there and is swept."""
import os
import re

import numpy as np
import pytest

import fmt10
import frames
import packfmt
from phaneron_amd import capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SIZES = [(2, 2), (1920, 1080), (1280, 720), (718, 480)] + [(w, h) for w in range(2, 34, 2) for h in (2, 6)] + [(64 + r, 10) for r in range(0, 8, 2)] + [(258, 4)]
ODD_SIZES = [(3, 2), (2, 3), (7, 5), (719, 480), (718, 479), (1919, 1081)] + [(65 + r, 4) for r in range(0, 8, 2)]


def test_the_helper_names_every_format_of_the_library():
    assert packfmt.NAMES == list(capi.FORMATS)
    assert [capi.FORMATS[n] for n in packfmt.NAMES] == list(range(len(packfmt.NAMES)))
    for n in packfmt.NAMES:
        assert packfmt.get(n).code_range == capi.FORMAT_RANGE[n]
    assert packfmt.PLANAR_10_420 == list(fmt10.FORMATS)  # (the formats fmt10.py defines through F')


@pytest.mark.parametrize("fmt", list(capi.FORMATS))
def test_plane_sizes_and_even_size_rule_are_the_library_s(fmt):
    f = packfmt.get(fmt)
    assert {w % 8 for w, _ in SIZES} == {0, 2, 4, 6}
    for w, h in SIZES:
        assert f.plane_bytes(w, h) == capi.pack_plane_bytes(fmt, w, h), (fmt, w, h)
        assert [p.nbytes for p in f.random_planes(w, h, 1)] == f.plane_bytes(w, h) == [p.nbytes for p in f.poisoned(w, h)]
        assert all((p.view(np.uint8) == packfmt.POISON).all() for p in f.poisoned(w, h))
        assert f.even(w, h) == (w, h)
    for w, h in ODD_SIZES:
        try:
            capi.pack_plane_bytes(fmt, w, h)
            refused = False
        except capi.PhaneronError as e:
            refused = True
            assert "even width and height" in str(e)
        assert refused == f.even_size, (fmt, w, h)
        ew, eh = f.even(w, h)  # the stand-in a sweep uses instead of dropping the case
        assert (ew, eh) >= (w, h) and ew - w <= 1 and eh - h <= 1 and capi.pack_plane_bytes(fmt, ew, eh)
        assert not (f.v420 and eh & 1)


def test_constraints_follow_the_format_table_of_the_kernels():
    """the traits the kernels and entry points branch on (ph_formats.h kFmts: planes, rgb8, v420, wide, msb, even_size, deint, chan_out)"""
    text = open(os.path.join(ROOT, "phaneron_amd", "csrc", "ph_formats.h")).read()
    rows = re.findall(r'\{PH_FMT_\w+,\s*"(\w+)",\s*PH_SRC_\w+,\s*(\d),\s*(true|false),\s*(true|false),\s*(true|false),\s*(\d),\s*(true|false),\s*(true|false),\s*(true|false)\}', text)
    assert [r[0] for r in rows] == packfmt.NAMES
    for name, planes, rgb8, v420, wide, msb, even, deint, chan_out in rows:
        f = packfmt.get(name)
        assert len(f.plane_bytes(64, 16)) == int(planes), name
        assert (f.code_range is None) == (rgb8 == "true"), name
        assert f.planar == (int(planes) > 1), name
        assert (f.v420, f.even_size, f.deint, f.chan_out) == (v420 == "true", even == "true", deint == "true", chan_out == "true"), name
        assert f.chan_source and name in capi.SRC_PLANAR or name in ("v210", "rgba8", "bgra8")
        if f.via422:
            assert wide == "true" and f.v420 and packfmt.get(f.sibling8).v420 and len(packfmt.get(f.sibling8).plane_bytes(64, 16)) == int(planes)


def parametrised_with(module, test, arg):
    fn = getattr(__import__(module), test)
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and arg in [a.strip() for a in mark.args[0].split(",")]:
            return list(mark.args[1])
    raise AssertionError("%s::%s is not parametrised with %r" % (module, test, arg))


# every sweep over formats: (module, test, argument, the formats it must run)
SWEEPS = [
    ("test_hip_sweep", "test_pack_formats_random_sizes", "fmt", packfmt.STANDALONE),
    ("test_chan_gpu", "test_planar_eight_bit_sources", "fmt", packfmt.PLANAR_8),
    ("test_chan_gpu", "test_ten_bit_420_sources", "fmt", packfmt.PLANAR_10_420),
    ("test_chan_gpu", "test_planar_clips_at_their_own_scale", "fmt", packfmt.PLANAR),
    ("test_chan_gpu", "test_enlarged_decoder_frames_on_both_routes", "fmt", packfmt.CLIPS),
    ("test_chan_gpu", "test_packed_rgb_sources_with_alpha", "fmt", packfmt.RGB8),
    ("test_chan_gpu", "test_other_output_formats", "fmt", packfmt.CHAN_OUT),
    ("test_chan_gpu", "test_other_output_formats_at_1280", "fmt", packfmt.CHAN_OUT),
    ("test_chan_gpu", "test_other_consumers_frames_from_every_kind_of_program", "src", ["v210", "yuv420p", "yuv422p10"] + packfmt.PLANAR_10_420),
    ("test_chan_gpu", "test_ten_bit_420_clips_take_the_routes_of_their_eight_bit_siblings", "fmt", packfmt.PLANAR_10_420),
    ("test_chan_gpu", "test_small_ragged_ten_bit_420_clips_whose_taps_leave_the_frame", "fmt", packfmt.PLANAR_10_420),
    ("test_chan_gpu", "test_transitions_between_ten_bit_420_frames", "fmt", packfmt.PLANAR_10_420),
    ("test_chan_gpu", "test_chan_batch_with_ten_bit_420_jobs", "fmt", packfmt.PLANAR_10_420),
    ("test_chan_gpu", "test_refusals_of_the_formats_the_kernel_does_not_write", "fmt", packfmt.NOT_CHAN_OUT),
    ("test_fmt10_gpu", "test_read_at_the_edges", "fmt", packfmt.PLANAR_10_420),
    ("test_fmt10_gpu", "test_write_at_the_edges", "fmt", packfmt.PLANAR_10_420),
    ("test_fmt10_gpu", "test_batch_read_of_small_ragged_frames_equals_separate_reads", "fmt", packfmt.PLANAR_10_420),
    ("test_fmt10_gpu", "test_odd_frames_are_refused_on_the_device_entry_points", "fmt", packfmt.names(even_size=True)),
    ("test_fmt10_gpu", "test_deinterlacing_reader_refuses_the_formats", "fmt", [n for n in packfmt.NOT_DEINT if packfmt.get(n).planar]),
    # between guard bands (tests/guard.py): no byte read or written outside the planes the format's sizes promise
    ("test_guard_gpu", "test_pack_formats_between_guards", "fmt", packfmt.STANDALONE),
    ("test_guard_gpu", "test_deinterlacing_reader_between_guards", "fmt", packfmt.names(deint=True)),
    ("test_guard_gpu", "test_channel_kernel_between_guards", "fmt", packfmt.names(chan_source=True)),
]


@pytest.mark.parametrize("module,test,arg,want", SWEEPS, ids=["%s::%s" % s[:2] for s in SWEEPS])
def test_a_sweep_runs_the_formats_the_helper_lists_for_it(module, test, arg, want):
    assert sorted(parametrised_with(module, test, arg)) == sorted(want)


def test_the_sweeps_together_run_every_format():
    """each format is read and written standalone, used as a channel source where it can be one, and either written by the channel
    kernel or refused by it; the random campaigns draw from every source format"""
    run = lambda names: {f for s in SWEEPS if s[1] in names for f in parametrised_with(*s[:3])}
    everything = set(capi.FORMATS)
    assert run({"test_pack_formats_random_sizes"}) | set(packfmt.V210) == everything
    sources = run({"test_planar_clips_at_their_own_scale", "test_enlarged_decoder_frames_on_both_routes", "test_packed_rgb_sources_with_alpha"})
    assert sources | set(packfmt.V210) == set(packfmt.names(chan_source=True)) == everything
    assert run({"test_other_output_formats"}) | set(packfmt.V210) == set(packfmt.names(chan_out=True))
    assert run({"test_refusals_of_the_formats_the_kernel_does_not_write"}) == everything - set(packfmt.names(chan_out=True))
    assert set(packfmt.SWEPT) == everything
    assert run({"test_pack_formats_between_guards"}) | set(packfmt.V210) == everything == run({"test_channel_kernel_between_guards"})
    assert run({"test_deinterlacing_reader_between_guards"}) == everything - set(packfmt.NOT_DEINT)
    import test_chan_gpu
    assert set(test_chan_gpu.RANDOM_FORMATS_10) | set(packfmt.V210) == everything
    new = [f for f in test_chan_gpu.RANDOM_FORMATS_10 if f in packfmt.PLANAR_10_420]
    assert 3 * len(new) >= len(test_chan_gpu.RANDOM_FORMATS_10)
    assert test_chan_gpu.RANDOM_FORMATS == ("yuv422p10", "yuv422p8", "yuv420p", "nv12", "rgba8", "bgra8")  # the older campaigns' cases depend on it


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
def test_the_422_frame_and_the_write_made_from_it_are_inverse(fmt):
    """to_422 then from_422_write gives the frame back (p010: its samples, the words' low six bits cleared) whichever line of a pair the
    chroma is taken from - widths 2 ... 258, heights 2, 6, 10"""
    for w in list(range(2, 82, 2)) + [250, 256, 258]:
        for h in (2, 6, 10):
            planes = fmt10.random_frame(fmt, w, h, 31 * w + h)
            f422 = fmt10.to_422(fmt, planes, w, h)
            assert [p.size for p in f422] == [fmt10.pitch(w) * h, fmt10.pitch(w) * h // 2, fmt10.pitch(w) * h // 2]
            for il in (0, 1, 3):
                back = fmt10.from_422_write(fmt, f422, w, h, il)
                for a, b in zip(back, planes):
                    assert np.array_equal(a, b & 0xFFC0 if fmt == "p010" else b), (fmt, w, h, il)


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
def test_expected_planes_of_a_single_field_keep_the_destination(fmt):
    """the helper's expected planes of one write call (the oracle's yuv422p10 Writer, special float values included): the other field's luma
    rows hold the destination's bytes untouched - for p010 too, whose definition shifts whole planes - every chroma row is written, and
    the two fields one after the other equal the definition applied to the whole 4:2:2 frame"""
    from oracle import orc
    f = packfmt.get(fmt)
    for w, h in ((2, 2), (6, 6), (12, 10), (74, 6), (78, 2), (250, 10)):
        line = 2 * fmt10.pitch(w)
        rgba = frames.rgba_specials(w, h, 77 + w)
        cm, lut = f.oracle_writer("2020")
        for il in (0, 1, 3):
            dst = f.poisoned(w, h)
            out = f.oracle_write(rgba, w, h, il, cm, lut, dst)
            assert all((p == packfmt.POISON).all() for p in dst), "the destination given is not changed"
            keep, made = f.rows_untouched(h, il), fmt10.rows_written(h, il)
            assert (out[0].reshape(h, line)[keep] == packfmt.POISON).all() and len(keep) + len(made) == h
            full = fmt10.as_bytes(fmt10.from_422_write(fmt, [p.view(np.uint16) for p in orc.pack_write("yuv422p10", rgba, w, h, 0, cm, lut)], w, h, il))
            assert np.array_equal(out[0].reshape(h, line)[made], full[0].reshape(h, line)[made])
            assert all(np.array_equal(a, b) for a, b in zip(out[1:], full[1:]))
        both = f.oracle_write(rgba, w, h, 3, cm, lut, f.oracle_write(rgba, w, h, 1, cm, lut, f.poisoned(w, h)))
        p422 = orc.pack_write("yuv422p10", rgba, w, h, 3, cm, lut, planes=orc.pack_write("yuv422p10", rgba, w, h, 1, cm, lut))
        assert all(np.array_equal(a, b) for a, b in zip(both, fmt10.as_bytes(fmt10.from_422_write(fmt, [p.view(np.uint16) for p in p422], w, h, 3))))
