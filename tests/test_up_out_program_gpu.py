"""GPU tests (-m gpu) of the by-name program compose_up_multi_<n>: ph_compose_up_write_multi through ph_run_program's named arguments,
one and three outputs, the twin (the other field's images and planes) included; every plane against the oracle's chain, which pins
the typed call in test_up_out_gpu.py."""
import numpy as np
import pytest

from oracle import orc
from test_chan_multi_gpu import POISON, ByName, oracle_frame
from test_up_out_gpu import composite, images

pytestmark = pytest.mark.gpu

W, H, SW, SH = 384, 108, 192, 54


@pytest.fixture
def by_name():
    b = ByName(W, H)
    yield b
    b.close()


def layer_params(b, layers, suffix=""):
    p = {}
    for i, (img, mat) in enumerate(layers):
        p["l%dIn%s" % (i, suffix)] = b.upload(np.ascontiguousarray(img[..., :3]), svm="coarse")
        if not suffix:
            p["l%dWidth" % i], p["l%dHeight" % i] = img.shape[1], img.shape[0]
            p["l%dMatrix" % i] = b.upload(np.ascontiguousarray(mat, np.float32))
    return p


def three_outputs(b, prefix="output"):
    """v210 (output 0), yuv422p8 (1) and rgba8, field 3 (2): the planes by their argument names"""
    o0, o1, o2 = b.planes("v210"), b.planes("yuv422p8"), b.planes("rgba8")
    one = prefix + "1"
    return {prefix: o0[0], one: o1[0], one + "U": o1[1], one + "V": o1[2], prefix + "2": o2[0]}, (o0, o1, o2)


def recipe(b):
    capi = b.capi
    return dict(packedRgb=1, outColMatrix=b.recipe["outColMatrix"], outGammaLut=b.recipe["outGammaLut"], interlace=0,
                out1Packing=capi.FORMATS["yuv422p8"], out1ColMatrix=b.cm8, out1GammaLut=b.recipe["outGammaLut"], interlace1=0,
                out2Packing=capi.FORMATS["rgba8"], out2GammaLut=b.recipe["outGammaLut"], interlace2=3)


def expect_three(comp):
    wlut = orc.linear2gamma_lut("709")
    return [oracle_frame("v210", comp, W, H, 0, orc.rgb2ycbcr_matrix("709"), wlut),
            oracle_frame("yuv422p8", comp, W, H, 0, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["yuv422p8"]), wlut),
            oracle_frame("rgba8", comp, W, H, 3, None, wlut)]


def compare(b, outs, want, what):
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), np.asarray(x).reshape(-1).view(np.uint8)), "%s: output %d plane %d" % (what, i, pl)


def test_one_output(by_name):
    b = by_name
    layers = images(W, H, [(SW, SH, dict())] * 2, True, 300)
    planes = b.planes("nv12")
    params = dict(layer_params(b, layers), packedRgb=1, outPacking=b.capi.FORMATS["nv12"], output=planes[0], outputC=planes[1],
                  outColMatrix=b.upload(b.capi.rgb2ycbcr_matrix("709", *b.capi.FORMAT_RANGE["nv12"])), outGammaLut=b.recipe["outGammaLut"])
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:up", "compose_up_multi_2", [W, H])
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == "compose_up_multi<rgb>x1j1", t.route
    comp = composite(layers, W, H)
    compare(b, [planes], [oracle_frame("nv12", comp, W, H, 0, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["nv12"]), orc.linear2gamma_lut("709"))], "nv12")
    prog.destroy()


def test_three_outputs_and_the_twin(by_name):
    b = by_name
    first, second = images(W, H, [(SW, SH, dict())], True, 310), images(W, H, [(SW, SH, dict())], True, 320)
    names, outs = three_outputs(b)
    twin_names, twin_outs = three_outputs(b, "twinOutput")
    params = dict(layer_params(b, first), **recipe(b), **names)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("", "compose_up_multi_1", [W, H])
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == "compose_up_multi<rgb>x3j1", t.route
    compare(b, outs, expect_three(composite(first, W, H)), "one job")
    # both fields' images in one launch, through ph_run_programs
    names, outs = three_outputs(b)
    params = dict(layer_params(b, first), **layer_params(b, second, "2"), **recipe(b), **names, **twin_names)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    with b.capi.trace() as t:
        b.ctx.run_programs([(prog, params)])
    b.ctx.wait()
    assert t.route == "compose_up_multi<rgb>x3j2", t.route
    compare(b, outs, expect_three(composite(first, W, H)), "first job")
    compare(b, twin_outs, expect_three(composite(second, W, H)), "twin")
    prog.destroy()


def test_a_defect_names_its_argument(by_name):
    b = by_name
    names, outs = three_outputs(b)
    params = dict(layer_params(b, images(W, H, [(SW, SH, dict())], True, 330)), **recipe(b), **names)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:up", "compose_up_multi_1", [W, H])
    defects = [({k: v for k, v in params.items() if k != "out1GammaLut"}, "out1GammaLut"), (dict(params, out1Packing=99), "out1Packing"),
               (dict(params, out2Packing=b.capi.FORMATS["p010"]), "out2Packing"), (dict(params, output1=params["output"]), "output1"),
               ({k: v for k, v in params.items() if not k.startswith("output1")}, "output2")]  # a gap: output 2 without output 1
    for job, name in defects:
        seen = []
        for check_only in (True, False):
            with pytest.raises(b.capi.PhaneronError) as e:
                b.ctx.run_program(prog, job, check_only=check_only)
            seen.append(str(e.value))
        assert seen[0] == seen[1] and "'%s'" % name in seen[0], seen
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
    prog.destroy()
