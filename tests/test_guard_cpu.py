"""tests/guard.py proves itself on CPU tensors: geometry, fills, bit-exact payloads, and check() finding each flipped guard byte."""
import numpy as np
import pytest
import torch

import guard


@pytest.fixture(autouse=True)
def fresh():
    guard.reset()
    yield
    guard.reset()


def rec():
    return guard.live()[-1]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.int32, np.float32])
def test_payload_round_trips_bit_for_bit(dtype):
    r = np.random.default_rng(7)
    a = r.integers(0, 256, 4 * 611, dtype=np.uint8).view(dtype)  # every bit pattern, NaNs among the floats
    t = guard.dev(a, "src", device="cpu")
    assert t.numel() == a.size and t.element_size() == a.itemsize
    assert np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8))
    assert np.array_equal(rec().raw[rec().g:rec().g + a.nbytes].numpy(), a.view(np.uint8))
    assert t.data_ptr() == rec().raw.data_ptr() + rec().g  # the middle of the one allocation, not a copy
    assert guard.check() == (1, 0)


def test_two_dimensional_arrays_keep_their_shape():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    t = guard.dev(a, "dst", device="cpu")
    assert tuple(t.shape) == a.shape and np.array_equal(t.numpy(), a)


@pytest.mark.parametrize("nbytes", [1, 6, 255, 256, 4099, 70000])
def test_geometry(nbytes):
    t = guard.dev(np.zeros(nbytes, np.uint8), "dst", device="cpu")
    r = rec()
    assert r.g % 256 == 0 and (t.data_ptr() - r.raw.data_ptr()) % 256 == 0 and t.data_ptr() - r.raw.data_ptr() == r.g
    assert r.raw.numel() == r.g + nbytes + r.g          # before == after == G, the after-guard starts at nbytes exactly
    assert (r.raw[r.g + nbytes:].numpy() == guard.DST_FILL).all() and (r.raw[:r.g].numpy() == guard.DST_FILL).all()
    assert r.g >= 4096 and r.g >= 2 * nbytes + 64        # the pitch defaults to the whole payload


@pytest.mark.parametrize("pitch,want", [(1, 4096), (128, 4096), (2016, 4096), (2017, 4352), (5120, 10496), (30720, 61696)])
def test_guard_size_follows_the_pitch(pitch, want):
    g = guard.guard_bytes(10 * pitch, pitch)
    assert g == want and g % 256 == 0 and g >= 4096 and g >= 2 * pitch + 64 and g - 256 < max(4096, 2 * pitch + 64)
    guard.dev(np.zeros(10 * pitch, np.uint8), "src", pitch=pitch, device="cpu")
    assert rec().g == want


def test_fills():
    guard.dev(np.zeros(5, np.float32), "src", device="cpu")
    before, after = rec().raw[:rec().g].numpy(), rec().raw[rec().g + 20:].numpy()
    for side in (before, after):
        assert (side.view("<u4") == 0x7FC00000).all() and np.isnan(side.view("<f4")).all()
    for dtype in (np.uint8, np.uint16, np.uint32):
        guard.dev(np.zeros(3, dtype), "src", device="cpu")
        assert (rec().raw[:rec().g].numpy() == 0xFF).all() and (rec().raw[rec().g + rec().nbytes:].numpy() == 0xFF).all()
    guard.dev(np.zeros(3, np.uint8), "src", fill="float", device="cpu")   # an odd byte count: the dwords keep their phase
    assert rec().raw[rec().g + 3:rec().g + 8].numpy().tolist() == [0x7F, 0x00, 0x00, 0xC0, 0x7F]
    guard.dev(np.zeros(4, np.int32), "src", fill="float", device="cpu")
    assert np.isnan(rec().raw[:rec().g].numpy().view("<f4")).all()
    for dtype in (np.uint8, np.float32):
        guard.zeros(7, dtype, device="cpu")
        assert (rec().raw[:rec().g].numpy() == 0xC3).all() and (rec().raw[rec().g + rec().nbytes:].numpy() == 0xC3).all()
    assert 0xC3 not in (0xA5, 0x5A)
    assert guard.check() == (6, 2)


def test_zeros_and_full():
    z = guard.zeros(9, np.float32, device="cpu")
    f = guard.full(6, 0xA5, np.uint8, device="cpu")
    w = guard.full(3, 0xA5A5A5A5, np.uint32, device="cpu")
    assert z.dtype == torch.float32 and (z == 0).all() and f.dtype == torch.uint8 and (f == 0xA5).all()
    assert w.dtype == torch.int32 and (w.numpy().view(np.uint32) == 0xA5A5A5A5).all()
    assert guard.check() == (0, 3)


FLIPS = {"last of before": (lambda r: r.g - 1, "before", -1), "first of after": (lambda r: r.g + r.nbytes, "after", 0),
         "first of allocation": (lambda r: 0, "before", None), "last of allocation": (lambda r: r.raw.numel() - 1, "after", None)}


@pytest.mark.parametrize("role", ["src", "dst"])
@pytest.mark.parametrize("nbytes", [6, 4099, 4096])
@pytest.mark.parametrize("flip", list(FLIPS))
def test_check_finds_one_flipped_byte(flip, nbytes, role):
    guard.dev(np.zeros(16, np.float32), "src", label="bystander", device="cpu")
    guard.dev(np.zeros(nbytes, np.uint8), role, label="the victim", device="cpu")
    guard.zeros(5, np.uint8, label="another", device="cpu")
    counts = (2, 1) if role == "src" else (1, 2)
    assert guard.check() == counts
    r = guard.live()[1]
    at, side, offset = FLIPS[flip]
    at = at(r)
    if offset is None:
        offset = -r.g if side == "before" else r.g - 1
    r.raw[at] ^= 0x01
    with pytest.raises(AssertionError) as e:
        guard.check()
    msg = str(e.value)
    assert "'the victim'" in msg and "side %s" % side in msg and "1 bytes differ" in msg
    assert "first at offset %d, last at offset %d" % (offset, offset) in msg
    r.raw[at] ^= 0x01
    assert guard.check() == counts


def test_a_run_of_damage_reports_its_first_and_last_byte():
    guard.zeros(10, np.uint8, label="plane", device="cpu")
    r = rec()
    r.raw[r.g + 10:r.g + 26] = 0
    r.raw[r.g + 100] = 0
    with pytest.raises(AssertionError, match=r"'plane' \(dst, 10 bytes\), side after: 17 bytes differ, first at offset 0, last at offset 90"):
        guard.check()


def test_a_write_of_the_fill_value_inside_the_payload_is_not_damage_and_reset_forgets():
    t = guard.zeros(8, np.uint8, device="cpu")
    t[:] = 0xC3
    assert guard.check() == (0, 1)
    guard.reset()
    assert guard.check() == (0, 0) and guard.live() == []
