"""Device buffers between guard bands: a test that makes every buffer of a call with this module finds the kernel that touches
memory outside the buffers it was given.

Each buffer is ONE allocation of `G + nbytes + G` bytes.  The payload sits in the middle and is what the caller gets, as a tensor
slice in the array's dtype (capi._ptr takes its data_ptr(), so it goes through every capi.Context method and hh.host()); the G bytes
on either side hold a known fill and are compared with it by check().  A stray access therefore lands in memory the test itself
owns, inside the same allocation: nothing here provokes a fault.

Geometry.  G is a multiple of 256 bytes, so the payload starts on the alignment a real allocation has and only the neighbourhood
changes; G is at least 4096 bytes and at least two rows of the buffer's row pitch plus 64 bytes (`pitch`, default: the whole
payload), so that one row too many, or one vector too many, still lands in the guard.  The guard after the payload starts at the
very first byte after it - no rounding, also for planes of odd byte counts.

Fill.  Destination guards hold bytes 0xC3 (neither poison value of the suite, 0xA5 and 0x5A).  Source guards hold what changes a
result that uses them: dwords 0x7FC00000 for float data (a NaN, which survives a zero weight), bytes 0xFF for planes of codes
(v210 code 1023; opaque white in rgba8 / bgra8, where the border is transparent black).

What this can and cannot see:
  * a store outside a buffer is always found (source guards are compared too: a kernel must not write there either);
  * a load outside a buffer is found when its value reaches an output - the caller compares the outputs with the oracle;
  * a stray load whose value is thrown away cannot be seen this way, and nothing here claims to.

Offsets in a failure message are relative to the payload: on the side "before" they are negative (-1: the byte just in front of
the payload), on the side "after" they count from the first byte behind it (0).

The module keeps every allocation alive until reset() (the launches are asynchronous: hip_harness._TorchOrdered) and synchronises
after filling, as hh.dev does.  It is a plain module: no fixture, no conftest, no pytest setting."""
import numpy as np
import torch

DST_FILL = 0xC3
CODE_FILL = 0xFF
NAN_DWORD = 0x7FC00000
MIN_GUARD = 4096
ALIGN = 256

_TORCH_VIEW = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}  # bit-preserving, as hh.dev carries uint32
_live = []


class _Guarded:
    def __init__(self, label, role, raw, g, nbytes, pattern):
        self.label, self.role, self.raw, self.g, self.nbytes, self.pattern = label, role, raw, g, nbytes, pattern


def guard_bytes(nbytes, pitch=None):
    """G of a buffer of nbytes whose rows are pitch bytes apart"""
    pitch = nbytes if pitch is None else pitch
    need = max(MIN_GUARD, 2 * int(pitch) + 64)
    return (need + ALIGN - 1) // ALIGN * ALIGN


def fill_pattern(role, dtype):
    """the four bytes a guard repeats, in memory order"""
    if role == "dst":
        return np.full(4, DST_FILL, np.uint8)
    if np.dtype(dtype) == np.float32:
        return np.array([NAN_DWORD], "<u4").view(np.uint8).copy()
    return np.full(4, CODE_FILL, np.uint8)


def _expected(pattern, start, n):
    """n guard bytes from allocation offset start (G is a multiple of 4, so the phase is the offset's)"""
    return np.resize(np.roll(pattern, -(start % 4)), n) if n else np.zeros(0, np.uint8)


def default_device():
    return "cuda" if torch.cuda.is_available() else "cpu"


def dev(array, role, pitch=None, label=None, device=None, fill=None):
    """the array between guards on the device; returns the payload (a view, not a copy, of the one allocation).
    fill: "float" / "codes" overrides what a source guard holds (default: by dtype - float32 is float data, the rest codes)"""
    assert role in ("src", "dst"), role
    a = np.ascontiguousarray(array)
    a = a.view(_TORCH_VIEW.get(a.dtype, a.dtype))
    nbytes = a.nbytes
    g = guard_bytes(nbytes, pitch)
    pattern = fill_pattern(role, {None: a.dtype, "float": np.float32, "codes": np.uint8}[fill])
    host = np.empty(g + nbytes + g, np.uint8)
    host[:g] = _expected(pattern, 0, g)
    host[g:g + nbytes] = a.reshape(-1).view(np.uint8)
    host[g + nbytes:] = _expected(pattern, g + nbytes, g)
    raw = torch.from_numpy(host).to(device or default_device())
    if raw.is_cuda:
        torch.cuda.synchronize()
    _live.append(_Guarded(label or "%s#%d" % (role, len(_live)), role, raw, g, nbytes, pattern))
    return raw[g:g + nbytes].view(torch.from_numpy(a.reshape(-1)[:0]).dtype).reshape(a.shape)


def full(n, value, dtype=np.float32, role="dst", **kw):
    return dev(np.full(n, value, dtype), role, **kw)


def zeros(n, dtype=np.float32, role="dst", **kw):
    return dev(np.zeros(n, dtype), role, **kw)


def reset():
    del _live[:]


def live():
    return list(_live)


def owner(t):
    """the record of the guarded buffer whose payload this tensor starts at, or None"""
    p = t.data_ptr()
    for r in _live:
        if p == r.raw.data_ptr() + r.g and t.device == r.raw.device:
            return r
    return None


def _sync():
    if any(r.raw.is_cuda for r in _live):
        import hip_harness as hh
        hh.ctx().wait()
        torch.cuda.synchronize()


def check():
    """compare every guard made since reset() with its fill; returns (sources, destinations) checked"""
    _sync()
    n = {"src": 0, "dst": 0}
    for r in _live:
        n[r.role] += 1
        host = r.raw.cpu().numpy()
        for side, start, origin in (("before", 0, r.g), ("after", r.g + r.nbytes, r.g + r.nbytes)):
            bad = np.flatnonzero(host[start:start + r.g] != _expected(r.pattern, start, r.g))
            if bad.size:
                raise AssertionError("guard damaged: buffer %r (%s, %d bytes), side %s: %d bytes differ, first at offset %d, last at offset %d"
                                     % (r.label, r.role, r.nbytes, side, bad.size, start + bad[0] - origin, start + bad[-1] - origin))
    return n["src"], n["dst"]
