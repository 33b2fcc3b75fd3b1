"""Job lists for ph_run_programs whose jobs read and write each other's buffers: the hazard generator the call-order tests share.

ph_run_programs promises "exactly ph_run_program for j = 0 .. n_jobs - 1 in that order" while it puts consecutive jobs of one kind and
shape into shared launches; a job that reads what an earlier job of its launch writes (RAW), writes what one reads (WAR) or writes what
one writes (WAW) has to start the next launch.  This module draws such calls (plain Python, no device), says for every consecutive pair
of jobs that could share a launch which hazards it carries, and lists the directed cells [A, B, C] the GPU tests run.

Shapes: frames are 384 x 54 v210 (55 296 B), layer images 192 x 30 - what the other ph_run_programs tests use; the grouping looks at
byte ranges, never at sizes.

The pool: N_IMAGE *universal* buffers - 192 * 30 * 16 = 92 160 B, created as images with dims (192, 30) - and N_PLAIN buffers of the
same size without dims.  A universal buffer is a v210 source or output of the headline kernel, an output of any job, an RGBA layer
image, a packed-RGB layer image (69 120 B) and a chroma plane.  One thing it cannot be: the channel program reads a buffer that HAS image
dims as an f32 RGBA image (chan_source_parse), so a channel job's v210 source has to be a buffer without dims - the two plain ones are
in the pool for that (a channel job that draws a universal buffer reads it as a 192 x 30 image).  The pool is filled with
frames.v210_random words: their top two bits are zero, so every word read as f32 is finite and below 2, v210 outputs keep that, no
NaN ever enters an image and byte equality between two routes stays meaningful.

A job is a dict:
  kind    "fused" (fused_v210_combine_<n>) | "chan" (chan_compose_v210_<n>) | "up" (compose_up_write_v210_<n>)
  n       layers
  ins     pool index per layer: l<i>In - for a planar channel layer the CHROMA plane l<i>InU (its Y and V planes are fixed read-only frames)
  out     pool index of `output`
  ins2    None, or (the two-field form of "up") pool index per layer: l<i>In2
  out2    None, or the pool index of `output2`
  packed  "up": packedRgb = 1
  planar  "chan": per layer, the source is a yuv422p8 frame whose U plane is ins[i]
  small   "chan": per layer, the placement is the half-size one (else the fill)
A job never names its own output as its own input: that is a race in any context."""
import numpy as np

W, H, SW, SH = 384, 54, 192, 30
FRAME_BYTES = W * 8 // 3 * H          # 384 is a multiple of 48: no line padding
IMAGE_BYTES = SW * SH * 16
PACKED_BYTES = SW * SH * 12
N_IMAGE, N_PLAIN = 6, 2
POOL = N_IMAGE + N_PLAIN
IMAGES = tuple(range(N_IMAGE))
PLAIN = tuple(range(N_IMAGE, POOL))
ANY = tuple(range(POOL))

CLASSES = ("fused", "chan", "up_rgba", "up_packed", "up_pair")
HAZARDS = ("RAW", "WAR", "WAW")
DEFAULT_SEED, DEFAULT_CASES = 77, 25


def job(kind, n, ins, out, ins2=None, out2=None, packed=False, planar=None, small=None):
    return dict(kind=kind, n=n, ins=list(ins), out=out, ins2=None if ins2 is None else list(ins2), out2=out2, packed=bool(packed),
                planar=[False] * n if planar is None else list(planar), small=[False] * n if small is None else list(small))


def reads(j):
    return set(j["ins"]) | set(j["ins2"] or ())


def writes(j):
    return {j["out"]} | ({j["out2"]} if j["out2"] is not None else set())


def shape(j):
    """what two consecutive jobs must have in common to share a launch (ph_run_programs: recipe, frame size and placements are the same
    for every job drawn here)"""
    if j["kind"] == "fused":
        return ("fused", j["n"])
    if j["kind"] == "chan":
        return ("chan",)
    return ("up", j["n"], j["packed"])  # (one field or two: both fit the compositor's launch)


def pair_class(a, b):
    if a["kind"] != "up":
        return a["kind"]
    if a["out2"] is not None or b["out2"] is not None:
        return "up_pair"
    return "up_packed" if a["packed"] else "up_rgba"


def hazards(a, b):
    """the hazards job b (the later one) carries against job a.  Pool buffers are separate allocations of one size, so two byte ranges
    overlap exactly when they are the same buffer."""
    found = set()
    if reads(b) & writes(a):
        found.add("RAW")
    if writes(b) & reads(a):
        found.add("WAR")
    if writes(b) & writes(a):
        found.add("WAW")
    return frozenset(found)


def classify(spec):
    """[(index of the later job, class, hazards)] for every consecutive pair of jobs of `spec` that could share a launch"""
    return [(k, pair_class(spec[k - 1], spec[k]), hazards(spec[k - 1], spec[k])) for k in range(1, len(spec)) if shape(spec[k - 1]) == shape(spec[k])]


def valid(j):
    """the job is one the library takes, and does not feed on itself"""
    ok = not (reads(j) & writes(j)) and j["out"] != j["out2"] and len(j["ins"]) == j["n"] and (j["ins2"] is None) == (j["out2"] is None)
    if j["kind"] == "up" and not j["packed"]:  # RGBA layer images: buffers with image dims
        ok = ok and all(i in IMAGES for i in j["ins"] + (j["ins2"] or []))
    if j["kind"] != "up":
        ok = ok and j["out2"] is None and not j["packed"]
    return ok and all(0 <= i < POOL for i in reads(j) | writes(j))


# ---- seeded random calls ------------------------------------------------------------------------------------------------------------
# Fifteen cells (class x hazard) have to turn up in ~100 candidate pairs, so the class of a run and what a candidate pair carries are
# dealt, not thrown: the class that has had the fewest candidate pairs so far, and within it the kind of pair that is furthest behind
# its share (ties are thrown).  Which buffers, which layer, which field, how many layers and jobs are thrown.
P_SAME_SHAPE = 0.9  # a job repeats the shape of the job in front of it: a candidate pair
# of a candidate pair: one hazard put there on purpose / buffers the earlier job does not touch / anything - and its share
SHARE = {"RAW": 1.0, "WAR": 1.0, "WAW": 1.0, "free": 1.5, "any": 0.5}


class _Decks:
    def __init__(self, r):
        self.r, self.pairs, self.dealt = r, {c: 0 for c in CLASSES}, {c: {m: 0 for m in SHARE} for c in CLASSES}

    def _least(self, score):
        low = min(score.values())
        return str(self.r.choice(sorted(k for k, v in score.items() if v == low)))

    def next_class(self):
        return self._least(self.pairs)

    def next_mode(self, cls):
        return self._least({m: self.dealt[cls][m] / SHARE[m] for m in SHARE})

    def done(self, cls, mode):
        self.pairs[cls] += 1
        self.dealt[cls][mode] += 1


def _draw_shape(r, cls):
    if cls == "fused":
        return dict(kind="fused", n=int(r.integers(1, 4)), packed=False, cls=cls)
    if cls == "chan":
        return dict(kind="chan", n=int(r.integers(1, 3)), packed=False, cls=cls)
    return dict(kind="up", n=int(r.integers(1, 3)), packed=cls == "up_packed" or (cls == "up_pair" and bool(r.random() < 0.5)), cls=cls)


def _pick(r, allowed, avoid):
    best = [i for i in allowed if i not in avoid]
    return int(r.choice(best if best else list(allowed)))


def _draw_job(r, sh, prev, mode):
    kind, n, packed = sh["kind"], sh["n"], sh["packed"]
    # a run of the two-field class: every later job has two fields (so every pair of the run is of the class), the first one may
    two = sh["cls"] == "up_pair" and (prev is not None or r.random() < 0.5)
    allowed_in = IMAGES if kind == "up" and not packed else ANY
    n_in, n_out = n * (2 if two else 1), 2 if two else 1
    ins, outs = [None] * n_in, [None] * n_out
    if mode == "RAW":
        from_prev = [i for i in writes(prev) if i in allowed_in]
        if from_prev:
            ins[int(r.integers(0, n_in))] = int(r.choice(sorted(from_prev)))
        else:  # (an RGBA layer cannot be a buffer without dims)
            mode = "WAR"
    if mode == "WAR":
        outs[int(r.integers(0, n_out))] = int(r.choice(sorted(reads(prev))))
    if mode == "WAW":
        outs[int(r.integers(0, n_out))] = int(r.choice(sorted(writes(prev))))
    # everything else: away from the earlier job where one hazard (or none) is wanted, anywhere otherwise
    away = (reads(prev) | writes(prev)) if mode in HAZARDS + ("free",) else set()
    for k in range(n_out):
        if outs[k] is None:
            outs[k] = _pick(r, ANY, away | {i for i in ins if i is not None} | {o for o in outs if o is not None})
    for k in range(n_in):
        if ins[k] is None:
            ins[k] = _pick(r, [i for i in allowed_in if i not in outs], away)
    j = job(kind, n, ins[:n], outs[0], ins[n:] if two else None, outs[1] if two else None, packed,
            planar=[kind == "chan" and bool(r.random() < 0.3) for _ in range(n)], small=[kind == "chan" and bool(r.random() < 0.5) for _ in range(n)])
    return (j, mode) if valid(j) else None


def draw_case(r, decks=None):
    """one call: 2 - 8 jobs"""
    decks = decks or _Decks(r)
    spec, sh = [], None
    for _ in range(int(r.integers(2, 9))):
        prev = spec[-1] if spec else None
        if sh is None or r.random() >= P_SAME_SHAPE:
            sh, prev = _draw_shape(r, decks.next_class()), None  # (a new run; should its shape be the last one's again, whatever comes of it)
        mode = decks.next_mode(sh["cls"]) if prev is not None else None
        drawn = None
        while drawn is None:  # (a draw that names a buffer twice where it may not is thrown again)
            drawn = _draw_job(r, sh, prev, mode)
        if prev is not None:
            decks.done(sh["cls"], drawn[1])  # (what came of it: a read-after-write that the buffers' kinds rule out becomes a write-after-read)
        spec.append(drawn[0])
    return spec


def draw_cases(seed=DEFAULT_SEED, cases=DEFAULT_CASES):
    r = np.random.default_rng(int(seed))
    decks = _Decks(r)
    return [draw_case(r, decks) for _ in range(int(cases))]


def census(specs):
    """{(class, hazard or "none"): how many candidate pairs}, candidate pairs in all"""
    count, total = {}, 0
    for spec in specs:
        for _, cls, hz in classify(spec):
            total += 1
            for h in hz or ("none",):
                count[(cls, h)] = count.get((cls, h), 0) + 1
    return count, total


# ---- directed cells -----------------------------------------------------------------------------------------------------------------
def _cell(a, b, c, slot, clash):
    """[A, B, C] twice: B with `slot` (a key, or (key, layer)) naming the buffer `clash`, and B as it stands (a buffer nobody else touches)"""
    hot = dict(b, ins=list(b["ins"]), ins2=None if b["ins2"] is None else list(b["ins2"]))
    if isinstance(slot, tuple):
        hot[slot[0]][slot[1]] = clash
    else:
        hot[slot] = clash
    return [a, hot, c], [a, b, c]


def directed_cells():
    """name -> (class, hazard, the call with the hazard, the same call without it).  A reads buffer 1 in its last layer (buffer 0
    elsewhere) and writes 2 (3: its second field); B reads 0 and writes 4 (5: its second field); C reads 0 and writes a buffer of its own -
    B's clashing argument is swapped in.  The channel cells' A reads the plain buffer 6 as a v210 frame and writes the plain buffer 7."""
    cells = {}

    def add(name, cls, hazard, a, b, c, slot, clash):
        hot, free = _cell(a, b, c, slot, clash)
        cells[name] = (cls, hazard, hot, free)

    fa, fb, fc = job("fused", 2, [0, 1], 2), job("fused", 2, [0, 0], 4), job("fused", 2, [0, 0], 6)
    add("fused-RAW", "fused", "RAW", fa, fb, fc, ("ins", 0), 2)
    add("fused-WAR", "fused", "WAR", fa, fb, fc, "out", 1)
    add("fused-WAW", "fused", "WAW", fa, fb, fc, "out", 2)
    # (every layer under the half-size placement: the channel kernel's own frames - under the fill the library hands a frame of enlarged
    # sources to the 2 x 2-block compositor, another launch)
    ca, cb, cc = job("chan", 1, [6], 7, small=[True]), job("chan", 1, [0], 4, small=[True]), job("chan", 1, [0], 5, small=[True])
    add("chan-RAW", "chan", "RAW", ca, cb, cc, ("ins", 0), 7)  # (B reads A's frame as a v210 frame: a channel routed into another)
    add("chan-WAR", "chan", "WAR", ca, cb, cc, "out", 6)
    add("chan-WAW", "chan", "WAW", ca, cb, cc, "out", 7)
    pb = job("chan", 1, [1], 4, planar=[True], small=[True])
    add("chan-RAW-chroma", "chan", "RAW", ca, pb, cc, ("ins", 0), 7)  # (B's chroma plane l0InU is A's frame)
    for packed, cls in ((False, "up_rgba"), (True, "up_packed")):
        ua, ub, uc = job("up", 1, [1], 2, packed=packed), job("up", 1, [0], 4, packed=packed), job("up", 1, [0], 5, packed=packed)
        add(cls + "-RAW", cls, "RAW", ua, ub, uc, ("ins", 0), 2)   # B's l0In is A's output
        add(cls + "-WAR", cls, "WAR", ua, ub, uc, "out", 1)        # B's output is A's l0In
        add(cls + "-WAW", cls, "WAW", ua, ub, uc, "out", 2)
        # two layers: the clash sits at layer 1
        ua, ub, uc = job("up", 2, [0, 1], 2, packed=packed), job("up", 2, [0, 0], 4, packed=packed), job("up", 2, [0, 0], 5, packed=packed)
        add(cls + "-RAW-l1", cls, "RAW", ua, ub, uc, ("ins", 1), 2)  # B's l1In is A's output
        add(cls + "-WAR-l1", cls, "WAR", ua, ub, uc, "out", 1)       # B's output is A's l1In
    # the two-field form.  A launch holds four frames, so a cell has one two-field job: B against a one-field A through its second
    # field's arguments (l0In2 / output2), and a one-field B against the second field of a two-field A
    for packed in (False, True):
        tag = "up_pair-packed" if packed else "up_pair"
        ua, ub, uc = job("up", 1, [1], 2, packed=packed), job("up", 1, [0], 4, [0], 5, packed=packed), job("up", 1, [0], 6, packed=packed)
        add(tag + "-RAW", "up_pair", "RAW", ua, ub, uc, ("ins2", 0), 2)  # B's l0In2 is A's output
        add(tag + "-WAR", "up_pair", "WAR", ua, ub, uc, "out2", 1)       # B's output2 is A's l0In
        if not packed:
            add(tag + "-WAW", "up_pair", "WAW", ua, ub, uc, "out2", 2)
    ua, ub, uc = job("up", 1, [0], 2, [1], 3), job("up", 1, [0], 4), job("up", 1, [0], 5)
    add("up_pair-RAW-field2", "up_pair", "RAW", ua, ub, uc, ("ins", 0), 3)   # B reads the frame of A's second field
    add("up_pair-WAR-field2", "up_pair", "WAR", ua, ub, uc, "out", 1)        # B's frame is the image of A's second field
    return cells
