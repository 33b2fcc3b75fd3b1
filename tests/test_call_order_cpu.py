"""The hazard generator of the call-order tests (tests/call_order.py) must not be vacuous: checked here from the specs alone, no device.
What the GPU tests (tests/test_call_order_gpu.py) then run is known to hold every kind of hazard between jobs that could share a launch -
and enough pairs without one, so that sharing itself is exercised."""
import call_order as co


def test_default_cases_hold_every_hazard_in_every_class_of_launch_sharing_jobs():
    """the default seed and number of cases: every cell of {fused, chan, compose_up RGBA, compose_up packed, compose_up two fields} x {RAW,
    WAR, WAW} at least three times among the launch-sharing candidates, at least a quarter of the candidates without any hazard"""
    specs = co.draw_cases()
    assert len(specs) == co.DEFAULT_CASES == 25 and co.DEFAULT_SEED == 77
    assert all(2 <= len(spec) <= 8 for spec in specs)
    count, total = co.census(specs)
    for cls in co.CLASSES:
        for hazard in co.HAZARDS:
            assert count.get((cls, hazard), 0) >= 3, "%s x %s: %d candidate pairs" % (cls, hazard, count.get((cls, hazard), 0))
    free = sum(1 for spec in specs for _, _, hz in co.classify(spec) if not hz)
    assert free * 4 >= total, "%d of %d candidate pairs carry no hazard" % (free, total)
    # the draw is a function of the seed
    assert specs == co.draw_cases() and specs != co.draw_cases(co.DEFAULT_SEED + 1)


def test_drawn_jobs_are_ones_the_library_takes_and_none_feeds_on_itself():
    for seed in range(20):
        for spec in co.draw_cases(seed):
            for j in spec:
                assert co.valid(j), j
                assert not (co.reads(j) & co.writes(j)), j
                if j["kind"] == "up" and not j["packed"]:  # an RGBA layer image is a buffer with image dims
                    assert all(i in co.IMAGES for i in co.reads(j)), j
    kinds = {(j["kind"], j["n"], j["packed"], j["out2"] is not None) for spec in co.draw_cases() for j in spec}
    assert {("fused", n, False, False) for n in (1, 2, 3)} <= kinds and {("chan", n, False, False) for n in (1, 2)} <= kinds
    assert {("up", n, p, two) for n in (1, 2) for p in (False, True) for two in (False, True)} <= kinds
    chan = [j for spec in co.draw_cases() for j in spec if j["kind"] == "chan"]
    assert any(any(j["planar"]) for j in chan) and any(i in co.PLAIN and not p for j in chan for i, p in zip(j["ins"], j["planar"]))


def test_classifier_names_the_hazard_of_a_pair():
    a = co.job("up", 1, [1], 2, [0], 3)
    assert co.hazards(a, co.job("up", 1, [3], 4)) == {"RAW"}
    assert co.hazards(a, co.job("up", 1, [5], 0)) == {"WAR"}
    assert co.hazards(a, co.job("up", 1, [5], 4, [5], 3)) == {"WAW"}
    assert co.hazards(a, co.job("up", 1, [2], 1)) == {"RAW", "WAR"}
    assert co.hazards(a, co.job("up", 1, [0], 4)) == frozenset()  # (two readers of one image: no hazard)
    # pairs that cannot share a launch are no candidates: another kind, another layer count, another image format
    spec = [co.job("fused", 2, [0, 1], 2), co.job("fused", 1, [2], 3), co.job("chan", 1, [3], 4), co.job("chan", 2, [4, 4], 5),
            co.job("up", 1, [5], 0), co.job("up", 1, [0], 1, packed=True), co.job("up", 1, [1], 2, [1], 3, packed=True)]
    assert co.classify(spec) == [(3, "chan", frozenset({"RAW"})), (6, "up_pair", frozenset({"RAW"}))]


def test_directed_cells_carry_exactly_the_hazard_they_are_named_for():
    """[A, B, C]: B has exactly one hazard against A, C is independent of both and of the same shape; the hazard-free twin of the call has none"""
    cells = co.directed_cells()
    for cls in co.CLASSES:
        for hazard in co.HAZARDS:
            assert any(c == cls and h == hazard for c, h, _, _ in cells.values()), (cls, hazard)
    for name, (cls, hazard, hot, free) in cells.items():
        assert all(co.valid(j) for j in hot + free), name
        found = co.classify(hot)
        assert [k for k, _, _ in found] == [1, 2], name  # (all three of one shape)
        assert found[0][1:] == (cls, frozenset({hazard})), (name, found)
        assert not found[1][2] and not co.hazards(hot[0], hot[2]), name
        assert all(not hz for _, _, hz in co.classify(free)) and not co.hazards(free[0], free[2]), name
        changed = [k for k in ("ins", "ins2", "out", "out2") if hot[1][k] != free[1][k]]
        assert len(changed) == 1 and hot[0] == free[0] and hot[2] == free[2], name  # (one argument of B is all that differs)
    # the compositor's ground: layer 1 as the clashing argument, both fields' arguments, both image formats
    for name in ("up_rgba-RAW-l1", "up_rgba-WAR-l1", "up_packed-RAW", "up_packed-WAR", "up_packed-RAW-l1", "up_pair-RAW", "up_pair-WAR",
                 "up_pair-packed-RAW", "up_pair-packed-WAR", "up_pair-RAW-field2", "up_pair-WAR-field2", "chan-RAW-chroma"):
        assert name in cells
