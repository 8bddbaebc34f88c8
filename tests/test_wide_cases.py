"""The designed cases of tests/wide_cases.py, without a GPU: the oracle alone admits every one of them, every tile case
reaches the search-tile size it is named for, and the host plan of the fused step (glh_point_plan.h: pt_plan, compiled
for the CPU by tests/hostcheck) takes exactly the cases the module calls fused.  The device runs of the same cases:
tests/test_gpu_wide_cases.py."""
import pytest

from tests import wide_cases as wc
from tests.test_hostcheck import _plan, hc  # noqa: F401  (hc: the fixture that builds tests/hostcheck)


@pytest.mark.parametrize("name", wc.NAMES)
def test_the_oracle_admits_the_case_at_its_size(name):
    """option_cases.admit_case: equal indices with the SSD accumulated in float64 and row-wise in float32, no track
    raises, no search box leaves its frame; P = 2, T = 3; a tile case's largest search tile lies in its size class (for
    u16_250 that includes 60 000 <= n <= 65 025, for u16rgb_1117 a width of at least 1100) and inside the context's
    workspace; a count case keeps the narrow prior's small tiles."""
    cs, a = wc.case(name), wc.admit(name)
    assert a["ok"], f"{name}: {a['why']} -- give the case another seed (tests/wide_cases.py) and record it there"
    assert cs["P"] == 2 and cs["T"] == 3 and a["ref"]["idx"].shape == (2, 2, cs["N"])
    w, h = wc.largest_tile(a["run"])
    sizes = sorted({(step, tw, th) for step, _, _, tw, th in wc.tiles_reached(a["run"])})
    print(f"{name}: N {cs['N']}, frames {cs['imgsz']} {cs['ftype']} x{cs['channels']}, largest search tile {w} x {h} "
          f"({w * h} px), (step, w, h) {sizes}, f64 / row_f32 moments within rtol {a['spread']:.1e}")
    assert all(max(tw, th) <= cs["max_search_dim"] for _, tw, th in sizes)
    assert max(cs["imgsz"]) <= (1280 if name == "u16rgb_1117" else 640)
    if name in wc.TILE_CASES:
        assert 500 <= cs["N"] <= 1500
        assert wc.in_class(name, w, h), (name, w, h, wc.SIZE_CLASS[name])
    else:
        assert max(w, h) <= 48 and cs["tile"] == (15, 15) and cs["ftype"] == "uint8" and cs["channels"] == 1


def test_the_table_of_tile_cases_is_what_the_module_says():
    """Every frame type with one channel and with three; one 31 x 31 and one 47 x 47 template, 15 x 15 otherwise; a 7 x 7
    window with 'wrap'; orders (1, 1) once; the 16-bit and float cases above a 255-pixel workspace are the staged ones."""
    specs = wc.TILE_CASES
    assert {(s["ftype"], s["channels"]) for s in specs.values()} == {(t, c) for t in wc.oc.FRAME_TYPES for c in (1, 3)}
    tiles = sorted(s["tile"] for s in specs.values())
    assert tiles.count((31, 31)) == 1 and tiles.count((47, 47)) == 1 and tiles.count((15, 15)) == len(tiles) - 2
    assert specs["u8rgb_300x70"]["window"] == (7, 7) and specs["u8rgb_300x70"]["mode"] == "wrap"
    assert [n for n, s in specs.items() if s["interp"] == (1, 1)] == ["f64_260"]
    staged = {n for n, s in specs.items() if s["ftype"] != "uint8" and s["max_search_dim"] > 255}
    assert staged == set(specs) - set(wc.FUSED_TILE_CASES)
    assert set(wc.SIZE_CLASS) == set(specs)
    assert wc.SIZE_CLASS["u16_250"]["n"] == (60000, 65025) and wc.SIZE_CLASS["u16rgb_1117"]["w"][0] >= 1100


@pytest.mark.parametrize("name", wc.NAMES)
def test_the_plan_takes_exactly_the_fused_cases(hc, name):  # noqa: F811
    cs = wc.case(name)
    frames, k = wc.plan_frames(cs)
    got = _plan(hc, cs["N"], len(cs["cams"]), tile=cs["tile"], frames=frames, interp_k=k)
    print(f"{name}: pt_plan {got}")
    assert bool(got[0]) == (name in wc.FUSED), (name, got)
    if not got[0]:
        assert got == (0, 0, 0, 0, 0, 0)
    if name == "n10976":
        assert got[1:3] == (1024, 0)  # the shape (1024, 0, 1)


def test_the_particle_limits_are_the_plans_and_glh_creates(hc):  # noqa: F811
    """FUSED_LAST is what pt_plan gives for the count cases' context (15 x 15 templates, one-channel 8-bit frames, no
    rasters) with one observer and with two, rasters lower it; CREATE_LAST is what the check of glh_create gives.  Over
    the four counts: accepted up to 10 976, refused from 10 977, and 14 951 is beyond glh_create."""
    def plan(n, o, tile, rasters):
        return _plan(hc, n, o, tile=tile, frames=(8, 1, 160), rasters=rasters)

    last = {(o, r): wc.fused_last(plan, o, r) for o in (1, 2) for r in (0, 1)}
    print(f"last particle count pt_plan accepts (observers, rasters): {last}; glh_create: {wc.create_last()}")
    assert last[1, 0] == last[2, 0] == wc.FUSED_LAST == 10976
    assert last[1, 1] == last[2, 1] == 10740
    assert wc.create_last() == wc.CREATE_LAST == 14950
    counts = sorted({wc.COUNT_CASES[n]["N"] for n in wc.COUNT_CASES})
    assert counts == [wc.FUSED_LAST, wc.FUSED_LAST + 1, 12000, wc.CREATE_LAST]
    for n in counts:
        for o in (1, 2):
            assert bool(plan(n, o, (15, 15), 0)[0]) == (n <= wc.FUSED_LAST), (n, o)
    assert wc.COUNT_CASES["n14950x2"]["observers"] == 2
    assert not wc.create_refuses(14950) and wc.create_refuses(14951)  # (the device test asks glh_create itself)
