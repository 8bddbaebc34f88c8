"""The recipe table of tests/launch_shape_cases.py, checked without a GPU: it maps every instantiation the build carries to
a case, its flag mapping is pt_code's expression (glh_point_plan.h), its particle counts select the shapes it names, and the
cases compared with the oracle index for index pass the admission rule (both accumulations of the SSD give the same
indices).  tests/test_hostcheck.py runs the compiled pt_plan / pt_code against the same table."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import launch_shape_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pt_shape(n, o):
    """glh_point_plan.h: pt_shape, restated (tests/test_hostcheck.py pins the compiled one at the same counts)."""
    big = n > 10 * 512
    tb = 1024 if big else 512
    p = 4 if n <= 4 * tb else (10 if n <= 10 * tb else 0)
    if (big or o == 2) and p == 4:
        p = 10
    if (big and p != 10) or o >= 3:
        p = 0
    return tb, p


def test_the_table_accounts_for_every_instantiation_the_build_carries():
    from glimpse_amd import build

    carried = set(build.variants())
    assert len(carried) == len(build.variants()) == 88
    covered = lc.covered()
    unreachable = set(lc.UNREACHABLE)
    assert not covered & unreachable
    assert not (covered | unreachable) - carried, sorted((covered | unreachable) - carried)
    missing = carried - covered - unreachable
    assert not missing, f"instantiations without a case: {sorted(missing)}"
    for why in lc.UNREACHABLE.values():
        assert re.search(r"pt_(plan|code)", why), why
    print(f"{len(carried)} instantiations: {len(covered)} mapped to a case, {len(unreachable)} documented unreachable")
    # every shape runs all eight codes, and the table names every shape once
    shapes = [shape for shape, _ in lc.SHAPES]
    assert len(set(shapes)) == len(shapes) == 11
    for shape in shapes:
        assert len(lc.instantiations(shape)) + sum(u[:3] == shape for u in unreachable) == 8, shape


def test_the_counts_select_the_shapes_they_are_listed_under():
    for (tb, ppt, o), counts in lc.SHAPES:
        for n in counts:
            assert _pt_shape(n, o) == (tb, ppt), (n, o)
    for shape, q in lc.ORACLE_CASES.items():
        assert _pt_shape(q["N"], shape[2]) == shape[:2] and q["N"] in dict(lc.SHAPES)[shape]
    # the edges: each neighbour across a threshold is listed too, under the other shape
    listed = {(n, shape[2]) for shape, counts in lc.SHAPES for n in counts}
    assert {(2048, 1), (2049, 1)} <= listed
    for o in (1, 2, 3, 4):
        assert {(5120, o), (5121, o)} <= listed, o
    for o in (1, 2):
        assert {(10240, o), (10241, o)} <= listed, o
    # the five shapes no other GPU test launches are the ones compared with the oracle
    assert set(lc.ORACLE_CASES) == {(1024, 0, 1), (1024, 0, 2), (1024, 0, 3), (1024, 0, 4), (1024, 10, 2)}


def test_the_flag_mapping_is_the_expression_of_fused_step():
    """`rast ? 2 : surf ? 1 : 0`, `fast`, `surf ? common : fast` over every flag word, and the text of that expression in
    the source (glh_point_plan.h: pt_code, which fused_step launches by); the codes the recipe expects are codes the
    header lists."""
    for fast, surf, common, rast in itertools.product((0, 1), repeat=4):
        flags = fast | surf << 1 | common << 2 | rast << 3
        want = ((2 if rast else (1 if surf else 0)), fast, (common if surf else fast))
        assert lc.flags_to_code(flags) == want, flags
    src = open(os.path.join(ROOT, "glimpse_amd", "csrc", "glh_point_plan.h")).read()
    assert "PtCode{rast ? 2 : (surf ? 1 : 0), fast, surf ? common : fast," in src
    assert "(fast ? 1 : 0) | (surf ? 2 : 0) | (common ? 4 : 0) | (rast ? 8 : 0)" in src
    hip = open(os.path.join(ROOT, "glimpse_amd", "csrc", "glimpse_hip.hip")).read()
    assert "pt_kernel(plan.tb, plan.ppt, O, code.surf, code.fast, code.con)" in hip
    assert "c->last_variant[3] = code.flags;" in hip
    # the recipe's table (configuration x arithmetic x step), written out: one observer and several
    table = {("plain", "exact"): [(0, 0, 0)] * 3, ("general", "exact"): [(1, 0, 0)] * 3, ("rasters", "exact"): [(2, 0, 0)] * 3,
             ("plain", "fast"): [(1, 1, 0), (0, 1, 1), (0, 1, 1)], ("general", "fast"): [(1, 1, 0), (1, 1, 1), (1, 1, 1)],
             ("rasters", "fast"): [(2, 1, 0), (2, 1, 1), (2, 1, 1)]}
    for (config, math), codes in table.items():
        assert [lc.expected_code(config, math, s, 1) for s in (1, 2, 3)] == codes
        # (frame 2 of several observers: the last one has no image -- not the contract's input)
        several = [codes[0], codes[0] if math == "fast" else codes[1], codes[2]]
        assert [lc.expected_code(config, math, s, 3) for s in (1, 2, 3)] == several


@pytest.mark.parametrize("shape", sorted(lc.ORACLE_CASES), ids=lambda s: "x".join(map(str, s)))
def test_oracle_compared_cases_pass_the_admission_rule(shape):
    """Both accumulations of the SSD give the same resample indices at every step of every point and no search box leaves
    its frame: the committed scene seed is admitted (about a second per shape, most of it rendering the frames)."""
    a = lc.admit(shape)
    assert a["ok"], a["why"]
    q = lc.ORACLE_CASES[shape]
    assert a["ref"]["idx"].shape == (lc.ORACLE_T - 1, q["P"], q["N"])
    assert np.isfinite(a["ref"]["means"]).all()
