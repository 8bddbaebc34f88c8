"""The admission rule of tests/option_cases.py over the committed seed list: the oracle alone decides which cases the
device sweep (tests/test_gpu_option_sweep.py) runs, and the list covers the option space."""
import collections

from tests import option_cases as oc

COUNT = 40


def test_the_rule_admits_the_committed_seeds_and_they_cover_the_option_space():
    seeds, skipped = oc.admitted(COUNT)
    # every seed in the list passes, and the list is what the generator's own rule yields
    assert len(oc.SEEDS) == COUNT
    for seed in oc.SEEDS:
        a = oc.admit(seed)
        assert a["ok"], f"seed {seed}: {a['why']}"
    assert seeds == tuple(oc.SEEDS), (seeds, skipped)
    # at most a quarter of the seeds tried were skipped to fill the list
    tried = len(seeds) + len(skipped)
    print(f"{len(skipped)} of {tried} seeds skipped: {[(s, oc.admit(s)['why']) for s in skipped]}")
    assert 4 * len(skipped) <= tried
    # every value of every axis at least twice, every frame type with every boundary mode at least once
    count = collections.defaultdict(collections.Counter)
    pairs = collections.Counter()
    facts = {}
    for seed in seeds:
        cs = oc.case(seed)
        for axis, value in oc.axes(cs).items():
            count[axis][value] += 1
        pairs[cs["ftype"], cs["mode"]] += 1
        facts[seed] = dict(oc.admit(seed)["facts"], ftype=cs["ftype"], tile=cs["tile"], interp=cs["interp"])
        assert cs["window"] != (1, 1) and all(7 <= v for v in cs["tile"])
        assert cs["P"] == 3 and cs["T"] == 4 and all(300 <= v <= 520 for v in cs["imgsz"])
    for axis, values in oc.AXIS_VALUES.items():
        print(axis, dict(count[axis]))
        for value in values:
            assert count[axis][value] >= 2, (axis, value, dict(count[axis]))
    for ftype in oc.FRAME_TYPES:
        for mode in oc.MODES:
            assert pairs[ftype, mode] >= 1, (ftype, mode)
    # the places where the kernels branch
    assert sum(f["ftype"] == "uint16" and f["frame_levels"] < 1024 for f in facts.values()) >= 1
    assert sum(f["ftype"] in ("float32", "float64") and f["template_repeats"] > 40 for f in facts.values()) >= 1
    assert sum(49 <= max(f["tile"]) <= 63 for f in facts.values()) >= 2
    assert sum(max(f["tile"]) > 63 for f in facts.values()) >= 1
    assert sum(f["max_surface"] > 40 for f in facts.values()) >= 1  # the banded spline fit
    half = sum(f["interp"] in oc.FUSED_ORDERS for f in facts.values())
    assert COUNT // 2 <= half <= COUNT * 5 // 8, half


def test_existing_callers_of_the_oracle_keep_the_default_window():
    """An Observer without the high-pass options, and a plain dict as older callers pass it, take the 5 x 5 'reflect'
    median: the same tiles as extract_tile's defaults."""
    import numpy as np

    from oracle import tiles as otiles
    from oracle import tracker as otracker

    cs = oc.case(oc.SEEDS[0])
    frame, cam = cs["frames"][0][0], cs["cams"][0]
    obs = otracker.Observer([frame], cam[None], 0.3)
    assert obs["highpass_size"] == (5, 5) and obs["highpass_mode"] == "reflect"
    assert otracker.Observer([frame], cam[None], 0.3, highpass_size=3)["highpass_size"] == (3, 3)
    xyz = np.array([cs["params"][0, 0], cs["params"][0, 1], 0.0])
    t = otiles.initialize_template(frame, cam, xyz, (15, 15))
    tile, hist = otiles.extract_tile(frame, t["box"], return_histogram=True)
    np.testing.assert_array_equal(t["tile"], tile)
    other = otiles.initialize_template(frame, cam, xyz, (15, 15), highpass_size=(7, 3), highpass_mode="wrap")
    want, _ = otiles.extract_tile(frame, t["box"], return_histogram=True, highpass_size=(7, 3), highpass_mode="wrap")
    np.testing.assert_array_equal(other["tile"], want)
    assert not np.array_equal(other["tile"], tile)
    particles = np.array([xyz + (0.01, 0.0, 0.0), xyz - (0.01, 0.02, 0.0)])
    particles = np.column_stack((particles, np.zeros((2, 3))))
    plain = {"frames": [frame], "cams": cam[None], "sigma": 0.3}
    np.testing.assert_array_equal(otracker.observer_log_likelihoods(plain, 0, t, particles),
                                  otracker.observer_log_likelihoods(obs, 0, t, particles))
