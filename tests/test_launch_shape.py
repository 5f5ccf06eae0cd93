"""A plan's launch shape (launch_shape.cpp: workgroup ranges, striding, dispatch order, tiles per wave, written-through y, the kernel table's flags), without a GPU.

The expected values are tests/golden/launch_shapes.json: what uploads on an MI355X decided before the rules were gathered into one function (launch_shape_cases.py).  For
every case the pure function, given the recorded facts about the device, must give the recorded ints exactly."""
import numpy as np
import pytest

import launch_shape_cases as LC

NAMES = [c["name"] for c in LC.CASES]
N_INTS = sum(n for _, n in __import__("dasp_amd").SHAPE_FIELDS)


def field(seq, name):
    at = 0
    for f, n in __import__("dasp_amd").SHAPE_FIELDS:
        if f == name:
            return seq[at] if n == 1 else seq[at:at + n]
        at += n
    raise KeyError(name)


@pytest.fixture(scope="module")
def golden():
    return LC.golden()


def test_recording_covers_every_case_and_every_branch(golden):
    assert sorted(golden) == sorted(NAMES)
    for c in LC.CASES:
        g = golden[c["name"]]
        assert g["options"] == c["options"] and g["env"] == c["env"] and g["panel"] == c["panel"] and g["precision"] == c["precision"] and g["matrix"] == c["matrix"], c["name"]
        assert len(g["shape"]) == N_INTS == 60 and g["cus"] == 256
    seen = {f: {tuple(np.atleast_1d(field(g["shape"], f)).tolist()) for g in golden.values()} for f, _ in __import__("dasp_amd").SHAPE_FIELDS}
    for f in ("nt", "win1", "seven_waves", "long16", "shared_ids", "med_stride", "xcd_on", "ywt", "win_xcd"):          # every flag is seen both ways
        assert {(0,), (1,)} <= seen[f], f
    assert {(1,), (4,)} <= seen["short_tpw"] and len(seen["wg_rot"]) >= 3 and len(seen["win_tiles"]) >= 2 and len(seen["wg_rt"]) >= 2 and len(seen["wpw"]) >= 3
    assert golden["f16_uniform_above_persistent"]["shape"][7] == 256 * 7 and golden["f16_uniform_below_persistent"]["shape"][7] == 1790      # the persistent set, and one block per wave


@pytest.mark.parametrize("name", NAMES)
def test_pure_function_gives_the_recorded_shape(dasp, golden, name):
    case, g = next(c for c in LC.CASES if c["name"] == name), golden[name]
    with LC.knobs(case["env"]):
        plan, view = LC.build(dasp, case)
        if case["policy_after"] is not None:
            plan.set_stream_policy(case["policy_after"])
        got = view.launch_shape(cus=g["cus"], f16_resident=g["f16_resident"])
        assert got == g["shape"], [(f, field(got, f), field(g["shape"], f)) for f, _ in dasp.SHAPE_FIELDS if field(got, f) != field(g["shape"], f)]
        if view.stats["x_window_on"]:          # a device of 4 CUs: only win1 may move, and it is "at most one window workgroup per CU" (and never on under DASP_WIN1=0)
            small = view.launch_shape(cus=4, f16_resident=g["f16_resident"])
            want = list(g["shape"])
            want[1] = int(view.stats["n_windows"] <= 4 and case["env"].get("DASP_WIN1", "1") != "0")
            assert small == want
        if name == "f16_uniform_above_persistent":      # the persistent set is CUs x resident workgroups, at most 7 per CU, 7 where the occupancy is unknown
            for cus, res, wg in ((256, 5, 1280), (256, 0, 1792), (256, 9, 1792), (100, 7, 700)):
                assert field(view.launch_shape(cus=cus, f16_resident=res), "wg_med") == wg
        plan.close()


def test_shape_of_a_plan_that_is_not_uploaded(dasp):
    rp, ci, v, n = LC.matrix("mixed")
    plan = dasp.Plan(rp, ci, v, n)
    with pytest.raises(dasp.DaspError) as e:
        plan.launch_shape(uploaded=True)
    assert e.value.status == -22 and "not uploaded" in str(e.value)
    plan.close()
