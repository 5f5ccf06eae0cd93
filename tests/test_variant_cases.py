"""The recipes of tests/variant_cases.py, checked without a GPU: every recipe reaches the kernel variant it names, the recipes name exactly the compiled variants (the 46
single-plan rows of the selection and the 8 merged-panel kernels), and every recipe's plan holds what its variant exists for.

What a recipe's plan LAUNCHES is asserted on the device (tests/test_variant_exact_gpu.py: Plan.kernel_variant() / Plan.panels_kernel() of the uploaded plan); here the nine
key bits are formed from the pure launch-shape function for a device of 256 CUs and the plan's own counters, and handed to the selection."""
import importlib.util
import os

import pytest

import launch_shape_cases as LC
import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = [r["id"] for r in V.RECIPES if r["kind"] != "merged"]
MERGED = [r["id"] for r in V.RECIPES if r["kind"] == "merged"]


def chosen(dasp, precision, bits):
    return dasp._lib.lib().dasp_debug_spmv_variant(precision, bits).decode()


@pytest.mark.parametrize("rid", SINGLE)
def test_recipe_reaches_its_variant(dasp, rid):
    """single plans, and every panel of the plans whose panels are launched one by one"""
    r = V.recipe(rid)
    with LC.knobs(r["env"]):
        plan = V.build(dasp, r)
        views = V.views(plan, r)
        assert views and (r["kind"] == "single") == (plan.n_panels == 0)
        for k, view in enumerate(views):
            bits = V.key_bits(dasp, view)
            assert chosen(dasp, r["precision"], bits) == r["variant"], (k, dict(zip(V.KEY, [bits >> i & 1 for i in range(len(V.KEY))])))
        plan.close()


@pytest.mark.parametrize("rid", MERGED)
def test_merged_recipe_has_panels_that_merge(dasp, rid):
    """at most kMaxMergedPanels panels that share one id width, one load policy and one medium stride, none windowed or with one-byte ids (kernels.hip
    select_panels_variant; the uploaded parent is asked on the device): each by itself would run the row-tile kernel of the same <T,nt,c16>"""
    r = V.recipe(rid)
    with LC.knobs(r["env"]):
        plan = V.build(dasp, r)
        views = V.views(plan, r)
        assert 1 < len(views) <= V.MAX_MERGED
        strides = set()
        for view in views:
            st = view.stats
            assert st["x_window_on"] == 0 and st["cid8_chunks"] == 0 and st["two_phase"] == 0 and view.n_panels == 0
            strides.add(V.shape_field(dasp, view.launch_shape(cus=256, f16_resident=7), "med_stride"))
            assert chosen(dasp, r["precision"], V.key_bits(dasp, view)).replace("dasp_spmv_rt_kernel<", "dasp_spmv_panels_kernel<") == r["variant"]
        assert len(strides) == 1
        plan.close()


@pytest.fixture(scope="module")
def compiled():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return set(m.report())


def test_recipes_name_exactly_the_compiled_variants(dasp, compiled):
    """both directions: no variant without a recipe, no recipe for a name that is not a variant"""
    table = {chosen(dasp, precision, bits) for precision in (64, 16) for bits in range(1 << len(V.KEY))}
    single = {r["variant"] for r in V.RECIPES if r["kind"] != "merged"}
    merged = {r["variant"] for r in V.RECIPES if r["kind"] == "merged"}
    assert len(table) == 46 and single == table, (sorted(table - single), sorted(single - table))
    panels = {k for k in compiled if k.startswith("dasp_spmv_panels_kernel<")}
    assert len(panels) == 8 and merged == panels, (sorted(panels - merged), sorted(merged - panels))
    assert single | merged <= compiled
    print("\n".join(sorted(single | merged)))
    assert len(single | merged) == 46 + 8 and len(V.IDS) == 46 + 8 + 2          # (+ the second recipe of the two shared-id kernels)


@pytest.mark.parametrize("rid", V.IDS)
def test_recipe_plan_holds_what_its_variant_is_for(dasp, rid):
    r = V.recipe(rid)
    plan = V.build(dasp, r)
    V.taken(r)(plan)
    plan.close()


def test_every_non_temporal_recipe_has_a_plain_load_twin():
    """the pairs the policy-after-upload test of the device file walks: every nt = 1 recipe differs from an nt = 0 recipe in stream_policy only"""
    nt1 = [r for r in V.RECIPES if V.nt_of(r) == 1]
    assert len({r["variant"] for r in nt1}) == 21 + 4 and len(nt1) == 21 + 4 + 1
    for r in nt1:
        q = V.plain_load_twin(r)
        assert q is not None and V.nt_of(q) == 0 and q["id"] != r["id"], r["id"]


def test_panels_kernel_needs_an_uploaded_parent(dasp):
    plan = V.build(dasp, V.recipe(MERGED[0]))
    with pytest.raises(dasp.DaspError) as e:
        plan.panels_kernel()
    assert e.value.status == -22 and "not uploaded" in str(e.value)
    plan.close()
