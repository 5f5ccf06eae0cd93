"""The compiled form of dasp_tp_reduce_exact_kernel (the exact phase 2 of the two-phase form), read from the gfx950 code object the way
tests/test_isa_guard.py does: compile-only, no GPU.  What the kernel's cost model rests on: its sums go to LDS as native no-return 64-bit integer adds
(two per run), never as a compare-and-swap loop, and nothing spills."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "dasp_tp_reduce_exact_kernel"


@pytest.fixture(scope="module")
def tool():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def listing(tool):
    """the instructions of the kernel, one mnemonic + operands per entry"""
    with tempfile.TemporaryDirectory() as work:
        co = tool.code_object(os.path.join(ROOT, "dasp_amd", "csrc", "build", "kernels.o"), work)
        txt = subprocess.run([os.path.join(tool.LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    secs = [s for s in re.split(r"\n(?=[0-9a-f]+ <)", txt) if KERNEL in s.split("\n", 1)[0]]
    assert len(secs) == 1, [s.split("\n", 1)[0] for s in secs]
    return [line.strip() for line in secs[0].splitlines()[1:] if line.startswith("\t")]


def test_no_scratch_and_the_workgroup_it_is_launched_with(tool):
    rows = tool.report()
    assert KERNEL in rows, sorted(k for k in rows if "tp_" in k)
    r = rows[KERNEL]
    assert r["private_segment_fixed_size"] == 0 and r["scratch"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["max_flat_workgroup_size"] == 512 and r["vgpr_count"] <= 128, r                  # 512 threads: 2 waves per SIMD, 128 registers each
    assert r["mfma"] == 0 and r["flat"] == 0 and r["s_barrier"] == 2 and r["group_segment_fixed_size"] == 0, r      # streams with global loads; LDS is dynamic
    # the atomic form beside it is untouched: what tests/test_isa_guard.py asserts of it still holds in this build
    assert rows["dasp_tp_reduce_kernel<half>"]["s_barrier"] == 2 and rows["dasp_tp_reduce_kernel<half>"]["scratch"] == 0


def test_sums_are_64_bit_lds_integer_adds_without_a_compare_and_swap_loop(listing):
    adds = [l for l in listing if re.match(r"ds_add_u64\b", l)]
    assert len(adds) >= 2 and len(adds) % 2 == 0, adds                                          # (high, low) pairs
    assert not [l for l in listing if re.match(r"ds_add_rtn_u64\b", l)]                         # no-return form: nothing waits for the old value
    assert not [l for l in listing if re.match(r"ds_(cmpst|cmpswap|cmpstore)", l)], "a compare-and-swap loop stands in for an LDS atomic"
    assert not [l for l in listing if re.match(r"ds_add(_rtn)?_f(32|64)\b", l)]                  # no floating-point accumulator is left
    assert [l for l in listing if re.match(r"ds_or_b32\b", l)]                                  # the sticky flags of non-finite products
    # the streams: three 16-byte loads per lane and step, as in the atomic form
    assert len([l for l in listing if re.match(r"global_load_dwordx4\b", l)]) >= 3
