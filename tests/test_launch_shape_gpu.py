"""A plan's launch shape on the device: for every case of launch_shape_cases.py, what the uploaded plan carries is what the pure function decides from the device's own
two facts, both are the recording where the device has the recording's CU count, and one SpMV of the plan is the CSR product (the suite's standing bounds: 1e-12 (f64) /
1e-2 (f16) of sum |a_ij x_j| against the CPU oracle)."""
import numpy as np
import pytest

import launch_shape_cases as LC

TOL = {64: 1e-12, 16: 1e-2}
_ref = {}


def reference(oracle, case):
    """x, the oracle's product and sum |a_ij x_j| in the plan's precision: once per (matrix, precision), shared, read-only"""
    key = (case["matrix"], case["precision"])
    if key not in _ref:
        rp, ci, v, n = LC.matrix(case["matrix"])
        dt = np.float64 if case["precision"] == 64 else np.float16
        x = np.random.default_rng(77).uniform(0.5, 1.5, n).astype(dt)
        v64, x64 = v.astype(dt).astype(np.float64), x.astype(np.float64)
        _ref[key] = (x, oracle.csr_spmv(rp, ci, v64, x64), oracle.csr_absrow(rp, ci, v64, x64))
        for a in _ref[key]:
            a.setflags(write=False)
    return _ref[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in LC.CASES])
def test_uploaded_shape_is_the_pure_function_and_the_recording(dasp, oracle, torch_cuda, name):
    torch = torch_cuda
    case, g = next(c for c in LC.CASES if c["name"] == name), LC.golden()[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with LC.knobs(case["env"]):
        plan, view = LC.build(dasp, case)
        res = int(dasp._lib.lib().dasp_debug_f16_resident(int(view.stats["cid16_on"])))
        before = view.launch_shape(cus=cus, f16_resident=res)
        plan.upload()
        if case["policy_after"] is not None:
            before = None
            plan.set_stream_policy(case["policy_after"])
        carried = view.launch_shape(uploaded=True)
        assert carried == view.launch_shape(cus=cus, f16_resident=res) and before in (None, carried)
        if cus == g["cus"] and res == g["f16_resident"]:
            assert carried == g["shape"]
        x_h, ref, scale = reference(oracle, case)
        tdt = torch.float64 if case["precision"] == 64 else torch.float16
        x = torch.from_numpy(x_h.copy()).cuda()
        y = torch.zeros(plan.rowA, dtype=tdt, device="cuda")
        plan.spmv(x.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = y.double().cpu().numpy()
        at = np.arange(plan.rowA) if plan.y_order == dasp.Y_NATURAL else plan.order_rid
        err = np.abs(got - ref[at])
        assert (err <= TOL[case["precision"]] * np.maximum(scale[at], 1e-300)).all(), float(err.max())
        plan.close()
