"""pta_dgemm on every case of tests/gemm_cases.py, on the NaN slabs of tests/gemm_reference.py: bit equality with the int64 product on
integer operands, the derived elementwise bound against a long double reference on real ones, and every element the call must not
write bit-identical to its pre-image.  The idft and clnl forms run their calls in the callers' order on one allocation.  Each call
is first asked of pta_dgemm_plan with the byte offsets of the pointers it really passes, so a case cannot drift to another kernel
unnoticed.  The last test prints the worst error over the bound per kernel instance."""
import ctypes

import numpy as np
import pytest

import gemm_cases as gc
import gemm_reference as gr

pytestmark = pytest.mark.gpu

WORST = {}          # kernel instance -> (worst error / bound, case)
EXACT = {}          # kernel instance -> calls held to bit equality


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(torch=torch, lib=_lib, dv=dv, s=dv.stream_ptr())


def run_case(gpu, case, kind):
    torch, lib = gpu["torch"], gpu["lib"]
    slab = gr.Slab(case, kind)
    for i, c in enumerate(case["calls"]):
        pre = slab.prepare(i)
        d = torch.from_numpy(pre).to("cuda")
        base = d.data_ptr()
        assert base % 16 == 0 and d.numel() == slab.size
        at = {k: base + 8 * (slab.base[c[k]["reg"]] + c[k]["off"]) for k in "ABC"}
        A, B, C = c["A"], c["B"], c["C"]
        p = lib.launch_plan("pta_dgemm", c["transB"], c["M"], c["N"], c["K"], A["ld"], A["sk"], B["ld"], A["stride"], B["stride"], at["A"] % 16,
                            at["B"] % 16, c["lower"], c["algo"], c["batch"])
        kernel = gc.DGEMM_KERNELS[p["kernel"]]
        assert kernel == c["expect"]["kernel"] and gc.DGEMM_LOWER[p["lower_mode"]] == c["expect"].get("lower_mode", gc.DGEMM_LOWER[p["lower_mode"]])
        alpha, beta = gr.scalars(c, kind)
        lib.call("pta_dgemm", c["transB"], c["M"], c["N"], c["K"], alpha, ctypes.c_void_p(at["A"]), A["ld"], A["sk"], ctypes.c_void_p(at["B"]), B["ld"],
                 beta, ctypes.c_void_p(at["C"]), C["ld"], c["lower"], c["batch"], A["stride"], B["stride"], C["stride"], c["algo"], gpu["s"])
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        worst = slab.check(i, pre, got)
        if kind == "bound":
            print(f"{case['name']} call {i}: {kernel} worst error / bound {worst:.4f}")
            if worst >= WORST.get(kernel, (-1.0, ""))[0]:
                WORST[kernel] = (worst, case["name"])
        else:
            EXACT[kernel] = EXACT.get(kernel, 0) + 1


@pytest.mark.parametrize("case", gc.CASES, ids=[c["name"] for c in gc.CASES])
def test_dgemm_bit_equal_to_the_integer_product(gpu, case):
    run_case(gpu, case, "exact")


@pytest.mark.parametrize("case", [c for c in gc.CASES if not c["deep"]], ids=[c["name"] for c in gc.CASES if not c["deep"]])
def test_dgemm_inside_the_derived_bound(gpu, case):
    run_case(gpu, case, "bound")


def test_worst_ratio_per_instance(gpu):
    """the figures DESIGN.md 4.19 quotes, over everything the two tests above ran in this process (an instance they did not run here,
    as when this test is selected alone, runs its first case now)"""
    for k in gc.DGEMM_KERNELS:
        for kind, seen in (("exact", EXACT), ("bound", WORST)):
            if k not in seen:
                run_case(gpu, next(c for c in gc.CASES if not c["deep"] and c["calls"][0]["expect"]["kernel"] == k), kind)
    for k in gc.DGEMM_KERNELS:
        print(f"{k}: worst error / bound {WORST.get(k, (np.nan, ''))[0]:.4f} ({WORST.get(k, (0, 'not run'))[1]}), {EXACT.get(k, 0)} calls bit-exact")
    assert set(WORST) == set(gc.DGEMM_KERNELS) and set(EXACT) == set(gc.DGEMM_KERNELS)
    assert all(0.0 <= w <= 1.0 for w, _ in WORST.values())
