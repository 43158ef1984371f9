#!/usr/bin/env python3
"""(Test infrastructure: run as a child process by tests/test_gpu_wgrad_h16.py under the kernel-selection switches, which the
library reads once at load.) Runs the named variant of tests/wgrad_h16_cases.py: asserts, through yolo_switches_describe and
yolo_wgrad_plan, that the environment took effect (the kernel, the slices and the look-ahead the restatement gives for that
environment), then the exact and the random assertion of the GPU test on every named case in bf16 and fp16. One line per case and
dtype: ``case <name> <dtype> <kernel> slices=<n> per_slice=<n> G=<n> variant=<n> rel_err=<e> ok``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _switches(lib):
    import ctypes as C
    need = lib.yolo_switches_describe(None, 0)
    buf = C.create_string_buffer(need + 1)
    lib.yolo_switches_describe(buf, need + 1)
    return dict(ln.split("=") for ln in buf.value.decode().splitlines())


def run(variant):
    from tests import test_gpu_wgrad_h16 as T
    from tests import wgrad_h16_cases as W
    from yolo_for_turbines_amd import _lib as L
    env, names, restated = W.VARIANTS[variant]
    sw = _switches(L.lib())
    for key, value in env.items():
        assert os.environ.get(key) == value, f"{key} is not set for this run"
        assert sw[key] == value, f"the library read {key}={sw[key]}"
    for key in W.SWITCHES:
        assert key in env or key not in os.environ, f"{key} is set and no part of this variant"
    for name in names:
        case, _ = W.by_name(name)
        for dtype in T.DTYPES:
            plan = T.assert_geometry(L, case, T._dt(L, dtype)[0], None, **restated)
            if variant == "fallback":
                assert plan[0] == W.PATCH and case[5:7] == (3, 1), "the fall-back route is wgrad_patch_h16<T, 3, 1>"
            elif name.startswith("dma"):
                assert plan[0] == W.DMA and plan[7] == 5, "the look-ahead-5 instantiation"
            else:
                assert plan[0] == W.STEM and plan[3] == 1, "one stem workgroup"
            T.run_exact(L, case, dtype)
            err = T.run_random(L, case, dtype)
            print(f"case {name} {dtype} {W.KERNEL_NAMES[plan[0]]} slices={plan[3]} per_slice={plan[4]} G={plan[5]} variant={plan[7]} "
                  f"rel_err={err:.3e} ok", flush=True)


if __name__ == "__main__":
    run(sys.argv[1])
