"""The one-shot cfg-2 kernel's register allocation, pinned (CPU test).

tests/test_isa_shape.py pins the persisting kernels; the headline runs the one-shot form 2
instantiation of the fused four-wave kernel (solve_wave.hip::launch_setup_solve), which nothing
held in shape.  Its S_k^{-1} tiles are swizzled (solve_phases.h::tile_at) at the run start and in
the factorisation, outside the ADMM loop -- and edits outside that loop have moved its register
assignment before.  Read from the code object that ships in libmpcqp.so:

* no spilled VGPR;
* the ADMM loop (the shortest call-free loop with four workgroup barriers): four barriers, no
  scratch access, no `v_readlane`;
* the loop's instruction count: 197 in the library before the swizzle, LOOP_NOW with it -- it may
  not exceed either.
"""
import os

import pytest

import isa_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "python-mpc_amd", "osqp_amd", "libmpcqp.so")

# k_setup_solve_w4<6, 4, 5, 6, 2, false, 6, false, ONE = true, GL = 1>
ONE_SHOT = {"cfg2_one": ("_ZN5mpcqp16k_setup_solve_w4ILi6ELi4ELi5ELi6ELi2ELb0ELi6ELb0ELb1ELi1EE", "w4")}
LOOP_BEFORE = 197  # row-major tiles (the parent of the swizzle)
LOOP_NOW = 197     # swizzled tiles


@pytest.fixture(scope="module")
def shape():
    if not isa_shape.tools_present():
        pytest.skip("ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf, llvm-objdump) absent")
    if not os.path.exists(LIB):
        pytest.skip("libmpcqp.so not built")
    return isa_shape.report(LIB, ONE_SHOT)["cfg2_one"]


def test_one_shot_kernel_keeps_its_registers(shape):
    assert shape["vgpr_spill_count"] == 0, shape
    assert shape["vgpr_count"] + shape["agpr_count"] <= 256, shape  # two workgroups per CU


def test_one_shot_admm_loop_shape(shape):
    loop = shape["loop"]
    assert loop["scratch"] == 0 and loop["readlane"] == 0 and loop["barriers"] == 4, loop
    assert loop["instructions"] <= min(LOOP_BEFORE, LOOP_NOW), loop
