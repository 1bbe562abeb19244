"""The code-object shape of the one-shot cfg-2 kernel the headline runs (CPU test).

The headline runs k_setup_solve_w4<6, 4, 5, 6, 2, false, 6, false, ONE = true, GL = 3>: the form-2
one-shot instantiation whose ADMM loop issues phase A's b_j reads at once and phase B's b_w reads
ahead of the reduction, and whose Gauss-Jordan takes the pivot by v_readlane (solve_wave.hip::
solve_w4_body WV, solve_phases.h::gj_seg SEG 3 / 4).  tests/test_isa_shape_one_shot*.py keep
pinning the GL = 1 instantiation it replaces (MPCQP_ONE_SHOT_LOOP=lds); this file holds the new
symbol, read from the code object that ships in libmpcqp.so:

* no spilled VGPR, and VGPR + AGPR <= 256 (two workgroups per CU);
* the ADMM loop (the shortest call-free loop with four workgroup barriers): four barriers, no
  scratch access, and the intended number of v_readlane.  That number is 0: the hand-off of c_w
  from phase A to phase B by 2 QR = 10 v_readlane was built, measured slower than the L.cor round
  trip in each of three forms and left out, so nothing in the loop is meant to
  pass through scalar registers -- a v_readlane there would be a value the compiler turned scalar
  (rho);
* the loop's instruction count, the kernel's scratch bytes and its scalar-register spills (all
  outside the loop) do not grow past what this tree shipped with.

`python tests/isa_shape.py`-style output of the symbol: profiles/r9/isa_shape_one_shot.txt.
"""
import json
import os

import pytest

import isa_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "python-mpc_amd", "osqp_amd", "libmpcqp.so")

ONE_SHOT_WAVE = {"cfg2_wave": ("_ZN5mpcqp16k_setup_solve_w4ILi6ELi4ELi5ELi6ELi2ELb0ELi6ELb0ELb1ELi3EE", "w4")}
LOOP_READLANE = 0    # (the in-wave hand-off would make it 2 QR = 10)
LOOP_NOW = 195       # (197 in the GL = 1 instantiation)
SCRATCH_BYTES = 12
SGPR_SPILLS = 204


@pytest.fixture(scope="module")
def shape():
    if not isa_shape.tools_present():
        pytest.skip("ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf, llvm-objdump) absent")
    if not os.path.exists(LIB):
        pytest.skip("libmpcqp.so not built")
    r = isa_shape.report(LIB, ONE_SHOT_WAVE)["cfg2_wave"]
    print(json.dumps(r, indent=1))
    return r


def test_wave_kernel_keeps_its_registers(shape):
    assert shape["vgpr_spill_count"] == 0, shape
    assert shape["vgpr_count"] + shape["agpr_count"] <= 256, shape


def test_wave_admm_loop_shape(shape):
    loop = shape["loop"]
    assert loop["barriers"] == 4 and loop["scratch"] == 0, loop
    assert loop["readlane"] == LOOP_READLANE, loop
    assert loop["instructions"] <= LOOP_NOW, loop


def test_wave_kernel_scratch_and_sgpr_spills(shape):
    assert shape["private_segment_fixed_size"] <= SCRATCH_BYTES, shape
    assert shape["sgpr_spill_count"] <= SGPR_SPILLS, shape
