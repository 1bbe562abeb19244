"""What tests/test_isa_shape_one_shot.py leaves open for the one-shot cfg-2 kernel (CPU test).

The instantiation's code between the ADMM runs is its own (solve_wave.hip::solve_w4_body, LEAN), and
edits there move the register assignment of the whole kernel.  Beside the existing pin (no spilled
VGPR, the loop's four barriers and 197 instructions), read from the code object in libmpcqp.so:

* the scratch the kernel reserves stays at 12 bytes;
* the scalar-register spills (v_writelane / v_readlane pairs, all outside the ADMM loop) do not
  grow past what this tree shipped with: SGPR_SPILLS (175 before the between-run cut).

`python tests/isa_shape.py`-style output of the symbol: profiles/r8/isa_shape_one_shot.txt.
"""
import json
import os

import pytest

import isa_shape
from test_isa_shape_one_shot import LIB, ONE_SHOT

SGPR_SPILLS = 204


@pytest.fixture(scope="module")
def shape():
    if not isa_shape.tools_present():
        pytest.skip("ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf, llvm-objdump) absent")
    if not os.path.exists(LIB):
        pytest.skip("libmpcqp.so not built")
    r = isa_shape.report(LIB, ONE_SHOT)["cfg2_one"]
    print(json.dumps(r, indent=1))
    return r


def test_one_shot_kernel_scratch_bytes(shape):
    assert shape["private_segment_fixed_size"] == 12, shape


def test_one_shot_kernel_sgpr_spills(shape):
    print("sgpr_spill_count", shape["sgpr_spill_count"])
    assert shape["sgpr_spill_count"] <= SGPR_SPILLS, shape
