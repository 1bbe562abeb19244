"""The code-object shape of the one-shot cfg-2 kernel with one ADMM loop per wave role (CPU test).

The headline runs k_setup_solve_w4<6, 4, 5, 6, 2, false, 6, false, ONE = true, GL = 4>: GL 3 with
the run's loop compiled once per wave index (solve_wave.hip::solve_w4_body admm_run<W>,
solve_w4_run.inc), reached through a switch on the wave.  tests/test_isa_shape_one_shot*.py keep
pinning GL 1 and GL 3, which stay in the library; this file holds the new symbol, read from the
code object that ships in libmpcqp.so:

* no spilled VGPR, VGPR + AGPR <= 256 (two workgroups per CU), at most 12 bytes of scratch;
* the call-free loops with exactly four workgroup barriers (rhs, phase B, phase C, rows) have four
  distinct headers, one per role.  Each header has two back edges: the shorter closes an iteration
  of a wave that owns no rows (it branches back at the last barrier), the longer one of a wave
  that does (the rows phase lies after that branch);
* in each role's loop, over its longer back edge: no scratch access and no v_readlane (nothing in
  the loop is meant to pass through scalar registers; a v_readlane there is a spilled mask --
  one copy of rows_wave per role did that to one role);
* every role's longer back edge is below the 195 instructions of GL 3's whole shared loop, whose
  rows phase came on top of them: every wave's path is shorter than the shared loop was;
* the counts are pinned at what this tree ships: (short, long) back edges per role, in ascending
  order; the sum over roles may not grow.

`python tests/isa_shape.py`-style output next to the parent's: profiles/r10/isa_shape_one_shot.txt.
"""
import json
import os
import tempfile

import pytest

import isa_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "python-mpc_amd", "osqp_amd", "libmpcqp.so")

SYMBOL = "_ZN5mpcqp16k_setup_solve_w4ILi6ELi4ELi5ELi6ELi2ELb0ELi6ELb0ELb1ELi4EE"
GL3_LOOP = 195       # tests/test_isa_shape_one_shot_wave.py::LOOP_NOW: the shared loop before its rows phase
LOOP_READLANE = 0
SCRATCH_BYTES = 12
# (without rows, with rows) instructions per role loop, ascending (the roles differ by their phase
# A pairs and phase C slots: wave 0 has no pair and two slots, wave 3 three pairs and no slot)
ROLE_LOOPS = [(130, 160), (131, 161), (136, 166), (139, 169)]


def role_loops(ins, labels):
    """{header: [census of each back edge, shortest first]} of the call-free loops with exactly
    four workgroup barriers."""
    out = {}
    for lo, hi in isa_shape.loops(ins, labels):
        if isa_shape.count(ins, lo, hi, "s_swappc") == 0 and isa_shape.count(ins, lo, hi, "s_barrier") == 4:
            out.setdefault(lo, []).append(isa_shape.census(ins, lo, hi))
    for v in out.values():
        v.sort(key=lambda c: c["instructions"])
    return out


def shape_of(lib, symbol=SYMBOL):
    """Metadata of the symbol plus "roles": per header (in code order) the census of its back edges."""
    with tempfile.TemporaryDirectory() as d:
        for co in isa_shape.code_objects(lib, d):
            md = isa_shape.metadata(co)
            hit = [k for k in md if symbol in k]
            if hit:
                ins, labels = isa_shape.instructions(co, hit[0])
                r = dict(md[hit[0]], symbol=hit[0])
                r["roles"] = [v for _, v in sorted(role_loops(ins, labels).items())]
                return r
    return None


@pytest.fixture(scope="module")
def shape():
    if not isa_shape.tools_present():
        pytest.skip("ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf, llvm-objdump) absent")
    if not os.path.exists(LIB):
        pytest.skip("libmpcqp.so not built")
    r = shape_of(LIB)
    assert r is not None, "the GL 4 instantiation is not in libmpcqp.so"
    print(json.dumps(r, indent=1))
    return r


def test_roles_kernel_keeps_its_registers(shape):
    assert shape["vgpr_spill_count"] == 0, shape
    assert shape["vgpr_count"] + shape["agpr_count"] <= 256, shape
    assert shape["private_segment_fixed_size"] <= SCRATCH_BYTES, shape


def test_one_loop_per_role(shape):
    roles = shape["roles"]
    assert len(roles) == 4, roles  # four distinct headers
    for edges in roles:
        assert len(edges) == 2, edges  # a wave without rows, a wave with rows
        for c in edges:
            assert c["barriers"] == 4 and c["scratch"] == 0, c
            assert c["readlane"] == LOOP_READLANE, c


def test_every_role_is_shorter_than_the_shared_loop(shape):
    for edges in shape["roles"]:
        assert edges[-1]["instructions"] < GL3_LOOP, edges


def test_role_loop_counts_pinned(shape):
    got = sorted((e[0]["instructions"], e[-1]["instructions"]) for e in shape["roles"])
    print("role loops (without rows, with rows):", got)
    assert sum(b for _, b in got) <= sum(b for _, b in ROLE_LOOPS), got
    for (a, b), (pa, pb) in zip(got, ROLE_LOOPS):
        assert a <= pa and b <= pb, (got, ROLE_LOOPS)


if __name__ == "__main__":
    import sys
    print(json.dumps(shape_of(sys.argv[1] if len(sys.argv) > 1 else LIB,
                              sys.argv[2] if len(sys.argv) > 2 else SYMBOL), indent=1))
