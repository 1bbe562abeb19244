"""The code-object shape of every rung of the one-shot cfg-2 kernel ladder, pinned (CPU test).

tests/test_isa_shape.py pins the persisting kernels.  The headline runs the one-shot form 2
instantiation of the fused four-wave kernel, k_setup_solve_w4<6, 4, 5, 6, 2, false, 6, false, ONE =
true, GL>, which exists in four rungs (solve_wave.hip::one_shot_gl picks one): GL 5
by default, GL 1 / 3 / 4 as the A/B baselines MPCQP_ONE_SHOT_LOOP=lds / wave / roles.  Edits outside
the ADMM loop have moved these kernels' register assignment before, so each rung is
held to what the tree ships, read once from the code objects in libmpcqp.so (PINS):

* every rung: no spilled VGPR, VGPR + AGPR <= 256 (two workgroups per CU); the scratch the kernel
  reserves (12 bytes in GL 1; no more in GL 3 and GL 4; in GL 5 no more than GL 4's);
* GL 1, GL 3: the scalar-register spills (v_writelane / v_readlane pairs, all outside the ADMM
  loop) do not grow past SGPR_SPILLS; the ADMM loop -- the shortest call-free loop with four
  workgroup barriers (rhs, phase B, phase C, rows) -- has four barriers, no scratch access, no
  v_readlane and at most PINS' instructions (197 for GL 1, with row-major and with swizzled
  tiles; 195 for GL 3).  Nothing in the loop is meant to pass through scalar registers: the
  hand-off of c_w from phase A to phase B by 2 QR = 10 v_readlane was built, measured slower than
  the L.cor round trip in each of three forms and left out, so a v_readlane there
  would be a value the compiler turned scalar (rho) or a spilled mask (one copy of
  rows_wave per role did that to one role);
* GL 4: the loop is compiled once per wave role (admm_run<W>, solve_w4_run.inc), so the call-free
  four-barrier loops have four distinct headers.  Each header has two back edges: the shorter
  closes an iteration of a wave that owns no rows (it branches back at the last barrier), the
  longer one of a wave that does.  Each edge has four barriers, no scratch access and no
  v_readlane; every longer edge is below the 195 instructions of GL 3's shared loop; the (short,
  long) counts per role are pinned in ascending order, element-wise and in sum (ROLE_LOOPS);
* GL 5: GL 4 with the out-of-line factorisation factorize_gq_nl<256, true, 5, 5> (solve_phases.h::
  factorize_w4q / gj_q) in place of factorize_gp_nl.  Its role loops are exactly GL 4's.  A pivot
  step of the new callee is shorter than one of factorize_gp_nl: a wave barrier emits no
  instruction, so a step is taken between the pivot reciprocals (one v_rcp_f64 per step, right
  after the publish; isa_shape.step_paths).  The median over the function's steps is a stage-1
  step (59 of its 64 are: 32 for wave 0, 27 for waves 1-3, 5 corner pivots; 32 of factorize_gp_nl's
  41 reciprocals); it stays at or below STEP_NOW and below factorize_gp_nl's taken the same way.
  The callee touches scratch only in its prologue and epilogue (the callee-saved registers), never
  inside a step.

`python tests/test_isa_shape_one_shot.py [library [GL]]` prints the JSON that
profiles/r8 ... r11/isa_shape_one_shot.txt were made from.
"""
import json
import os
import tempfile

import pytest

import isa_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "python-mpc_amd", "osqp_amd", "libmpcqp.so")

SYMBOL = "_ZN5mpcqp16k_setup_solve_w4ILi6ELi4ELi5ELi6ELi2ELb0ELi6ELb0ELb1ELi%dEE"
NEW_CALLEE = "_ZN5mpcqp15factorize_gq_nlILi256ELb1ELi5ELi5EEEbPKNS_7KParamsEld"
OLD_CALLEE = "_ZN5mpcqp15factorize_gp_nlILi256ELb0ELb1EEEbPKNS_7KParamsEld"
SGPR_SPILLS = 204
# per GL: the shared ADMM loop's instructions (GL 1, GL 3), the kernel's scratch bytes
PINS = {
    1: dict(loop=197, scratch=12),  # (exactly 12)
    3: dict(loop=195, scratch=12),
    4: dict(scratch=12),
    5: dict(),                      # (scratch: GL 4's)
}
# GL 4 (and GL 5): (without rows, with rows) instructions per role loop, ascending (the roles differ
# by their phase A pairs and phase C slots: wave 0 has no pair and two slots, wave 3 three pairs
# and no slot)
ROLE_LOOPS = [(130, 160), (131, 161), (136, 166), (139, 169)]
STEP_NOW = 72  # median pivot step of factorize_gq_nl, instructions
EDGE = 12      # prologue / epilogue: instructions from either end that may touch scratch


def shapes_of(lib, gls=tuple(PINS)):
    """{GL: isa_shape.shape_of}, with the two factorisations' censuses under "new" / "old" for GL 5;
    the library is unbundled and each symbol disassembled once."""
    with tempfile.TemporaryDirectory() as d:
        cos = isa_shape.code_objects(lib, d)
        out = {gl: isa_shape.shape_of(cos, SYMBOL % gl) for gl in gls}
        if 5 in gls:
            out["new"], out["old"] = (isa_shape.callee_census(cos, c) for c in (NEW_CALLEE, OLD_CALLEE))
    return out


@pytest.fixture(scope="module")
def shapes():
    if not isa_shape.tools_present():
        pytest.skip("ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf, llvm-objdump) absent")
    if not os.path.exists(LIB):
        pytest.skip("libmpcqp.so not built")
    r = shapes_of(LIB)
    print(json.dumps(r, indent=1))
    for gl in PINS:
        assert r[gl] is not None, f"the GL {gl} instantiation is not in libmpcqp.so"
    return r


def _keeps_its_registers(s):
    assert s["vgpr_spill_count"] == 0, s
    assert s["vgpr_count"] + s["agpr_count"] <= 256, s


def test_one_shot_kernel_keeps_its_registers(shapes):  # (GL 1, under the id it has had)
    _keeps_its_registers(shapes[1])


@pytest.mark.parametrize("gl", [3, 4, 5])
def test_kernel_keeps_its_registers(shapes, gl):
    _keeps_its_registers(shapes[gl])


@pytest.mark.parametrize("gl", list(PINS))
def test_kernel_scratch_bytes(shapes, gl):
    s = shapes[gl]
    if gl == 1:
        assert s["private_segment_fixed_size"] == PINS[1]["scratch"], s
    elif gl == 5:
        assert s["private_segment_fixed_size"] <= shapes[4]["private_segment_fixed_size"], (s, shapes[4])
    else:
        assert s["private_segment_fixed_size"] <= PINS[gl]["scratch"], s


@pytest.mark.parametrize("gl", [1, 3])
def test_kernel_sgpr_spills(shapes, gl):
    print("sgpr_spill_count", shapes[gl]["sgpr_spill_count"])
    assert shapes[gl]["sgpr_spill_count"] <= SGPR_SPILLS, shapes[gl]


def _shared_admm_loop_shape(shapes, gl):
    loop = shapes[gl]["loop"]
    assert loop["barriers"] == 4 and loop["scratch"] == 0 and loop["readlane"] == 0, loop
    assert loop["instructions"] <= PINS[gl]["loop"], loop


def test_one_shot_admm_loop_shape(shapes):  # (GL 1, under the id it has had)
    _shared_admm_loop_shape(shapes, 1)


def test_wave_admm_loop_shape(shapes):
    _shared_admm_loop_shape(shapes, 3)


def test_one_loop_per_role(shapes):
    roles = shapes[4]["roles"]
    assert len(roles) == 4, roles  # four distinct headers
    for edges in roles:
        assert len(edges) == 2, edges  # a wave without rows, a wave with rows
        for c in edges:
            assert c["barriers"] == 4 and c["scratch"] == 0 and c["readlane"] == 0, c


def test_every_role_is_shorter_than_the_shared_loop(shapes):
    for edges in shapes[4]["roles"]:
        assert edges[-1]["instructions"] < PINS[3]["loop"], edges


def test_role_loop_counts_pinned(shapes):
    got = sorted((e[0]["instructions"], e[-1]["instructions"]) for e in shapes[4]["roles"])
    print("role loops (without rows, with rows):", got)
    assert sum(b for _, b in got) <= sum(b for _, b in ROLE_LOOPS), got
    for (a, b), (pa, pb) in zip(got, ROLE_LOOPS):
        assert a <= pa and b <= pb, (got, ROLE_LOOPS)


def test_factor_kernels_role_loops_are_the_roles_kernels(shapes):
    assert len(shapes[5]["roles"]) == 4, shapes[5]["roles"]
    assert shapes[5]["roles"] == shapes[4]["roles"], (shapes[5]["roles"], shapes[4]["roles"])


def test_pivot_step_is_shorter(shapes):
    new, old = shapes["new"], shapes["old"]
    assert new["steps"] == 64 and old["steps"] == 41, (new, old)  # 32 + 27 + 5; 32 + 8 and the eliminated columns' division
    print("pivot step, instructions (median):", new["step_median"], "against", old["step_median"])
    assert new["step_median"] <= STEP_NOW, new
    assert new["step_median"] < old["step_median"], (new, old)


def test_no_scratch_inside_a_step(shapes):
    new = shapes["new"]
    assert new["step_scratch"] == 0, new
    n = new["instructions"]
    assert all(i < EDGE or i >= n - EDGE for i in new["scratch_at"]), new


if __name__ == "__main__":
    import sys
    lib = sys.argv[1] if len(sys.argv) > 1 else LIB
    print(json.dumps(shapes_of(lib, (int(sys.argv[2]),) if len(sys.argv) > 2 else tuple(PINS)), indent=1))
