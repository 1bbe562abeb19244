"""The code-object shape of the one-shot cfg-2 kernel with the factorisation compiled for the
headline's plan constants (CPU test).

The headline runs k_setup_solve_w4<6, 4, 5, 6, 2, false, 6, false, ONE = true, GL = 5>: GL 4 with the
out-of-line factorisation factorize_gq_nl<256, true, 5, 5> (solve_phases.h::factorize_w4q / gj_q) in
place of factorize_gp_nl.  GL 4 stays in the library (MPCQP_ONE_SHOT_LOOP=roles) and
tests/test_isa_shape_one_shot_roles.py keeps pinning it; this file holds the new symbols, read from
the code object that ships in libmpcqp.so:

* the GL 5 kernel has no spilled VGPR, VGPR + AGPR <= 256 and no more scratch than the GL 4 kernel;
* its four role loops have exactly the GL 4 kernel's instruction counts, barriers and back edges:
  the kernel body around the call is GL 4's (the callee names the registers factorize_gp_nl
  changes as changed, see factorize_gq_nl);
* a pivot step of the new callee is shorter than one of factorize_gp_nl.  A wave barrier emits no
  instruction, so a step is taken between the pivot reciprocals (one v_rcp_f64 per step, right
  after the publish): the shortest executed path from one reciprocal to the next, every divergent
  branch entered (s_cbranch_execz never taken, s_cbranch_execnz always) and scalar branches either
  way.  The median over the function's steps is a stage-1 step (59 of its 64 steps are: 32 for
  wave 0, 27 for waves 1-3, 5 corner pivots; 32 of factorize_gp_nl's 41 reciprocals).  It stays at or below STEP_NOW, the value of this build
  (profiles/r11/isa_shape_one_shot.txt), which is below factorize_gp_nl's taken the same way;
* the callee touches scratch only in its prologue and epilogue (the callee-saved registers), never
  inside a step.
"""
import collections
import json
import os
import statistics
import subprocess
import tempfile

import pytest

import isa_shape
from test_isa_shape_one_shot_roles import LIB, SYMBOL as GL4_SYMBOL, shape_of

GL5_SYMBOL = "_ZN5mpcqp16k_setup_solve_w4ILi6ELi4ELi5ELi6ELi2ELb0ELi6ELb0ELb1ELi5EE"
NEW_CALLEE = "_ZN5mpcqp15factorize_gq_nlILi256ELb1ELi5ELi5EEEbPKNS_7KParamsEld"
OLD_CALLEE = "_ZN5mpcqp15factorize_gp_nlILi256ELb0ELb1EEEbPKNS_7KParamsEld"
STEP_NOW = 72        # median pivot step of factorize_gq_nl, instructions (this build)
EDGE = 12            # prologue / epilogue: instructions from either end that may touch scratch


def _is_scratch(s):
    return s.startswith(("scratch_", "buffer_store", "buffer_load"))


def step_paths(ins, labels):
    """Per v_rcp_f64 that reaches another one: the instructions on the shortest executed path
    to the next reciprocal (module docstring), as a list of instruction indices."""
    rcp = {i for i, s in enumerate(ins) if s.startswith("v_rcp_f64")}

    def succ(i):
        s = ins[i]
        op, _, arg = s.partition(" ")
        tgt = labels.get(arg.strip())
        if op == "s_branch":
            return [tgt]
        if op == "s_cbranch_execz":
            return [i + 1]
        if op == "s_cbranch_execnz":
            return [tgt]
        if op.startswith("s_cbranch"):
            return [i + 1, tgt]
        if op in ("s_setpc_b64", "s_endpgm"):
            return []
        return [i + 1]

    out = {}
    for r in sorted(rcp):
        prev = {r: None}
        q = collections.deque([r])
        hit = None
        while q and hit is None:
            i = q.popleft()
            for j in succ(i):
                if j is None or j >= len(ins) or j in prev:
                    continue
                prev[j] = i
                if j in rcp:
                    hit = j
                    break
                q.append(j)
        if hit is not None:
            path = []
            while hit is not None:
                path.append(hit)
                hit = prev[hit]
            out[r] = path[::-1][1:]  # (from the instruction after this reciprocal to the next one)
    return out


def callee(lib, name):
    """(instructions, labels) of the out-of-line function `name`, or None."""
    with tempfile.TemporaryDirectory() as d:
        for co in isa_shape.code_objects(lib, d):
            txt = subprocess.run([os.path.join(isa_shape.LLVM, "llvm-readelf"), "-s", "-W", co], check=True,
                                 capture_output=True, text=True).stdout
            if any(ln.split()[-1:] == [name] for ln in txt.splitlines()):
                return isa_shape.instructions(co, name)
    return None


def callee_census(lib, name):
    ins, labels = callee(lib, name)
    paths = step_paths(ins, labels)
    lens = sorted(len(p) for p in paths.values())
    on_path = sorted({i for p in paths.values() for i in p})
    return dict(symbol=name, instructions=len(ins), steps=len(ins) and sum(s.startswith("v_rcp_f64") for s in ins),
                step_median=statistics.median(lens), step_min=lens[0], step_max=lens[-1],
                step_scratch=sum(_is_scratch(ins[i]) for i in on_path),
                scratch_at=[i for i, s in enumerate(ins) if _is_scratch(s)])


@pytest.fixture(scope="module")
def shapes():
    if not isa_shape.tools_present():
        pytest.skip("ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf, llvm-objdump) absent")
    if not os.path.exists(LIB):
        pytest.skip("libmpcqp.so not built")
    gl5, gl4 = shape_of(LIB, GL5_SYMBOL), shape_of(LIB, GL4_SYMBOL)
    assert gl5 is not None, "the GL 5 instantiation is not in libmpcqp.so"
    assert gl4 is not None, "the GL 4 instantiation is not in libmpcqp.so"
    new, old = callee_census(LIB, NEW_CALLEE), callee_census(LIB, OLD_CALLEE)
    print(json.dumps(dict(gl5=gl5, gl4=gl4, new=new, old=old), indent=1))
    return gl5, gl4, new, old


def test_factor_kernel_keeps_its_registers(shapes):
    gl5, gl4, _, _ = shapes
    assert gl5["vgpr_spill_count"] == 0, gl5
    assert gl5["vgpr_count"] + gl5["agpr_count"] <= 256, gl5
    assert gl5["private_segment_fixed_size"] <= gl4["private_segment_fixed_size"], (gl5, gl4)


def test_role_loops_are_the_roles_kernels(shapes):
    gl5, gl4, _, _ = shapes
    assert len(gl5["roles"]) == 4, gl5["roles"]
    assert gl5["roles"] == gl4["roles"], (gl5["roles"], gl4["roles"])


def test_pivot_step_is_shorter(shapes):
    _, _, new, old = shapes
    assert new["steps"] == 64 and old["steps"] == 41, (new, old)  # 32 + 27 + 5; 32 + 8 and the eliminated columns' division
    print("pivot step, instructions (median):", new["step_median"], "against", old["step_median"])
    assert new["step_median"] <= STEP_NOW, new
    assert new["step_median"] < old["step_median"], (new, old)


def test_no_scratch_inside_a_step(shapes):
    _, _, new, _ = shapes
    assert new["step_scratch"] == 0, new
    n = new["instructions"]
    assert all(i < EDGE or i >= n - EDGE for i in new["scratch_at"]), new


if __name__ == "__main__":
    import sys
    lib = sys.argv[1] if len(sys.argv) > 1 else LIB
    print(json.dumps(dict(gl5=shape_of(lib, GL5_SYMBOL), gl4=shape_of(lib, GL4_SYMBOL),
                          new=callee_census(lib, NEW_CALLEE), old=callee_census(lib, OLD_CALLEE)), indent=1))
