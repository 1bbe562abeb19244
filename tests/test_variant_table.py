"""The solve variants' table (csrc/solve.hip, struct Variant in kernels.h), host only.

For configs 1 to 5 and MPCQP_VARIANT unset and 0 to 19, under the production and the
experimental build: the variant mpcqp_plan_preview takes, its threads per QP and its solve
kernel's LDS bytes -- or the refusal "does not fit this plan".  EXPECTED was recorded from the
libraries of the commit before the table existed (seven hand-kept switches), so the table has
to reproduce every one of them."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (1, 2, 3, 4, 5)
VARIANTS = (None,) + tuple(range(20))

# MPCQP_VARIANT is read once per process: one child per (build, variant), the five configs in it
CHILD = """
import json
import osqp_amd
from osqp_amd import mpc
rows = []
for cfg in (1, 2, 3, 4, 5):
    b = mpc.make_batch(cfg, B=2, seed=3)
    P, _ = osqp_amd._drop_common_zeros(b["P"], b["Px"])
    A, _ = osqp_amd._drop_common_zeros(b["A"], b["Ax"])
    try:
        info = osqp_amd.plan_preview(P, A, **b["settings"])
        rows.append([info["variant"], info["threads_per_qp"], info["lds_bytes_solve"]])
    except Exception as e:
        if "does not fit this plan" not in str(e):
            raise
        rows.append(None)
print(json.dumps(rows))
"""

R = None  # refused: "MPCQP_VARIANT=%d does not fit this plan"
# [variant, threads_per_qp, lds_bytes_solve] per config 1..5
EXPECTED = {
    "prod": {
        None: [[17, 256, 78816], [17, 256, 72032], [17, 256, 78816], [17, 256, 78816], [12, 512, 152948]],
        0: [R, [0, 256, 39264], R, R, R],
        1: [R] * 5,
        2: [[2, 256, 47600], R, [2, 256, 47600], [2, 256, 47600], R],
        3: [[3, 256, 47600], R, [3, 256, 47600], [3, 256, 47600], R],
        4: [[4, 256, 47600], [4, 256, 39264], [4, 256, 47600], [4, 256, 47600], R],
        5: [[5, 256, 47600], [5, 256, 39264], [5, 256, 47600], [5, 256, 47600], [5, 256, 99104]],
        6: [[6, 256, 47600], [6, 256, 39264], [6, 256, 47600], [6, 256, 47600], [6, 256, 99104]],
        7: [R, [7, 256, 39264], R, R, R],
        8: [R] * 5,
        9: [R] * 5,
        10: [R, [10, 128, 72032], R, R, R],
        11: [[11, 512, 80416], R, [11, 512, 80416], [11, 512, 80416], R],
        12: [[12, 512, 80416], R, [12, 512, 80416], [12, 512, 80416], [12, 512, 152948]],
        13: [[13, 512, 80416], R, [13, 512, 80416], [13, 512, 80416], [13, 512, 152948]],
        14: [R] * 5,
        15: [R] * 5,
        16: [R] * 5,
        17: [[17, 256, 78816], [17, 256, 72032], [17, 256, 78816], [17, 256, 78816], R],
        18: [R] * 5,
        19: [R] * 5,
    },
    "exp": {
        None: [[17, 256, 78816], [17, 256, 72032], [17, 256, 78816], [17, 256, 78816], [12, 512, 152948]],
        0: [R, [0, 256, 39264], R, R, R],
        1: [R] * 5,
        2: [[2, 256, 47600], R, [2, 256, 47600], [2, 256, 47600], R],
        3: [[3, 256, 47600], R, [3, 256, 47600], [3, 256, 47600], R],
        4: [[4, 256, 47600], [4, 256, 39264], [4, 256, 47600], [4, 256, 47600], R],
        5: [[5, 256, 47600], [5, 256, 39264], [5, 256, 47600], [5, 256, 47600], [5, 256, 99104]],
        6: [[6, 256, 47600], [6, 256, 39264], [6, 256, 47600], [6, 256, 47600], [6, 256, 99104]],
        7: [R, [7, 256, 39264], R, R, R],
        8: [R, [8, 64, 39264], R, R, R],
        9: [R] * 5,
        10: [R, [10, 128, 72032], R, R, R],
        11: [[11, 512, 80416], R, [11, 512, 80416], [11, 512, 80416], R],
        12: [[12, 512, 80416], R, [12, 512, 80416], [12, 512, 80416], [12, 512, 152948]],
        13: [[13, 512, 80416], R, [13, 512, 80416], [13, 512, 80416], [13, 512, 152948]],
        14: [[14, 128, 80416], R, [14, 128, 80416], [14, 128, 80416], R],
        15: [[15, 256, 80416], R, [15, 256, 80416], [15, 256, 80416], [15, 256, 152948]],
        16: [R, [16, 256, 47680], R, R, R],
        17: [[17, 256, 78816], [17, 256, 72032], [17, 256, 78816], [17, 256, 78816], R],
        18: [[18, 512, 139760], R, [18, 512, 139760], [18, 512, 139760], R],
        19: [R, [19, 512, 82944], R, R, R],
    },
}


def run_child(build, variant, root=ROOT):
    env = dict(os.environ, MPCQP_BUILD="" if build == "prod" else build,
               PYTHONPATH=os.path.join(root, "python-mpc_amd"))
    env.pop("MPCQP_VARIANT", None)
    env.pop("MPCQP_DENSE_W4", None)
    if variant is not None:
        env["MPCQP_VARIANT"] = str(variant)
    out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True)
    assert out.returncode == 0, (build, variant, out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def recorded():
    keys = [(b, v) for b in ("prod", "exp") for v in VARIANTS]
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(keys, ex.map(lambda k: run_child(*k), keys)))


@pytest.mark.parametrize("build", ["prod", "exp"])
def test_variant_table_matches_the_switches_it_replaced(recorded, build):
    for v in VARIANTS:
        got = recorded[(build, v)]
        assert got == EXPECTED[build][v], (build, v, got, EXPECTED[build][v])


def test_production_build_has_no_experimental_entry(recorded):
    for v in (8, 9, 14, 15, 16, 18, 19):
        assert recorded[("prod", v)] == [R] * len(CONFIGS), (v, recorded[("prod", v)])
    for cfg, row in zip(CONFIGS, recorded[("prod", None)]):
        assert row is not None, cfg
