"""Earlier ids of rows of tests/test_one_shot_ladder.py's matrix: each is that row's ladder case
-- the roles rung (GL 4) among its five handles --, which runs once per process.  N = 22 skips
where its plan does not take one-shot form 2 (the MI355X)."""
import pytest

from test_one_shot_ladder import cut_case, horizon_case


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["defaults", "max_iter=110", "scaled_termination", "check_termination=10",
                                   "adaptive_rho=False max_iter=500"])
def test_role_loops_match_wave_lds_persisting_and_oracle(label):
    cut_case(label)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [18, 22])
def test_role_loops_at_other_row_ownerships(N):
    horizon_case({18: "N18-ladder-seed", 22: "N22-seed1"}[N])
