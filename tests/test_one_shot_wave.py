"""Earlier ids of five rows of tests/test_one_shot_ladder.py's matrix: each is that row's ladder
case -- the wave rung (GL 3) among its five handles --, which runs once per process."""
import pytest

from test_one_shot_ladder import cut_case


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["defaults", "max_iter=110", "scaled_termination", "check_termination=10",
                                   "adaptive_rho=False max_iter=500"])
def test_wave_loop_matches_lds_loop_persisting_and_oracle(label):
    cut_case(label)
