"""Earlier ids of five rows of tests/test_one_shot_ladder.py's matrix (the paths of the outer pass):
each is that row's ladder case, all five handles, which runs once per process."""
import pytest

from test_one_shot_ladder import cut_case


@pytest.mark.gpu
def test_passes_defaults():
    cut_case("defaults")


@pytest.mark.gpu
def test_passes_iteration_cap():
    cut_case("max_iter=110")


@pytest.mark.gpu
def test_passes_scaled_termination():
    cut_case("scaled_termination")


@pytest.mark.gpu
def test_passes_check_every_10():
    cut_case("check_termination=10")


@pytest.mark.gpu
def test_passes_single_factorisation():
    cut_case("adaptive_rho=False max_iter=500")
