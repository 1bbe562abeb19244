"""Earlier ids of rows of tests/test_one_shot_ladder.py's matrix: each is that row's ladder case
-- the default rung (GL 5: the factorisation compiled for amax = bmax = 5) against the other
four handles --, which runs once per process."""
import pytest

from test_one_shot_ladder import cut_case, horizon_case, refused_case


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["defaults", "adaptive_rho_interval=25", "rho=1e-3", "rho=10", "adaptive_rho=False",
                                   "scaling=0", "max_iter=110"])
def test_factor_matches_roles_persisting_and_oracle(label):
    cut_case(label)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [18, 19])
def test_factor_at_other_block_sizes(N):
    horizon_case(f"N{N}-seed1")


@pytest.mark.gpu
def test_refused_factor_matches_roles_and_persisting():
    refused_case()
