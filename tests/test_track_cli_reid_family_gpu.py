"""GPU: tracker/track.py with the OSNet family as the appearance network (--reid_model_path random:osnet_x0_5 ..., --reid_half).  The cases are
tests/track_cli_reid_family_gpu_cases.py; the command-line runs happen in one child process (tests/child_cases.py) and every test function of that file is one
test here."""
import pytest

from tests import child_cases

pytestmark = pytest.mark.gpu
CASES = "tests/track_cli_reid_family_gpu_cases.py"


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return child_cases.run_cases(CASES, tmp_path_factory.mktemp("track_cli_reid_family"))


@pytest.mark.parametrize("name", child_cases.case_names(CASES))
def test_track_cli_reid_family(results, name):
    child_cases.check(results, name)
