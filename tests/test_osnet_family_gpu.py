"""GPU: the general OSNet path (csrc/y7t_reid_osnet.hip; DESIGN.md section 4 "OSNet family") -- one-op plans, whole networks, behaviour.  The cases are
tests/osnet_family_gpu_cases.py; they run in one child process (tests/child_cases.py says why) and every test function of that file is one test here."""
import pytest

from tests import child_cases

pytestmark = pytest.mark.gpu
CASES = "tests/osnet_family_gpu_cases.py"


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return child_cases.run_cases(CASES, tmp_path_factory.mktemp("osnet_family"))


@pytest.mark.parametrize("name", child_cases.case_names(CASES))
def test_osnet_family(results, name):
    child_cases.check(results, name)
