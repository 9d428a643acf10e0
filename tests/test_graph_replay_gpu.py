"""GPU: launch lists captured into a hipGraph and replayed -- one-op plans of every stateful conv form, whole networks through Detector.capture -- against eager runs
(DESIGN.md section 2 "What a replayed launch list relies on").  The cases are tests/graph_replay_gpu_cases.py; they run in one child process (graph capture uses a
private pool of the caching allocator; tests/child_cases.py says why that must not reach later tests) and every test function of that file is one test here."""
import pytest

from tests import child_cases

pytestmark = pytest.mark.gpu
CASES = "tests/graph_replay_gpu_cases.py"


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return child_cases.run_cases(CASES, tmp_path_factory.mktemp("graph_replay"))


@pytest.mark.parametrize("name", child_cases.case_names(CASES))
def test_graph_replay(results, name):
    child_cases.check(results, name)
