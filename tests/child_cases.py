"""Run a file of GPU test cases with pytest in a CHILD process and report every case of it in the parent.

Why a child: block reuse in torch's caching allocator, and the addresses the driver hands out, follow the whole history of a process, and the suite runs as one
process.  Cases that allocate a lot (whole networks, the tracker CLI) therefore run in a process of their own, so that the tests that come later in the suite find
the allocator as they found it before these cases existed.  One child per file; its output (the MARGIN / NET lines under -s) is passed on."""
import ast
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_names(path):
    """the test functions of a cases file, read from its source (collection must not import torch-heavy code twice)"""
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")]


def run_cases(path, tmp_dir, timeout=900):
    """-> {function name: [(case id, outcome, message)]} with outcome passed / failed / error / skipped"""
    xml = os.path.join(str(tmp_dir), "cases.xml")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", path, "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu", "--junitxml", xml]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    assert os.path.exists(xml), "the child wrote no report (exit status %d):\n%s" % (r.returncode, r.stderr[-2000:])
    out = {}
    for tc in ET.parse(xml).getroot().iter("testcase"):
        outcome, msg = "passed", ""
        for kind in ("failure", "error", "skipped"):
            node = tc.find(kind)
            if node is not None:
                outcome, msg = {"failure": "failed"}.get(kind, kind), (node.get("message") or "") + "\n" + (node.text or "")[-1500:]
        out.setdefault(tc.get("name").split("[")[0], []).append((tc.get("name"), outcome, msg))
    return out


def check(results, name):
    rows = results.get(name, [])
    assert rows, "the child ran no case of %s" % name
    bad = [r for r in rows if r[1] != "passed"]
    assert not bad, "%d of %d cases of %s did not pass; first: %s %s\n%s" % (len(bad), len(rows), name, bad[0][0], bad[0][1], bad[0][2])
