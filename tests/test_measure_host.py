"""tools/common/measure.py without a GPU: the alternating child runner (start order, CRL_LIB_PATH per child, the marked
result line, no child started after one that failed or outlived its limit), the statistics, and that importing the module
leaves torch alone.  The children are `python -c` one-liners that never import torch; each appends its tag to a file, which
is how starts are counted."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# appends CRL_LIB_PATH (or "-") to the file argv[1] names, then runs argv[2] (a statement) and prints a result behind "R "
CHILD = ("import json, os, sys, time; lib = os.environ.get('CRL_LIB_PATH', '-'); open(sys.argv[1], 'a').write(lib + '\\n'); "
         "bad = lib.endswith('bad.so'); exec(sys.argv[2]); print('noise'); print('R [\"early\"]'); print('R ' + json.dumps([lib])); print('trailing')")


def _run(tmp_path, builds, rounds, statement="pass", timeout=60):
    from tools.common import measure as M
    log = tmp_path / "starts"
    argv = [sys.executable, "-c", CHILD, str(log), statement]
    return M, log, M.alternate(argv, builds, rounds, timeout, "R ")


def test_children_alternate_and_see_their_library(tmp_path, no_gpu_context):
    a, b = str(tmp_path / "a.so"), str(tmp_path / "b.so")
    M, log, runs = _run(tmp_path, [("this", None), ("a", a), ("b", b)], 2)
    got = list(runs)
    assert [tag for tag, _ in got] == ["this", "a", "b", "this", "a", "b"]
    assert [r for _, r in got] == [["-"], [a], [b]] * 2       # the LAST line behind the marker, and nothing unmarked
    assert log.read_text().split() == ["-", a, b] * 2


def test_a_library_of_the_callers_environment_does_not_reach_the_shipped_build(tmp_path, no_gpu_context, monkeypatch):
    monkeypatch.setenv("CRL_LIB_PATH", "/somewhere/else.so")
    M, log, runs = _run(tmp_path, [("this", None)], 1)
    assert list(runs) == [("this", ["-"])]


@pytest.mark.parametrize("statement,says", [
    ("if bad: sys.exit(3)", "status 3"),
    ("if bad: os.kill(os.getpid(), 9)", "status -9"),
    ("if bad: os._exit(0)", "status 0"),                     # ends well but prints no result line
    ("if bad: time.sleep(30)", "ran past 1 s"),
], ids=["exit", "signal", "no-result", "timeout"])
def test_no_child_starts_after_one_that_failed(tmp_path, no_gpu_context, statement, says):
    good, bad = str(tmp_path / "good.so"), str(tmp_path / "bad.so")
    M, log, runs = _run(tmp_path, [("good", good), ("bad", bad), ("never", good)], 3, statement, timeout=1 if "sleep" in statement else 60)
    got = []
    with pytest.raises(M.ChildFailed) as e:
        for item in runs:
            got.append(item)
    assert got == [("good", [good])]
    assert "the bad build" in str(e.value) and says in str(e.value)
    assert log.read_text().split() == [good, bad]            # two starts: nothing after the failure
    assert isinstance(e.value, SystemExit) and e.value.code not in (0, None)     # uncaught, it ends a tool with status 1


def test_refuses_to_start_children_from_a_process_with_a_gpu_context(tmp_path, no_gpu_context, monkeypatch):
    import types
    fake = types.SimpleNamespace(cuda=types.SimpleNamespace(is_initialized=lambda: True))
    monkeypatch.setitem(sys.modules, "torch", fake)
    M, log, runs = _run(tmp_path, [("this", None)], 1)
    with pytest.raises(RuntimeError, match="GPU context"):
        list(runs)
    assert not log.exists()


def test_statistics():
    from tools.common import measure as M
    assert M.median([4, 1, 3, 2]) == 3                       # the upper median
    assert M.median([5]) == 5 and M.median([2, 9, 4]) == 4
    assert M.spread([4, 1, 3, 2]) == (3, [1, 4])
    assert M.shape_name((3, 3, 3), 3, 4) == "3x3x3_k3_p4"
    assert [M.shape_name(*s) for s in M.TTT_SHAPES] == ["3x3_k3_p2", "3x5_k3_p3", "3x3x3_k3_p4", "5x5_k4_p3"]


def test_rows_are_written_as_json_lines(tmp_path, capsys):
    import json
    from tools.common import measure as M
    rows = [{"a": 1, "b": [1.5, None]}, {"a": 2}]
    M.write_rows(str(tmp_path / "new" / "dir" / "rows.jsonl"), rows)
    assert [json.loads(ln) for ln in (tmp_path / "new" / "dir" / "rows.jsonl").read_text().splitlines()] == rows
    M.emit(rows[0])
    assert json.loads(capsys.readouterr().out) == rows[0]


def test_importing_the_module_does_not_import_torch(no_gpu_context):
    code = "import sys; sys.path.insert(0, %r); from tools.common import measure; assert 'torch' not in sys.modules" % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
