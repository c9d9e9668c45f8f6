"""What eirgrid-hip prints and returns before it touches a device, pinned byte for byte: the --help text (tests/golden/cli_help.txt) and
every refusal of the argument parser and of main()'s checks ahead of the world and the device (tests/golden/cli_refusals.json: argv,
returncode, stderr, and whether the "World:" line was reached; the files of a case are named by placeholders).  Both fixtures are the
driver's own output, recorded through _run() below from the binary of the commit before the driver was split into units, so a change
that alters a message, an exit code or the order of the checks fails here, without a GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_ACTION = ('{"action_type": "AddGenerator", "generator_type": "OffshoreWind", "generator_id": null, "operation_percentage": null, '
           '"offset_type": null, "cost_multiplier": %d}')
_PLAN = '{"best_actions": {"2025": [%s]}, "best_deficit_actions": {}, "name": "%s"}\n'
FILES = {"{ONE}": _PLAN % (_ACTION % 150, "ok"),
         "{TWO}": _PLAN % (_ACTION % 150, "a") + _PLAN % ("", "b"),
         "{BROKEN}": _PLAN % (_ACTION % 150, "ok") + '{"best_actions": 3}\n'}


def _run(argv, tmp):
    """the case with its placeholders filled in; the paths in what it printed are turned back into the placeholders"""
    paths = {"{WORLD}": os.path.join(GOLDEN, "world_v1.json"), "{CK}": os.path.join(tmp, "ck")}
    for key, text in FILES.items():
        paths[key] = os.path.join(tmp, key.strip("{}").lower() + ".jsonl")
        with open(paths[key], "w") as f:
            f.write(text)
    out = subprocess.run([CLI] + [paths.get(x, x) for x in argv], capture_output=True, text=True, timeout=60)
    stderr = out.stderr
    for key, path in paths.items():
        stderr = stderr.replace(path, key)
    assert not os.path.exists(paths["{CK}"]), argv
    return {"argv": argv, "returncode": out.returncode, "stderr": stderr, "stdout_has_world": "World:" in out.stdout}


def test_help_text_is_unchanged(built):
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == ""
    assert out.stdout == open(os.path.join(GOLDEN, "cli_help.txt"), encoding="utf-8").read()


def test_refusals_are_unchanged_and_write_nothing(built, tmp_path):
    want = json.load(open(os.path.join(GOLDEN, "cli_refusals.json"), encoding="utf-8"))
    assert len(want) == 50
    for w in want:
        assert w["returncode"] in (1, 2), w
        assert _run(w["argv"], str(tmp_path)) == w

