"""The conv / weight-gradient dispatch decides what it decided before: for a fixed grid of descriptors (the bench / README
layer shapes at batch 1 and 4, the knob settings the kernel tests use, misaligned operands, refused descriptors) the query
functions return, and the launches instantiate, exactly what tests/golden/conv_dispatch.txt records, line for line.

The table is recorded from the commit BEFORE a change of the dispatch, never from the code under test.  A deliberate policy
change regenerates it from a build of the new code and shows up as a readable diff of that file:

    python tests/emul/build_emul.py && python tools/conv_dispatch_dump.py > tests/golden/conv_dispatch.txt
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_dispatch_table_unchanged():
    sys.path.insert(0, os.path.join(HERE, "emul"))
    import build_emul
    lib = build_emul.build()
    env = {k: v for k, v in os.environ.items() if not k.startswith("ADP_")}  # the dump sets every knob it wants itself
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_dispatch_dump.py"), lib], capture_output=True, text=True,
                         env=env)
    assert run.returncode == 0, run.stderr[-2000:]  # (also: a kernel family of either table that the grid never reached)
    with open(os.path.join(HERE, "golden", "conv_dispatch.txt")) as f:
        want = f.read().splitlines()
    got = run.stdout.splitlines()
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} lines differ; first: line {diff[0][0]}\n  recorded: {diff[0][1]}\n  now:      {diff[0][2]}"
    assert len(got) == len(want)
