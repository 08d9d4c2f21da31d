"""The kernel-launch sequences of the VQ-VAE host drivers against their recorded digests (no GPU, no library).

tools/launch_trace.py replaces every launching wrapper of arcweld.kernels by a recorder and runs the model's paths on
CPU tensors; tests/golden/launch_trace.json holds one digest per case and path.  A host-side refactor must leave them
as they are.  A change that alters launches on purpose regenerates the file and says so in its description:

    python tools/launch_trace.py --digests tests/golden/launch_trace.json
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
# the chain routes with every fold on and with the three boundary folds off, the f32 BatchNorm per-conv route, and
# the stacks of no blocks
CASES = ["bf16 bn=0 R=3 p=0.1", "bf16 bn=0 R=3 p=0.1 CHAIN_HEAD=0,CONVT_TAIL=0,SEP_TAIL=0", "f32 bn=1 R=1 p=0.1",
         "bf16 bn=0 R=0 p=0.0"]


def test_launch_digests_match_golden(tmp_path):
    """A fresh child process: the tool replaces arcweld.kernels functions in the process it runs in."""
    out = tmp_path / "digests.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_trace.py"), "--digests", str(out),
                        "--cases", *CASES], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(out.read_text())
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(CASES)
    for case in CASES:
        diff = {p: (got[case].get(p), d) for p, d in want[case].items() if got[case].get(p) != d}
        assert not diff and got[case].keys() == want[case].keys(), f"{case}: (got, golden) per path: {diff}"
