"""tools/bench_packed.py without a GPU: --help, and its seeded length
distributions."""

import os
import subprocess
import sys

import numpy as np

from tools import bench_packed


def test_help_runs_without_gpu():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run(
        [sys.executable, os.path.join(repo, "tools", "bench_packed.py"),
         "--help"], capture_output=True, text=True, timeout=90, cwd=repo)
    assert res.returncode == 0, res.stderr[-400:]
    for flag in ("--json", "--gpu", "--rounds", "--dists"):
        assert flag in res.stdout
    for dist in bench_packed.DISTS:
        assert dist in res.stdout


def test_length_distributions():
    C, n = 200, 1024
    full = bench_packed.draw_lengths("full", n, C, np.random.default_rng(0))
    assert full.tolist() == [C] * n
    short = bench_packed.draw_lengths("short", n, C, np.random.default_rng(0))
    again = bench_packed.draw_lengths("short", n, C, np.random.default_rng(0))
    assert np.array_equal(short, again)
    assert short.min() >= 1 and short.max() <= C
    assert 30 < short.mean() < 50
    tail = bench_packed.draw_lengths("longtail", n, C,
                                     np.random.default_rng(0))
    assert int((tail == 10 * C).sum()) == 10
    assert int((tail > C).sum()) == 10 and tail.min() >= 1
