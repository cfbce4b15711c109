"""examples/score_sweep.c -- a parameter sweep ranked by drift per distance travelled on the device -- compiles against
include/pronto_batch.h as C99 and, on a GPU, runs and names a winner inside the batch.  Which candidate wins is not asserted."""
import re
import subprocess

import pytest

from test_c_example import build


def test_example_links():
    build("score_sweep")


@pytest.mark.gpu
def test_score_sweep_example_runs_on_gpu():
    exe = build("score_sweep")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    m = re.search(r"best mean %DDT\s*: filter\s+(\d+)", r.stdout)
    assert m and 0 <= int(m.group(1)) < 128
    assert "best log-likelihood" in r.stdout
