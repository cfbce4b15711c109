"""bench.py's two modes: a plain run prints the headline line and nothing it does not need; --full adds the 1 M-filter legs and
the CPU baselines after the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "PRONTO_BENCH_REHEARSE", "PRONTO_BENCH_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                        "--batch-per-gpu", "4096", *flags], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_has_a_full_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_extra_legs():
    plain = _run()
    full = _run("--full", "--min-timed-ms", "0", "--cpu-seconds", "0.5")
    for d in (plain, full):
        assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 6 and d["warmup"] == 2
    assert "cpu_baseline" not in plain
    assert not any(k.startswith(("cache_", "frac_cache")) for k in plain["roofline"])
    cb = full["roofline"]["cache_busting"]
    assert cb["batch"] == 1 << 20 and cb["nonfinite"] == 0 and 0 < full["roofline"]["frac_cache_busting"] == cb["frac"]
    assert full["roofline"]["cache_blocked"]["batch"] == 1 << 20
    cpu = full["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["parity_max_rel_err"] < 1e-9 and "structured_error" not in cpu
    # the extra legs run after the timed steps: both modes leave the same posterior
    a, b = plain["summary"], full["summary"]
    assert abs(a["sum_loglik"] - b["sum_loglik"]) <= 1e-12 * abs(b["sum_loglik"])
    assert abs(a["checksum_abs"] - b["checksum_abs"]) <= 1e-12 * abs(b["checksum_abs"])
    assert a["nonfinite"] == 0
