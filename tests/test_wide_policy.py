"""wide_update_choice (pronto_amd/csrc/pb_policy.hpp), the kernel choice of pb_update_indexed_wide, on the CPU: up to six rows it answers
what update_choice answers -- for every combination tests/test_kernel_policy.py's table tests walk -- and for seven to nine rows
UPD_WIDE, never the argument form.  UPD_WIDE is the last enumerator of UpdateFamily.  tests/cpp/wide_policy.cpp, plain g++."""
import os
import subprocess

import pytest

import update_exact as ue
from test_kernel_policy import BUILDS, HEADER, MAPPING, R_BROADCAST, R_DIAG, R_FULL, R_KIND, ROOT, update_query
from test_update_ill_conditioned import _cases

H = ue.HANDLER_LISTS
MAPS = ("lane15", "coop15", "quad21", "coop21")


def build_exe(build):
    exe = os.path.join(ROOT, "tests", "build", "wide_policy_" + build)
    src = os.path.join(ROOT, "tests", "cpp", "wide_policy.cpp")
    deps = [src, HEADER, os.path.join(ROOT, "include", "pronto_batch.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", '-DPOLICY_HEADER="%s"' % HEADER] + BUILDS[build]
                              + ["-o", exe, src])
    return exe


def ask(build, queries=None, mode="query"):
    r = subprocess.run([build_exe(build), mode], input="".join(q + "\n" for q in queries or []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert queries is None or len(out) == len(queries)
    return out


def narrow_queries():
    """every m <= 6 combination the table tests of test_kernel_policy.py walk"""
    q = []
    for mapping, n, idx, orient, kind, _ in _cases():
        pm, generic = MAPPING[(mapping, n)]
        q += [update_query(pm, generic, idx, orient, R_KIND[kind], 0, masked) for masked in (0, 1)]
    for pm, n in (("lane15", 15), ("coop15", 15), ("quad21", 21), ("coop21", 21)):
        other = ue.EXTRA_LISTS[n] + [(idx, not o) for idx, o in H[3:10]] + [([5, 4, 3], False), ([9, 10, 11, 5, 4, 3], False), ([3, 4, 5, 0, 1], False)]
        q += [update_query(pm, 0, idx, o, rkind) for idx, o in other for rkind in (R_BROADCAST, R_DIAG, R_FULL)]
    for pm in MAPS:
        for idx, o in H:
            for generic in (0, 1):
                for all_bc, rkind in ((0, R_BROADCAST), (0, R_DIAG), (0, R_FULL), (1, R_BROADCAST), (1, R_FULL)):
                    q += [update_query(pm, generic, idx, o, rkind, all_bc, masked) for masked in (0, 1)]
    return q


@pytest.mark.parametrize("build", list(BUILDS))
def test_up_to_six_rows_answer_update_choice(build):
    queries = narrow_queries()
    assert len(queries) > 1000
    for q, line in zip(queries, ask(build, queries)):
        w = line.split()
        assert w[0] == "wide" and w[4] == "narrow" and w[1:4] == w[5:8], (q, line)


@pytest.mark.parametrize("build", list(BUILDS))
def test_seven_to_nine_rows_run_the_wide_kernel(build):
    wide, old = ask(build, mode="enum")[0].split(" | ")
    assert all(int(wide) > int(o) for o in old.split()) and len(old.split()) == 7
    lists = [list(range(3, 12)), [17, 3, 9, 10, 11, 15, 20], [0, 14, 3, 9, 10, 11, 8, 6], [9, 10, 11, 6, 7, 8, 15, 16, 17]]
    queries = [update_query(pm, generic, idx, o, rkind, all_bc, masked) for pm in MAPS for idx in lists if pm.endswith("21") or max(idx) < 15
               for generic in (0, 1) for o in (0, 1) for rkind in (R_BROADCAST, R_DIAG, R_FULL) for all_bc in (0, 1) for masked in (0, 1)]
    assert ask(build, queries) == ["wide %s -1 0" % wide] * len(queries)
