"""Which kernel runs, checked on the CPU: pronto_amd/csrc/pb_policy.hpp holds every decision of a kernel, a grid shape or a cache policy
(pb_create makes one Policy per context; the launchers switch on its answers), and tests/cpp/policy_table.cpp prints those answers
without HIP or the library.  Built with g++ like estimator_trace, plain and with -fsanitize=address,undefined.

tests/golden/kernel_policy/contexts.txt is the policy of 828 contexts -- both state sizes, batches on both sides of every threshold,
every switch unset / at each documented value / out of range, the combinations the GPU tests run -- as the code of pb_create, pb_hot_kernel
and the smoother launchers decided them BEFORE the header existed (recorded by compiling those lines as they stood into the same driver).
It is the record that the move changed no decision and is not to be regenerated from the header it checks."""
import os
import subprocess

import pytest

import update_exact as ue
from test_update_ill_conditioned import CORR_NAME, _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pronto_amd", "csrc", "pb_policy.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_policy")
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
H = ue.HANDLER_LISTS
R_BROADCAST, R_DIAG, R_FULL = 0, 1, 2                       # enum pb_rkind
R_KIND = {"host": R_BROADCAST, "diag": R_DIAG, "full": R_FULL}
# the mapping a case of test_update_ill_conditioned.py names -> (policy mapping, generic_update)
MAPPING = {("generic", 15): ("coop15", 1), ("default", 15): ("coop15", 0), ("generic", 21): ("quad21", 1), ("default", 21): ("quad21", 0),
           ("quad21=0", 21): ("coop21", 0)}


def build_exe(build):
    exe = os.path.join(ROOT, "tests", "build", "policy_table_" + build)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "policy_table.cpp")
    deps = [src, HEADER, os.path.join(ROOT, "include", "pronto_batch.h")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", '-DPOLICY_HEADER="%s"' % HEADER] + BUILDS[build]
                          + ["-o", exe, src])
    return exe


def run(build, mode, stdin="", env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("PRONTO_")}
    e.update(env or {})
    r = subprocess.run([build_exe(build), mode], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=e)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    return r.stdout.splitlines()


def ask(build, queries, env=None):
    out = run(build, "query", "".join(q + "\n" for q in queries), env)
    assert len(out) == len(queries)
    return out


def update_query(mapping, generic, idx, orient, rkind, all_broadcast=0, masked=0):
    return "update %s %d %d %d %d %d %s" % (mapping, generic, orient, rkind, all_broadcast, masked, " ".join(str(i) for i in idx))


def rt_kernel(n, idx, orient):
    """the run-time-index family of a state size"""
    if n == 21:
        return "k_update_quad_rt<%d>" % len(idx)
    return "k_update_lane_rt<15,%d,%s>" % (len(idx), str(bool(orient)).lower()) if len(idx) <= 4 else "k_update_coop_rt<%d>" % len(idx)


@pytest.mark.parametrize("build", list(BUILDS))
def test_context_policies_equal_golden(build):
    got = run(build, "contexts")
    with open(os.path.join(GOLDEN, "contexts.txt")) as f:
        want = f.read().splitlines()
    assert len(want) == 828
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff and len(got) == len(want), "%d lines differ, first:\n  got:    %s\n  golden: %s" % ((len(diff),) + (diff[0] if diff else ("", "")))


@pytest.mark.parametrize("build", list(BUILDS))
def test_hot_kernel_names(build):
    """pb_hot_kernel's twelve names, byte for byte as include/pronto_batch.h documents them"""
    want = ["%s %d %s" % (m, h, fmt % h) for m, fmt in (("lane15", "k_step<15,true,%d>"), ("coop15", "k_step_coop<15,true,%d>"),
                                                       ("coop21", "k_step_coop<21,true,%d>"), ("quad21", "k_step_quad<true,%d>")) for h in range(3)]
    assert run(build, "names") == want
    # k_update_coop_rt / k_update_quad_rt / k_update_quad_list are built for two cache policies: non-temporal falls back to the default
    assert run(build, "hints") == ["0 1 0"]


@pytest.mark.parametrize("build", list(BUILDS))
def test_update_choice_names_the_kernel_each_gpu_case_means_to_run(build):
    """every case of test_update_ill_conditioned.py's table, without and with a mask: the policy names the kernel the table names, and
    none of them takes the argument form (their z is a per-filter block)"""
    cases = _cases()
    assert len(cases) >= 100
    queries, want = [], []
    for mapping, n, idx, orient, kind, kernel in cases:
        pm, generic = MAPPING[(mapping, n)]
        for masked in (0, 1):
            queries.append(update_query(pm, generic, idx, orient, R_KIND[kind], 0, masked))
            want.append(kernel + " host_args=0")
    assert ask(build, queries) == want


@pytest.mark.parametrize("build", list(BUILDS))
def test_lists_without_a_compile_time_kernel_fall_through(build):
    """a list the handlers' table lacks for a mapping -- another list, the right list with the orientation measurement missing or
    unwanted, a six-row list on the two-role 21-state mapping -- runs on the run-time-index family of its state size"""
    queries, want = [], []
    for pm, n in (("lane15", 15), ("coop15", 15), ("quad21", 21), ("coop21", 21)):
        other = ue.EXTRA_LISTS[n] + [(idx, not o) for idx, o in H[3:10]] + [([5, 4, 3], False), ([9, 10, 11, 5, 4, 3], False), ([3, 4, 5, 0, 1], False)]
        if n == 15:
            other.append(([3, 4, 5, 0, 1, 2], True))
        for idx, o in other:
            for rkind in (R_BROADCAST, R_DIAG, R_FULL):
                queries.append(update_query(pm, 0, idx, o, rkind))
                want.append(rt_kernel(n, idx, o) + " host_args=0")
    # PRONTO_BATCH_QUAD21=0: no six-row kernel on the two-role mapping ...
    for idx, o in (H[2], H[3], H[8]):
        for all_bc in (0, 1):
            queries.append(update_query("coop21", 0, idx, o, R_BROADCAST, all_bc))
            want.append("k_update_quad_rt<6> host_args=0")
    # ... while lin_rot_rate's list keeps its 21-state list kernel on either mapping, with or without an orientation measurement, as it
    # did before the policy header (pbk_update21_m6 looked at the list and at PRONTO_BATCH_GENERIC_UPDATE only)
    for pm in ("quad21", "coop21"):
        for o in (0, 1):
            queries += [update_query(pm, 0, H[10][0], o, R_DIAG), update_query(pm, 1, H[10][0], o, R_DIAG)]
            want += ["k_update_quad_list<.,3,4,5,0,1,2> host_args=0", "k_update_quad_rt<6> host_args=0"]
    assert ask(build, queries) == want


def ct_kernel(pm, idx, orient):
    """the compile-time kernel of a handler list on a mapping, None where there is none"""
    k = H.index((idx, orient))
    if k == 10:
        return "k_update_lane<15,6,IdxVelOmega>" if pm in ("lane15", "coop15") else None
    if pm in ("lane15", "coop15"):
        return "k_step_coop<15,false,.,%s>" % CORR_NAME[k]
    if pm == "quad21":
        return "k_update_quad<%s>" % CORR_NAME[k]
    return "k_step_coop<21,false,.,%s>" % CORR_NAME[k] if len(idx) <= 4 else None


@pytest.mark.parametrize("build", list(BUILDS))
def test_argument_form_exactly_under_its_three_conditions(build):
    """z, R and the quaternion travel as kernel arguments exactly when every input is a PB_HOST_BROADCAST value (R a broadcast diagonal),
    no mask came with it and a compile-time kernel takes the list (none does under PRONTO_BATCH_GENERIC_UPDATE=1)"""
    queries, want = [], []
    for pm in ("lane15", "coop15", "quad21", "coop21"):
        for idx, o in H:
            for generic in (0, 1):
                for all_bc, rkind in ((0, R_BROADCAST), (0, R_DIAG), (0, R_FULL), (1, R_BROADCAST), (1, R_FULL)):
                    for masked in (0, 1):
                        ct = None if generic else ct_kernel(pm, idx, o)
                        queries.append(update_query(pm, generic, idx, o, rkind, all_bc, masked))
                        want.append("host_args=%d" % (ct is not None and all_bc == 1 and rkind == R_BROADCAST and not masked))
    got = ask(build, queries)
    assert [g.split()[1] for g in got] == want
    assert sum(w == "host_args=1" for w in want) == 11 + 11 + 10 + 7


@pytest.mark.parametrize("build", list(BUILDS))
def test_legodo_correct_argument_form(build):
    """pb_step_legodo_correct passes one robot's correction as kernel arguments for 15 states, on the four-wave mapping, and for POS_YAW
    on the two-wave 21-state mapping; POS_ORIENT there has no six-row kernel that takes them (enum pb_corr: POS_ORIENT 0, POS_YAW 1)"""
    maps = ("lane15", "coop15", "quad21", "coop21")
    got = ask(build, ["args %s %d" % (pm, kind) for pm in maps for kind in (0, 1)])
    assert got == ["1", "1", "1", "1", "1", "1", "0", "1"]


@pytest.mark.parametrize("build", list(BUILDS))
def test_pair_replay_and_smoother_kernels(build):
    maps = ("lane15", "coop15", "coop21", "quad21")
    # a pair kernel: the two-wave 15-state and the four-wave 21-state mapping; with the world constraint on, mode pos_and_lin_rate (2) only
    got = ask(build, ["pair %s %d %d" % (pm, wc, mode) for pm in maps for wc in (0, 1) for mode in (0, 1, 2)])
    assert got == [str(int(pm in ("coop15", "quad21") and (not wc or mode == 2))) for pm in maps for wc in (0, 1) for mode in (0, 1, 2)]
    # the replay kernel: the one-lane kernel only when asked for, for 15 states, without write-through
    got = ask(build, ["replay %s %d %d" % (pm, one, wt) for pm in maps for one in (0, 1) for wt in (0, 1)])
    want = {"lane15": "k_replay_coop<15>", "coop15": "k_replay_coop<15>", "coop21": "k_replay_coop<21>", "quad21": "k_replay_quad<1>"}
    assert got == ["k_replay_fused<15>" if (pm.endswith("15") and one and not wt) else want[pm] for pm in maps for one in (0, 1) for wt in (0, 1)]
    # the smoother and the wide kernel's grid: min(tiles, workgroups asked for or one per CU)
    q = ["smooth coop15 1024 256", "smooth coop15 100 256", "smooth quad21 1024 256", "smooth lane15 1024 304"]
    assert ask(build, q) == ["k_smooth_wide<15> 256", "k_smooth_wide<15> 100", "k_smooth_lane 256", "k_smooth_wide<15> 304"]
    assert ask(build, q[:3], {"PRONTO_SMOOTH_KERNEL": "lane"}) == ["k_smooth_lane 256", "k_smooth_lane 100", "k_smooth_lane 256"]
    assert ask(build, q[:3], {"PRONTO_SMOOTH_KERNEL": "reg"}) == ["k_smooth_reg<false> 256", "k_smooth_reg<false> 100", "k_smooth_reg<false> 256"]
    assert ask(build, q[:3], {"PRONTO_SMOOTH_PIVOT": "1"}) == ["k_smooth_reg<true> 256", "k_smooth_reg<true> 100", "k_smooth_reg<true> 256"]
    assert ask(build, q[:2], {"PRONTO_SMOOTH_GRID": "64"}) == ["k_smooth_wide<15> 64", "k_smooth_wide<15> 64"]
