"""Leg-odometry parameter sweeps above the C ABI and below it: LegOdoHandler::setSweep (tests/cpp/test_leg_param_sweep.cpp),
examples/leg_noise_sweep.c, the binding's shape check -- and, on the CPU tier, the ISA hipcc emits for the pair kernels that read the
per-filter block (pb_legpar.hip: k_pair_legpar / k_pair_quad_legpar), held to what tests/test_isa_hazard.py asks of their scalar siblings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pronto_amd import _lib
from test_isa_hazard import ROOT, _asm, _kernel_metadata


def sweep_exe(oracle):
    from test_cpp_shim import build_exe
    return build_exe(oracle, "test_leg_param_sweep")


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [15, 21])
def test_parameter_block_pair_kernels_keep_their_siblings_budget(ns):
    """pb_legpar.hip compiles for gfx950 with nine kernels per object (three modes x three cache policies); two waves per SIMD --
    <= 256 registers, no AGPRs -- and no more scratch than tests/test_isa_hazard.py allows k_step_leg / k_step_quad_leg: none for 15
    states (80 bytes in pos_and_lin_rate), 64 bytes for 21; the 16-byte-store guard holds."""
    path = _asm("pb_legpar%d.s" % ns, "pb_legpar.hip", "-DPB_LEG_NS=%d" % ns)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "chk_store_hazard.py"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert int(r.stdout.strip().splitlines()[-1].split()[1]) > 100      # the kernels' row stores really were in that file
    meta = _kernel_metadata(path)
    assert len(meta) == 9 and all(("k_pair_legpar" if ns == 15 else "k_pair_quad_legpar") in k for k in meta), sorted(meta)
    for name in meta:     # the names the scalar kernels' tests and profiles key on do not match the new ones
        assert "k_step_leg" not in name and "k_step_quad_leg" not in name and "k_legodo" not in name, name
    for name, (vgpr, agpr, scratch) in meta.items():
        assert vgpr <= 256 and agpr == 0, (name, vgpr, agpr)
        six2 = "ELi2EEEv" in name and ns == 15      # <15, MH, SIX = 2>: pos_and_lin_rate
        assert scratch <= (64 if ns == 21 else 80 if six2 else 0), (name, scratch)


def test_noise_sweep_example_links():
    from test_c_example import build
    build("leg_noise_sweep")


def test_binding_refuses_misshaped_blocks():
    """BatchEstimator.legodo_set_param_block raises ValueError before any call into the library (no context here: any call would fail
    differently)"""
    from pronto_amd.batch import BatchEstimator
    est = object.__new__(BatchEstimator)
    est.B = 100
    est._h = None
    for bad in (np.zeros((_lib.PB_LEGPAR_ROWS, 99)), np.zeros((_lib.PB_LEGPAR_ROWS - 1, 100)), np.zeros(_lib.PB_LEGPAR_ROWS * 100),
                np.zeros((100, _lib.PB_LEGPAR_ROWS)), [[0.0] * 100] * _lib.PB_LEGPAR_ROWS):
        with pytest.raises(ValueError):
            est.legodo_set_param_block(bad)
    assert _lib.PB_LEGPAR_ROWS == 11 and _lib.PB_LEGPAR_R_VXYZ == 0 and _lib.PB_LEGPAR_STANDING_SCHMITT_LEVEL == 10
    assert "pb_legodo_set_param_block" in _lib.exported_names()


def test_set_sweep_refuses_unknown_keys_and_wrong_lengths_host_only(oracle):
    r = subprocess.run([sweep_exe(oracle), "host"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("args", [["fuse"], ["nofuse"], ["fuse", "late"]])
def test_handler_sweep_equals_batches_of_one_on_gpu(oracle, n, args):
    """one robot's IMU + joint-state log into 96 filters with setSweep on r_vxyz and schmitt_high_threshold: filters 0, 47 and 95 are
    what a batch of one computes when its .cfg carries their values (relative 1e-12); with fuse_ins_legodo on and off, and with a
    late VO message every 10th tick that forces a replay of the kept leg-odometry update."""
    from test_cpp_shim import NARG
    r = subprocess.run([sweep_exe(oracle)] + args + NARG[n], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_noise_sweep_example_runs_on_gpu():
    from test_c_example import build
    r = subprocess.run([build("leg_noise_sweep")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
