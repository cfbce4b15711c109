"""The predicted-slot step kernels (k_step_coop_pred, k_step_quad_pred: pb_step_pred.hip) on the CPU tier: hipcc's ISA keeps the
16-byte-store guard (rbis_tile_io.hpp stg2: the update overwrites the very registers the predicted rows were just stored from) and
the resource budget of the kernel each one extends:
  k_step_coop_pred<15>  two waves per SIMD, no AGPRs, no scratch (k_step_coop<15>: the same);
  k_step_quad_pred      two waves per SIMD, no AGPRs, <= 16 bytes of scratch -- the bound tests/test_isa_hazard.py holds k_step_quad
                        to (it carries 12 bytes today), so "no scratch" is not asked of the variant either;
  k_step_coop_pred<21>  no scratch, at k_step_coop<21>'s own budget: ONE wave per SIMD (launch bounds 128, 1; 256 VGPRs + AGPRs).
                        Two waves per SIMD is not a budget this two-wave 21-state mapping has ever had (its 15 x 15 sub-matrix alone
                        fills a wave's architectural registers); it is the A/B alternative to k_step_quad (PRONTO_BATCH_QUAD21=0)."""
import os
import subprocess
import sys

from test_isa_hazard import ROOT, _asm, _kernel_metadata


def _dump():
    return _asm("pb_step_pred.s", "pb_step_pred.hip")


def test_pred_kernels_keep_the_store_guard():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "chk_store_hazard.py"), _dump()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert int(r.stdout.strip().splitlines()[-1].split()[1]) > 500


def test_pred_kernels_fit_their_budget():
    meta = _kernel_metadata(_dump())
    pred = {k: v for k, v in meta.items() if k.startswith("_ZN2pb16k_step_coop_pred")}
    assert len(pred) == 6, sorted(meta)   # two state sizes x three cache policies
    for name, (vgpr, agpr, scratch) in pred.items():
        if "ILi15E" in name:
            assert vgpr <= 256 and agpr == 0 and scratch == 0, (name, vgpr, agpr, scratch)
        else:   # (k_step_coop<21>'s own budget: one wave per SIMD, architectural + accumulation registers)
            assert vgpr <= 512 and scratch == 0, (name, vgpr, agpr, scratch)
    quad = {k: v for k, v in meta.items() if k.startswith("_ZN2pb16k_step_quad_pred")}
    assert len(quad) == 3, sorted(meta)   # three cache policies
    for name, (vgpr, agpr, scratch) in quad.items():
        assert vgpr <= 256 and agpr == 0 and scratch <= 16, (name, vgpr, agpr, scratch)
