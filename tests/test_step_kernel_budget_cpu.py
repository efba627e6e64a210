"""Register and LDS budget of the shipped per-step kernels, parsed from the built library with tools/kernel_resources.py (no GPU).

The single-arm Newton kernel k_step<10,16,1,4,false> (the headline launch: 1024 single-wave workgroups, one per SIMD, four per CU)
must not need more than it did before its forward kinematics moved its link-frame exchange into registers: 384 VGPRs, 128 AGPRs,
35 168 bytes of LDS per workgroup, no scratch.  The two-arm Newton per-step kernels, which that change does not touch, stay within
432 + 176 registers without scratch (the compiler this was written with allots them 428 + 172, before that change and after it: the
figures are ceilings, not equalities)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

ONE_ROW_NEWTON = dict(vgpr=384, agpr=128, lds=35168)
TWO_ARM = dict(vgpr=432, agpr=176)


def _rows():
    import build_matrix as BM
    so = os.path.join(ROOT, "gym_kmanip_amd", "libkmanip_hip.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    rows = {}
    for k in BM.kernels(so, "k_step"):
        nl, g, solver, epb, chunk = k.args
        rows[(nl, g, solver, epb, int(chunk))] = dict(vgpr=k.vgpr, agpr=k.agpr, scratch=k.scratch, lds=k.lds)
    return rows


def test_one_row_newton_step_kernel_stays_inside_its_budget():
    r = _rows()[(10, 16, 1, 4, 0)]
    print("\nk_step<10,16,1,4,false>: %s" % r)
    assert r["vgpr"] <= ONE_ROW_NEWTON["vgpr"] and r["agpr"] <= ONE_ROW_NEWTON["agpr"]
    assert r["vgpr"] + r["agpr"] <= 512
    assert r["lds"] <= ONE_ROW_NEWTON["lds"] and 4 * r["lds"] <= 160 * 1024
    assert r["scratch"] == 0


def test_two_arm_per_step_kernels_keep_their_registers():
    rows = _rows()
    two_arm = {k: v for k, v in rows.items() if k[0] == 20 and k[2] == 1 and k[4] == 0}
    assert len(two_arm) == 2, sorted(two_arm)          # one and two envs per wave
    for k, r in two_arm.items():
        print("\nk_step<%d,%d,%d,%d,false>: %s" % (k[:4] + (r,)))
        assert r["vgpr"] <= TWO_ARM["vgpr"] and r["agpr"] <= TWO_ARM["agpr"], (k, r)
        assert r["scratch"] == 0, (k, r)
