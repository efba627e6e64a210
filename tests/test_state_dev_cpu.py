"""The device-state entry points as far as a machine without a GPU can check them: the library exports them, the ctypes mirror of
KStateDev has the header's size, and BranchRollouts' candidate layout is the documented one (include/kmanip.h).
tests/test_abi.py compares the header, exports.map, lib.EXPORTS and the symbol table name by name; tests/test_state_dev_gpu.py runs
the kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from gym_kmanip_amd import lib as klib

NEW = ("kmanip_get_state_dev", "kmanip_set_state_dev", "kmanip_copy_envs", "kmanip_state_index_errors")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(klib.LIB_PATH):
        klib.build()
    return klib.load()


def test_library_exports_the_state_entry_points(L):
    for name in NEW:
        assert name in klib.EXPORTS, name
        assert hasattr(L, name), name
    assert (klib.KM_COPY_EPISODE, klib.KM_COPY_ENV_PARAMS) == (1, 2)


def test_kstatedev_mirror_is_six_pointers():
    assert C.sizeof(klib.KStateDev) == 6 * C.sizeof(C.c_void_p)
    assert [f[0] for f in klib.KStateDev._fields_] == ["qpos", "qvel", "ctrl", "qacc_warm", "step_idx", "episode"]


@pytest.mark.parametrize("n,k", [(1, 1), (3, 5), (70, 3)])
def test_branch_indices_candidate_layout(n, k):
    """Candidate j of real env e is plan env e * k + j: dst is 0 .. n*k-1 in order, src[e * k + j] = e."""
    from gym_kmanip_amd.pipeline import branch_indices
    src, dst = branch_indices(n, k)
    assert src.dtype == np.int32 and dst.dtype == np.int32 and src.shape == dst.shape == (n * k,)
    assert np.array_equal(dst, np.arange(n * k))
    for e in range(n):
        for j in range(k):
            assert src[e * k + j] == e
    assert np.array_equal(src.reshape(n, k), np.arange(n)[:, None].repeat(k, axis=1))


def test_branch_indices_rejects_empty():
    from gym_kmanip_amd.pipeline import branch_indices
    with pytest.raises(ValueError):
        branch_indices(0, 3)
    with pytest.raises(ValueError):
        branch_indices(3, 0)
