"""CPU: the two grid-maintenance entry points added beside mf_nerf_density_grid_update are in the ABI table, check their arguments before they touch the
device, and state the served grid sizes in one place (mf_nerf_occupancy_shape in the library, HipHeadRenderer.check_grid_size in Python), named in the error."""
import ctypes as C
import glob
import os

import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("mf_nerf_torso_grid_update", "mf_nerf_mark_untrained", "mf_nerf_torso_set_grid")


def test_abi_table_has_the_new_symbols(lib_built):
    from mere_fusion_amd import _lib
    lib = C.CDLL(lib_built)
    for n in NEW:
        assert n in _lib.SIGNATURES and n in _lib.HEADER.functions and hasattr(lib, n), n
    assert _lib.lib().mf_abi_version() == 4


def test_library_checks_arguments_before_the_device(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    one = C.c_void_p(16)                     # non-null stand-ins: the arguments are checked, never dereferenced
    K = (1.0, 1.0, 0.5, 0.5)
    assert l.mf_nerf_mark_untrained(one, 1, *K, 1.0, 1, 48, one, None) == -1
    assert b"nerf_mark_untrained: grid_size 48 is not served (32, 64 or 128)" in l.mf_last_error()
    assert l.mf_nerf_mark_untrained(one, 1, *K, 1.0, 9, 32, one, None) == -1 and b"nerf_mark_untrained: cascades 9 outside 1..8" in l.mf_last_error()
    assert l.mf_nerf_mark_untrained(one, 0, *K, 1.0, 1, 32, one, None) == -1 and b"at least one pose" in l.mf_last_error()
    assert l.mf_nerf_mark_untrained(None, 1, *K, 1.0, 1, 32, one, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_nerf_torso_grid_update(None, one, None, 0.95, one, one, None, one, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_nerf_torso_set_grid(None, one) == -1 and b"null" in l.mf_last_error()


def test_served_sizes_are_stated_in_one_place(lib_built):
    pkg = os.path.join(ROOT, "mere-fusion_amd")
    count = lambda pattern: sum(open(f).read().count("is not served (") for f in glob.glob(os.path.join(pkg, pattern)))
    assert count("csrc/*") == 1 and count("ernerf/*.py") == 1
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    from mere_fusion_amd.ernerf.torso import HipTorso
    assert HipHeadRenderer.GRID_SIZES == (32, 64, 128)
    r = HipHeadRenderer(None, torch.zeros(48 ** 3 // 8, dtype=torch.uint8), grid_size=48)
    with pytest.raises(RuntimeError, match=r"HipHeadRenderer.mark_untrained: grid_size 48 is not served \(32, 64 or 128\)"):
        r.mark_untrained(torch.zeros(1, 48 ** 3), torch.zeros(1, 4, 4), (1.0, 1.0, 0.5, 0.5))
    r = HipHeadRenderer(None, torch.zeros(32 ** 3 // 8, dtype=torch.uint8), grid_size=32)
    with pytest.raises(RuntimeError, match="density_grid must be a contiguous float32 CUDA tensor"):
        r.mark_untrained(torch.zeros(1, 32 ** 3), torch.zeros(1, 4, 4), (1.0, 1.0, 0.5, 0.5))
    t = HipTorso.__new__(HipTorso)           # the size rule needs no handle
    t.grid_size = 48
    with pytest.raises(RuntimeError, match=r"HipTorso.update_density_grid: grid_size 48 is not served \(32, 64 or 128\)"):
        t.update_density_grid(torch.zeros(48 * 48), torch.eye(4)[None], None, None)
