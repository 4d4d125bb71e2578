"""CPU: the occupancy-grid entry points of the `_raymarching_face` shim exist as real functions, training stays refused, and the Python surface of the
device rebuild rejects what it cannot serve before anything reaches the GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
GRID_NAMES = ("morton3D", "morton3D_invert", "packbits", "morton3D_dilation")
TRAINING_NAMES = ("sph_from_ray", "march_rays_train", "march_rays_train_backward", "composite_rays_train_forward", "composite_rays_train_backward",
                  "composite_rays", "composite_rays_ambient", "composite_rays_train_sigma_forward", "composite_rays_train_sigma_backward",
                  "composite_rays_ambient_sigma", "composite_rays_train_uncertainty_forward", "composite_rays_train_uncertainty_backward",
                  "composite_rays_uncertainty", "composite_rays_train_triplane_forward", "composite_rays_train_triplane_backward")


def _rm():
    d = os.path.join(ROOT, "mere-fusion_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    import _raymarching_face
    return _raymarching_face


def test_grid_entry_points_are_real_functions(lib_built):
    rm = _rm()
    refusing = rm.march_rays_train.__code__
    for n in GRID_NAMES:
        f = getattr(rm, n)
        assert callable(f) and f.__name__ == n and f.__code__ is not refusing, n
        assert f.__closure__ is None, f"{n} is still the refusing closure"
    # they check their tensors like the other entry points: a CPU tensor raises as the extension's CHECK_CUDA would
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        rm.morton3D(torch.zeros(4, 3, dtype=torch.int32), 4, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        rm.packbits(torch.zeros(1, 16), 2, 0.5, torch.zeros(2, dtype=torch.uint8))


def test_training_entry_points_still_refuse(lib_built):
    rm = _rm()
    for n in TRAINING_NAMES:
        with pytest.raises(RuntimeError) as e:
            getattr(rm, n)()
        assert str(e.value) == f"_raymarching_face.{n}: training / occupancy-grid maintenance is outside the MI355X inference path"


def test_update_density_grid_rejects_what_it_cannot_serve(lib_built):
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    r = HipHeadRenderer(None, torch.zeros(32 ** 3 // 8, dtype=torch.uint8), grid_size=32)
    with pytest.raises(RuntimeError, match="density_grid must be a CUDA tensor"):
        r.update_density_grid(torch.zeros(1, 32 ** 3), torch.zeros(1, 32))
    r = HipHeadRenderer(None, torch.zeros(48 ** 3 // 8, dtype=torch.uint8), grid_size=48)
    with pytest.raises(RuntimeError, match="grid_size 48 is not served \\(32, 64 or 128\\)"):
        r.update_density_grid(torch.zeros(1, 48 ** 3), torch.zeros(1, 32))
    r = HipHeadRenderer(None, torch.zeros(32 ** 3 // 8, dtype=torch.uint8), grid_size=32)
    with pytest.raises(RuntimeError, match="cascades 9 outside 1..8"):
        r.update_density_grid(torch.zeros(9, 32 ** 3), torch.zeros(1, 32), cascades=9)


def test_library_refuses_null_and_oversized_arguments(lib_built):
    """The C entry points check their arguments before they touch the device (the grid-size limit of mf_nerf_density_grid_update needs a real field handle:
    tests/test_ernerf_occupancy.py::test_library_names_the_grid_size_limit)."""
    import ctypes as C
    from mere_fusion_amd import _lib
    l = _lib.lib()
    one = C.c_void_p(16)                     # non-null stand-ins: the arguments are checked, never dereferenced
    assert l.mf_nerf_density_grid_update(None, one, one, 1, 128, 1.0, one, 0.0, 0, 1.0, 0.95, 10.0, None, one, None, one, None) == -1
    assert b"null" in l.mf_last_error()
    assert l.mf_morton3d(None, 4, None, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_morton3d_dilation(one, 1, 2048, C.c_void_p(32), None) == -1 and b"H <= 1024" in l.mf_last_error()
