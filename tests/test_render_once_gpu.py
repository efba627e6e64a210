"""The render kernels with and without link capsules are instantiations of one body each (run with -m gpu on
an MI355X): label_cast<.., LINKS> of kmanip_render_label_cast.hpp is k_render_labels and k_render_links, and
k_render_points<.., LINKS> has been one template since section 16.  What couples them is checked here: a capsule list that every
camera masks out (cam_mask = 0: every rectangle is empty, no capsule is ever tested) must give the bytes of no list at all.  The
library of the commit before section 33 passes all twelve cases too.
Since section 35 k_render_depth, k_render_depth_links and k_render_points are one source text, kmanip_render_depth_cast.inc, and
the depth images of the four routes through it are held to each other byte for byte (six more cases; the library of the commit
before section 35, the same device code, passes them)."""
import ctypes as C

import numpy as np
import pytest

from gym_kmanip_amd import model as M
from gym_kmanip_amd.model import KM_CAM_INDEX
from test_kernel_paths_gpu import _cams, _stepped

pytestmark = pytest.mark.gpu

N = 4
# COLFIXED and the quad path; the general loop with width % 4 != 0; one pixel
SHAPES = [(64, 64), (30, 50), (1, 1)]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", params=["off", "camera_offset"])
def handle(request):
    """KManipSoloArm, 4 envs after 12 random steps; "camera_offset": explicit per-env camera offsets (the VIS kernels)."""
    dev, _ = _stepped("KManipSoloArm", N, 6, 12)
    if request.param == "camera_offset":
        dev.set_visual_params(camera_offset=np.random.default_rng(5).uniform(-0.06, 0.06, (N, 3)))
    masked = [dict(c, cam_mask=0) for c in M.link_capsules(dev.cm)]
    assert masked
    yield dev, masked
    dev.k_close()


def _labels(dev, cam, h, w, with_rgb):
    """One kmanip_render_labels_multi launch of one job: (rgb or None, seg)."""
    torch = _torch()
    seg = torch.full((N, h, w), 255, dtype=torch.uint8, device=dev.device)
    rgb = torch.full((N, h, w, 3), 255, dtype=torch.uint8, device=dev.device) if with_rgb else None
    one = lambda v: (C.c_int32 * 1)(v)
    ptr = lambda t: (C.c_void_p * 1)(t.data_ptr())
    dev._check(dev.L.kmanip_render_labels_multi(dev.h, 1, one(KM_CAM_INDEX[cam]), one(h), one(w), ptr(rgb) if with_rgb else None, ptr(seg),
                                                dev._stream()), "kmanip_render_labels_multi")
    return rgb, seg


def _points(dev, cam, h, w, frame):
    torch = _torch()
    depth = torch.full((N, h, w), -1.0, dtype=torch.float32, device=dev.device)
    xyz = dev.render_points(cam, h, w, frame=frame, depth_out=depth)
    return xyz, depth


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_list_is_no_list_in_the_label_kernels(handle, shape):
    """k_render_links with a list no camera shows against k_render_labels: RGB and labels from one launch, and labels only."""
    torch = _torch()
    dev, masked = handle
    h, w = shape
    for cam in _cams(dev.cm):
        dev.set_render_links(None)
        want = {rgb: _labels(dev, cam, h, w, rgb) for rgb in (True, False)}
        dev.set_render_links(masked)
        for with_rgb in (True, False):
            rgb, seg = _labels(dev, cam, h, w, with_rgb)
            assert torch.equal(seg, want[with_rgb][1]), (cam, h, w, with_rgb, "labels")
            if with_rgb:
                assert torch.equal(rgb, want[True][0]), (cam, h, w, "rgb")
    dev.set_render_links(None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_list_is_no_list_in_the_point_kernels(handle, shape):
    """k_render_points<.., LINKS = true> with a list no camera shows (the depth flag on) against LINKS = false (the flag off), in
    both frames with depth_out."""
    torch = _torch()
    dev, masked = handle
    h, w = shape
    dev.set_render_links(masked)
    for cam in _cams(dev.cm):
        for frame in ("world", "camera"):
            dev.set_depth_links(False)
            xyz0, depth0 = _points(dev, cam, h, w, frame)
            dev.set_depth_links(True)
            xyz1, depth1 = _points(dev, cam, h, w, frame)
            assert torch.equal(xyz1.view(torch.int32), xyz0.view(torch.int32)), (cam, h, w, frame, "xyz")
            assert torch.equal(depth1.view(torch.int32), depth0.view(torch.int32)), (cam, h, w, frame, "depth")
    dev.set_depth_links(False)
    dev.set_render_links(None)


# The four routes to a depth image that the one text of kmanip_render_depth_cast.inc feeds, by kernel
DEPTH_ROUTES = ("k_render_depth", "k_render_depth_links", "k_render_points<LINKS=false>", "k_render_points<LINKS=true>")
# ... and the pairs of them held to each other byte for byte: every pair that is byte-equal on the library of the commit before
# section 35, whose device code is this one's instruction for instruction.  That is all six: no pair is left out
DEPTH_PAIRS = [(a, b) for i, a in enumerate(DEPTH_ROUTES) for b in DEPTH_ROUTES[i + 1:]]


def _depth_routes(dev, masked, cam, h, w):
    """The depth image of one camera by each route: render_depth and depth_out of render_points, without a list (the depth flag
    off) and with the list every camera masks out (the flag on)."""
    out = {}
    dev.set_render_links(None)
    dev.set_depth_links(False)
    out["k_render_depth"] = dev.render_depth(cam, h, w)
    out["k_render_points<LINKS=false>"] = _points(dev, cam, h, w, "world")[1]
    dev.set_render_links(masked)
    dev.set_depth_links(True)
    out["k_render_depth_links"] = dev.render_depth(cam, h, w)
    out["k_render_points<LINKS=true>"] = _points(dev, cam, h, w, "world")[1]
    dev.set_depth_links(False)
    dev.set_render_links(None)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_depth_routes_of_the_one_cast_agree(handle, shape):
    """k_render_depth, k_render_depth_links and both k_render_points instantiations are one text: with no capsule to test, the
    depth images they write are the same bytes."""
    torch = _torch()
    dev, masked = handle
    h, w = shape
    for cam in _cams(dev.cm):
        d = _depth_routes(dev, masked, cam, h, w)
        for a, b in DEPTH_PAIRS:
            ne = int((d[a].view(torch.int32) != d[b].view(torch.int32)).sum())
            print("%s %dx%d  %s | %s: %d pixels differ, max |diff| %.3g" % (cam, h, w, a, b, ne, float((d[a] - d[b]).abs().max())))
            assert ne == 0, (cam, h, w, a, b)
