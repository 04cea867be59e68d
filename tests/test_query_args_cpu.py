"""What GpuScene's five query methods reject before any launch, message by message.

trace_rays, occluded, crossings, distance and march check their arrays the same way (one checker in the package);
this pins the ValueError text of every rejected input, so folding the checks cannot change which one fires first or
what it says.  No GPU and no library call: the scene is a bare object with device = 0, and every input here fails
before the first upload.
"""
import numpy as np
import pytest
import torch

from conftest import load_package

rtm = load_package()

# method -> (the array's name, its width, the verb of the "host memory is not ... in place" text)
QUERIES = {
    "trace_rays": ("rays", 6, "traced"),
    "occluded": ("rays", 6, "traced"),
    "crossings": ("rays", 6, "traced"),
    "distance": ("points", 3, "read"),
    "march": ("rays", 6, "read"),
}
NUMPY_TMM = "tminmax: a C-contiguous float32 array of shape [n, 2], as the rays"


@pytest.fixture(scope="module")
def scene():
    gs = object.__new__(rtm.GpuScene)
    gs._h, gs.device = None, 0
    return gs


def rejected(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


@pytest.mark.parametrize("method", sorted(QUERIES))
def test_array_checks(scene, method):
    name, w, verb = QUERIES[method]
    call = getattr(scene, method)
    good = np.zeros((4, w), np.float32)
    host = f"{name}: a C-contiguous float32 array of shape [n, {w}]"
    dev = f"{name}: a float32 tensor of shape [n, {w}]"
    for bad in (good.astype(np.float64), good.view(np.int32),          # dtype
                np.zeros(4 * w, np.float32), np.zeros((4, w, 1), np.float32),       # rank
                np.zeros((4, w - 1), np.float32), np.zeros((4, w + 1), np.float32),     # width
                np.zeros((4, 2 * w), np.float32)[:, ::2], np.asfortranarray(good)):     # a strided view
        assert rejected(call, bad) == host
        assert rejected(call, bad, sort=True) == host
    for bad in (torch.zeros((4, w), dtype=torch.float64), torch.zeros(4 * w), torch.zeros((4, w + 1))):
        assert rejected(call, bad) == dev
    # a CPU tensor of the right dtype and shape, contiguous or not: the device is checked before the strides
    for bad in (torch.zeros((4, w)), torch.zeros((4, 2 * w))[:, ::2]):
        assert rejected(call, bad) == f"{name}: a tensor on cuda:0 (host memory is not {verb} in place)"
    for bad in ([[0.0] * w], (1.0,) * w, None, 1.0):
        assert rejected(call, bad) == f"{name}: a torch CUDA tensor or a numpy array"


@pytest.mark.parametrize("method", ["occluded", "crossings"])
def test_tminmax_checks(scene, method):
    call = getattr(scene, method)
    rays, tm = np.zeros((4, 6), np.float32), np.zeros((4, 2), np.float32)
    for bad in ([[0.0, 1.0]] * 4, torch.zeros((4, 2)), 1.0,                         # kind
                np.zeros((3, 2), np.float32), np.zeros((4, 3), np.float32), np.zeros(8, np.float32),    # shape
                tm.astype(np.float64), tm.view(np.int32),                           # dtype
                np.zeros((4, 4), np.float32)[:, ::2], np.asfortranarray(tm)):       # a strided view
        assert rejected(call, rays, bad) == NUMPY_TMM
        assert rejected(call, rays, bad, sort=True) == NUMPY_TMM
    # the rays are checked first
    assert rejected(call, rays.astype(np.float64), tm.astype(np.float64)) == "rays: a C-contiguous float32 array of shape [n, 6]"
    assert rejected(call, torch.zeros((4, 6)), tm) == "rays: a tensor on cuda:0 (host memory is not traced in place)"


def test_march_parameter_checks(scene):
    rays = np.zeros((4, 6), np.float32)
    for bad in (0, 4097, True, -1, 1.0, "8", None):
        assert rejected(scene.march, rays, max_steps=bad) == "max_steps: an integer in [1, 4096]"
    assert rejected(scene.march, rays, min_dist=float("nan")) == "min_dist: not NaN"
    assert rejected(scene.march, rays, min_dist=np.float32("nan")) == "min_dist: not NaN"
    for bad in ("x", None, [1.0, 2.0]):
        assert rejected(scene.march, rays, min_dist=bad) == "min_dist: a number"
    # in the order rays, max_steps, min_dist
    assert rejected(scene.march, rays.astype(np.float64), max_steps=0) == "rays: a C-contiguous float32 array of shape [n, 6]"
    assert rejected(scene.march, rays, max_steps=0, min_dist="x") == "max_steps: an integer in [1, 4096]"
