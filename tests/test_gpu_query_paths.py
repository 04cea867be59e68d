"""The one launch path of the five queries (csrc/rt_queries.hip launch_query; GpuScene._query) on the GPU.

Scene 1 (the Cornell box, 44 triangles); its 128 primary rays of an 8 x 8 frame at spp 2 followed by a fixed permutation
of them; prefixes of n = 1, 63, 64, 65 and 130 rays (a lone lane, a wave less one, a whole wave, a wave and one, two
waves and a tail that reaches into the permuted half).  The distance query takes the points origin + 0.25 direction.

For each of trace_rays, occluded, crossings, distance and march:
  * the unsorted call on torch's default stream is the baseline;
  * three sorted calls on two other streams in the order A, B, A -- every one after the first waits for the event of the
    call before it (rays_ev) -- each give the baseline's bytes;
  * the numpy call gives the torch call's bytes;
  * n = 0 gives empty outputs.
Whether those bytes are the right ones is the business of test_gpu_rays, test_gpu_occlusion, test_gpu_crossings,
test_gpu_distance and test_gpu_march (which also drive the reciprocal vote); this file holds the paths to one another.
"""
import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
QUERIES = ("trace_rays", "occluded", "crossings", "distance", "march")
SIZES = (1, 63, 64, 65, 130)
POISON = 0x5A


@pytest.fixture(scope="module")
def box():
    """(GpuScene, rays f32 [256, 6], tminmax f32 [256, 2], points f32 [256, 3]) as numpy arrays, made once."""
    import torch
    hs = rtm.HostScene.load(1)
    gs = rtm.GpuScene(hs, 0)
    prim = gs.primary_rays(gs.frame(8, 8, 2)).cpu().numpy()
    assert prim.shape == (128, 6)
    perm = np.random.Generator(np.random.PCG64(7)).permutation(128)
    rays = np.ascontiguousarray(np.concatenate([prim, prim[perm]]), np.float32)
    tmm = np.ascontiguousarray(np.tile(np.array([1e-3, 1e30], np.float32), (rays.shape[0], 1)))
    pts = np.ascontiguousarray(rays[:, :3] + np.float32(0.25) * rays[:, 3:], np.float32)
    torch.cuda.synchronize()
    yield gs, rays, tmm, pts
    gs.close()
    hs.close()


def run(gs, query, rays, tmm, pts, **kw):
    """One query through GpuScene -> the arrays the library wrote, as the method returns them."""
    if query == "trace_rays":
        return (gs.trace_rays(rays, **kw).hits,)
    if query == "occluded":
        return (gs.occluded(rays, tmm, **kw),)
    if query == "crossings":
        return (gs.crossings(rays, tmm, **kw).raw,)
    if query == "distance":
        r = gs.distance(pts, closest=True, **kw)
        return (r.raw, r.closest)
    return (gs.march(rays, **kw).raw,)


def as_bytes(outs):
    """The outputs as uint8 arrays; a tensor is then overwritten, so that memory the allocator hands out again cannot
    pass for a later call's result."""
    import torch
    res = []
    for o in outs:
        if isinstance(o, np.ndarray):
            res.append(np.frombuffer(np.ascontiguousarray(o).tobytes(), np.uint8))
        else:
            res.append(np.frombuffer(o.cpu().numpy().tobytes(), np.uint8))
            o.fill_(POISON)
    torch.cuda.synchronize()                        # the fills are done before any stream writes that memory again
    return res


def same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w, err_msg=what)


@pytest.mark.parametrize("query", QUERIES)
def test_sorted_calls_across_streams_and_numpy_calls_give_the_baseline(box, query):
    import torch
    gs, rays, tmm, pts = box
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for n in SIZES:
        h = (rays[:n].copy(), tmm[:n].copy(), pts[:n].copy())
        d = tuple(torch.from_numpy(x).cuda() for x in h)
        torch.cuda.synchronize()                    # the inputs are there before any stream reads them
        base = as_bytes(run(gs, query, *d))
        assert sum(x.size for x in base) > 0
        for name, st in (("A", a), ("B", b), ("A again", a)):
            outs = run(gs, query, *d, sort=True, stream=st.cuda_stream)
            torch.cuda.synchronize()
            same(as_bytes(outs), base, f"{query}, n = {n}: sorted on stream {name} vs the unsorted default-stream call")
        same(as_bytes(run(gs, query, *h)), base, f"{query}, n = {n}: numpy input vs torch input")
        same(as_bytes(run(gs, query, *h, sort=True, stream=b.cuda_stream)), base,
             f"{query}, n = {n}: numpy input, sorted on a stream, vs torch input")


@pytest.mark.parametrize("query", QUERIES)
def test_no_elements_give_empty_outputs(box, query):
    import torch
    gs, rays, tmm, pts = box
    h = (rays[:0].copy(), tmm[:0].copy(), pts[:0].copy())
    d = tuple(torch.from_numpy(x).cuda() for x in h)
    st = torch.cuda.Stream()
    for args in (d, h):
        for kw in ({}, {"sort": True}, {"sort": True, "stream": st.cuda_stream}):
            outs = run(gs, query, *args, **kw)
            assert all(o.shape[0] == 0 for o in outs), (query, kw, [tuple(o.shape) for o in outs])
    torch.cuda.synchronize()
