"""The per-wave fixed-cost changes on the GPU: process_item's coordinates carried across the
walk (one packed VGPR, no divisions) and the DDA setup's quotients over one reciprocal per axis
(csrc/rt_setup_div.h).  Both must leave every frame, hit id and record bit-identical.

* Frames of scene 1 at 256x144 and 250x141 (partial edge blocks) with 1, 4 and 16 samples -- the wave's pixel
  block is then 8x8, 4x4 and 2x2 -- byte-equal to the RT_KERNEL_LANES arm and to the CPU oracle, the hits launch
  equal to the oracle's hit ids, the records launch equal to the plain walk's records (k_trace_records); the
  same for shard 1 of 3 (the deal's row rotation through the multiply-high division) and a batch [1, 8].
* An unaligned tile region at the edge of a frame 65536 wide or high, whose last tile overhangs 2^16.
* Other cameras: scene 5's own (inside the grid box: no box test, the reciprocals serve the quotients alone)
  and scene 1 orbited 180 degrees (the box behind the camera: every ray misses).
* The division on the device: k_primitives kind 8 evaluates dda_setup's quotient, wave vote included, and the
  plain n / d on 2^20 crafted pairs -- the CPU checker's families, plus +-0, inf and NaN -- bit for bit, also in
  waves where one lane forces the fall-back for the other 63.
* The divisions through the walk: rt_trace_rays_device (the plain walk, RT_RAYS_COUNT records) on camera
  rays.  Scaled by 2^40, 2^41 and 2^-40 (exact in every step of Grid::Intersect) the directions sit at the
  window's upper edge and leave it on either side, and their records must equal k_trace_records' of the
  unscaled rays where both apply: scaled down (scenes 8 and 1) every determinant falls below the absolute 1e-8
  gate, nothing is hit, and a ray that missed before must walk the same cells and test the same records;
  scaled up (scene 1, whose 44 triangles let the test decide per ray that no determinant crosses the gate) a
  hit keeps its record with t scaled back.  Axis-parallel rays and rays with zero or 1e-30 components mixed
  one per wave into scene 8's ordinary rays force those waves to the fall-back: the ordinary rays' records
  must not change by a bit.

Small frames and one 2^20-record launch: a second or two per case.
"""
import numpy as np
import pytest

from conftest import load_package, nan_equal_bits

pytestmark = pytest.mark.gpu
rtm = load_package()
SHAPES = [(256, 144), (250, 141)]
GEOM = [0, 1, 2, 3, 4, 5, 6, 7]          # rt_sample_rec words: hit, tri, voxel, steps, tests, t, u, v
PRODUCT = [0, 1, 2, 5, 6, 7, 8, 9, 10]   # what a product walk's record defines (no step / test counts)


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(sid):
        if sid not in cache:
            hs = rtm.HostScene.load(sid)
            cache[sid] = (hs, rtm.GpuScene(hs, 0))
        return cache[sid]
    yield get
    for hs, gs in cache.values():
        gs.close()
        hs.close()


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    cache = {}

    def get(sid, W, H, spp):
        if (sid, W, H, spp) not in cache:
            img, hits, _ = oracle.render(sid, W, H, spp, hits=True)
            cache[(sid, W, H, spp)] = (img, hits)
        return cache[(sid, W, H, spp)]
    return get


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def rec_words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 12)


# ------------------------------------------------------------------------------------ frames
@pytest.mark.parametrize("spp", [1, 4, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scene1_frames_hits_and_records(scenes, oracle_frames, shape, spp):
    import torch
    W, H = shape
    hs, gs = scenes(1)
    want, want_hits = oracle_frames(1, W, H, spp)
    f = gs.frame(W, H, spp)
    auto = gs.render_frame(f)
    lanes = gs.render_frame(gs.frame(W, H, spp, kernel=rtm.RT_KERNEL_LANES))
    assert auto.tobytes() == lanes.tobytes(), f"{(auto != lanes).sum()} pixels differ from RT_KERNEL_LANES"
    assert auto.tobytes() == want.tobytes(), f"{(auto != want).sum()} pixels differ from the oracle"
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    hits = torch.full((W * H * spp,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gs.render_hits_device(f, 0, 1, out.data_ptr(), hits.data_ptr(), st)
    torch.cuda.synchronize()
    assert u32(out).tobytes() == want.tobytes()
    np.testing.assert_array_equal(u32(hits), want_hits)
    out.zero_()
    recs = torch.full((W * H * spp * 12,), -1, dtype=torch.int32, device="cuda")
    rtm.render_records_device([gs], [f], [out.data_ptr()], [(0, 0, W, H)], [recs.data_ptr()], stream=st)
    torch.cuda.synchronize()
    assert u32(out).tobytes() == want.tobytes()
    plain = rec_words(gs.trace_samples(f, 0, 0, W, H))
    np.testing.assert_array_equal(u32(recs).reshape(-1, 12)[:, PRODUCT], plain[:, PRODUCT])


@pytest.mark.parametrize("spp", [1, 4, 16])
def test_scene1_shard_1_of_3(scenes, oracle_frames, spp):
    import torch
    W, H = 250, 141
    hs, gs = scenes(1)
    want, want_hits = oracle_frames(1, W, H, spp)
    e = rtm.shard_elems(W, H, 3)
    f = gs.frame(W, H, spp)
    st = torch.cuda.current_stream().cuda_stream
    shard = torch.zeros(e, dtype=torch.int32, device="cuda")
    gs.render_shard_device(f, 1, 3, shard.data_ptr(), st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(shard), rtm.shard_from_frame(want, 1, 3))
    shard.zero_()
    hits = torch.full((W * H * spp,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gs.render_hits_device(f, 1, 3, shard.data_ptr(), hits.data_ptr(), st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(shard), rtm.shard_from_frame(want, 1, 3))
    # the rank's own samples hold the oracle's hit ids, every other sample is untouched
    h = u32(hits).reshape(H, W, spp)
    mine = np.zeros((H, W), bool)
    for t in rtm.shard_tile_ids(W, H, 1, 3):
        tx, ty = t % ((W + 15) // 16), t // ((W + 15) // 16)
        mine[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    np.testing.assert_array_equal(h[mine], want_hits.reshape(H, W, spp)[mine])
    assert (h[~mine] == 0x5A5A5A5A).all()
    # the records launch of the same shard: the rank's samples equal the plain walk's, frame-absolute
    shard.zero_()
    recs = torch.full((W * H * spp * 12,), -1, dtype=torch.int32, device="cuda")
    rtm.render_records_device([gs], [f], [shard.data_ptr()], [(0, 0, W, H)], [recs.data_ptr()], rank=1, nranks=3,
                              stream=st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(shard), rtm.shard_from_frame(want, 1, 3))
    r = u32(recs).reshape(H, W, spp, 12)
    plain = rec_words(gs.trace_samples(f, 0, 0, W, H)).reshape(H, W, spp, 12)
    np.testing.assert_array_equal(r[mine][..., PRODUCT], plain[mine][..., PRODUCT])
    assert (r[~mine] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_of_scenes_1_and_8(scenes, oracle_frames, shape):
    import torch
    W, H = shape
    spp = 4
    gss = [scenes(1)[1], scenes(8)[1]]
    fs = [g.frame(W, H, spp) for g in gss]
    st = torch.cuda.current_stream().cuda_stream
    outs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in gss]
    hits = [torch.full((W * H * spp,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in gss]
    before = gss[0].info()["batch_launches"]
    rtm.render_batch_device(gss, fs, [o.data_ptr() for o in outs], d_hits=[h.data_ptr() for h in hits], stream=st)
    torch.cuda.synchronize()
    assert gss[0].info()["batch_launches"] == before + 1
    for sid, o, h in zip((1, 8), outs, hits):
        want, want_hits = oracle_frames(sid, W, H, spp)
        assert u32(o).tobytes() == want.tobytes(), sid
        np.testing.assert_array_equal(u32(h), want_hits, err_msg=str(sid))
    # the records launch of the same batch
    for o in outs:
        o.zero_()
    recs = [torch.full((W * H * spp * 12,), -1, dtype=torch.int32, device="cuda") for _ in gss]
    rtm.render_records_device(gss, fs, [o.data_ptr() for o in outs], [(0, 0, W, H)] * 2, [r.data_ptr() for r in recs],
                              stream=st)
    torch.cuda.synchronize()
    assert gss[0].info()["batch_launches"] == before + 2
    for sid, g, f, o, r in zip((1, 8), gss, fs, outs, recs):
        assert u32(o).tobytes() == oracle_frames(sid, W, H, spp)[0].tobytes(), sid
        plain = rec_words(g.trace_samples(f, 0, 0, W, H))
        np.testing.assert_array_equal(u32(r).reshape(-1, 12)[:, PRODUCT], plain[:, PRODUCT], err_msg=str(sid))


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("spp", [1, 4])
def test_unaligned_region_whose_last_tile_overhangs_2_16(scenes, oracle, axis, spp):
    """A frame 65536 wide (or high) and a tile region that starts 6 pixels before its edge: the region's one
    16-pixel tile column (row) holds lanes at 65536 .. 65545, which no 16-bit field can carry.  They are invalid
    before the walk and must be after it (item_coord_post rebuilds the coordinates from the tile origin in
    32 bits): the region's pixels equal the oracle's and the pixel-loop kernel's (which never packs anything),
    also with a second tile beside it in the same launch (an unaligned
    bounding region of three tiles, the last one overhanging)."""
    hs, gs = scenes(1)
    W, H = (65536, 20) if axis == "x" else (20, 65536)
    want, _, _ = oracle.render(1, W, H, spp)
    tile = (65530, 3, 65536, 20) if axis == "x" else (3, 65530, 20, 65536)
    near = (65536 - 42, 0, 65536 - 20, 16) if axis == "x" else (0, 65536 - 42, 16, 65536 - 20)   # (unaligned too)
    for tiles in ([tile], [near, tile]):
        got = gs.render_tiles(gs.frame(W, H, spp), tiles)
        loop = gs.render_tiles(gs.frame(W, H, spp, kernel=rtm.RT_KERNEL_PIXEL_LOOP), tiles)
        for (x0, y0, x1, y1), g, l in zip(tiles, got, loop):
            assert g.tobytes() == want[y0:y1, x0:x1].tobytes(), (axis, spp, (x0, y0, x1, y1))
            assert g.tobytes() == l.tobytes()


def test_camera_inside_the_box(scenes, oracle_frames):
    """Scene 5's own camera sits inside the grid box: dda_setup takes no box test, so the reciprocals feed the
    six quotients alone."""
    hs, gs = scenes(5)
    info = hs.grid()[0]
    org = np.asarray(hs.cam, np.float32).reshape(4, 4)[3, :3]
    assert (org >= np.asarray(info["aabb_min"], np.float32)).all() and (org <= np.asarray(info["aabb_max"], np.float32)).all()
    for W, H in SHAPES:
        want, _ = oracle_frames(5, W, H, 4)
        got = gs.render_frame(gs.frame(W, H, 4))
        assert got.tobytes() == want.tobytes(), f"{(got != want).sum()} pixels differ from the oracle"


def test_box_behind_the_camera(scenes, oracle):
    """Scene 1's camera turned 180 degrees about the y axis where it stands (an orbit about the origin would
    keep facing the box): it looks away from the box and every sample takes the miss colour of its row."""
    hs, gs = scenes(1)
    a = np.deg2rad(180.0)
    r = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]], np.float64)
    m = np.asarray(hs.cam, np.float64).reshape(4, 4).copy()
    m[:3, :3] = m[:3, :3] @ r
    cam = m.astype(np.float32).reshape(16)
    W, H, spp = 250, 141, 4
    want, want_hits = oracle.render_cam(1, W, H, spp, cam, hs.fov)
    assert (want_hits == 0xFFFFFFFF).all()
    f = gs.frame(W, H, spp)
    for k in range(16):
        f.cam[k] = float(cam[k])
    got = gs.render_frame(f)
    assert got.tobytes() == want.tobytes(), f"{(got != want).sum()} pixels differ from the oracle"


# ------------------------------------------------------------------- the division on the device
def rand_floats(r, n, elo, ehi):
    """Random sign and mantissa, binary exponent uniform in [elo, ehi] (normal range)."""
    e = r.integers(elo + 127, ehi + 128, n, dtype=np.uint32)
    return ((r.integers(0, 2, n, dtype=np.uint32) << 31) | (e << 23) | r.integers(0, 1 << 23, n, dtype=np.uint32)).view(np.float32)


def crafted_pairs():
    """2^20 (n, d) pairs: the families of tests/setup_div_check.cpp, then specials."""
    r = np.random.Generator(np.random.PCG64(20261019))
    m = 1 << 17
    fam = []
    d = (rand_floats(r, m, -39, 39).view(np.uint32) | np.uint32(0x7FFFFF)).view(np.float32)      # all-ones mantissa
    fam.append((rand_floats(r, m, -39, 39), d))
    d = np.ldexp(r.choice(np.array([-1.0, 1.0], np.float32), m), r.integers(-40, 41, m)).astype(np.float32)
    fam.append((rand_floats(r, m, -39, 39), d))                                                    # powers of two
    d = np.ldexp(r.integers(1, 4096, m).astype(np.float32), r.integers(-40, 21, m)).astype(np.float32)
    fam.append((d * r.integers(1, 4096, m).astype(np.float32) * r.choice(np.array([-1.0, 1.0], np.float32), m), d))
    d = rand_floats(r, m, -19, 19)                                                                 # binade edges
    q = (np.ldexp(np.float32(1.0), r.integers(-19, 20, m)).astype(np.float32).view(np.int32) + r.integers(-2, 3, m)).astype(np.int32).view(np.float32)
    n = (q.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
    fam.append(((n.view(np.int32) + r.integers(-1, 2, m)).astype(np.int32).view(np.float32), d))
    d = rand_floats(r, m, -19, 19)                                                                 # rounding midpoints
    q = rand_floats(r, m, -19, 19)
    q1 = (q.view(np.int32) + 1).astype(np.int32).view(np.float32)          # the next float away from zero
    n = ((q.astype(np.float64) + q1.astype(np.float64)) * 0.5 * d.astype(np.float64)).astype(np.float32)
    fam.append(((n.view(np.int32) + r.integers(-1, 2, m)).astype(np.int32).view(np.float32), d))
    fam.append((rand_floats(r, m, -126, 127), rand_floats(r, m, -126, 127)))                       # all magnitudes
    sub = lambda k: ((r.integers(0, 2, k, dtype=np.uint32) << 31) | r.integers(1, 1 << 23, k, dtype=np.uint32)).view(np.float32)
    fam.append((np.concatenate([sub(m // 2), rand_floats(r, m // 2, -60, 60)]),                    # subnormals
                np.concatenate([rand_floats(r, m // 2, -60, 60), sub(m // 2)])))
    edge = np.array([2.0 ** -40, 2.0 ** 40], np.float32)                                           # the window's edges
    e = (r.choice(edge, m).view(np.int32) + r.integers(-3, 4, m)).astype(np.int32).view(np.float32)
    e *= r.choice(np.array([-1.0, 1.0], np.float32), m)
    o = rand_floats(r, m, -45, 45)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    k = r.integers(0, 64, m)
    o[k < 5] = special[k[k < 5]]
    swap = r.integers(0, 2, m).astype(bool)
    fam.append((np.where(swap, e, o), np.where(swap, o, e)))
    n = np.concatenate([f[0] for f in fam]).astype(np.float32)
    d = np.concatenate([f[1] for f in fam]).astype(np.float32)
    assert n.size == 1 << 20
    return n, d


def in_window(x):
    a = np.abs(x)
    return (a >= np.float32(2.0 ** -40)) & (a <= np.float32(2.0 ** 40))


def test_setup_quotient_on_the_device():
    n, d = crafted_pairs()
    # waves (64 consecutive records) of in-window pairs where ONE lane forces the fall-back, at the front
    r = np.random.Generator(np.random.PCG64(7))
    nw = 256
    n[:64 * nw] = rand_floats(r, 64 * nw, -30, 30)
    d[:64 * nw] = rand_floats(r, 64 * nw, -30, 30)
    forced = np.arange(0, nw, 2)                    # every other wave; the waves between stay on the reciprocal form
    lane = r.integers(0, 64, forced.size)
    bad = np.array([0.0, -0.0, np.inf, np.nan, 1e-30, 1e30, 2.0 ** -41, 2.0 ** 41], np.float32)
    which = r.integers(0, 2, forced.size).astype(bool)
    idx = forced * 64 + lane
    n[idx[which]] = bad[r.integers(0, bad.size, int(which.sum()))]
    d[idx[~which]] = bad[r.integers(0, bad.size, int((~which).sum()))]
    out = rtm.debug_primitives(8, np.stack([n, d], axis=1))
    q, ref, fast = out[:, 0], out[:, 1], out[:, 2]
    assert q.view(np.uint32).tobytes() == ref.view(np.uint32).tobytes(), \
        f"{(q.view(np.uint32) != ref.view(np.uint32)).sum()} quotients differ from the device's n / d"
    with np.errstate(all="ignore"):
        assert nan_equal_bits(ref, n / d)            # (and the device's n / d is the IEEE one)
    # the vote: a wave takes the reciprocal form exactly when all of its lanes are inside the window
    ok = (in_window(n) & in_window(d)).reshape(-1, 64).all(axis=1)
    np.testing.assert_array_equal(fast.reshape(-1, 64), np.repeat(ok[:, None], 64, axis=1).astype(np.float32))
    assert not ok[forced].any() and ok[forced + 1].all()
    assert ok.sum() > 1000 and (~ok).sum() > 1000


# ------------------------------------------------------------------- the divisions through the walk
@pytest.fixture(scope="module")
def camera_rays(scenes):
    """A scene's camera rays at 128x72x1 and the plain walk's records of them (k_trace_records)."""
    cache = {}

    def get(sid):
        if sid not in cache:
            hs, gs = scenes(sid)
            f = gs.frame(128, 72, 1)
            rays = gs.primary_rays(f).cpu().numpy()
            plain = rec_words(gs.trace_samples(f, 0, 0, 128, 72))
            got = gs.trace_rays(rays, count=True)
            np.testing.assert_array_equal(rec_words(got.rec)[:, GEOM], plain[:, GEOM])
            assert (plain[:, 0] == 1).sum() > 1000 and (plain[:, 0] == 0).sum() > 1000
            cache[sid] = (hs, gs, rays, plain)
        return cache[sid]
    return get


@pytest.mark.parametrize("sid,k", [(8, -40), (8, 40), (8, 41), (1, -40), (1, 40), (1, 41)])
def test_directions_scaled_out_of_the_window(camera_rays, sid, k):
    """2^40 keeps a normalised direction just inside the window (|d| <= 2^40: the reciprocal form at its upper
    edge), 2^41 pushes every component above 1/2 out of it, 2^-40 every component.  Every case: the fast arm
    equals the RT_RAYS_COUNT arm on the same scaled rays.  Against k_trace_records' records of the UNSCALED
    rays, scaled up, only rays clear of the determinant gate compare (decided over every triangle of the
    mesh): most of scene 1's, few or none of killeroo's 24,336-triangle mesh, whatever there are.  Scene 8 at
    2^41 (the division) is also held against scene 8 at 2^40 (the reciprocal form): between the two only a
    determinant of 4.5e-21 .. 9.1e-21 could change sides of the gate, far below what float32 sums of this
    mesh's products can leave other than zero, so every record must be equal with t halved."""
    hs, gs, rays, plain = camera_rays(sid)
    scaled = rays.copy()
    scaled[:, 3:] = np.ldexp(rays[:, 3:], k)
    out = (~in_window(scaled[:, 3:])).any(axis=1).mean()
    assert out < 0.01 if k == 40 else out > 0.9, out
    rc = rec_words(gs.trace_rays(scaled, count=True).rec)
    fast = gs.trace_rays(scaled).hits.view(np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(fast[:, 0], rc[:, 1])
    np.testing.assert_array_equal(fast[:, 1:], rc[:, 5:8])
    if sid == 8 and k == 41:
        other = rays.copy()
        other[:, 3:] = np.ldexp(rays[:, 3:], 40)
        r40 = rec_words(gs.trace_rays(other, count=True).rec)
        r40[:, 5] = np.ldexp(r40[:, 5].view(np.float32), -1).view(np.uint32)
        assert (r40[:, 0] == 1).sum() > 1000
        np.testing.assert_array_equal(rc[:, GEOM], r40[:, GEOM])
    if k > 0:
        # every |det| grows by 2^k: a ray keeps its hits when no triangle's |det| = |d . (e2 x e1)| (fp64) was
        # within 1e-6 -- the float32 evaluation's error, generously -- of the absolute 1e-8 gate (triangle.h:77)
        v, t = hs.mesh()
        p0, p1, p2 = (v[t[:, j], :3].astype(np.float32) for j in range(3))
        nrm = np.cross((p2 - p0).astype(np.float64), (p1 - p0).astype(np.float64))
        det = np.zeros(rays.shape[0])
        for i in range(0, rays.shape[0], 1024):
            det[i:i + 1024] = np.abs(rays[i:i + 1024, 3:].astype(np.float64) @ nrm.T).min(axis=1)
        clear = det > 1e-8 + 1e-6
        print(f"2^{k}: {int(clear.sum())} of {clear.size} rays clear of the gate")
        assert sid != 1 or clear.mean() > 0.5
        want = plain.copy()
        want[:, 5] = np.ldexp(plain[:, 5].view(np.float32), -k).view(np.uint32)
        np.testing.assert_array_equal(rc[clear][:, GEOM], want[clear][:, GEOM])
    else:
        # every |det| shrinks below the gate: nothing is hit; a ray that missed before walks the same cells
        # and tests the same records
        assert (rc[:, 0] == 0).all()
        miss = plain[:, 0] == 0
        np.testing.assert_array_equal(rc[miss][:, GEOM], plain[miss][:, GEOM])


def test_one_odd_ray_per_wave_changes_nothing_for_the_others(camera_rays):
    hs, gs, rays, plain = camera_rays(8)
    r = np.random.Generator(np.random.PCG64(11))
    nw = rays.shape[0] // 63
    base = rays[:nw * 63]
    mixed = np.zeros((nw * 64, 6), np.float32)
    odd = np.zeros(nw * 64, bool)
    odd[np.arange(nw) * 64 + r.integers(0, 64, nw)] = True
    mixed[~odd] = base
    o = base[r.integers(0, base.shape[0], nw)].copy()
    kind = np.arange(nw) % 4
    ax = r.integers(0, 3, nw)
    for i in range(nw):
        if kind[i] == 0:                                   # axis-parallel
            o[i, 3:] = 0.0
            o[i, 3 + ax[i]] = r.choice([-1.0, 1.0])
        elif kind[i] == 1:                                 # one exactly zero component
            o[i, 3 + ax[i]] = r.choice([0.0, -0.0])
        elif kind[i] == 2:                                 # one component of 1e-30
            o[i, 3 + ax[i]] = r.choice([-1e-30, 1e-30])
        else:                                              # two components of 1e-30
            o[i, 3 + ax[i]] = 1e-30
            o[i, 3 + (ax[i] + 1) % 3] = -1e-30
    # every other odd ray starts at the grid box's centre, so whatever its direction it walks the grid
    meta = hs.grid()[0]
    o[1::2, :3] = (meta["aabb_min"] + meta["aabb_max"]) * np.float32(0.5)
    mixed[odd] = o
    got = gs.trace_rays(mixed, count=True)
    rc = rec_words(got.rec)
    np.testing.assert_array_equal(rc[~odd][:, GEOM], plain[:nw * 63][:, GEOM])
    # the odd rays themselves: both arms agree, and the same rays alone (whole waves of them) give the same bits
    fast = gs.trace_rays(mixed).hits.view(np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(fast[:, 0], rc[:, 1])
    np.testing.assert_array_equal(fast[:, 1:], rc[:, 5:8])
    alone = rec_words(gs.trace_rays(np.ascontiguousarray(o), count=True).rec)
    np.testing.assert_array_equal(alone[:, GEOM], rc[odd][:, GEOM])
    print(f"odd rays: {int((rc[odd][:, 0] == 1).sum())} hits of {int(odd.sum())}, {int((rc[odd][:, 3] > 0).sum())} walk the grid")
    inside = rc[odd][1::2]                           # the rays from the centre do walk it: a hit, or a last cell
    assert ((inside[:, 0] == 1) | (inside[:, 2] != 0xFFFFFFFF)).all()
