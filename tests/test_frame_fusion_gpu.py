"""VR_OPT_FRAME_FUSION: vr_frame_submit shading inside the tile pass (the KEEP flavour of k_raster) against the same frames
with the option off - the unfused pair of passes, which is the reference.  Every comparison is exact: the five planes,
depth, HdrColor, the region census and what the library knows about the emissive plane."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, flythrough_camera, params, scaled_camera
from tests.fusion_common import (FUSED, LIGHTING, PLANES, assert_same_frames, download_frame, submit_frames,
                                 terrain_fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(product_lib):
    with terrain_fixture(256) as f:
        yield f


def _fly(i, w, h, size=256):
    return vr.make_view(*scaled_camera(flythrough_camera(i), size), w, h)


def _both(fx, what, expect_fused, *args, **kw):
    """The same frames with the option off (reference) and on; expect_fused: per frame, or one value for all."""
    off, on = submit_frames(fx, 0, *args, **kw), submit_frames(fx, 1, *args, **kw)
    assert not any(f["fused"] for f in off), what + ": the option is off and a frame was fused"
    exp = expect_fused if isinstance(expect_fused, (list, tuple)) else [expect_fused] * len(on)
    assert [f["fused"] for f in on] == list(exp), what + f": fused frames {[f['fused'] for f in on]}"
    if not kw.get("tiled"):         # a frame that is not fused launches the lighting pass
        assert all(f["fused"] != f["lighting"] for f in off + on), what
    assert_same_frames(off, on, what)
    return off, on


@pytest.mark.parametrize("w,h", [(256, 144), (252, 132)])
def test_small_frames_three_consecutive_views(fx, w, h):
    """Three consecutive flythrough views (region states evolve from frame to frame); 252x132 has a partial last tile column
    and row.  Every frame holds an all-sky tile, all-terrain regions and mixed regions."""
    views = [_fly(i, w, h) for i in range(3)]
    off, _ = _both(fx, f"{w}x{h}", True, w, h, views)
    for i, f in enumerate(off):
        cov = f["depth"] < 1.0
        assert any(not cov[y:y + 32, x:x + 32].any() for y in range(0, h, 32) for x in range(0, w, 32)), f"frame {i}: no all-sky tile"
        c = f["census"]
        assert c["clear"] > 0 and c["specular_constant"] > 0 and c["unknown"] > 0, f"frame {i}: {c}"


def test_clear_handling_and_state_changes_between_frames(fx):
    w, h = 256, 144
    views = [_fly(i, w, h) for i in range(3)]
    # RenderTargets.Clear() before each frame: a lazy clear is pending, consumed by the whole-frame pass
    _both(fx, "Clear before each frame", True, w, h, views, clear=True, assume_cleared=0)
    # no clear, the caller's promise instead
    _both(fx, "assume_cleared", True, w, h, [vr.make_view(*scaled_camera(CAMERAS[k], 256), w, h) for k in (0, 5, 3)])
    # a foreign write into the specular plane: the region states drop to unknown, the specular plane is written again
    rng = np.random.default_rng(5)
    foreign = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)

    def spec_upload(i, rt):
        if i == 1:
            rt.upload("specular", foreign)
    _both(fx, "specular upload", True, w, h, views, before=spec_upload)
    # a non-zero emissive plane: nothing is known about it, the frame takes the two passes (and knows the plane again afterwards)
    emi = rng.integers(1, 1 << 15, (h, w, 4), dtype=np.uint64).astype(np.uint16)

    def emi_upload(i, rt):
        if i == 1:
            rt.upload("emissive", emi)
    _both(fx, "emissive upload", [True, False, True], w, h, views, before=emi_upload)


def test_light_lists(fx):
    w, h = 256, 144
    views = [_fly(0, w, h), _fly(7, w, h)]
    sun = vr.reference_sun()
    pts = vr.synthetic_point_lights(16, 256.0, fx["h"], 400.0, seed=9001)
    _both(fx, "no light", True, w, h, views, lights=[])
    _both(fx, "sun", True, w, h, views, lights=[sun])
    _both(fx, "16 lights", True, w, h, views, lights=[sun] + pts[:15])
    # more than the streaming pass's 16: only the tiled pass takes them
    _both(fx, "17 lights (tiled)", False, w, h, views, lights=[sun] + pts, tiled=True)
    for fusion in (0, 1):
        with pytest.raises(Exception, match="16 lights"):
            submit_frames(fx, fusion, w, h, views[:1], lights=[sun] + pts)
    spot = vr.spot_light((-2.5, 7.5, 1.25), (0.3, -1.0, -0.2), 6000.0, 25.0, 12.0, 25.0, (0.2, 1.0, 0.4))
    _both(fx, "spot light", False, w, h, views, lights=[sun, spot])


def test_ineligible_render_params_fall_back(fx):
    w, h = 256, 144
    views = [_fly(0, w, h), _fly(1, w, h)]
    _both(fx, "wireframe", False, w, h, views, wireframe=1)
    _both(fx, "depth only", False, w, h, views, depth_only=1)
    _both(fx, "depth ranges", False, w, h, views, depth_ranges=1)
    _both(fx, "64-pixel tiles", False, w, h, views, tile=64)
    # assume_cleared = 0 over what the first frame left (no clear in between): the second frame keeps what it does not cover
    # (the frame's render parameters are read at submit time: the second frame changes them in place)
    ctx, tp = fx["ctx"], fx["tp"]
    outs = []
    for fusion in (0, 1):
        ctx.set_frame_fusion(fusion)
        rt, hdr = vr.RenderTargets(ctx).Init(w, h), vr.HdrImage(ctx, w, h)
        rp = vr.default_render_params(400.0, assume_cleared=1)
        fr = vr.Frame(tp, rt, rp, [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)
        try:
            fr.submit(views[0], hdr)
            rp.assume_cleared = 0
            ctx.timing_enable(2)
            fr.submit(vr.make_view(*scaled_camera(CAMERAS[4], 256), w, h), hdr)
            ctx.synchronize()
            ran = ctx.timing_collect()
            ctx.timing_enable(0)
            assert LIGHTING in ran and FUSED not in ran, sorted(ran)
            f = download_frame(rt, hdr)
            f.update(census=rt.region_census(), emissive_known_zero=rt.plane_known_zero("emissive"))
            outs.append([f])
        finally:
            ctx.set_frame_fusion(1)
            hdr.close()
            rt.close()
    assert_same_frames(outs[0], outs[1], "assume_cleared = 0 over a drawn target")


@pytest.mark.parametrize("w,h", [(256, 144), (1024, 576)])
def test_tonemap_stage_on_a_second_stream(fx, w, h):
    """The tone-map stage on another context's stream, two HdrImages rotating over six frames without a host synchronisation
    in between: the fused tile pass waits for the reader of the image it overwrites, and the stage waits for the fused
    launch's own stop event (two frames are prepared ahead after every launch)."""
    import torch
    ctx, tp = fx["ctx"], fx["tp"]
    views = [_fly(3 * i, w, h) for i in range(6)]
    tmp = vr.default_tonemap_params()
    side = torch.cuda.Stream()
    tctx = vr.Context(0)
    tctx.set_stream(side.cuda_stream)

    def run(fusion):
        ctx.set_frame_fusion(fusion)
        rt = vr.RenderTargets(ctx).Init(w, h)
        hdrs = [vr.HdrImage(ctx, w, h) for _ in range(2)]
        ldrs = [vr.LdrImage(tctx, w, h) for _ in range(2)]
        tm = vr.ToneMappingPass(tctx)
        tm.AdvanceFrame(1.0 / 60.0)
        fr = vr.Frame(tp, rt, vr.default_render_params(400.0, assume_cleared=1), [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM,
                      tonemap=tm, tonemap_params=tmp, ldr=ldrs[0])
        outs = []
        try:
            for i, v in enumerate(views):
                b = i % 2
                if i >= 2:                                   # the host reads a buffer back before its slot is used again
                    ctx.synchronize(); tctx.synchronize()
                    outs.append((hdrs[b].download().copy(), ldrs[b].download().copy()))
                fr.submit(v, hdrs[b], views[i + 1:i + 3], ldr=ldrs[b])
            ctx.synchronize(); tctx.synchronize()
            for b in (0, 1):
                outs.append((hdrs[b].download().copy(), ldrs[b].download().copy()))
            exposure = tm.download()[1]
        finally:
            ctx.synchronize(); tctx.synchronize()
            ctx.set_frame_fusion(1)
            tm.close()
            for o in ldrs + hdrs + [rt]:
                o.close()
        return outs, exposure
    try:
        (want, e0), (got, e1) = run(0), run(1)
        assert len(want) == len(got) == 6
        for k, ((h0, l0), (h1, l1)) in enumerate(zip(want, got)):
            assert np.array_equal(h0, h1), f"HdrColor of frame slot {k} differs"
            assert np.array_equal(l0, l1), f"LdrColor of frame slot {k} differs"
        assert np.float32(e0).view(np.uint32) == np.float32(e1).view(np.uint32), (e0, e1)
    finally:
        torch.cuda.synchronize()
        tctx.close()


@pytest.mark.parametrize("world", [2, 3])
def test_partition_takes_the_two_passes(fx, world):
    """A rank's share (packed tiles) is not fused: every rank's frame is queued as before, and is the same."""
    w, h = 384, 256
    views = [_fly(0, w, h), _fly(1, w, h)]
    for rank in range(world):
        _both(fx, f"rank {rank} of {world}", False, w, h, views, part=vr.Partition(rank, world))


def test_prepare_two_frames_ahead(fx):
    w, h = 256, 144
    views = [_fly(i, w, h) for i in range(4)]
    off, on = _both(fx, "two frames ahead", True, w, h, views, ahead=2)
    assert_same_frames(on, submit_frames(fx, 1, w, h, views), "prepared ahead vs not prepared")
    assert_same_frames(off, submit_frames(fx, 0, w, h, views), "prepared ahead vs not prepared (option off)")


def test_one_8k_frame():
    """The bench's frame (7680x4320, 2048^2 heightmap, flythrough view 0): HdrColor and depth on a seeded sample of 2^21 pixels."""
    w, h, size = 7680, 4320, 2048
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, vr.synth_albedo(ctx, size, hm))
    pick = np.sort(np.random.default_rng(20261016).choice(w * h, size=1 << 21, replace=False))
    v = vr.make_view(*flythrough_camera(0), w, h)
    res = []
    try:
        for fusion in (0, 1):
            ctx.set_frame_fusion(fusion)
            rt, hdr = vr.RenderTargets(ctx).Init(w, h), vr.HdrImage(ctx, w, h)
            try:
                fr = vr.Frame(tp, rt, vr.default_render_params(400.0, assume_cleared=1), [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)
                ctx.timing_enable(2)
                fr.submit(v, hdr)
                ctx.synchronize()
                ran = ctx.timing_collect()
                ctx.timing_enable(0)
                assert (FUSED in ran) == bool(fusion) and (LIGHTING in ran) != bool(fusion), sorted(ran)
                res.append((hdr.download().reshape(-1, 4)[pick].copy(), rt.download("depth").reshape(-1)[pick].view(np.uint32).copy(),
                            rt.region_census()))
            finally:
                hdr.close()
                rt.close()
    finally:
        tp.close()
        ctx.close()
    assert (res[0][1] != 0x3f800000).mean() > 0.3, "the frame shows little terrain"
    assert np.array_equal(res[0][0], res[1][0]), "HdrColor"
    assert np.array_equal(res[0][1], res[1][1]), "depth"
    assert res[0][2] == res[1][2], "region census"


@pytest.mark.parametrize("split", [False, True], ids=["whole", "rank0of2"])
def test_a_refused_frame_leaves_no_trace(fx, split):
    """vr_frame_submit refuses before it queues anything.  With a Clear pending, sentinels in HdrColor and the LDR buffer (a
    rank's packed buffers with `split`), known bins and an adapted luminance of 0.25, a frame whose tone-map stage is refused -
    no parameters, an LDR capacity one byte short, an empty log-luminance range - or whose hdr_out is too small (by one pixel:
    an image's capacity is a whole number of them) returns VR_ERR_INVALID_ARGUMENT with the message it always had, queues no
    kernel at all, leaves both buffers, the bins and the adapted luminance as they were, and leaves the Clear pending: every
    region still counts as clear and the planes' first download is what writes it.  The corrected descriptor then gives the
    planes, HdrColor, LdrColor and tone-mapper state of the per-call sequence, bit for bit."""
    import ctypes as C
    from vrenderer_amd.passes import partition_info
    ctx, tp = fx["ctx"], fx["tp"]
    w, h = 256, 144
    v = _fly(0, w, h)
    rp = vr.default_render_params(400.0, assume_cleared=1)
    lights = [vr.reference_sun()]
    tmp, bad = vr.default_tonemap_params(), vr.default_tonemap_params(max_log_luminance=-10.0)
    assert bad.max_log_luminance == bad.min_log_luminance
    part = vr.Partition(0, 2) if split else None
    hdr_bytes = partition_info(w, h, 0, 2)["packed_bytes"] if split else w * h * 8
    ldr_bytes = hdr_bytes // 2
    mk_hdr = lambda px: vr.HdrImage(ctx, vr.VR_OWNER_TILE, px // vr.VR_OWNER_TILE) if px % vr.VR_OWNER_TILE == 0 else vr.HdrImage(ctx, px, 1)
    hdrs, small = [mk_hdr(hdr_bytes // 8) for _ in range(2)], mk_hdr(hdr_bytes // 8 - 1)
    ldrs = [vr.LdrImage(ctx, w, h, capacity_bytes=ldr_bytes) for _ in range(2)]
    rts = [vr.RenderTargets(ctx).Init(w, h) for _ in range(2)]
    tms = [vr.ToneMappingPass(ctx) for _ in range(2)]
    sent_hdr, sent_ldr = np.full(hdr_bytes // 2, 0x3c00, np.uint16), np.full(ldr_bytes, 0x5a, np.uint8)
    rt, hdr, ldr, tm = rts[0], hdrs[0], ldrs[0], tms[0]
    try:
        for t in tms:
            t.AdvanceFrame(1.0 / 60.0)
        hdr.upload(sent_hdr)
        tm.AddFrameToHistogram(tmp, hdr, w, h, part)
        tm.ResetExposure(0.25)
        bins, lum = tm.download()
        assert bins.any() and lum == 0.25
        fr = vr.Frame(tp, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, part, tonemap=tm, tonemap_params=tmp, ldr=ldr)
        d = fr.desc
        for case, text in (("params", "tone-map stage: params / ldr_out missing"),
                           ("ldr_capacity", "ldr buffer is smaller than vr_partition_packed_bytes_ldr()" if split else "ldr buffer is smaller than the frame"),
                           ("log_range", "max_log_luminance must exceed min_log_luminance"),
                           ("hdr_out", "hdr_out is smaller than vr_partition_packed_bytes()" if split else "hdr_out is smaller than the frame")):
            rt.upload("diffuse", np.full((h, w), 0x01020304, np.uint32))
            rt.Clear()                                           # lazy: nothing is written yet
            hdr.upload(sent_hdr); small.upload(sent_hdr[:-4]); ldr.upload(sent_ldr)
            d.tonemap_params = None if case == "params" else C.addressof(bad if case == "log_range" else tmp)
            d.ldr_capacity = ldr.capacity - (1 if case == "ldr_capacity" else 0)
            ctx.synchronize()
            ctx.timing_enable(1)
            with pytest.raises(vr.VrError) as e:
                fr.submit(v, small if case == "hdr_out" else hdr, [_fly(1, w, h)])
            ctx.synchronize()
            ran = ctx.timing_collect()
            assert e.value.code == vr.capi.VR_ERR_INVALID_ARGUMENT and text in str(e.value), (case, e.value)
            assert not ran, f"{case}: the refused frame queued {sorted(ran)}"
            census = rt.region_census()
            assert census["clear"] == census["total"] > 0, (case, census)
            assert np.array_equal(hdr.download(hdr_bytes), sent_hdr) and np.array_equal(small.download(hdr_bytes - 8), sent_hdr[:-4]), f"{case}: HdrColor"
            assert np.array_equal(ldr.download(ldr_bytes), sent_ldr), f"{case}: the LDR buffer"
            bins1, lum1 = tm.download()
            assert np.array_equal(bins, bins1) and np.float32(lum1).view(np.uint32) == np.float32(lum).view(np.uint32), f"{case}: bins / adapted luminance"
            planes = {p: rt.download(p) for p in PLANES}         # (the first of them writes the pending clear)
            written = ctx.timing_collect()
            ctx.timing_enable(0)
            assert len(written) == 1 and [n for _, n in written.values()] == [1], f"{case}: the Clear was no longer pending: {written}"
            assert (planes["depth"] == 1.0).all() and not any(planes[p].any() for p in PLANES[1:]), f"{case}: the planes do not read as cleared"
        # the corrected descriptor against the per-call sequence
        d.tonemap_params, d.ldr_capacity = C.addressof(tmp), ldr.capacity
        rt.Clear()
        fr.submit(v, hdr, [_fly(1, w, h)])
        rts[1].Clear(); hdrs[1].upload(sent_hdr); ldrs[1].upload(sent_ldr)
        tms[1].ResetExposure(0.25)
        tp.Render(v, v, rts[1], rp, part)
        vr.DeferredLightingPass(ctx).Render(v, rts[1], lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdrs[1], partition=part)
        tms[1].ResetHistogram()
        tms[1].AddFrameToHistogram(tmp, hdrs[1], w, h, part)
        tms[1].ComputeExposure(tmp)
        tms[1].Render(tmp, hdrs[1], ldrs[1], w, h, part)
        ctx.synchronize()
        for p in PLANES:
            assert np.array_equal(rts[0].download(p).view(np.uint8), rts[1].download(p).view(np.uint8)), p
        assert np.array_equal(hdrs[0].download(hdr_bytes), hdrs[1].download(hdr_bytes)), "HdrColor"
        assert np.array_equal(ldrs[0].download(ldr_bytes), ldrs[1].download(ldr_bytes)), "LdrColor"
        assert not np.array_equal(ldrs[0].download(ldr_bytes), sent_ldr)
        (b0, l0), (b1, l1) = tms[0].download(), tms[1].download()
        assert np.array_equal(b0, b1) and np.float32(l0).view(np.uint32) == np.float32(l1).view(np.uint32), (l0, l1)
    finally:
        ctx.synchronize()
        ctx.timing_enable(0)
        for o in tms + ldrs + hdrs + [small] + rts:
            o.close()
