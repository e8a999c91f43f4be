"""Every tone-mapping kernel against the float64 model (tests/f64_tonemap.py): k_tm_histogram / k_tonemap on row-major
frames (w % 4 == 0) and on packed tiles (world 2, 3, 8), k_tm_histogram_scalar / k_tonemap_scalar (w % 4 of 1, 2, 3),
k_tm_exposure, vr_frame_detile_ldr, vr_tonemap_simple_render and the tone-map stage of vr_frame_submit.  No kernel is
compared with another."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_tonemap as ft
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, flythrough_camera, params, scaled_camera
from vrenderer_amd import partition as vp
from vrenderer_amd.passes import frame_detile_ldr, partition_info, partition_prepare

pytestmark = pytest.mark.gpu

EDGE_A = 0.18


@pytest.fixture(scope="module")
def terrain(gpu_ctx):
    out = {}
    for size in (256, 2048):
        h = vr.synth_heightmap(gpu_ctx, size)
        a = vr.synth_albedo(gpu_ctx, size, h)
        out[size] = vr.TerrainPass(gpu_ctx, params(size)).Init(h, a)
    yield out
    for tp in out.values():
        tp.close()


def _report(what, r):
    print(f"{what}: ratios hist {r['hist']:.3f} exposure (i) {r['exp_i']:.3f} (ii) {r['exp_ii']:.3f} ldr {r['ldr']:.3f}, "
          f"flags {r['flags']}")


def _simple_render(gpu_ctx, tm, p, frame, dt, old, what):
    """SimpleRender on the device, then the step against the model."""
    h, w = frame.shape[:2]
    hdr, ldr = vr.HdrImage(gpu_ctx, w, h), vr.LdrImage(gpu_ctx, w, h)
    hdr.upload(frame)
    tm.AdvanceFrame(dt)
    tm.SimpleRender(p, hdr, ldr)
    hist, lum = tm.download()
    got = ldr.download()
    assert (got[..., 3] == 255).all()
    r = ft.check_step(hist, lum, got[..., :3].reshape(-1, 3), ft.PixelSet.from_frame(frame), p, dt, old, what,
                      codes=frame[..., :3].reshape(-1, 3))
    _report(what, r)
    hdr.close(); ldr.close()
    return lum


@pytest.mark.parametrize("w", [512, 509, 510, 511])
def test_edge_frame_row_major(gpu_ctx, w):
    """Vector kernels at w % 4 == 0, scalar kernels at 1, 2, 3: SimpleRender (histogram, exposure, operator), then the
    operator alone at the adapted value the frame's OETF-threshold and white-point pixels were built for."""
    p = vr.default_tonemap_params()
    frame = ft.as_frame(ft.edge_pixels(p, EDGE_A), w)
    h = frame.shape[0]
    tm = vr.ToneMappingPass(gpu_ctx)
    _simple_render(gpu_ctx, tm, p, frame, 1 / 60, 0.0, f"edge frame, w {w}")
    hdr, ldr = vr.HdrImage(gpu_ctx, w, h), vr.LdrImage(gpu_ctx, w, h)
    hdr.upload(frame)
    tm.ResetExposure(EDGE_A)
    tm.Render(p, hdr, ldr)
    got = ldr.download()
    worst, counts, checked = ft.check_ldr(got[..., :3].reshape(-1, 3), frame[..., :3].reshape(-1, 3), EDGE_A, p, f"edge, A {EDGE_A}")
    print(f"edge frame w {w}, A = {EDGE_A}: ratio {worst:.3f}, flags {counts}")
    assert checked > 0.99 * got[..., :3].size and counts["rounding"] > 0 and counts["inf_nan"] > 0 and counts["saturated"] > 0
    for o in (hdr, ldr, tm):
        o.close()


def _owned_pixels(frame, rank, world):
    h, w = frame.shape[:2]
    tx = vp.owner_grid(w, h)[0]
    blocks = [frame[(t // tx) * 128:(t // tx) * 128 + 128, (t % tx) * 128:(t % tx) * 128 + 128, :3].reshape(-1, 3)
              for t in vp.owned_tiles(w, h, rank, world)]
    return np.concatenate(blocks) if blocks else np.zeros((0, 3), np.uint16)


def _upload_packed(gpu_ctx, packed):
    raw = packed.reshape(-1).view(np.uint8)
    rows = (raw.nbytes + 8 * 128 - 1) // (8 * 128)
    pad = np.zeros(rows * 8 * 128, np.uint8)
    pad[:raw.nbytes] = raw
    buf = vr.HdrImage(gpu_ctx, 128, rows)
    buf.upload(pad.view(np.uint16).reshape(rows, 128, 4))
    return buf


@pytest.mark.parametrize("world", [2, 3, 8])
def test_edge_frame_packed_tiles(gpu_ctx, world):
    """Packed RGB16F tiles: every rank's own histogram against the model of its pixels (the whole frame's Q), the ranks'
    histograms summed on the host against the whole frame's model, the exposure of the sum, every rank's packed RGB8
    tiles through vr_frame_detile_ldr against the operator."""
    w = 1024                                                    # 8 x 2 tiles: every rank of 8 owns some
    p = vr.default_tonemap_params()
    frame = ft.as_frame(ft.edge_pixels(p, EDGE_A), w)
    h = frame.shape[0]
    info = partition_info(w, h, 0, world)
    bufs, total = [], np.zeros(256, np.int64)
    for r in range(world):
        buf = _upload_packed(gpu_ctx, vp.pack(frame, r, world))
        tm = vr.ToneMappingPass(gpu_ctx)
        tm.ResetHistogram()
        tm.AddFrameToHistogram(p, buf, w, h, vr.Partition(r, world))
        hist, _ = tm.download()
        tm.close()
        hm = ft.histogram_model(ft.PixelSet(_owned_pixels(frame, r, world)), p, frame_pixels=w * h)
        ft.check_histogram(hist, hm, f"rank {r} of {world}")
        total += hist
        bufs.append(buf)
    hm = ft.histogram_model(ft.PixelSet.from_frame(frame), p)
    print(f"world {world}: summed histogram ratio {ft.check_histogram(total, hm, f'sum of {world} ranks'):.3f}")
    tm = vr.ToneMappingPass(gpu_ctx)
    tm.ResetHistogram()
    for r in range(world):
        tm.AddFrameToHistogram(p, bufs[r], w, h, vr.Partition(r, world))      # accumulates: what the all-reduce leaves
    tm.AdvanceFrame(1 / 60)
    tm.ComputeExposure(p)
    hist, lum = tm.download()
    assert np.array_equal(hist.astype(np.int64), total)
    print("exposure ratios", ft.check_exposure(lum, hist, hm, p, 1 / 60, 0.0, f"world {world}"))
    gathered = np.zeros(world * info["packed_bytes_ldr"], np.uint8)
    for r in range(world):
        out = vr.LdrImage(gpu_ctx, w, h, capacity_bytes=info["packed_bytes_ldr"])
        tm.Render(p, bufs[r], out, w, h, vr.Partition(r, world))
        gathered[r * info["packed_bytes_ldr"]:(r + 1) * info["packed_bytes_ldr"]] = out.download(info["packed_bytes_ldr"])
        out.close()
    g_rows = (gathered.nbytes + 8 * 1024 - 1) // (8 * 1024)
    g_dev = vr.HdrImage(gpu_ctx, 1024, g_rows)
    pad = np.zeros(g_rows * 8 * 1024, np.uint8); pad[:gathered.nbytes] = gathered
    g_dev.upload(pad)
    ldr = vr.LdrImage(gpu_ctx, w, h)
    partition_prepare(gpu_ctx, w, h, vr.Partition(0, world))
    frame_detile_ldr(gpu_ctx, g_dev.device_ptr, world, w, h, ldr)
    got = ldr.download()
    assert (got[..., 3] == 255).all()
    worst, counts, checked = ft.check_ldr(got[..., :3].reshape(-1, 3), frame[..., :3].reshape(-1, 3), lum, p, f"world {world} LDR")
    print(f"world {world} LDR: ratio {worst:.3f}, flags {counts}")
    assert checked > 0.99 * got[..., :3].size
    for b in bufs:
        b.close()
    g_dev.close(); ldr.close(); tm.close()


def _lit(gpu_ctx, tp, size, cam, w, h):
    eye, tgt = scaled_camera(cam, size)
    view = vr.make_view(eye, tgt, w, h)
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    hdr = vr.HdrImage(gpu_ctx, w, h)
    tp.Render(view, view, rt, vr.default_render_params(400.0, assume_cleared=1))
    vr.DeferredLightingPass(gpu_ctx).Render(view, rt, [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
    rt.close()
    out = hdr.download()
    hdr.close()
    return out


@pytest.mark.parametrize("size", [256, 2048])
def test_lit_terrain_frames(gpu_ctx, terrain, size):
    """Lit terrain frames with sky (640x360, four cameras in sequence, each step from the device's previous value)."""
    p = vr.default_tonemap_params()
    tm = vr.ToneMappingPass(gpu_ctx)
    old, sky = 0.0, []
    for cam in (0, 7, 3, 1):
        frame = _lit(gpu_ctx, terrain[size], size, CAMERAS[cam], 640, 360)
        sky.append(float((frame[..., :3] == 0).all(-1).mean()))
        old = _simple_render(gpu_ctx, tm, p, frame, 1 / 60, old, f"{size}^2 camera {cam}")
    assert max(sky) > 0.02, ("some frame shows sky", sky)
    tm.close()


def test_frame_submit_tone_map_stage(gpu_ctx, terrain):
    """The single-rank vr_frame_submit path with its tone-map stage."""
    w, h, size = 640, 360, 256
    tp = terrain[size]
    eye, tgt = scaled_camera(CAMERAS[5], size)
    view = vr.make_view(eye, tgt, w, h)
    p = vr.default_tonemap_params()
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    hdr, ldr = vr.HdrImage(gpu_ctx, w, h), vr.LdrImage(gpu_ctx, w, h)
    tm = vr.ToneMappingPass(gpu_ctx)
    tm.AdvanceFrame(1 / 60)
    fr = vr.Frame(tp, rt, vr.default_render_params(400.0), [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM, tonemap=tm,
                  tonemap_params=p, ldr=ldr)
    fr.submit(view, hdr)
    gpu_ctx.synchronize()
    frame = hdr.download()
    hist, lum = tm.download()
    got = ldr.download()
    r = ft.check_step(hist, lum, got[..., :3].reshape(-1, 3), ft.PixelSet.from_frame(frame), p, 1 / 60, 0.0, "frame submit",
                      codes=frame[..., :3].reshape(-1, 3))
    _report("frame submit", r)
    for o in (hdr, ldr, tm, rt):
        o.close()


def test_8k_flythrough_frame(gpu_ctx, terrain):
    """The bench's 8K flythrough frame: the histogram bound over all 33.2 M pixels, the exposure, LDR on a fixed
    2^20-pixel sample."""
    w, h = 7680, 4320
    frame = _lit(gpu_ctx, terrain[2048], 2048, flythrough_camera(7), w, h)
    p = vr.default_tonemap_params()
    tm = vr.ToneMappingPass(gpu_ctx)
    hdr, ldr = vr.HdrImage(gpu_ctx, w, h), vr.LdrImage(gpu_ctx, w, h)
    hdr.upload(frame)
    tm.AdvanceFrame(1 / 60)
    tm.SimpleRender(p, hdr, ldr)
    hist, lum = tm.download()
    got = ldr.download()
    hm = ft.histogram_model(ft.PixelSet.from_frame(frame), p)
    rh = ft.check_histogram(hist, hm, "8K")
    r1, r2 = ft.check_exposure(lum, hist, hm, p, 1 / 60, 0.0, "8K")
    idx = np.random.default_rng(8).choice(w * h, 1 << 20, replace=False)
    worst, counts, checked = ft.check_ldr(got.reshape(-1, 4)[idx, :3], frame.reshape(-1, 4)[idx, :3], lum, p, "8K sample")
    print(f"8K: hist {rh:.3f}, exposure {r1:.3f} / {r2:.3f} (adapted {lum}), LDR {worst:.3f}, flags {counts}, hist cancel {hm['cancel']}")
    assert checked > 0.99 * 3 * len(idx)
    for o in (hdr, ldr, tm):
        o.close()


@pytest.mark.parametrize("case", [c[0] for c in ft.adaptation_cases()])
def test_adaptation_sequences(gpu_ctx, case):
    """Bright / dark frames alternating, dt 0, 1/60, 1, speeds of 0, low == high, percentiles 0 and 1, min == max adapted:
    each step from the device's previous value; dt = 0 holds the value."""
    name, kw, steps = next(c for c in ft.adaptation_cases() if c[0] == case)
    p = vr.default_tonemap_params(**kw)
    tm = vr.ToneMappingPass(gpu_ctx)
    old = 0.0
    for i, (kind, dt) in enumerate(steps):
        lum = _simple_render(gpu_ctx, tm, p, ft.sequence_frame(kind, i), dt, old, f"{case} step {i}")
        if dt == 0.0 and old > 0.0 and p.eye_adaptation_speed_up > 0.0 and p.eye_adaptation_speed_down > 0.0:
            assert lum == old
        old = lum
    tm.close()


def test_frame_above_2_26_pixels(gpu_ctx):
    """16384 x 4200: 4100 black rows, 100 rows at 0.3 (68.8 M pixels, Q = 32).  With a 64-count quantum the black bin
    wrapped and the frame adapted to the bright band; the window lies in the black rows: minimum adapted luminance.
    Closed-form model; then a world-2 share of the same frame."""
    w, h, rows = 16384, 4200, 100
    p = vr.default_tonemap_params()
    frame = np.zeros((h, w, 4), np.uint16)
    frame[h - rows:, :, :3] = ft._to_half(0.3)
    hdr = vr.HdrImage(gpu_ctx, w, h)
    hdr.upload(frame)
    tm = vr.ToneMappingPass(gpu_ctx)
    tm.ResetHistogram()
    tm.AddFrameToHistogram(p, hdr)
    tm.ComputeExposure(p)
    hist, lum = tm.download()
    hm = ft.histogram_model(ft.banded(w, h, rows, 0.3), p)
    assert hm["q"] == 32
    ft.check_histogram(hist, hm, "16384x4200")
    ft.check_exposure(lum, hist, hm, p, 0.0, 0.0, "16384x4200")
    assert np.float32(lum) == np.float32(0.02)
    ldr = vr.LdrImage(gpu_ctx, w, h)
    tm.Render(p, hdr, ldr)
    got = ldr.download()[h - rows - 2:h - rows + 2]
    ldr.close(); hdr.close()
    ft.check_ldr(got[..., :3].reshape(-1, 3), frame[h - rows - 2:h - rows + 2, :, :3].reshape(-1, 3), lum, p, "16384x4200 LDR")
    buf = _upload_packed(gpu_ctx, vp.pack(frame, 1, 2))
    del frame
    tm.ResetHistogram()
    tm.AddFrameToHistogram(p, buf, w, h, vr.Partition(1, 2))
    hist, _ = tm.download()
    share = ft.histogram_model(ft.banded_share(w, h, rows, 0.3, 1, 2), p, frame_pixels=w * h)
    ft.check_histogram(hist, share, "16384x4200, rank 1 of 2")
    buf.close(); tm.close()


@pytest.mark.parametrize("w", [8, 6], ids=["vector", "scalar"])
@pytest.mark.parametrize("how", ["reset_exposure", "min_adapted_unset", "min_adapted_computed"])
def test_extreme_exposure_saturates(gpu_ctx, how, w):
    """adapted = 1e-30 (through vr_tonemap_reset_exposure, through min_adapted_luminance with the exposure unset, and
    through compute_exposure with min = max): the fused mapped / src overflows; bright pixels must be 255, not 0."""
    vals = [60000.0, 1.0, 1e-4, 0.0]
    h5 = ft._to_half
    codes = [[h5(v)] * 3 for v in vals] + [[h5(0.5), 0, 0], [0, h5(65504.0), 0], [h5(2.0), h5(-1.0), h5(1.0)], [0, 0, 0]]
    frame = ft.as_frame(np.array(codes[:w], np.uint16), w)
    p = vr.default_tonemap_params(**({} if how == "reset_exposure" else dict(min_adapted_luminance=1e-30, max_adapted_luminance=1e-30)))
    hdr, ldr = vr.HdrImage(gpu_ctx, w, 1), vr.LdrImage(gpu_ctx, w, 1)
    hdr.upload(frame)
    tm = vr.ToneMappingPass(gpu_ctx)
    if how == "reset_exposure":
        tm.ResetExposure(1e-30)
    elif how == "min_adapted_unset":
        tm.ResetExposure(0.0)
    else:
        tm.ResetHistogram()
        tm.ComputeExposure(p)
    tm.Render(p, hdr, ldr)
    _, lum = tm.download()
    a = lum if lum > 0 else 1e-30
    got = ldr.download()[0, :, :3]
    ft.check_ldr(got, frame[0, :, :3], a, p, f"extreme exposure ({how}, w {w})")
    assert got[:3].tolist() == [[255] * 3] * 3 and got[3].tolist() == [0, 0, 0]
    assert got[4].tolist() == [255, 0, 0] and got[5].tolist() == [0, 255, 0]
    for o in (hdr, ldr, tm):
        o.close()


@pytest.mark.parametrize("w", [8, 6], ids=["vector", "scalar"])
def test_a_refused_simple_render_leaves_bins_and_adapted_luminance(gpu_ctx, w):
    """vr_tonemap_simple_render with an LDR buffer one byte short is refused before its first step: the bins keep their
    (non-zero) content instead of being reset, and the adapted luminance is not advanced."""
    tmp = vr.default_tonemap_params()
    hdr, ldr = vr.HdrImage(gpu_ctx, w, 1), vr.LdrImage(gpu_ctx, w, 1, capacity_bytes=w * 4 - 1)
    tm = vr.ToneMappingPass(gpu_ctx)
    try:
        hdr.upload(np.tile(np.array([0x3800, 0x3c00, 0x4000, 0], np.uint16), w))
        tm.AdvanceFrame(1.0 / 60.0)
        tm.AddFrameToHistogram(tmp, hdr)
        tm.ResetExposure(0.25)
        bins, lum = tm.download()
        assert bins.any() and lum == 0.25
        with pytest.raises(vr.VrError) as e:
            tm.SimpleRender(tmp, hdr, ldr)
        assert e.value.code == vr.capi.VR_ERR_INVALID_ARGUMENT and "ldr buffer is smaller than the frame" in str(e.value), e.value
        bins1, lum1 = tm.download()
        assert np.array_equal(bins, bins1), "the refused call touched the histogram"
        assert np.float32(lum1).view(np.uint32) == np.float32(lum).view(np.uint32), (lum, lum1)
    finally:
        for o in (tm, ldr, hdr):
            o.close()
