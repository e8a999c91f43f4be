"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol the header
declares, its pure-host entry points behave, and it fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from vrenderer_amd import partition as pt
from tests.common import DEFAULT_EYE, DEFAULT_TARGET
from tests.host_check import build_allgather_example, build_host_example, build_host_check, run_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu(lib):
    h = C.c_void_p()
    rc = lib.vr_context_create(0, C.byref(h))
    if rc == capi.VR_OK:
        lib.vr_context_destroy(h)
        return True
    return False


def test_library_exports_every_declared_symbol(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    declared = re.findall(r"VR_API\s+[\w\s\*]+?\b(vr_\w+)\s*\(", header)
    assert len(declared) >= 30
    assert sorted(set(declared)) == sorted(set(capi.EXPORTS)), "capi.EXPORTS and include/vrterrain.h disagree"
    for name in declared:
        assert hasattr(product_lib, name), name


def test_the_tables_read_back_is_declared_exported_and_refuses_before_the_device(product_lib):
    """vr_debug_terrain_tables: the header's signature and table ids, capi's export and argtypes, and every argument refusal - each
    comes before any use of the device (there is none here) and leaves out_dims, `out` and the terrain as they were.  A terrain with
    no chain (zeroed memory stands in for it) has no level 0: VR_OK, zero out_dims, `out` untouched."""
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_debug_terrain_tables\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*int table,\s*int32_t level,\s*int32_t out_dims\[2\],"
                     r"\s*void\*\s*out,\s*size_t capacity_bytes\)", header)
    assert re.search(r"enum\s*\{\s*VR_DEBUG_TABLE_QUAD = 0,\s*VR_DEBUG_TABLE_QUADF = 1,\s*VR_DEBUG_TABLE_FAST = 2,\s*VR_DEBUG_TABLE_RGBF = 3\s*\}", header)
    assert (capi.VR_DEBUG_TABLE_QUAD, capi.VR_DEBUG_TABLE_QUADF, capi.VR_DEBUG_TABLE_FAST, capi.VR_DEBUG_TABLE_RGBF) == (0, 1, 2, 3)
    fn = product_lib.vr_debug_terrain_tables
    assert "vr_debug_terrain_tables" in capi.EXPORTS and fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t]
    fake = C.create_string_buffer(1 << 20)
    t = C.cast(fake, C.c_void_p)
    dims, out = (C.c_int32 * 2)(-1, -1), (C.c_uint8 * 16)(*([5] * 16))
    inv = capi.VR_ERR_INVALID_ARGUMENT
    for args in ((None, 0, 2, 0, dims, out, 16), (None, 0, 2, 0, dims, None, 0), (t, 2, 2, 0, dims, out, 16), (t, -1, 2, 0, dims, out, 16),
                 (t, 0, 4, 0, dims, out, 16), (t, 0, -1, 0, dims, out, 16), (t, 1, 2, -1, dims, out, 16), (t, 0, 0, 0, None, out, 16),
                 (t, 0, 0, 0, dims, None, 16)):
        assert fn(*args) == inv, args[1:4]
    assert b"capacity" in product_lib.vr_last_error()
    assert list(dims) == [-1, -1] and list(out) == [5] * 16 and bytes(fake) == bytes(1 << 20)
    for which in (0, 1):
        for table in range(4):
            for args in ((None, 0), (out, 16)):
                dims[0] = dims[1] = -1
                assert fn(t, which, table, 0, dims, *args) == capi.VR_OK and list(dims) == [0, 0], (which, table)
    assert list(out) == [5] * 16 and bytes(fake) == bytes(1 << 20)


def test_struct_layouts_match_header():
    assert C.sizeof(capi.Instance) == 112 and C.sizeof(capi.Light) == 64
    assert C.sizeof(capi.TerrainParams) == 40 and C.sizeof(capi.RenderParams) == 32
    assert C.sizeof(capi.View) == 16 * 4 * 4 + 16 + 96 + 8 * 4
    assert C.sizeof(capi.Partition) == 8


def test_defaults_are_the_reference_settings(product_lib):
    p = vr.default_terrain_params()
    # TerrainSettings (TerrainPass.h:23-30), minLodDistance (QuadTree.cpp:236), morph start (terrain_vs.hlsl:20)
    assert (p.max_instances, p.surface_size, p.world_size, p.grid_size) == (4096, 2048.0, 2048.0, 32)
    assert p.min_lod_distance == 4.0 and abs(p.morph_start - 0.85) < 1e-7
    rp = vr.default_render_params()
    assert rp.max_height == 400.0 and not (rp.wireframe or rp.lock_view or rp.depth_only)   # Renderer.h:37-40


def test_shadow_and_tonemap_defaults_and_argument_checks(product_lib, oracle):
    assert C.sizeof(capi.ShadowParams) == 32 and C.sizeof(capi.TonemapParams) == 40 and C.sizeof(capi.ShadowBinding) == 24
    sp = vr.default_shadow_params(2048.0)                      # CascadedShadowMap(device, 2048, 1, 0, fmt), WORLD_SIZE x3 (Renderer.cpp:83,349-352)
    assert (sp.resolution, sp.max_shadow_distance, sp.light_space_z_up, sp.light_space_z_down, sp.depth_bias) == (2048, 2048.0, 2048.0, 2048.0, 0.0)
    tm = vr.default_tonemap_params()                           # ToneMappingParameters() defaults
    assert [round(getattr(tm, n), 4) for n, _ in capi.TonemapParams._fields_] == [0.8, 0.95, 1.0, 0.5, 0.02, 0.5, -0.5, 3.0, -10.0, 4.0]
    cam = vr.make_view(DEFAULT_EYE, DEFAULT_TARGET, 1920, 1080)
    sun, out = vr.reference_sun(), vr.View()
    assert product_lib.vr_shadow_view_setup(C.byref(sun), C.byref(cam), C.byref(sp), C.byref(out)) == capi.VR_OK
    assert bytes(out) == bytes(oracle.shadow_view(sun, cam, sp))                     # host code == restatement, every field
    assert out.viewport_w == out.viewport_h == 2048 and out.view_to_clip[15] == 1.0 and out.view_to_clip[11] == 0.0   # orthographic
    lamp = vr.point_light((0, 10, 0), 100.0, 50.0)
    assert product_lib.vr_shadow_view_setup(C.byref(lamp), C.byref(cam), C.byref(sp), C.byref(out)) == capi.VR_ERR_INVALID_ARGUMENT
    assert b"directional" in product_lib.vr_last_error()
    bad = vr.default_shadow_params(2048.0, resolution=0)
    assert product_lib.vr_shadow_view_setup(C.byref(sun), C.byref(cam), C.byref(bad), C.byref(out)) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_shadow_view_setup(None, C.byref(cam), C.byref(sp), C.byref(out)) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_partition_packed_bytes_ldr(7680, 4320, 8) * 2 == product_lib.vr_partition_packed_bytes(7680, 4320, 8)


def test_view_helper_matches_oracle_bit_for_bit(product_lib, oracle):
    for (w, h) in ((1920, 1080), (7680, 4320), (333, 777)):
        for eye, tgt in ((DEFAULT_EYE, DEFAULT_TARGET), ((600.0, 250.0, 0.0), (0.0, 0.0, 0.0)), ((3.0, 9.0, -4.0), (100.0, 0.0, 50.0))):
            assert bytes(vr.make_view(eye, tgt, w, h)) == bytes(oracle.view_from_camera(eye, tgt, w, h))


def test_view_helper_rejects_bad_arguments(product_lib):
    v = vr.View()
    f3 = (C.c_float * 3)(0, 0, 0)
    assert product_lib.vr_view_from_camera(f3, f3, f3, 1.0, 0.1, 100.0, 0, 10, C.byref(v)) == capi.VR_ERR_INVALID_ARGUMENT
    assert b"projection" in product_lib.vr_last_error()
    assert product_lib.vr_view_from_camera(f3, f3, f3, 1.0, 1.0, 0.5, 10, 10, C.byref(v)) == capi.VR_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("w,h,world", [(7680, 4320, 8), (7680, 4320, 1), (3840, 2160, 4), (1920, 1080, 2), (300, 260, 3), (64, 64, 8)])
def test_partition_tables_agree_with_python_mirror(product_lib, w, h, world):
    tx, ty = pt.owner_grid(w, h)
    counts = []
    for r in range(world):
        info = vr.passes.partition_info(w, h, r, world)
        assert (info["tiles_x"], info["tiles_y"]) == (tx, ty)
        assert info["owned"] == len(pt.owned_tiles(w, h, r, world))
        assert info["max_owned"] == pt.max_owned(w, h, world)
        assert info["packed_bytes"] == pt.max_owned(w, h, world) * 128 * 128 * 6
        counts.append(info["owned"])
    assert sum(counts) == tx * ty
    if (w, h, world) == (7680, 4320, 8):
        # 60 x 34 = 2,040 owner tiles, ~255 per rank (the diagonal interleave is balanced to within 2 tiles)
        assert (tx, ty) == (60, 34) and max(counts) - min(counts) <= 2 and max(counts) == 256
    slots = pt.tile_slots(w, h, world)
    assert len(set(slots.tolist())) == tx * ty


def test_fails_loudly_without_a_gpu(product_lib):
    if _has_gpu(product_lib):
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    assert product_lib.vr_context_create(0, C.byref(h)) == capi.VR_ERR_NO_DEVICE
    assert b"no HIP device" in product_lib.vr_last_error()
    with pytest.raises(vr.VrError):
        vr.Context(0)


def test_missing_extension_raises(monkeypatch, tmp_path):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        capi.load_library()


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under vrenderer_amd/ may reference it."""
    pkg = os.path.join(ROOT, "vrenderer_amd")
    for dirpath, _, files in os.walk(pkg):
        if os.path.basename(dirpath) in ("build", "lib", "__pycache__"):
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "vr_oracle" not in text and "pyoracle" not in text and "from oracle" not in text, os.path.join(dirpath, f)


def test_product_build_has_no_experiment_switch():
    """Timing experiments that render wrong images on purpose (VR_EXP_*) and instrumented kernels live behind
    csrc/vr_experiments.h and -DVR_EXPERIMENT_BUILD: the library the tests and the bench load was built with none of them,
    the kernel sources test constexpr flags instead of the preprocessor, and the product's compiler flags define nothing."""
    lib = capi.load_library()
    assert lib.vr_build_experiments() == 0
    csrc = os.path.join(ROOT, "vrenderer_amd", "csrc")
    for f in os.listdir(csrc):
        text = open(os.path.join(csrc, f), errors="ignore").read()
        if f == "vr_experiments.h":
            assert "#error" in text and "VR_EXPERIMENT_BUILD" in text
            continue
        assert "VR_EXP_" not in text and "VR_LDS_PAD" not in text, f"{f}: experiment switches belong in vr_experiments.h"
        if f.endswith(".hip") and ("VR_RASTER_PROFILE" in text or "VR_SELECT_PROFILE" in text):
            assert '#include "vr_experiments.h"' in text, f"{f}: profiling switches are guarded by vr_experiments.h"
    from vrenderer_amd import build as b
    flags = list(b.FLAGS) + [x for v in b.PER_FILE_FLAGS.values() for x in v]
    assert not any(x.startswith("-DVR_") for x in flags), flags


def test_geometry_slot_policy_lives_in_its_header_alone():
    """Which geometry set a call gets is vr_geosets.h's: no other file under csrc names the fields and functions it replaced, and
    the .hip files and vr_internal.h reach vr_terrain::slots through its transitions - they read its fields and assign none."""
    csrc = os.path.join(ROOT, "vrenderer_amd", "csrc")
    write = re.compile(r"(\+\+|--)\s*[\w\->.]*\bslots\.|\bslots\.(cur|counter|slot\[[^\]]*\]\.\w+)\s*(=(?!=)|\+\+|--|[-+|&^]=)")
    for f in sorted(os.listdir(csrc)):
        if f == "vr_geosets.h":
            continue
        text = open(os.path.join(csrc, f), errors="ignore").read()
        for gone in ("prep_serial", "prep_counter", "prepared_matches", "vr_terrain_pick_set"):
            assert gone not in text, f"{f}: {gone} belongs to vr_geosets.h"
        assert not re.search(r"\.prepared\s*=(?!=)", text), f"{f}: a prepared frame is given up through geoslots_claim / geoslots_invalidate"
        assert not write.search(text), f"{f}: {write.search(text).group(0)!r} writes the slot state past vr_geosets.h"


def test_pack_detile_roundtrip_numpy():
    rng = np.random.default_rng(3)
    for (w, h, world) in ((300, 260, 3), (512, 256, 2), (130, 70, 8)):
        frame = rng.integers(0, 65535, (h, w, 4), dtype=np.uint16)
        frame[..., 3] = 0                                  # HdrColor's alpha is 0 on this path and is not exchanged
        gathered = np.concatenate([pt.pack(frame, r, world) for r in range(world)], 0)
        assert np.array_equal(pt.detile(gathered, w, h, world), frame)


def test_cpp_host_example_compiles_links_and_fails_soft_without_gpu(product_lib, tmp_path):
    """The header is usable from C++ and the library links; without a device the example reports it."""
    exe = build_host_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if _has_gpu(product_lib):
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 0 and "no device" in r.stdout and "no HIP device" in r.stderr, r.stdout + r.stderr


def test_raster_plan_matches_the_transcribed_decisions_and_invariants(tmp_path):
    """vr_raster_plan.h compiles without HIP and raster_plan() agrees, for every input, with the tile pass's decisions as
    they were written inside terrain_render_impl, and with the invariants of tests/host/raster_plan_check.cpp."""
    exe = build_host_check(tmp_path, "raster_plan_check")
    r = run_host_check(exe)
    assert "786432 cases" in r.stdout, r.stdout[-400:]          # 2^16 bools x 2 worlds x 2 tile edges x 3 requests


def test_devbuf_grow_is_all_or_nothing_at_every_failure_position(tmp_path):
    """vr_devbuf.h compiles without HIP; a single grow and group grows of 1..15 buffers keep every pointer, capacity and live
    block on a failure at any allocation (or a refusing quiesce) and free each old block once, behind quiesce, on success; the
    reserve reaches the doubling policy's capacity, or exactly the request where the doubled size is refused
    (tests/host/devbuf_check.cpp)."""
    exe = build_host_check(tmp_path, "devbuf_check")
    r = run_host_check(exe)
    # single: 3 x 6 x 2 x 2; groups: 4 patterns x 2 x (N + 1), N = 1..15; reserve: 4 x 5 x 2 x 3 allocators = 120
    assert "1272 cases" in r.stdout, r.stdout[-400:]


def test_stream_order_matches_the_transcribed_protocol_and_the_happens_before_model(tmp_path):
    """vr_order.h compiles without HIP.  Over every sequence of up to four API calls and a fixed sample of longer ones
    (tests/host/order_check.cpp) the protocol queues the records and waits the ordering code it replaced queued, apart from the
    intended differences the program names, and no two conflicting accesses to a geometry set, the node heights, an HDR image,
    a map, the query pyramid, the journal's arena, the brush buffers or the query staging are left unordered by the streams'
    vector clocks (or, where the host frees or rewrites memory, by what the host waited for); a transcription that loses any one
    wait is reported, but for the seven the program names with the reason each orders nothing.  The eleven calls of the editing
    path (the pyramid's read-back, a reader of the pyramid, is the youngest) run to the same exhaustive depth as the others: the
    program takes about 4 s.  The stamped launches take their events from vr_events.h with a ring of four, and a frame of another
    terrain is one of the calls: slots are reissued inside the sequences, every re-stamp must come behind the event's previous
    occupant, and one pinned sequence waits on a reissued slot across a stream change.  No wait site was added for it."""
    exe = build_host_check(tmp_path, "order_check")
    r = run_host_check(exe)
    # 33 + 33^2 + 33^3 + 33^4 of 33 calls (21 + the editing path's 11 + another terrain's frame), 200000 random
    assert "1422980 sequences" in r.stdout, r.stdout[-400:]
    assert "handle no longer live, waited for, ordered" in r.stdout, r.stdout[-4000:]
    run_host_check(exe, "--drop-each", expect="19 of 26 wait sites reported")      # 17 + 9 sites; 16 + 3 reported


def test_event_supply_keeps_its_invariants_over_random_transitions(tmp_path):
    """vr_events.h compiles without HIP.  Against a counting fake of its ops, over random sequences of its transitions
    (tests/host/events_check.cpp), no event is in two places at once, every event created is destroyed exactly once, a scope
    that ends without a launch leaves no never-recorded pair, a failed creation leaves the launch unstamped, collect returns
    exactly the pairs committed since the last recycle (and recycles when a query fails), and a handle is live exactly until
    its pool epoch passes or its ring slot is reissued; once more under the address and undefined-behaviour sanitizers."""
    r = run_host_check(build_host_check(tmp_path, "events_check"))
    assert "20000 cases" in r.stdout, r.stdout[-400:]
    san = build_host_check(tmp_path, "events_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "events_check_san")
    run_host_check(san)


def test_scratch_policy_matches_the_transcribed_code_and_its_invariants(tmp_path):
    """vr_scratch.h compiles without HIP.  Over every sequence of one and two events and a fixed sample of longer ones
    (tests/host/scratch_check.cpp: chains completing with boundary status words, polls, synchronous reads, reserves, a granting
    or refusing allocator) its functions leave the state, return the codes, request the allocations and pick the messages of
    the code they replaced, and keep the capacity, reporting and refusal invariants the program names."""
    exe = build_host_check(tmp_path, "scratch_check")
    r = run_host_check(exe)
    # 12 configurations x (730 + 730^2 of 730 events, 20000 random); 730 = 3 sets x 6 x 8 x 5 words + 2 + 2 + 4 + 2
    assert "6643560 sequences" in r.stdout, r.stdout[-400:]


def test_gbuffer_state_matches_the_transcribed_code_and_the_memory_model(tmp_path):
    """vr_gbuffer_state.h compiles without HIP.  Over every sequence of one and two events, every sequence of up to four of a
    smaller set and a fixed sample of longer ones (tests/host/gbuffer_state_check.cpp: clears, renders of every variant over
    every coverage - run or refused at each point -, lighting passes, uploads, download, describe, the tracking switched) its
    transitions leave the state, the answers and the fills of the code they replaced, apart from the two intended differences
    the program names, and the memory they describe is what it would be with every clear eager and nothing skipped; each
    transition weakened in turn is reported."""
    exe = build_host_check(tmp_path, "gbuffer_state_check")
    r = run_host_check(exe)
    # 2089 + 2089^2 of all events, 57 + .. + 57^4 of the smaller set, 200000 random
    assert "15310510 sequences" in r.stdout, r.stdout[-400:]
    run_host_check(exe, "--break-each", expect="15 of 15 weakenings reported")


def test_geometry_slot_policy_matches_the_transcribed_code_and_its_invariants(tmp_path):
    """vr_geosets.h compiles without HIP.  Over every sequence of up to four events and a fixed sample of longer ones
    (tests/host/geosets_check.cpp: prepares, renders with and without lock_view, selects, invalidations and materialising passes
    over six keys, any fallible step of any of them refused) its transitions choose the sets, answer and leave the state of the
    code they replaced in vr_raster.hip, vr_select.hip and vr_derive.hip, and keep the invariants the program names - the current
    set is never prepared, the pick is never the current set, a selection is never lost, a materialising pass leaves the current
    set alone; each rule weakened in turn is reported; once more under the address and undefined-behaviour sanitizers."""
    exe = build_host_check(tmp_path, "geosets_check")
    r = run_host_check(exe)
    # 32 + 32^2 + 32^3 + 32^4 of 32 events (4 x 6 keys, select, invalidate, 6 failing steps), 200000 random
    assert "1282400 sequences" in r.stdout, r.stdout[-400:]
    run_host_check(exe, "--break-each", expect="8 of 8 weakenings reported")
    san = build_host_check(tmp_path, "geosets_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "geosets_check_san")
    run_host_check(san)


def test_cpp_allgather_example_compiles_and_fails_soft_without_gpu(product_lib, tmp_path):
    """The N-rank C++ host (RCCL communicator + vr_frame_allgather_ldr + vr_tonemap_allreduce_histogram) builds against
    rccl.h and the C ABI; without a device it says so."""
    exe = build_allgather_example(tmp_path)
    if _has_gpu(product_lib):
        pytest.skip("run by the GPU suite")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "no device" in r.stdout, r.stdout + r.stderr


def test_library_does_not_link_rccl(product_lib):
    """RCCL is resolved at first use from the copy in the process (vr_comm.hip): no DT_NEEDED entry for it."""
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "vrenderer_amd", "lib", "libvrterrain.so")], capture_output=True, text=True).stdout
    assert "rccl" not in out.lower(), out


def test_header_is_valid_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include <vrterrain.h>\nint main(void) { vr_view v; vr_light l; (void)v; (void)l; return sizeof(vr_instance) == 112 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "c_check")], check=True, capture_output=True, text=True)
    assert subprocess.run([str(tmp_path / "c_check")]).returncode == 0


def test_ctypes_mirrors_have_the_header_s_struct_sizes(tmp_path):
    """The ctypes structures of vrenderer_amd/capi.py against sizeof() of the C declarations they mirror."""
    from vrenderer_amd import capi
    pairs = [("vr_view", capi.View), ("vr_light", capi.Light), ("vr_instance", capi.Instance), ("vr_terrain_params", capi.TerrainParams),
             ("vr_render_params", capi.RenderParams), ("vr_partition", capi.Partition), ("vr_shadow_params", capi.ShadowParams),
             ("vr_shadow_binding", capi.ShadowBinding), ("vr_tonemap_params", capi.TonemapParams), ("vr_frame_desc", capi.FrameDesc),
             ("vr_gbuffer_desc", capi.GBufferDesc)]
    src = tmp_path / "sizes.c"
    src.write_text("#include <stdio.h>\n#include <vrterrain.h>\nint main(void) {\n"
                   + "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n, _ in pairs) + "    return 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")], check=True,
                   capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "sizes")], capture_output=True, text=True, check=True).stdout.splitlines())
    import ctypes as C
    for n, t in pairs:
        assert int(out[n]) == C.sizeof(t), (n, out[n], C.sizeof(t))


def test_png_ingest_round_trip(tmp_path, oracle):
    """Row f4: PNG heightmap / albedo ingest gives back exactly the bytes TerrainPass.Init takes."""
    from vrenderer_amd import io as vio
    h = oracle.synth_heightmap(64)
    a = oracle.synth_albedo(64, h)
    vio.save_png(str(tmp_path / "h.png"), h)
    vio.save_png(str(tmp_path / "a.png"), a)
    assert np.array_equal(vio.load_heightmap_png(str(tmp_path / "h.png")), h)
    assert np.array_equal(vio.load_albedo_png(str(tmp_path / "a.png")), a)
    vio.save_png(str(tmp_path / "rgb.png"), a[..., :3])
    assert np.array_equal(vio.load_heightmap_png(str(tmp_path / "rgb.png")), a[..., 0])
