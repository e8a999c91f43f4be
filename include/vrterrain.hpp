// vrterrain.hpp — C++ host mirror of the reference's interface for the hot path, over the C ABI
// of vrterrain.h.  Header-only, no dependencies beyond the C++17 standard library.
//
// Names, argument meaning and error behaviour follow the reference so that a caller written
// against vRenderer::TerrainPass / QuadTree / RenderTargets / DeferredLightingPass reads the same:
//   vRenderer::TerrainPass      source/terrain/TerrainPass.h:32-159   (Init, Render, GetQuadTrees)
//   QuadTree                    source/terrain/QuadTree.h:64-127      (NodeSelect, GetSelectedNodes,
//                                                                      ClearSelectedNodes, GetNumLods, GetLodRanges)
//   vRenderer::RenderTargets    source/Renderer.h:50-110              (Init, Clear, IsUpdateRequired)
//   DeferredLightingPass        as called at source/Renderer.cpp:239-240,417-428 (Render(view, Inputs))
//   CascadedShadowMap           as called at source/Renderer.cpp:83-87,333-372 (SetupForPlanarViewStable, Clear, GetView)
//   ToneMappingPass             as called at source/Renderer.cpp:188-189,256-257,430-431 (AdvanceFrame, SimpleRender)
// Like the reference, nothing here throws: methods return bool / log through a callback
// (donut::log in the reference, TerrainPass.cpp:224-227, QuadTree.cpp:39).
#pragma once

#include "vrterrain.h"

#include <array>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <vector>

namespace vRenderer
{
    using LogFn = std::function<void(const char*)>;
    inline LogFn& Log() { static LogFn fn = [](const char* m) { std::fprintf(stderr, "[vrterrain] %s\n", m); }; return fn; }
    inline bool Check(int rc, const char* what)
    {
        if (rc == VR_OK) return true;
        char buf[640];
        std::snprintf(buf, sizeof(buf), "%s failed (%d): %s", what, rc, vr_last_error());
        Log()(buf);
        return false;
    }

    // nvrhi::IDevice + the frame's command list (main.cpp:57-61, Renderer.cpp:48)
    class Device
    {
        vr_context* m_Ctx = nullptr;
    public:
        explicit Device(int ordinal = 0) { Check(vr_context_create(ordinal, &m_Ctx), "vr_context_create"); }
        ~Device() { vr_context_destroy(m_Ctx); }
        Device(const Device&) = delete;
        Device& operator=(const Device&) = delete;
        explicit operator bool() const { return m_Ctx != nullptr; }
        vr_context* Get() const { return m_Ctx; }
        void SetStream(void* hipStream) { vr_context_set_stream(m_Ctx, hipStream); }
        void SetOption(int option, int value) { Check(vr_context_set_option(m_Ctx, option, value), "vr_context_set_option"); }   // VR_OPT_*
        void SetFrameFusion(bool enable) { SetOption(VR_OPT_FRAME_FUSION, enable ? 1 : 0); }
        void SetGbufferLazy(bool enable) { SetOption(VR_OPT_GBUFFER_LAZY, enable ? 1 : 0); }
        void WaitForIdle() { vr_context_synchronize(m_Ctx); }            // nvrhi::IDevice::waitForIdle
    };

    // EditorParams (Renderer.h:34-48): what the path reads and writes
    struct EditorParams
    {
        bool m_RenderTerrain = true;
        bool m_Wireframe = false;
        bool m_LockView = false;
        float m_MaxHeight = 400.0f;
        uint32_t m_NumChunks = 0;
        float m_AmbientIntensity = 0.01f;
    };

    // RenderTargets : GBufferRenderTargets (Renderer.h:50-110)
    class RenderTargets
    {
        vr_gbuffer* m_GBuffer = nullptr;
        vr_image* m_Hdr = nullptr;
        vr_ldr_image* m_Ldr = nullptr;             // LdrColor SRGBA8 (Renderer.h:81-92)
        int m_Width = 0, m_Height = 0;
        void Release() { vr_ldr_image_destroy(m_Ldr); vr_image_destroy(m_Hdr); vr_gbuffer_destroy(m_GBuffer); m_Ldr = nullptr; m_Hdr = nullptr; m_GBuffer = nullptr; }
    public:
        ~RenderTargets() { Release(); }
        bool Init(Device& device, int width, int height)
        {
            Release();
            m_Width = width; m_Height = height;
            return Check(vr_gbuffer_create(device.Get(), width, height, &m_GBuffer), "vr_gbuffer_create")
                && Check(vr_image_create(device.Get(), width, height, nullptr, &m_Hdr), "vr_image_create")
                && Check(vr_ldr_image_create(device.Get(), width, height, 0, nullptr, &m_Ldr), "vr_ldr_image_create");
        }
        void* LdrColor() const { return vr_ldr_image_device_ptr(m_Ldr); }                    // Renderer.h:81-92
        size_t LdrColorBytes() const { return vr_ldr_image_capacity(m_Ldr); }
        bool DownloadLdrColor(std::vector<uint8_t>& out) const
        {
            out.resize(LdrColorBytes());
            return Check(vr_ldr_image_download(m_Ldr, out.data(), out.size()), "vr_ldr_image_download");
        }
        [[nodiscard]] bool IsUpdateRequired(int width, int height) const { return width != m_Width || height != m_Height; }
        void Clear() { Check(vr_gbuffer_clear(m_GBuffer), "vr_gbuffer_clear"); }            // Renderer.cpp:382
        vr_gbuffer* GBufferFramebuffer() const { return m_GBuffer; }
        vr_image* HdrColor() const { return m_Hdr; }
        int Width() const { return m_Width; }
        int Height() const { return m_Height; }
    };

    // A stamp (vr_stamp): a patch of R8 (heightmap) or SRGBA8 (albedo) texels in device memory, owned by a device, for
    // TerrainPass::Stamp.  Destroyed before its device.
    class Stamp
    {
        vr_stamp* m_Stamp = nullptr;
    public:
        Stamp() = default;
        ~Stamp() { vr_stamp_destroy(m_Stamp); }
        Stamp(const Stamp&) = delete;
        Stamp& operator=(const Stamp&) = delete;
        // vr_stamp_create: w x h texels of `format` (VR_STAMP_R8 / VR_STAMP_SRGBA8), rows rowPitchBytes apart (0 = tightly packed);
        // from host memory the call returns once it has been consumed, from device memory the copy is stream-ordered.
        bool Create(Device& device, int format, int32_t w, int32_t h, const void* texels, size_t rowPitchBytes = 0, bool devicePointer = false)
        {
            vr_stamp_destroy(m_Stamp); m_Stamp = nullptr;
            return Check(vr_stamp_create(device.Get(), format, w, h, texels, rowPitchBytes, devicePointer ? 1 : 0, &m_Stamp), "vr_stamp_create");
        }
        // takes ownership of a stamp made elsewhere (TerrainPass::CaptureStamp)
        void Reset(vr_stamp* stamp = nullptr) { vr_stamp_destroy(m_Stamp); m_Stamp = stamp; }
        bool Info(int32_t& format, int32_t& w, int32_t& h) const { return Check(vr_stamp_info(m_Stamp, &format, &w, &h), "vr_stamp_info"); }
        bool Download(void* host, size_t bytes) const { return Check(vr_stamp_download(m_Stamp, host, bytes), "vr_stamp_download"); }
        vr_stamp* Get() const { return m_Stamp; }
    };

    class TerrainPass;

    // QuadTree (QuadTree.h:64-127).  The tree itself is implicit on the device; this object is the
    // reference's view of it: selection results of the last NodeSelect, LOD ranges, LOD count.
    class QuadTree
    {
        friend class TerrainPass;
        vr_terrain* m_Terrain = nullptr;
        std::vector<uint32_t> m_SelectedNodes;      // node ids in m_SelectedNodes order
        std::vector<vr_instance> m_Instances;       // what UpdateTransforms wrote for them
    public:
        static constexpr int MAX_LODS = VR_MAX_LODS;
        // NodeSelect(viewOrigin, root, numLods, frustum, maxHeight) + UpdateTransforms (TerrainPass.cpp:181-183)
        bool NodeSelect(const vr_view& view, float maxHeight)
        {
            vr_terrain_params p; vr_terrain_default_params(&p);
            m_SelectedNodes.assign(4096, 0u); m_Instances.assign(4096, vr_instance{});
            uint32_t n = 0;
            const bool ok = Check(vr_terrain_select(m_Terrain, &view, maxHeight, m_SelectedNodes.data(), m_Instances.data(), &n),
                                  "vr_terrain_select");
            m_SelectedNodes.resize(n); m_Instances.resize(n);
            return ok;
        }
        const std::vector<uint32_t>& GetSelectedNodes() const { return m_SelectedNodes; }
        const std::vector<vr_instance>& GetInstanceData() const { return m_Instances; }
        void ClearSelectedNodes() { m_SelectedNodes.clear(); m_Instances.clear(); }
        int GetNumLods() const { return vr_terrain_num_lods(m_Terrain); }
        std::array<float, MAX_LODS> GetLodRanges() const
        {
            std::array<float, MAX_LODS> r{};
            vr_terrain_lod_ranges(m_Terrain, r.data());
            return r;
        }
        // SetHeight over the whole tree + m_HeightLoaded (QuadTree.cpp:46-51,191-208)
        bool SetHeight(bool loaded) { return Check(vr_terrain_update_heights(m_Terrain, loaded ? 1 : 0), "vr_terrain_update_heights"); }
    };

    // vRenderer::TerrainPass (TerrainPass.h:32-159)
    class TerrainPass
    {
    public:
        struct CreateParameters { vr_terrain_params terrain; CreateParameters() { vr_terrain_default_params(&terrain); } };
        struct RenderParams { bool wireframe = false; bool lockView = false; bool depthOnly = false; };   // TerrainPass.h:68-73
    private:
        Device& m_Device;
        vr_terrain* m_Terrain = nullptr;
        std::vector<std::shared_ptr<QuadTree>> m_QuadTrees;
        float m_MaxHeight = 1.0f;
    public:
        explicit TerrainPass(Device& device) : m_Device(device) {}
        ~TerrainPass() { vr_terrain_destroy(m_Terrain); }
        TerrainPass(const TerrainPass&) = delete;
        TerrainPass& operator=(const TerrainPass&) = delete;

        // Init(shaderFactory, params, commandList, heightmapTexture, colorTexture, executor) (TerrainPass.cpp:34-141):
        // the two textures arrive as the decoded bytes Donut's TextureCache holds (R8 and SRGBA8).
        bool Init(const CreateParameters& params, const uint8_t* heightmapR8, int heightmapWidth, int heightmapHeight,
                  const uint8_t* colorSRGBA8, int colorWidth, int colorHeight)
        {
            if (!heightmapR8) { Log()("Heightmap texture data missing for QuadTree generation"); return false; }   // QuadTree.cpp:39
            vr_terrain_destroy(m_Terrain); m_Terrain = nullptr;
            if (!Check(vr_terrain_create(m_Device.Get(), &params.terrain, heightmapR8, heightmapWidth, heightmapHeight,
                                         colorSRGBA8, colorWidth, colorHeight, &m_Terrain), "vr_terrain_create"))
                return false;
            auto qt = std::make_shared<QuadTree>();
            qt->m_Terrain = m_Terrain;
            m_QuadTrees = { qt };          // all surfaces are swept together on the device; one facade covers them
            return true;
        }

        // Render(commandList, compositeView, compositeViewPrev, framebufferFactory, renderParams, editorParams)
        // (TerrainPass.cpp:143-232).  Asynchronous; editorParams.m_NumChunks is refreshed by UpdateNumChunks().
        bool Render(const vr_view& view, const vr_view* viewPrev, RenderTargets& targets, const RenderParams& renderParams,
                    EditorParams& editorParams, const vr_partition* partition = nullptr)
        {
            m_MaxHeight = editorParams.m_MaxHeight;
            vr_render_params rp; vr_render_default_params(&rp);
            rp.wireframe = renderParams.wireframe; rp.lock_view = renderParams.lockView; rp.depth_only = renderParams.depthOnly;
            rp.max_height = m_MaxHeight;
            if (!Check(vr_terrain_render(m_Terrain, &view, viewPrev ? viewPrev : &view, targets.GBufferFramebuffer(), &rp, partition),
                       "vr_terrain_render")) {
                Log()("TerrainPass::Render - Couldn't create PSO");          // TerrainPass.cpp:226, the reference's only failure path
                return false;
            }
            return true;
        }
        // editorParams.m_NumChunks = numNodes (TerrainPass.cpp:198); synchronises with the device
        bool UpdateNumChunks(EditorParams& editorParams)
        {
            uint32_t n = 0;
            const bool ok = Check(vr_terrain_num_chunks(m_Terrain, &n), "vr_terrain_num_chunks");
            editorParams.m_NumChunks = n;
            return ok;
        }
        // Terrain queries (grown from QuadTree::GetHeightValue, QuadTree.h:84) against the surface the last Render's max height
        // draws; host arrays, synchronous.  xz: n pairs; heights: n floats; normals: optional, 3 n floats.
        bool SampleHeights(const float* xz, uint32_t n, float* heights, float* normals = nullptr)
        {
            return Check(vr_terrain_query_heights(m_Terrain, xz, n, m_MaxHeight, heights, normals, 0), "vr_terrain_query_heights");
        }
        // first hit of each ray with the terrain (vr_ray_hit::status: VR_RAY_HIT / VR_RAY_MISS / VR_RAY_INVALID / VR_RAY_STEP_LIMIT)
        bool CastRays(const vr_ray* rays, uint32_t n, vr_ray_hit* hits)
        {
            return Check(vr_terrain_cast_rays(m_Terrain, rays, n, m_MaxHeight, hits, 0), "vr_terrain_cast_rays");
        }
        // vr_terrain_edit: the w x h texels at (x, y) of the heightmap's (which = 0, 1 byte each) or the albedo's (which = 1, 4 bytes
        // each) level 0 are replaced in place; afterwards the pass behaves as one initialised from the edited arrays.  Host memory
        // by default (the call returns once it has been consumed); devicePointer: stream-ordered, nothing is synchronised.
        bool Edit(int which, int32_t x, int32_t y, int32_t w, int32_t h, const void* texels, size_t rowPitchBytes = 0, bool devicePointer = false)
        {
            return Check(vr_terrain_edit(m_Terrain, which, x, y, w, h, texels, rowPitchBytes, devicePointer ? 1 : 0), "vr_terrain_edit");
        }
        // vr_terrain_brush: one stroke - stroke.op and n dabs in order - on level 0 of the heightmap or (VR_BRUSH_PAINT) the albedo,
        // computed on the device; stream-ordered, nothing is synchronised, and `dabs` is free again when the call returns.
        // outRect (optional): {x, y, w, h} of the level-0 rectangle treated as dirty.
        bool Brush(const vr_brush_stroke& stroke, const vr_brush_dab* dabs, uint32_t n, int32_t outRect[4] = nullptr)
        {
            return Check(vr_terrain_brush(m_Terrain, &stroke, dabs, n, outRect), "vr_terrain_brush");
        }
        // vr_terrain_texture: level 0 of the albedo painted by rule from the heightmap's shape - numLayers altitude and slope layers,
        // applied in order - under the mask the n dabs form (as for Erode, prepared for the albedo), or over the whole map
        // (wholeMap: dabs == nullptr, n == 0); computed on the device, stream-ordered like Brush, nothing is synchronised, and
        // `layers` and `dabs` are free again when the call returns.  maxHeight: the world height of byte 255.  outRect as for Brush.
        bool Texture(const vr_texture_layer* layers, int32_t numLayers, float maxHeight, const vr_brush_dab* dabs, uint32_t n, bool wholeMap = false,
                     int32_t outRect[4] = nullptr)
        {
            vr_texture_params p = {};
            p.num_layers = numLayers; p.flags = wholeMap ? (uint32_t)VR_TEXTURE_WHOLE_MAP : 0u; p.max_height = maxHeight;
            return Check(vr_terrain_texture(m_Terrain, &p, layers, dabs, n, outRect), "vr_terrain_texture");
        }
        // vr_terrain_occlusion: sky visibility baked into level 0 of the albedo by horizon marching over the heightmap (params: radius,
        // max_height, gain, bias, opacity, color, channel_mask, directions, mode) under the mask the n dabs form (as for Texture,
        // prepared for the albedo), or over the whole map (wholeMap: dabs == nullptr, n == 0; sets VR_OCCLUSION_WHOLE_MAP in a copy of
        // params); computed on the device, stream-ordered like Brush, nothing is synchronised, and `dabs` is free again when the call
        // returns.  outRect as for Brush.
        bool Occlusion(const vr_occlusion_params& params, const vr_brush_dab* dabs, uint32_t n, bool wholeMap = false, int32_t outRect[4] = nullptr)
        {
            vr_occlusion_params p = params;
            if (wholeMap) p.flags |= (uint32_t)VR_OCCLUSION_WHOLE_MAP;
            return Check(vr_terrain_occlusion(m_Terrain, &p, dabs, n, outRect), "vr_terrain_occlusion");
        }
        // vr_terrain_noise: fractal value or gradient noise (params: frequency, offset, lacunarity, gain, octaves, seed, basis, fractal)
        // added to or blended into level 0 of the heightmap (which = 0) or the albedo (1) under the mask the n dabs form (as for
        // Erode, prepared for that map), or over the whole map (wholeMap: dabs == nullptr, n == 0; sets VR_NOISE_WHOLE_MAP in a copy
        // of params); computed on the device, stream-ordered like Brush, nothing is synchronised, and `dabs` is free again when the
        // call returns.  outRect as for Brush.
        bool Noise(int which, const vr_noise_params& params, const vr_brush_dab* dabs, uint32_t n, bool wholeMap = false, int32_t outRect[4] = nullptr)
        {
            vr_noise_params p = params;
            if (wholeMap) p.flags |= (uint32_t)VR_NOISE_WHOLE_MAP;
            return Check(vr_terrain_noise(m_Terrain, which, &p, dabs, n, outRect), "vr_terrain_noise");
        }
        // vr_terrain_path: a corridor of half-width params.radius along the polyline through `points` (world x, z and a target height in
        // stored units each) - LEVEL, CUT or FILL on the heightmap (which = 0), PAINT on the albedo (1); every texel takes its weight and
        // its target from the nearest segment and changes once.  closed: the last point is joined to the first (sets VR_PATH_CLOSED in a
        // copy of params).  Computed on the device, stream-ordered like Brush, nothing is synchronised, and `points` is free again when
        // the call returns.  outRect as for Brush.
        bool Path(int which, const vr_path_params& params, const vr_path_point* points, uint32_t n, bool closed = false, int32_t outRect[4] = nullptr)
        {
            vr_path_params p = params;
            if (closed) p.flags |= (uint32_t)VR_PATH_CLOSED;
            return Check(vr_terrain_path(m_Terrain, which, &p, points, n, outRect), "vr_terrain_path");
        }
        // vr_terrain_region: the inside of the polygon through `points` (world x, z; contourCounts[c] points per closed contour, or none
        // for one contour of all n; even-odd, so a contour within another is a hole) - LEVEL, CUT, FILL or RAISE on the heightmap
        // (which = 0), PAINT on the albedo (1), with a feather of params.feather world units outside the outline, or inside it with
        // VR_REGION_FEATHER_INSIDE.  Computed on the device, stream-ordered like Path, nothing is synchronised, and `points` is free
        // again when the call returns.  outRect as for Brush.
        bool Region(int which, const vr_region_params& params, const vr_region_point* points, uint32_t n, const uint32_t* contourCounts = nullptr,
                    uint32_t numContours = 0, int32_t outRect[4] = nullptr)
        {
            return Check(vr_terrain_region(m_Terrain, which, &params, points, n, contourCounts, numContours, outRect), "vr_terrain_region");
        }
        // vr_stamp_from_terrain: the w x h texels at (x, y) of level 0 of the heightmap (which = 0) or the albedo (1) as they are on the
        // device, into `out` - the clone tool's source; a device copy on the context's stream, nothing is synchronised.
        bool CaptureStamp(int which, int32_t x, int32_t y, int32_t w, int32_t h, vRenderer::Stamp& out)
        {
            vr_stamp* s = nullptr;
            const bool ok = Check(vr_stamp_from_terrain(m_Terrain, which, x, y, w, h, &s), "vr_stamp_from_terrain");
            out.Reset(s);
            return ok;
        }
        // vr_terrain_stamp: `stamp` set into level 0 of map `which` at params' position, size and angle with its blend rule, computed
        // on the device; stream-ordered like Brush, nothing is synchronised.  outRect as for Brush.
        bool Stamp(int which, const vRenderer::Stamp& stamp, const vr_stamp_params& params, int32_t outRect[4] = nullptr)
        {
            return Check(vr_terrain_stamp(m_Terrain, which, stamp.Get(), &params, outRect), "vr_terrain_stamp");
        }
        // vr_terrain_erode: `iterations` sweeps of thermal erosion of the heightmap's level 0 under the mask the n dabs form (strength =
        // opacity; their order does not matter), computed on the device; stream-ordered like Brush, nothing is synchronised.
        // talus: the height step per texel that stays, in heightmap steps; rate: 0 < rate <= 0.125.  outRect as for Brush.
        bool Erode(const vr_brush_dab* dabs, uint32_t n, int32_t iterations, float talus, float rate, int32_t outRect[4] = nullptr)
        {
            vr_erode_params p = {};
            p.iterations = iterations; p.talus = talus; p.rate = rate;
            return Check(vr_terrain_erode(m_Terrain, &p, dabs, n, outRect), "vr_terrain_erode");
        }
        // vr_terrain_erode_hydraulic: `iterations` sweeps of hydraulic erosion of the heightmap's level 0 under the mask the n dabs form
        // (as for Erode): water rains on the mask, runs downhill, dissolves terrain where it runs and deposits where it slows.  rain
        // 0 .. 16 per sweep, flow in (0, 1], capacity 0 .. 64, dissolve, deposit and evaporation in [0, 1].  Stream-ordered like Brush.
        bool ErodeHydraulic(const vr_brush_dab* dabs, uint32_t n, int32_t iterations, float rain, float flow, float capacity, float dissolve, float deposit,
                            float evaporation, int32_t outRect[4] = nullptr)
        {
            vr_hydro_params p = {};
            p.iterations = iterations; p.rain = rain; p.flow = flow; p.capacity = capacity; p.dissolve = dissolve; p.deposit = deposit; p.evaporation = evaporation;
            return Check(vr_terrain_erode_hydraulic(m_Terrain, &p, dabs, n, outRect), "vr_terrain_erode_hydraulic");
        }
        // vr_terrain_history_*: undo and redo of Edit, Brush, Erode and ErodeHydraulic on the device.  EnableHistory(bytes) sets the arena (0: off);
        // CommitHistory closes the open step (mouse-up); Undo / Redo return whether a step was applied (*applied).
        bool EnableHistory(size_t budgetBytes) { return Check(vr_terrain_history_enable(m_Terrain, budgetBytes), "vr_terrain_history_enable"); }
        bool CommitHistory() { return Check(vr_terrain_history_commit(m_Terrain), "vr_terrain_history_commit"); }
        bool Undo() { int32_t applied = 0; return Check(vr_terrain_undo(m_Terrain, &applied), "vr_terrain_undo") && applied != 0; }
        bool Redo() { int32_t applied = 0; return Check(vr_terrain_redo(m_Terrain, &applied), "vr_terrain_redo") && applied != 0; }
        vr_history_status HistoryStatus() const { vr_history_status st = {}; (void)vr_terrain_history_status(m_Terrain, &st); return st; }
        void SetMaxHeight(float maxHeight) { m_MaxHeight = maxHeight; }      // for queries before the first Render
        const std::vector<std::shared_ptr<QuadTree>>& GetQuadTrees() const { return m_QuadTrees; }
        vr_terrain* Get() const { return m_Terrain; }
    };

    // the ray through the centre of pixel (px, py) of the view's viewport, near plane to far plane (picking)
    inline bool PixelRay(const vr_view& view, float px, float py, vr_ray& out)
    {
        return Check(vr_view_pixel_ray(&view, px, py, &out), "vr_view_pixel_ray");
    }

    // donut::render::CascadedShadowMap with the one cascade the reference creates (Renderer.cpp:83-87)
    class CascadedShadowMap
    {
        Device& m_Device;
        RenderTargets m_Targets;           // m_ShadowFramebuffer: only the depth plane is used
        vr_shadow_params m_Params;
        vr_view m_View{};
    public:
        CascadedShadowMap(Device& device, int resolution, float worldSize) : m_Device(device)
        {
            vr_shadow_default_params(&m_Params, worldSize);
            m_Params.resolution = resolution;
            m_Targets.Init(device, resolution, resolution);
        }
        vr_shadow_params& Params() { return m_Params; }
        // SetupForPlanarViewStable(light, projectionFrustum, inverseViewMatrix, maxShadowDistance, zUp, zDown, exponent, 0, 1)
        bool SetupForPlanarViewStable(const vr_light& light, const vr_view& cameraView)
        {
            return Check(vr_shadow_view_setup(&light, &cameraView, &m_Params, &m_View), "vr_shadow_view_setup");
        }
        void Clear() { m_Targets.Clear(); }                                                   // Renderer.cpp:354
        const vr_view& GetView() const { return m_View; }
        RenderTargets& Framebuffer() { return m_Targets; }
        vr_shadow_binding Binding(int lightIndex) { return vr_shadow_binding{ &m_View, m_Targets.GBufferFramebuffer(), lightIndex, m_Params.depth_bias }; }
    };

    // donut::render::DeferredLightingPass as used at Renderer.cpp:239-240,417-428
    class DeferredLightingPass
    {
        Device& m_Device;
    public:
        struct Inputs
        {
            RenderTargets* gbuffer = nullptr;                       // SetGBuffer(*m_RenderTargets)
            float ambientColorTop[3] = { 0, 0, 0 };
            float ambientColorBottom[3] = { 0, 0, 0 };
            const std::vector<vr_light>* lights = nullptr;
            CascadedShadowMap* shadowMap = nullptr;                 // DirectionalLight::shadowMap (Renderer.cpp:336)
            int shadowLightIndex = 0;
            vr_image* output = nullptr;                             // HdrColor
            void SetGBuffer(RenderTargets& targets) { gbuffer = &targets; output = targets.HdrColor(); }
        };
        explicit DeferredLightingPass(Device& device) : m_Device(device) {}
        void Init() {}
        void ResetBindingCache() {}                                 // Renderer.cpp:216: nothing is cached here
        bool Render(const vr_view& view, const Inputs& inputs, const vr_partition* partition = nullptr)
        {
            static const std::vector<vr_light> none;
            const std::vector<vr_light>& l = inputs.lights ? *inputs.lights : none;
            // More lights than DEFERRED_MAX_LIGHTS (16) - which used to be vr_deferred_light's "at most 16 lights" error - go to the
            // tiled pass for every light type, with the shadow map if there is one.  That pass needs a frame width that is a
            // multiple of 4, and reports a light tile that kept more than VR_TILE_LIGHT_CAP lights through vr_deferred_tiled_status
            // (asynchronously: call it once per frame or less), not through this return value.
            if (l.size() > 16) {
                vr_shadow_binding sb{};
                if (inputs.shadowMap) sb = inputs.shadowMap->Binding(inputs.shadowLightIndex);
                return Check(vr_deferred_light_tiled_ex(m_Device.Get(), &view, inputs.gbuffer->GBufferFramebuffer(), l.data(), (int32_t)l.size(),
                                                        inputs.ambientColorTop, inputs.ambientColorBottom, inputs.output, partition,
                                                        inputs.shadowMap ? &sb : nullptr),
                             "vr_deferred_light_tiled_ex");
            }
            if (inputs.shadowMap) {
                const vr_shadow_binding sb = inputs.shadowMap->Binding(inputs.shadowLightIndex);
                return Check(vr_deferred_light_shadowed(m_Device.Get(), &view, inputs.gbuffer->GBufferFramebuffer(), l.data(), (int32_t)l.size(),
                                                        inputs.ambientColorTop, inputs.ambientColorBottom, inputs.output, partition, &sb),
                             "vr_deferred_light_shadowed");
            }
            return Check(vr_deferred_light(m_Device.Get(), &view, inputs.gbuffer->GBufferFramebuffer(), l.data(), (int32_t)l.size(),
                                           inputs.ambientColorTop, inputs.ambientColorBottom, inputs.output, partition),
                         "vr_deferred_light");
        }
    };

    // donut::render::ToneMappingPass as used at Renderer.cpp:188-189,256-257,430-431
    class ToneMappingPass
    {
        vr_tonemap* m_Pass = nullptr;
        float m_FrameTime = 0.0f;
    public:
        struct ToneMappingParameters : vr_tonemap_params { ToneMappingParameters() { vr_tonemap_default_params(this); } };
        explicit ToneMappingPass(Device& device) { Check(vr_tonemap_create(device.Get(), &m_Pass), "vr_tonemap_create"); }
        ~ToneMappingPass() { vr_tonemap_destroy(m_Pass); }
        ToneMappingPass(const ToneMappingPass&) = delete;
        ToneMappingPass& operator=(const ToneMappingPass&) = delete;
        void AdvanceFrame(float frameTime) { m_FrameTime = frameTime; }                      // Renderer.cpp:188-189
        bool ResetExposure(float initialExposure = 0.0f) { return Check(vr_tonemap_reset_exposure(m_Pass, initialExposure), "vr_tonemap_reset_exposure"); }
        bool ResetHistogram() { return Check(vr_tonemap_reset_histogram(m_Pass), "vr_tonemap_reset_histogram"); }
        bool AddFrameToHistogram(const ToneMappingParameters& params, RenderTargets& targets)
        {
            return Check(vr_tonemap_add_frame_to_histogram(m_Pass, &params, targets.HdrColor(), targets.Width(), targets.Height(), nullptr),
                         "vr_tonemap_add_frame_to_histogram");
        }
        bool ComputeExposure(const ToneMappingParameters& params) { return Check(vr_tonemap_compute_exposure(m_Pass, &params, m_FrameTime), "vr_tonemap_compute_exposure"); }
        bool Render(const ToneMappingParameters& params, RenderTargets& targets)
        {
            return Check(vr_tonemap_render(m_Pass, &params, targets.HdrColor(), targets.Width(), targets.Height(), targets.LdrColor(),
                                           targets.LdrColorBytes(), nullptr), "vr_tonemap_render");
        }
        // SimpleRender(commandList, params, compositeView, sourceTexture) (Renderer.cpp:431)
        bool SimpleRender(const ToneMappingParameters& params, RenderTargets& targets)
        {
            return Check(vr_tonemap_simple_render(m_Pass, &params, m_FrameTime, targets.HdrColor(), targets.LdrColor(), targets.LdrColorBytes()),
                         "vr_tonemap_simple_render");
        }
        vr_tonemap* Get() const { return m_Pass; }
    };
} // namespace vRenderer
